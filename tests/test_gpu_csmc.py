"""GPU: the conditional SMC sweep with ancestor sampling (pfg_csmc_device, csrc/pfg_csmc.hip) against its NumPy restatement
(tests/helpers/csmc_model.py): the traced twin replayed in long double, structural properties of what it records, the
degenerate chain, and the invariance of the smoothing law on the device."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import csmc_model as cm  # noqa: E402
import keyed_draws as kd  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
RTOL, ATOL = 1e-8, 1e-8         # the device-replay tests' tolerance on states, weights and statistics (test_gpu_device_replay.py)
OFF, STEP = 11, 4


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def launch(model, theta, y, path, N, seed, off, step, has_ref=True, traced=True, pm=cm.PM, pv=cm.PV, sweeps=1):
    """`sweeps` launches of pfg_csmc_device on B chains (the counter advancing by one each); what the last one left."""
    import torch
    from sgmcmc_ssm_amd import _capi
    dev = torch.device("cuda", 0)
    B, P = theta.shape
    y = np.array(np.broadcast_to(y, (B, y.shape[-1])), dtype=np.float64, order="C")      # a writable row-major copy
    T = y.shape[1]
    th = np.zeros((B, _capi.MAX_THETA))
    th[:, :P] = theta
    sb = _capi.csmc_scratch_bytes(T, N)
    t = dict(theta=torch.from_numpy(th).to(dev), y=torch.from_numpy(y).to(dev),
             path=torch.from_numpy(np.ascontiguousarray(path, dtype=np.float64)).to(dev),
             scratch=torch.zeros(B * sb, dtype=torch.uint8, device=dev),
             out=torch.zeros((B, _capi.OUT_DOUBLES), dtype=torch.float64, device=dev),
             n_degenerate=torch.zeros(B, dtype=torch.int64, device=dev),
             trace_anc=torch.full((B, T, N), -1, dtype=torch.int32, device=dev),
             trace_ref_anc=torch.full((B, T), -1, dtype=torch.int32, device=dev),
             trace_w=torch.zeros((B, T, N), dtype=torch.float64, device=dev),
             trace_k=torch.full((B,), -1, dtype=torch.int32, device=dev))
    d = np.zeros(B, dtype=_capi.CSMC_PROBLEM_DTYPE)
    for name, ten in t.items():
        d[name] = ten.data_ptr() + np.arange(B, dtype=np.uint64) * np.uint64(ten.numel() // B * ten.element_size())
    d["prior_mean"], d["prior_var"], d["T"], d["N"], d["has_ref"] = pm, pv, T, N, int(has_ref)
    desc = torch.from_numpy(d.view(np.uint8).reshape(B, -1)).to(dev)
    ctr = torch.full((1,), int(step), dtype=torch.int64, device=dev)
    for _ in range(sweeps):
        _ctx().csmc_device(model, "f64", N, B, desc.data_ptr(), seed, off, ctr.data_ptr(), 0, traced=traced)
        ctr += 1
    torch.cuda.synchronize()
    raw = t["scratch"].cpu().numpy().reshape(B, sb)
    res = {k: v.cpu().numpy() for k, v in t.items() if k != "scratch"}
    res["x"] = raw[:, :T * N * 8].copy().view(np.float64).reshape(B, T, N)
    res["anc16"] = raw[:, T * N * 8:T * N * 10].copy().view(np.uint16).reshape(B, T, N)
    return res


@functools.lru_cache(maxsize=None)
def traced_case(model, N, T, B):
    th, y, path = cm.case_inputs(model, N, T, B)
    got = launch(model, th, y, path, N, cm.sweep_seed(cm.SEED), OFF, STEP)
    return th, y, path, got


# ---- 5. replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B", cm.CASES)
def test_traced_sweep_replays_on_the_host(model, N, T, B):
    """The traced twin's recorded indices are those the long-double model searches for the keyed uniforms (the neighbour only
    within 1e-12 of a CDF edge, on at most 1 % of the case's indices); teacher-forced on them, the states, the normalised
    weights, the new path and out[0..7] agree; the production instantiation writes the same path, bit for bit."""
    th, y, path, got = traced_case(model, N, T, B)
    assert not got["n_degenerate"].any()
    anc = got["trace_anc"].astype(np.int64)
    ref = cm.sweep(model, th, y, path, N, cm.sweep_seed(cm.SEED), kd.chain_ids(B, OFF), STEP, cm.PM, cm.PV, F=LD,
                   forced=dict(anc=anc, k=got["trace_k"]))
    wrong, edge, n = cm.index_mismatches(anc, got["trace_k"], ref)
    print("indices", n, "edge", edge, "wrong", wrong)
    assert wrong == 0 and edge <= cm.EDGE_SHARE * n, (wrong, edge, n)
    np.testing.assert_allclose(got["x"], ref["x"].astype(np.float64), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got["trace_w"], ref["w"].astype(np.float64), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got["path"], ref["path"].astype(np.float64), rtol=RTOL, atol=ATOL)
    scale = max(1.0, float(np.abs(ref["out"]).max()))
    np.testing.assert_allclose(got["out"], ref["out"].astype(np.float64), rtol=RTOL, atol=ATOL * scale)
    prod = launch(model, th, y, path, N, cm.sweep_seed(cm.SEED), OFF, STEP, traced=False)
    assert np.array_equal(prod["path"], got["path"]) and np.array_equal(prod["out"], got["out"])
    assert np.all(prod["trace_anc"] == -1) and np.all(prod["trace_k"] == -1)       # ... and leaves the trace buffers alone


# ---- 6. structure -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B", cm.CASES)
def test_recorded_genealogy(model, N, T, B):
    """Particle N-1 is x*_t bitwise at every step, parents are particle indices (and the uint16 history is the trace), the
    reference particle's recorded ancestor is its parent, the new path is a lineage of the genealogy."""
    th, y, path, got = traced_case(model, N, T, B)
    assert np.array_equal(got["x"][:, :, N - 1], path)
    anc = got["trace_anc"]
    assert np.all(anc[:, 0] == -1) and np.all((anc[:, 1:] >= 0) & (anc[:, 1:] < N))
    assert np.array_equal(got["anc16"][:, 1:], anc[:, 1:])
    assert np.array_equal(got["trace_ref_anc"][:, 1:], anc[:, 1:, N - 1])
    np.testing.assert_allclose(got["trace_w"].sum(axis=2), 1.0, rtol=1e-12)
    k = got["trace_k"].astype(np.int64)
    assert np.all((k >= 0) & (k < N))
    rows = np.arange(B)
    for t in range(T - 1, -1, -1):
        assert np.array_equal(got["path"][:, t], got["x"][rows, t, k])
        k = anc[rows, t, k].astype(np.int64)


@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B", [(5, 3, 3), (129, 37, 2)])
def test_unconditional_sweep_never_reads_the_path(model, N, T, B):
    """has_ref = 0 with a NaN-filled path buffer: all N particles are free, the path comes out finite and replays."""
    th, y, _ = cm.case_inputs(model, N, T, B)
    got = launch(model, th, y, np.full((B, T), np.nan), N, cm.sweep_seed(cm.SEED), OFF, 0, has_ref=False)
    assert np.all(np.isfinite(got["path"])) and np.all(np.isfinite(got["out"])) and not got["n_degenerate"].any()
    anc = got["trace_anc"].astype(np.int64)
    ref = cm.sweep(model, th, y, None, N, cm.sweep_seed(cm.SEED), kd.chain_ids(B, OFF), 0, cm.PM, cm.PV, has_ref=False, F=LD,
                   forced=dict(anc=anc, k=got["trace_k"]))
    wrong, edge, n = cm.index_mismatches(anc, got["trace_k"], ref)
    assert wrong == 0 and edge <= cm.EDGE_SHARE * n
    np.testing.assert_allclose(got["path"], ref["path"].astype(np.float64), rtol=RTOL, atol=ATOL)
    assert np.all(got["trace_ref_anc"] == -1)


@pytest.mark.parametrize("N", [5, 257])
def test_degenerate_chain_keeps_its_path(N):
    """SVM, one chain of the batch fed y = +-1e300: all its weights are zero, so it keeps its path, its record is that of the
    path -- the transition sums finite, out[3] = sum y_t^2 exp(-x_t) = +inf, the overflow of y^2 itself, never NaN --,
    n_degenerate == 1, and its neighbours are what they are without it."""
    T, B = 6, 3
    th, y, path = cm.case_inputs("svm", N, T, B)
    ys = np.tile(y, (B, 1))
    ys[1] = 1e300 * (-1.0) ** np.arange(T)
    got = launch("svm", th, ys, path, N, cm.sweep_seed(cm.SEED), OFF, STEP)
    assert got["n_degenerate"].tolist() == [0, 1, 0]
    assert np.array_equal(got["path"][1], path[1])
    exp = cm.record("svm", path[1:2], ys[1:2])[0]
    assert not np.isnan(got["out"][1]).any() and np.all(np.isfinite(got["out"][1, [0, 1, 2, 4, 5, 6, 7]]))
    np.testing.assert_allclose(got["out"][1], exp, rtol=1e-12)
    base = launch("svm", th, np.tile(y, (B, 1)), path, N, cm.sweep_seed(cm.SEED), OFF, STEP)
    for b in (0, 2):
        assert np.array_equal(got["path"][b], base["path"][b]) and np.array_equal(got["out"][b], base["out"][b])
    assert not np.isnan(got["path"]).any()


def test_entry_point_refusals():
    from sgmcmc_ssm_amd import _capi
    import torch
    buf = torch.zeros(_capi.CSMC_PROBLEM_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    ctx = _ctx()
    with pytest.raises(NotImplementedError, match="SVM and LGSSM"):
        ctx.csmc_device("garch", "f64", 8, 1, buf.data_ptr(), 1)
    with pytest.raises(NotImplementedError, match="f64 only"):
        ctx.csmc_device("svm", "f32", 8, 1, buf.data_ptr(), 1)
    for n in (1, 1025):
        with pytest.raises(NotImplementedError, match="2 <= N <= 1024"):
            ctx.csmc_device("svm", "f64", n, 1, buf.data_ptr(), 1)
    with pytest.raises(ValueError, match="NULL"):
        ctx.csmc_device("svm", "f64", 8, 1, 0, 1)
    # a zeroed record (every array NULL, T = 0) is refused by the kernel itself, without a store
    ctx.csmc_device("svm", "f64", 8, 1, buf.data_ptr(), 1)
    torch.cuda.synchronize()


# ---- 7. invariance on the device ----------------------------------------------------------------------------------------------
def test_smoothing_law_is_invariant_on_the_device():
    """LGSSM, fixed theta, T = 8, N = 16, 4096 chains, 20 sweeps from prior-drawn paths: E x_t and E x_t x_{t-1} inside 5
    standard errors of the Kalman smoother's values (the bound of tests/test_csmc_host.py, derived from the exact second
    moments and the Gaussian fourth moments)."""
    T, N, n = 8, 16, 4096
    theta = np.array(cm.THETA["lgssm"])
    rs = np.random.RandomState(17)
    x = cm.sample_prior_paths(theta, T, 1, cm.PM, cm.PV, rs)[0]
    y = x + rs.standard_normal(T) / theta[3]
    mean, cov = cm.lgssm_smoother(theta, y, cm.PM, cm.PV)
    e1, b1, e2, b2 = cm.moment_bounds(mean, cov, n)
    start = cm.sample_prior_paths(theta, T, n, cm.PM, cm.PV, rs)
    got = launch("lgssm", np.tile(theta, (n, 1)), y, start, N, 123, 0, 1, traced=False, sweeps=20)
    p = got["path"]
    off = np.concatenate([np.abs(p.mean(axis=0) - e1) / b1, np.abs((p[:, 1:] * p[:, :-1]).mean(axis=0) - e2) / b2])
    print("moment errors / bound", np.round(off, 3))
    assert not got["n_degenerate"].any() and off.max() <= 1.0, off
