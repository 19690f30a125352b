"""GPU: the score the two sorted filters carry (pfg_cpm_score_device, pfg_sqmc_score_device; csrc/pfg_cpm.hip, csrc/pfg_sqmc.hip,
STAT = PFG_STAT_SCORE) against the filters without it and against its NumPy restatement (tests/helpers/sorted_score_model.py):
the same filter bit for bit, the traced twin replayed in long double, the plain recursion at lambduh = 1, the global id alone,
the degenerate chain, refused descriptors and the entry points' refusals."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cpm_model as cp  # noqa: E402
import keyed_draws as kd  # noqa: E402
import sorted_score_model as ss  # noqa: E402
import sqmc_model as sq  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
OFF, STEP = 2 ** 32 - 3, 5          # the chain ids straddle 2^32: the high word takes part in the key
TOL = 1e-9                          # of the magnitude of the terms (sorted_score_model: mag), the project's pins to the oracle
ANC_FILL, LL_FILL, Z_FILL = -2, -7.0, 9.0
H = ss.H_DIM
LAMS = [1.0, 0.95]


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def _records(dtype, B, tensors):
    d = np.zeros(B, dtype=dtype)
    for name, ten in tensors.items():
        d[name] = ten.data_ptr() + np.arange(B, dtype=np.uint64) * np.uint64(ten.numel() // B * ten.element_size())
    return d


def _upload(d):
    import torch
    return torch.from_numpy(d.view(np.uint8).reshape(len(d), -1)).to("cuda:0")


def launch_cpm(model, theta, y, U, N, rho, lam, off=OFF, step=STEP, traced=True, which=None, n_max=None, edit=None):
    """One launch on B chains whose current normals are U [B, T+1, N+1] (chain b keeps them in buffer which[b], default b & 1).
    lam None: pfg_cpm_device; otherwise pfg_cpm_score_device with that lambduh.  Returns out, trace_anc, trace_ll, U_prop, U_cur."""
    import torch
    from sgmcmc_ssm_amd import _capi
    dev = torch.device("cuda", 0)
    B, P = theta.shape
    y = np.array(np.broadcast_to(y, (B, y.shape[-1])), dtype=np.float64, order="C")
    T = y.shape[1]
    th = np.zeros((B, _capi.MAX_THETA))
    th[:, :P] = theta
    sb, n = _capi.cpm_aux_bytes(T, N), (T + 1) * (N + 1)
    which = (np.arange(B) & 1 if which is None else np.asarray(which)).astype(np.int32)
    bufs = np.zeros((2, B, sb // 8))
    bufs[which, np.arange(B), :n] = np.asarray(U, dtype=np.float64).reshape(B, n)
    bufs[:, :, n:] = 7.0                # the padding of a slab: never touched
    aux = torch.from_numpy(bufs).to(dev)
    t = dict(theta=torch.from_numpy(th).to(dev), y=torch.from_numpy(y).to(dev), which=torch.from_numpy(which).to(dev),
             out=torch.full((B, _capi.OUT_DOUBLES), 3.0, dtype=torch.float64, device=dev),
             trace_anc=torch.full((B, T, N), ANC_FILL, dtype=torch.int32, device=dev),
             trace_ll=torch.full((B, T), LL_FILL, dtype=torch.float64, device=dev))
    d = _records(_capi.CPM_PROBLEM_DTYPE, B, t)
    d["u0"] = aux.data_ptr() + np.arange(B, dtype=np.uint64) * np.uint64(sb)
    d["u1"] = aux.data_ptr() + (np.arange(B, dtype=np.uint64) + np.uint64(B)) * np.uint64(sb)
    d["prior_mean"], d["prior_var"], d["T"], d["N"] = cp.PM, cp.PV, T, N
    if edit is not None:
        edit(d)
    desc = _upload(d)
    ctr = torch.full((1,), int(step), dtype=torch.int64, device=dev)
    seed = cp.filter_seed(cp.SEED)
    if lam is None:
        _ctx().cpm_device(model, "f64", n_max or N, B, desc.data_ptr(), rho, seed, off, ctr.data_ptr(), 0, traced=traced)
    else:
        _ctx().cpm_score_device(model, "f64", n_max or N, B, desc.data_ptr(), rho, lam, seed, off, ctr.data_ptr(), 0, traced=traced)
    torch.cuda.synchronize()
    after = aux.cpu().numpy()
    assert np.all(after[:, :, n:] == 7.0) and int(ctr.item()) == int(step)
    rows = np.arange(B)
    res = {k: v.cpu().numpy() for k, v in t.items() if k in ("out", "trace_anc", "trace_ll")}
    res["U_prop"] = after[1 - which, rows, :n].reshape(B, T + 1, N + 1)
    res["U_cur"] = after[which, rows, :n].reshape(B, T + 1, N + 1)
    return res


def launch_sqmc(model, theta, y, N, n_max, lam, off=OFF, step=STEP, traced=True, edit=None):
    """One launch on B chains.  lam None: pfg_sqmc_device; otherwise pfg_sqmc_score_device.  Returns out and the trace arrays."""
    import torch
    from sgmcmc_ssm_amd import _capi
    dev = torch.device("cuda", 0)
    B, P = theta.shape
    y = np.array(np.broadcast_to(y, (B, y.shape[-1])), dtype=np.float64, order="C")
    T = y.shape[1]
    th = np.zeros((B, _capi.MAX_THETA))
    th[:, :P] = theta
    t = dict(theta=torch.from_numpy(th).to(dev), y=torch.from_numpy(y).to(dev),
             out=torch.full((B, _capi.OUT_DOUBLES), 3.0, dtype=torch.float64, device=dev),
             trace_anc=torch.full((B, T, N), ANC_FILL, dtype=torch.int32, device=dev),
             trace_ll=torch.full((B, T), LL_FILL, dtype=torch.float64, device=dev),
             trace_z=torch.full((B, T + 1, N), Z_FILL, dtype=torch.float64, device=dev))
    d = _records(_capi.SQMC_PROBLEM_DTYPE, B, t)
    d["prior_mean"], d["prior_var"], d["T"], d["N"] = sq.PM, sq.PV, T, N
    if edit is not None:
        edit(d)
    desc = _upload(d)
    ctr = torch.full((1,), int(step), dtype=torch.int64, device=dev)
    seed = sq.filter_seed(sq.SEED)
    if lam is None:
        _ctx().sqmc_device(model, "f64", n_max, B, desc.data_ptr(), seed, off, ctr.data_ptr(), 0, traced=traced)
    else:
        _ctx().sqmc_score_device(model, "f64", n_max, B, desc.data_ptr(), lam, seed, off, ctr.data_ptr(), 0, traced=traced)
    torch.cuda.synchronize()
    assert int(ctr.item()) == int(step)
    return {k: v.cpu().numpy() for k, v in t.items() if k not in ("theta", "y")}


def current_u(U, rho):
    """rho = 0 reads no buffer: the current one is handed over full of NaN."""
    return np.full(U.shape, np.nan) if rho == 0 else U


@functools.lru_cache(maxsize=None)
def cpm_case(model, N, T, B, rho, lam):
    th, y, U = cp.case_inputs(model, N, T, B)
    U = current_u(U, rho)
    return th, y, U, launch_cpm(model, th, y, U, N, rho, lam)


@functools.lru_cache(maxsize=None)
def sqmc_case(model, N, T, B, n_max, lam):
    th, y, _ = sq.case_theta_y(model, N, T, B)
    return th, y, launch_sqmc(model, th, y, N, n_max, lam)


def check_score(model, got_out, ref, lam):
    """out[0..H-1] against the long-double replay to TOL of the terms' magnitude; slots H .. 3 and 5 .. 7 are 0."""
    h = H[model]
    want, mag = ref["score"].astype(np.float64), ref["mag"].astype(np.float64)
    err = np.abs(got_out[:, :h] - want) / mag
    print("score", model, "lambduh", lam, "max |d| / mag", float(err.max()), "mag", float(mag.min()), "..", float(mag.max()))
    assert np.all(np.isfinite(got_out[:, :h])) and np.all(mag > 0)
    assert np.all(err <= TOL), float(err.max())
    assert np.all(got_out[:, h:4] == 0.0) and np.all(got_out[:, 5:] == 0.0)


# ---- 1. the correlated filter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B,rho", cp.CASES)
def test_cpm_score_is_the_same_filter_and_replays_on_the_host(model, N, T, B, rho, lam):
    """out[4], U', trace_anc and trace_ll of the score launch are bitwise pfg_cpm_device's on the same inputs; the production twin
    of the score launch writes the same record and U' and leaves the trace alone; teacher-forced on the recorded parents, the
    long-double restatement reproduces out[0..H-1] to 1e-9 of the terms' magnitude.  lambduh = 1 is compared with the plain
    recursion, which reads no S."""
    th, y, U, got = cpm_case(model, N, T, B, rho, lam)
    _, _, _, base = cpm_case(model, N, T, B, rho, None)
    for k in ("U_prop", "U_cur", "trace_anc", "trace_ll"):
        assert np.array_equal(got[k], base[k], equal_nan=True), k
    assert np.array_equal(got["out"][:, 4], base["out"][:, 4])
    prod = launch_cpm(model, th, y, U, N, rho, lam, traced=False)
    assert np.array_equal(prod["out"], got["out"]) and np.array_equal(prod["U_prop"], got["U_prop"])
    assert np.all(prod["trace_anc"] == ANC_FILL) and np.all(prod["trace_ll"] == LL_FILL)
    ref = ss.cpm_score(model, th, y, got["U_prop"], cp.PM, cp.PV, lam=lam, F=LD, forced=got["trace_anc"].astype(np.int64))
    assert not ref["degenerate"].any()
    np.testing.assert_allclose(got["out"][:, 4], ref["ll"].astype(np.float64), rtol=TOL, atol=TOL)
    check_score(model, got["out"], ref, lam)


# ---- 2. the sequential quasi-Monte Carlo filter -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B,n_max", sq.CASES + [(8, 24, 70, 8), (512, 7, 3, 1024), (1024, 1, 2, 1024)])
def test_sqmc_score_is_the_same_filter_and_replays_on_the_host(model, N, T, B, n_max, lam):
    """As above for pfg_sqmc_score_device: out[4] and the three trace arrays bitwise pfg_sqmc_device's, production against traced,
    and the replay on the recorded parents and normals."""
    th, y, got = sqmc_case(model, N, T, B, n_max, lam)
    _, _, base = sqmc_case(model, N, T, B, n_max, None)
    for k in ("trace_anc", "trace_ll", "trace_z"):
        assert np.array_equal(got[k], base[k]), k
    assert np.array_equal(got["out"][:, 4], base["out"][:, 4])
    prod = launch_sqmc(model, th, y, N, n_max, lam, traced=False)
    assert np.array_equal(prod["out"], got["out"])
    assert np.all(prod["trace_anc"] == ANC_FILL) and np.all(prod["trace_ll"] == LL_FILL) and np.all(prod["trace_z"] == Z_FILL)
    ref = ss.sqmc_score(model, th, y, N, sq.PM, sq.PV, sq.filter_seed(sq.SEED), kd.chain_ids(B, OFF), STEP, lam=lam, F=LD,
                        forced=got["trace_anc"].astype(np.int64), z=got["trace_z"])
    assert not ref["degenerate"].any()
    np.testing.assert_allclose(got["out"][:, 4], ref["ll"].astype(np.float64), rtol=TOL, atol=TOL)
    check_score(model, got["out"], ref, lam)


# ---- 3. the global id alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("N", [100, 200])
def test_cpm_score_depends_on_the_global_id_alone(N, lam):
    """The buffers swapped, and chains 3 .. 5 launched on their own with chain_offset + 3: the same record and U', bit for bit;
    another counter gives another one."""
    T, B, rho = 7, 6, 0.5
    th, y, U = cp.case_inputs("lgssm", N, T, B)
    a = launch_cpm("lgssm", th, y, U, N, rho, lam, traced=False)
    b = launch_cpm("lgssm", th, y, U, N, rho, lam, traced=False, which=1 - (np.arange(B) & 1))
    c = launch_cpm("lgssm", th[3:], y, U[3:], N, rho, lam, off=OFF + 3, traced=False)
    for k in ("out", "U_prop"):
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k][3:], c[k])
    d = launch_cpm("lgssm", th, y, U, N, rho, lam, step=STEP + 1, traced=False)
    assert not np.array_equal(a["out"][:, :4], d["out"][:, :4])


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("N,n_max", [(64, 64), (256, 256)])
def test_sqmc_score_depends_on_the_global_id_alone(N, n_max, lam):
    T, B = 6, 6
    th, y, _ = sq.case_theta_y("svm", N, T, B)
    a = launch_sqmc("svm", th, y, N, n_max, lam, traced=False)
    c = launch_sqmc("svm", th[3:], y, N, n_max, lam, off=OFF + 3, traced=False)
    np.testing.assert_array_equal(a["out"][3:], c["out"])
    d = launch_sqmc("svm", th, y, N, n_max, lam, step=STEP + 1, traced=False)
    assert not np.array_equal(a["out"][:, :3], d["out"][:, :3])


# ---- 4. degenerate chains and refused descriptors ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("N", [4, 256])
def test_degenerate_chain(N, lam):
    """SVM, one chain of the batch fed y = +-1e300: out[4] is not finite and every other slot is 0 -- the score columns too -- under
    both filters; U' is still written in full and finite; the neighbours are what they are without it."""
    T, B, rho = 6, 3, 0.5
    th, y, U = cp.case_inputs("svm", N, T, B)
    ys = np.tile(y, (B, 1))
    ys[1] = 1e300 * (-1.0) ** np.arange(T)
    for run in (lambda yy: launch_cpm("svm", th, yy, U, N, rho, lam), lambda yy: launch_sqmc("svm", th, yy, N, N, lam)):
        got, base = run(ys), run(np.tile(y, (B, 1)))
        assert not np.abs(got["out"][1, 4]) < np.inf and np.all(got["out"][1, [0, 1, 2, 3, 5, 6, 7]] == 0.0)
        for b in (0, 2):
            assert np.array_equal(got["out"][b], base["out"][b])
        assert np.all(np.isfinite(base["out"])) and np.all(base["out"][:, :3] != 0.0)
        if "U_prop" in got:
            assert np.all(np.isfinite(got["U_prop"])) and np.array_equal(got["U_prop"], base["U_prop"])


def test_refused_descriptors_get_a_nan_record_and_no_other_store():
    """T = 0, N = 1, N above the launch's shape, a prior variance of 0, a NULL array (CPM: a NULL buffer or selector; SQMC: N not
    a power of two) each give a NaN record; neither a buffer nor a trace array of theirs is written; the last, sound chain of the
    batch gets its record."""
    N, T, lam = 8, 4, 0.95
    th, y, U = cp.case_inputs("svm", N, T, 1)
    bad = [dict(T=0), dict(N=1), dict(N=200), dict(prior_var=0.0), dict(prior_var=-1.0), dict(y=0)]
    for extra, run in (([dict(u1=0), dict(which=0)], "cpm"), ([dict(N=6)], "sqmc")):
        cases = bad + extra
        B = len(cases) + 1

        def edit(d):
            for b, kw in enumerate(cases):
                for k, v in kw.items():
                    d[k][b] = v
        thB, UB = np.tile(th, (B, 1)), np.tile(U, (B, 1, 1))
        if run == "cpm":
            got = launch_cpm("svm", thB, y, UB, N, 0.5, lam, n_max=128, edit=edit, which=np.zeros(B))
            assert np.all(got["U_prop"][:-1] == 0.0) and not np.all(got["U_prop"][-1] == 0.0)
        else:
            got = launch_sqmc("svm", thB, y, N, 128, lam, edit=edit)
            assert np.all(got["trace_z"][:-1] == Z_FILL)
        out = got["out"]
        assert np.all(np.isnan(out[:-1])) and np.all(np.isfinite(out[-1])) and np.all(out[-1, :3] != 0.0) and out[-1, 4] != 0.0
        assert np.all(got["trace_anc"][:-1] == ANC_FILL) and np.all(got["trace_ll"][:-1] == LL_FILL)


def test_entry_point_refusals():
    from sgmcmc_ssm_amd import _capi
    import torch
    buf = torch.zeros(_capi.CPM_PROBLEM_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    ctx = _ctx()
    for call in (lambda *a, lam=0.95, **k: ctx.cpm_score_device(*a, 0.5, lam, 1, **k),
                 lambda *a, lam=0.95, **k: ctx.sqmc_score_device(*a, lam, 1, **k)):
        with pytest.raises(NotImplementedError, match="SVM and LGSSM"):
            call("garch", "f64", 8, 1, buf.data_ptr())
        with pytest.raises(NotImplementedError, match="f64 only"):
            call("svm", "f32", 8, 1, buf.data_ptr())
        for n in (1, 1025):
            with pytest.raises(NotImplementedError, match="2 <= N <= 1024"):
                call("svm", "f64", n, 1, buf.data_ptr())
        with pytest.raises(ValueError, match="NULL"):
            call("svm", "f64", 8, 1, 0)
        with pytest.raises(ValueError, match="B must be >= 0"):
            call("svm", "f64", 8, -1, buf.data_ptr())
        with pytest.raises(ValueError, match="Unrecognized model"):
            call(7, "f64", 8, 1, buf.data_ptr())
        for lam in (0.0, 1.5, float("nan")):
            with pytest.raises(ValueError, match=r"lambduh must lie in \(0, 1\]"):
                call("svm", "f64", 8, 1, buf.data_ptr(), lam=lam)
        call("svm", "f64", 8, 0, buf.data_ptr())            # no chains: not an error
        call("svm", "f64", 8, 1, buf.data_ptr())            # a zeroed record: refused by the kernel without a store
    for rho in (1.0, -0.01, float("nan")):
        with pytest.raises(ValueError, match=r"rho must lie in \[0, 1\)"):
            ctx.cpm_score_device("svm", "f64", 8, 1, buf.data_ptr(), rho, 0.95, 1)
    torch.cuda.synchronize()
