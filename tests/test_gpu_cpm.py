"""GPU: the sorted, correlated filter of correlated pseudo-marginal PMMH (pfg_cpm_device, csrc/pfg_cpm.hip) against its NumPy
restatement (tests/helpers/cpm_model.py): the proposal of the normals entry by entry, the traced twin replayed in long double,
structural properties of what it records, production against traced, the degenerate chain, refused descriptors, the commit
kernel and the entry points' refusals."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cpm_model as cp  # noqa: E402
import keyed_draws as kd  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
OFF, STEP = 2 ** 32 - 3, 5          # the chain ids straddle 2^32: the high word takes part in the key
TOL_LL = 1e-9


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def launch(model, theta, y, U, N, rho, seed, off, step, traced=True, pm=cp.PM, pv=cp.PV, which=None):
    """One launch of pfg_cpm_device on B chains whose current normals are U [B, T+1, N+1]; chain b keeps them in buffer
    which[b] (default b & 1: both selector values in every batch).  Returns what the launch left: U_prop (the other buffer),
    U_cur (the current one afterwards), out, trace_anc, trace_ll."""
    import torch
    from sgmcmc_ssm_amd import _capi
    dev = torch.device("cuda", 0)
    B, P = theta.shape
    y = np.array(np.broadcast_to(y, (B, y.shape[-1])), dtype=np.float64, order="C")      # a writable row-major copy
    T = y.shape[1]
    th = np.zeros((B, _capi.MAX_THETA))
    th[:, :P] = theta
    sb = _capi.cpm_aux_bytes(T, N)
    n = (T + 1) * (N + 1)
    assert sb >= 8 * n and sb % 256 == 0
    which = (np.arange(B) & 1 if which is None else np.asarray(which)).astype(np.int32)
    bufs = np.zeros((2, B, sb // 8))
    bufs[which, np.arange(B), :n] = np.asarray(U, dtype=np.float64).reshape(B, n)
    bufs[:, :, n:] = 7.0                # the padding of a slab: never touched
    aux = torch.from_numpy(bufs).to(dev)
    t = dict(theta=torch.from_numpy(th).to(dev), y=torch.from_numpy(y).to(dev), which=torch.from_numpy(which).to(dev),
             out=torch.full((B, _capi.OUT_DOUBLES), 3.0, dtype=torch.float64, device=dev),
             trace_anc=torch.full((B, T, N), -1, dtype=torch.int32, device=dev),
             trace_ll=torch.full((B, T), -7.0, dtype=torch.float64, device=dev))
    d = np.zeros(B, dtype=_capi.CPM_PROBLEM_DTYPE)
    for name, ten in t.items():
        d[name] = ten.data_ptr() + np.arange(B, dtype=np.uint64) * np.uint64(ten.numel() // B * ten.element_size())
    d["u0"] = aux.data_ptr() + np.arange(B, dtype=np.uint64) * np.uint64(sb)
    d["u1"] = aux.data_ptr() + (np.arange(B, dtype=np.uint64) + np.uint64(B)) * np.uint64(sb)
    d["prior_mean"], d["prior_var"], d["T"], d["N"] = pm, pv, T, N
    desc = torch.from_numpy(d.view(np.uint8).reshape(B, -1)).to(dev)
    ctr = torch.full((1,), int(step), dtype=torch.int64, device=dev)
    _ctx().cpm_device(model, "f64", N, B, desc.data_ptr(), rho, seed, off, ctr.data_ptr(), 0, traced=traced)
    torch.cuda.synchronize()
    after = aux.cpu().numpy()
    assert np.all(after[:, :, n:] == 7.0) and int(ctr.item()) == int(step)
    rows = np.arange(B)
    res = {k: v.cpu().numpy() for k, v in t.items() if k in ("out", "trace_anc", "trace_ll")}
    res["U_prop"] = after[1 - which, rows, :n].reshape(B, T + 1, N + 1)
    res["U_cur"] = after[which, rows, :n].reshape(B, T + 1, N + 1)
    return res


def current_u(U, rho):
    """rho = 0 reads no buffer: the current one is handed over full of NaN."""
    return np.full(U.shape, np.nan) if rho == 0 else U


@functools.lru_cache(maxsize=None)
def traced_case(model, N, T, B, rho):
    th, y, U = cp.case_inputs(model, N, T, B)
    U = current_u(U, rho)
    got = launch(model, th, y, U, N, rho, cp.filter_seed(cp.SEED), OFF, STEP)
    return th, y, U, got


# ---- 1. the proposal of the normals -------------------------------------------------------------------------------------------
U_MATCH = {}        # (model, N, T, B, rho) -> "bitwise" | "1e-15": printed by the test below, quoted in DESIGN section 7


@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B,rho", cp.CASES)
def test_proposed_normals_match_the_keyed_draws(model, N, T, B, rho):
    """Every entry of U' [B, T+1, N+1] -- column N of rows 0 and 1 included -- against rho * U + sqrt(1 - rho * rho) * eps with
    eps regenerated from its key.  The model takes eps in long double and rounds it once; the device's normal_pair is the exact
    one in double (ocml log, sqrt, sincospi and two products, a handful of roundings), so the two agree bitwise or to 1e-15
    times the larger of 1 and the magnitude of the sum's terms (4.5 ulps of them).  Which of the two it was is printed per
    shape.  The current buffer is left as it was, and rho = 0 read none of it (it held NaN)."""
    th, y, U, got = traced_case(model, N, T, B, rho)
    want, e = cp.propose_u(U, rho, T, N, cp.filter_seed(cp.SEED), kd.chain_ids(B, OFF), STEP)
    assert np.all(np.isfinite(got["U_prop"]))
    np.testing.assert_array_equal(got["U_cur"], U)
    bitwise = np.array_equal(got["U_prop"], want)
    terms = np.abs(np.sqrt(1 - rho * rho) * e.astype(np.float64)) + (np.abs(rho * U) if rho else 0.0)
    err = np.abs(got["U_prop"] - want)
    U_MATCH[(model, N, T, B, rho)] = "bitwise" if bitwise else "1e-15"
    print("U'", model, (N, T, B, rho), U_MATCH[(model, N, T, B, rho)], "max abs", float(err.max()), "entries off",
          int((err > 0).sum()), "of", err.size)
    assert np.all(err <= 1e-15 * np.maximum(1.0, terms)), float((err / np.maximum(1.0, terms)).max())


# ---- 2. replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B,rho", cp.CASES)
def test_traced_filter_replays_on_the_host(model, N, T, B, rho):
    """On the U' the device wrote, every recorded parent is the one the long-double model's search selects (a search whose
    target lies within 1e-12 of a CDF entry is left out: at most 1 index in 10^4); teacher-forced on the parents, the per-step
    increments and out[4] agree to 1e-9; every other slot of the record is 0; the production instantiation writes the same
    out[4] and U', bit for bit, and leaves the trace buffers alone."""
    th, y, U, got = traced_case(model, N, T, B, rho)
    anc = got["trace_anc"].astype(np.int64)
    ref = cp.loglik(model, th, y, got["U_prop"], cp.PM, cp.PV, F=LD, forced=anc)
    assert not ref["degenerate"].any()
    wrong, left_out, n = cp.index_mismatches(anc, ref)
    print("indices", n, "left out", left_out, "wrong", wrong)
    assert wrong == 0 and left_out * 10000 <= n, (wrong, left_out, n)
    np.testing.assert_allclose(got["trace_ll"], ref["inc"].astype(np.float64), rtol=TOL_LL, atol=TOL_LL)
    np.testing.assert_allclose(got["out"][:, 4], ref["ll"].astype(np.float64), rtol=TOL_LL, atol=TOL_LL)
    assert np.all(got["out"][:, [0, 1, 2, 3, 5, 6, 7]] == 0.0)
    prod = launch(model, th, y, U, N, rho, cp.filter_seed(cp.SEED), OFF, STEP, traced=False)
    assert np.array_equal(prod["out"], got["out"]) and np.array_equal(prod["U_prop"], got["U_prop"])
    assert np.all(prod["trace_anc"] == -1) and np.all(prod["trace_ll"] == -7.0)


@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B,rho", cp.CASES)
def test_recorded_parents(model, N, T, B, rho):
    """Parents are sorted positions in [0, N), non-decreasing in the child's index -- systematic resampling on the CDF of the
    sorted particles -- and row 0 is not written."""
    _, _, _, got = traced_case(model, N, T, B, rho)
    anc = got["trace_anc"]
    assert np.all(anc[:, 0] == -1) and np.all((anc[:, 1:] >= 0) & (anc[:, 1:] < N))
    assert np.all(np.diff(anc[:, 1:].astype(np.int64), axis=2) >= 0)


def test_selector_and_batch_do_not_matter():
    """A chain's result depends on its global id alone: the same chains with the buffers swapped, and chains 3 .. 5 of the batch
    launched on their own with chain_offset + 3, give the same out[4] and U', bit for bit."""
    N, T, B, rho = 100, 7, 6, 0.5
    th, y, U = cp.case_inputs("svm", N, T, B)
    seed = cp.filter_seed(cp.SEED)
    a = launch("svm", th, y, U, N, rho, seed, OFF, STEP, traced=False)
    b = launch("svm", th, y, U, N, rho, seed, OFF, STEP, traced=False, which=1 - (np.arange(B) & 1))
    c = launch("svm", th[3:], y, U[3:], N, rho, seed, OFF + 3, STEP, traced=False)
    for k in ("out", "U_prop"):
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k][3:], c[k])
    d = launch("svm", th, y, U, N, rho, seed, OFF, STEP + 1, traced=False)
    assert not np.array_equal(a["U_prop"], d["U_prop"])


# ---- 3. degenerate chains and refused descriptors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 257])
def test_degenerate_chain_is_rejected_and_its_normals_stay_finite(N):
    """SVM, one chain of the batch fed y = +-1e300: its weight sum is zero, out[4] is a value pfg_pmmh_accept_device rejects (not
    finite), every other slot 0, and U' is written in full and is the proposal the model forms -- no NaN enters U; its
    neighbours are what they are without it."""
    T, B, rho = 6, 3, 0.5
    th, y, U = cp.case_inputs("svm", N, T, B)
    ys = np.tile(y, (B, 1))
    ys[1] = 1e300 * (-1.0) ** np.arange(T)
    seed = cp.filter_seed(cp.SEED)
    got = launch("svm", th, ys, U, N, rho, seed, OFF, STEP)
    assert not np.abs(got["out"][1, 4]) < np.inf and np.all(got["out"][1, [0, 1, 2, 3, 5, 6, 7]] == 0.0)
    assert np.all(np.isfinite(got["U_prop"]))
    want, _ = cp.propose_u(U, rho, T, N, seed, kd.chain_ids(B, OFF), STEP)
    np.testing.assert_allclose(got["U_prop"], want, rtol=0, atol=1e-14)
    base = launch("svm", th, np.tile(y, (B, 1)), U, N, rho, seed, OFF, STEP)
    for b in (0, 2):
        assert np.array_equal(got["out"][b], base["out"][b]) and np.array_equal(got["U_prop"][b], base["U_prop"][b])
    assert np.all(np.isfinite(base["out"]))


def test_refused_descriptors_get_a_nan_record_and_no_other_store():
    """A zeroed record (every array NULL, T = 0) is refused by the kernel without a store.  With arrays in place: T = 0, N = 1,
    N above the launch's shape, a prior variance of 0 and a NULL buffer each give a NaN record, and neither buffer nor the trace is
    written."""
    import torch
    from sgmcmc_ssm_amd import _capi
    dev = torch.device("cuda", 0)
    ctx = _ctx()
    buf = torch.zeros(_capi.CPM_PROBLEM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ctx.cpm_device("svm", "f64", 8, 1, buf.data_ptr(), 0.5, 1)
    torch.cuda.synchronize()
    N, T = 8, 4
    sb = _capi.cpm_aux_bytes(T, N)
    bad = [dict(T=0), dict(N=1), dict(N=200), dict(prior_var=0.0), dict(prior_var=-1.0), dict(u1=0), dict(which=0), dict(y=0)]
    B = len(bad) + 1
    aux = torch.full((2, B, sb // 8), 5.0, dtype=torch.float64, device=dev)
    t = dict(theta=torch.ones((B, _capi.MAX_THETA), dtype=torch.float64, device=dev),
             y=torch.zeros((B, T), dtype=torch.float64, device=dev), which=torch.zeros(B, dtype=torch.int32, device=dev),
             out=torch.full((B, _capi.OUT_DOUBLES), 3.0, dtype=torch.float64, device=dev),
             trace_anc=torch.full((B, T, N), -1, dtype=torch.int32, device=dev),
             trace_ll=torch.full((B, T), -7.0, dtype=torch.float64, device=dev))
    d = np.zeros(B, dtype=_capi.CPM_PROBLEM_DTYPE)
    idx = np.arange(B, dtype=np.uint64)
    for name, ten in t.items():
        d[name] = ten.data_ptr() + idx * np.uint64(ten.numel() // B * ten.element_size())
    d["u0"] = aux.data_ptr() + idx * np.uint64(sb)
    d["u1"] = aux.data_ptr() + (idx + np.uint64(B)) * np.uint64(sb)
    d["prior_mean"], d["prior_var"], d["T"], d["N"] = 0.0, 10.0, T, N
    for b, kw in enumerate(bad):
        for k, v in kw.items():
            d[k][b] = v
    desc = torch.from_numpy(d.view(np.uint8).reshape(B, -1)).to(dev)
    ctx.cpm_device("svm", "f64", 128, B, desc.data_ptr(), 0.5, 1, traced=True)
    torch.cuda.synchronize()
    out, a = t["out"].cpu().numpy(), aux.cpu().numpy()
    assert np.all(np.isnan(out[:-1])) and np.all(np.isfinite(out[-1])) and out[-1, 4] != 0.0
    assert np.all(a[:, :-1] == 5.0) and np.all(a[0, -1] == 5.0) and not np.all(a[1, -1] == 5.0)
    assert np.all(t["trace_anc"].cpu().numpy()[:-1] == -1) and np.all(t["trace_ll"].cpu().numpy()[:-1] == -7.0)


# ---- 4. the commit kernel and the entry points -----------------------------------------------------------------------------------
def test_commit_flips_the_chains_that_accepted():
    import torch
    dev = torch.device("cuda", 0)
    B = 300
    rs = np.random.RandomState(3)
    n_acc = rs.randint(0, 5, size=B).astype(np.int64)
    seen = n_acc - (rs.uniform(size=B) < 0.4)
    which = rs.randint(0, 2, size=B).astype(np.int32)
    for init in (False, True):
        tn, ts, tw = (torch.from_numpy(v.copy()).to(dev) for v in (n_acc, seen, which))
        _ctx().cpm_commit_device(B, tn.data_ptr(), ts.data_ptr(), tw.data_ptr(), init)
        torch.cuda.synchronize()
        moved = np.ones(B, bool) if init else n_acc != seen
        assert 0 < (n_acc != seen).sum() < B
        np.testing.assert_array_equal(tw.cpu().numpy(), which ^ moved.astype(np.int32))
        np.testing.assert_array_equal(ts.cpu().numpy(), n_acc)
        np.testing.assert_array_equal(tn.cpu().numpy(), n_acc)


def test_entry_point_refusals():
    from sgmcmc_ssm_amd import _capi
    import torch
    buf = torch.zeros(_capi.CPM_PROBLEM_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    ctx = _ctx()
    with pytest.raises(NotImplementedError, match="SVM and LGSSM"):
        ctx.cpm_device("garch", "f64", 8, 1, buf.data_ptr(), 0.5, 1)
    with pytest.raises(NotImplementedError, match="f64 only"):
        ctx.cpm_device("svm", "f32", 8, 1, buf.data_ptr(), 0.5, 1)
    for n in (1, 1025):
        with pytest.raises(NotImplementedError, match="2 <= N <= 1024"):
            ctx.cpm_device("svm", "f64", n, 1, buf.data_ptr(), 0.5, 1)
    with pytest.raises(ValueError, match="NULL"):
        ctx.cpm_device("svm", "f64", 8, 1, 0, 0.5, 1)
    with pytest.raises(ValueError, match="B must be >= 0"):
        ctx.cpm_device("svm", "f64", 8, -1, buf.data_ptr(), 0.5, 1)
    with pytest.raises(ValueError, match="Unrecognized model"):
        ctx.cpm_device(7, "f64", 8, 1, buf.data_ptr(), 0.5, 1)
    for rho in (1.0, -0.01, float("nan"), 1.5):
        with pytest.raises(ValueError, match=r"rho must lie in \[0, 1\)"):
            ctx.cpm_device("svm", "f64", 8, 1, buf.data_ptr(), rho, 1)
    with pytest.raises(ValueError, match="NULL"):
        ctx.cpm_commit_device(1, 0, buf.data_ptr(), buf.data_ptr(), False)
    with pytest.raises(ValueError, match="B must be >= 0"):
        ctx.cpm_commit_device(-1, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), False)
    ctx.cpm_device("svm", "f64", 8, 0, buf.data_ptr(), 0.5, 1)          # no chains: not an error
    ctx.cpm_commit_device(0, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), False)
    torch.cuda.synchronize()
