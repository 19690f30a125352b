"""GPU: the sequential quasi-Monte Carlo filter (pfg_sqmc_device, csrc/pfg_sqmc.hip) against its NumPy restatement
(tests/helpers/sqmc_model.py) -- the normals against Phi^-1 of the regenerated points, the traced twin replayed in long double,
production against traced, batch and counter, the degenerate chain, refused descriptors, the entry point's refusals -- and
ChainEnsemble(sampler='pmmh', sqmc=True): a whole step against the restatement, eager against hipGraph against resume, and the
exactness of the chain against Metropolis-Hastings on the Kalman likelihood."""
import functools
import os
import sys

import numpy as np
import pytest
from scipy.special import ndtri

from test_host_logic import GEN, PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import keyed_draws as kd  # noqa: E402
import pmmh_model as pm  # noqa: E402
import sqmc_model as sq  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
OFF, STEP = 2 ** 32 - 3, 5          # the chain ids straddle 2^32: the high word takes part in the key
TOL_LL = 1e-9                       # tests/test_gpu_cpm.py's
TOL_Z = 1e-13                       # |z - ndtri(v)| <= TOL_Z max(1, |z|): far below what moves a parent off an edge
ANC_FILL, LL_FILL, Z_FILL = -2, -7.0, 9.0


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def launch(model, theta, y, N, n_max, seed, off, step, traced=True, pm_=sq.PM, pv=sq.PV, edit=None):
    """One launch of pfg_sqmc_device on B chains.  Returns what it left: out, trace_anc, trace_ll, trace_z.  edit(d): changes
    the descriptors before the upload."""
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
    d = np.zeros(B, dtype=_capi.SQMC_PROBLEM_DTYPE)
    for name, ten in t.items():
        d[name] = ten.data_ptr() + np.arange(B, dtype=np.uint64) * np.uint64(ten.numel() // B * ten.element_size())
    d["prior_mean"], d["prior_var"], d["T"], d["N"] = pm_, pv, T, N
    if edit is not None:
        edit(d)
    desc = torch.from_numpy(d.view(np.uint8).reshape(B, -1)).to(dev)
    ctr = torch.full((1,), int(step), dtype=torch.int64, device=dev)
    _ctx().sqmc_device(model, "f64", n_max, B, desc.data_ptr(), seed, off, ctr.data_ptr(), 0, traced=traced)
    torch.cuda.synchronize()
    assert int(ctr.item()) == int(step)             # read, not incremented
    return {k: v.cpu().numpy() for k, v in t.items() if k not in ("theta", "y")}


@functools.lru_cache(maxsize=None)
def traced_case(model, N, T, B, n_max):
    th, y, _ = sq.case_theta_y(model, N, T, B)
    return th, y, launch(model, th, y, N, n_max, sq.filter_seed(sq.SEED), OFF, STEP)


# ---- 1. the normals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B,n_max", sq.CASES)
def test_normals_are_the_inverse_cdf_of_the_points(model, N, T, B, n_max):
    """Every recorded z -- row 0 by particle, rows 1 .. T by child -- against scipy's ndtri of v regenerated from the key, the
    points and the rank formula: |z - ndtri(v)| <= 1e-13 max(1, |z|).  The measured maximum is printed."""
    _, _, got = traced_case(model, N, T, B, n_max)
    want, v, _ = sq.normals(N, T, sq.filter_seed(sq.SEED), kd.chain_ids(B, OFF), STEP)
    assert np.all((v > 0) & (v < 1)) and np.all(np.isfinite(got["trace_z"]))
    err = np.abs(got["trace_z"] - want) / np.maximum(1.0, np.abs(want))
    print("z", model, (N, T, B, n_max), "max |dz| / max(1, |z|)", float(err.max()), "bitwise", int((err == 0).sum()), "of", err.size)
    assert np.all(err <= TOL_Z), float(err.max())
    assert np.array_equal(ndtri(v), want)


# ---- 2. replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("N,T,B,n_max", sq.CASES)
def test_traced_filter_replays_on_the_host(model, N, T, B, n_max):
    """On the z the device recorded, every recorded parent is the one the long-double model's search selects (a search whose
    target lies within 1e-12 of a CDF entry is left out: at most 1 index in 10^4); teacher-forced on the parents, the per-step
    increments and out[4] agree to 1e-9; every other slot of the record is 0; parents are sorted positions that do not decrease
    in the child's index, row 0 is -1; the production instantiation writes the same record, bit for bit, and leaves the trace
    buffers alone."""
    th, y, got = traced_case(model, N, T, B, n_max)
    anc = got["trace_anc"].astype(np.int64)
    assert np.all(anc[:, 0] == -1) and np.all((anc[:, 1:] >= 0) & (anc[:, 1:] < N)) and np.all(np.diff(anc[:, 1:], axis=2) >= 0)
    ref = sq.loglik(model, th, y, N, sq.PM, sq.PV, sq.filter_seed(sq.SEED), kd.chain_ids(B, OFF), STEP, F=LD, forced=anc,
                    z=got["trace_z"])
    assert not ref["degenerate"].any()
    wrong, left_out, n = sq.index_mismatches(anc, ref)
    print("indices", n, "left out", left_out, "wrong", wrong)
    assert wrong == 0 and left_out * 10000 <= n, (wrong, left_out, n)
    np.testing.assert_allclose(got["trace_ll"], ref["inc"].astype(np.float64), rtol=TOL_LL, atol=TOL_LL)
    np.testing.assert_allclose(got["out"][:, 4], ref["ll"].astype(np.float64), rtol=TOL_LL, atol=TOL_LL)
    assert np.all(got["out"][:, [0, 1, 2, 3, 5, 6, 7]] == 0.0)
    prod = launch(model, th, y, N, n_max, sq.filter_seed(sq.SEED), OFF, STEP, traced=False)
    assert np.array_equal(prod["out"], got["out"])
    assert np.all(prod["trace_anc"] == ANC_FILL) and np.all(prod["trace_ll"] == LL_FILL) and np.all(prod["trace_z"] == Z_FILL)


def test_launch_shape_does_not_matter():
    """N = 64 in one wave and in the 256 x 4 shape: the same normals and parents; the sums run in another order, so the
    estimates agree to 1e-12, not bitwise."""
    for model in ("svm", "lgssm"):
        a, b = traced_case(model, 64, 12, 5, 64)[2], traced_case(model, 64, 12, 5, 256)[2]
        assert np.array_equal(a["trace_z"], b["trace_z"]) and np.array_equal(a["trace_anc"], b["trace_anc"])
        np.testing.assert_allclose(a["out"], b["out"], rtol=1e-12, atol=1e-12)


# ---- 3. batch and counter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,n_max", [(64, 64), (256, 256)])
def test_batch_and_position_do_not_matter(N, n_max):
    """A chain's record depends on its global id alone: chains 3 .. 5 of the batch launched on their own with chain_offset + 3
    give the same record, bit for bit; another counter gives another one."""
    T, B = 6, 6
    th, y, _ = sq.case_theta_y("svm", N, T, B)
    seed = sq.filter_seed(sq.SEED)
    a = launch("svm", th, y, N, n_max, seed, OFF, STEP, traced=False)
    c = launch("svm", th[3:], y, N, n_max, seed, OFF + 3, STEP, traced=False)
    np.testing.assert_array_equal(a["out"][3:], c["out"])
    d = launch("svm", th, y, N, n_max, seed, OFF, STEP + 1, traced=False)
    assert np.all(a["out"][:, 4] != d["out"][:, 4])


# ---- 4. degenerate chains, refused descriptors, the entry point ------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 256])
def test_degenerate_chain_gives_minus_infinity(N):
    """SVM, one chain of the batch fed y = +-1e300: its weight sum is not finite, out[4] = -inf, every other slot 0; its
    neighbours are what they are without it."""
    T, B = 6, 3
    th, y, _ = sq.case_theta_y("svm", N, T, B)
    ys = np.tile(y, (B, 1))
    ys[1] = 1e300 * (-1.0) ** np.arange(T)
    seed = sq.filter_seed(sq.SEED)
    got = launch("svm", th, ys, N, N, seed, OFF, STEP)
    assert got["out"][1, 4] == -np.inf and np.all(got["out"][1, [0, 1, 2, 3, 5, 6, 7]] == 0.0)
    base = launch("svm", th, np.tile(y, (B, 1)), N, N, seed, OFF, STEP)
    assert np.all(np.isfinite(base["out"]))
    for b in (0, 2):
        assert np.array_equal(got["out"][b], base["out"][b])


def test_refused_descriptors_get_a_nan_record_and_no_other_store():
    """A zeroed record (every array NULL, T = 0) is refused by the kernel without a store.  With arrays in place: T = 0, N = 1,
    N above the launch's shape, N not a power of two, a prior variance of 0 or below and a NULL series each give a NaN record,
    and the trace is not written; the last chain of the batch is in order."""
    import torch
    from sgmcmc_ssm_amd import _capi
    buf = torch.zeros(_capi.SQMC_PROBLEM_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    _ctx().sqmc_device("svm", "f64", 8, 1, buf.data_ptr(), 1)
    torch.cuda.synchronize()
    bad = [dict(T=0), dict(N=1), dict(N=256), dict(N=6), dict(N=12), dict(prior_var=0.0), dict(prior_var=-1.0), dict(y=0),
           dict(theta=0)]
    B, N, T = len(bad) + 1, 8, 4

    def edit(d):
        for b, kw in enumerate(bad):
            for k, v in kw.items():
                d[k][b] = v

    got = launch("svm", np.ones((B, 3)), np.zeros(T), N, 128, 1, 0, 0, edit=edit)
    assert np.all(np.isnan(got["out"][:-1])) and np.all(np.isfinite(got["out"][-1])) and got["out"][-1, 4] != 0.0
    assert np.all(got["trace_anc"][:-1] == ANC_FILL) and np.all(got["trace_ll"][:-1] == LL_FILL)
    assert np.all(got["trace_z"][:-1] == Z_FILL) and not np.any(got["trace_z"][-1] == Z_FILL)


def test_entry_point_refusals():
    from sgmcmc_ssm_amd import _capi
    import torch
    buf = torch.zeros(_capi.SQMC_PROBLEM_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    ctx = _ctx()
    with pytest.raises(NotImplementedError, match="SVM and LGSSM"):         # (the binding maps UNSUPPORTED / INVALID to these)
        ctx.sqmc_device("garch", "f64", 8, 1, buf.data_ptr(), 1)
    with pytest.raises(NotImplementedError, match="f64 only"):
        ctx.sqmc_device("svm", "f32", 8, 1, buf.data_ptr(), 1)
    for n in (1, 1025):
        with pytest.raises(NotImplementedError, match="2 <= N <= 1024"):
            ctx.sqmc_device("svm", "f64", n, 1, buf.data_ptr(), 1)
    with pytest.raises(ValueError, match="NULL"):
        ctx.sqmc_device("svm", "f64", 8, 1, 0, 1)
    with pytest.raises(ValueError, match="B must be >= 0"):
        ctx.sqmc_device("svm", "f64", 8, -1, buf.data_ptr(), 1)
    with pytest.raises(ValueError, match="Unrecognized model"):
        ctx.sqmc_device(7, "f64", 8, 1, buf.data_ptr(), 1)
    ctx.sqmc_device("svm", "f64", 8, 0, buf.data_ptr(), 1)          # no chains: not an error
    torch.cuda.synchronize()


# ---- 5. the ensemble ---------------------------------------------------------------------------------------------------------
SEED = 0x5EED0000C0DE4321
ENS = dict(T=20, N=16, scale=[0.15, 1.0, 0.3, 0.3], free=(0, 2, 3))
PLAIN_KEYS = {"theta", "momentum", "step_ctr", "steps_done", "seed", "chain_offset", "model", "N", "C", "ess_threshold", "ll",
              "n_accept"}


@functools.lru_cache(maxsize=None)
def _series():
    """The data of tests/test_gpu_pmmh.py's exactness test."""
    np.random.seed(333)
    return GEN["lgssm"](T=ENS["T"], parameters=default_params("lgssm"))["observations"].reshape(-1)


def _prior():
    return PRIORS["lgssm"].generate_default_prior(var=100.0, n=1, m=1)


def _ensemble(C, **kw):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    kw.setdefault("proposal_scale", ENS["scale"])
    kw.setdefault("seed", SEED)
    kw.setdefault("N", ENS["N"])
    kw.setdefault("prior", _prior())
    kw.setdefault("sqmc", True)
    return ChainEnsemble("lgssm", _series(), default_params("lgssm"), num_chains=C, sampler="pmmh", **kw)


def _state(e):
    e.synchronize()
    return dict(theta=e.theta_dev.cpu().numpy(), prop=e.theta_prop_dev.cpu().numpy(), valid=e.valid_dev.cpu().numpy(),
                out4=e.out_dev.cpu().numpy()[:, 4], ll=e.ll_dev.cpu().numpy(), n=e.accept_dev.cpu().numpy(),
                ctr=int(e.step_ctr.item()))


def test_ensemble_steps_match_the_restatement():
    """C = 150 chains straddling 2^32, three eager steps.  The init pass is the model's filter at counter 0; each step is
    recomputed on the host from the device's state before it: the proposal within 1e-14, the estimate on the device's own
    theta' to 1e-9, the decision exact wherever |log u - log alpha| >= 1e-9; a chain that accepts takes theta' and the
    estimate, bitwise the device's, one that rejects keeps theta and ll."""
    C, off, N = 150, 2 ** 32 - 70, ENS["N"]
    prior, y = _prior(), _series()
    e = _ensemble(C, chain_offset=off)
    assert e.sqmc is True and e.correlation is None
    pmean, pvar = float(e._sqmc_desc["prior_mean"][0]), float(e._sqmc_desc["prior_var"][0])
    useed = pm.update_seed(SEED)
    st = _state(e)
    assert st["ctr"] == 1 and not st["n"].any()
    np.testing.assert_allclose(st["ll"], sq.chain_init("lgssm", st["theta"], y, N, pmean, pvar, SEED, off), rtol=TOL_LL, atol=TOL_LL)
    np.testing.assert_array_equal(st["ll"], st["out4"])
    accepted = rejected = skipped = 0
    for s in range(3):
        before = st
        e.step(1)
        st = _state(e)
        acc = (st["n"] - before["n"]).astype(np.int64) == 1
        ctr = pm.step_counter(s)
        assert before["ctr"] == ctr and st["ctr"] == ctr + 1
        m = sq.chain_step("lgssm", prior, before["theta"], before["ll"], ENS["scale"], y, N, pmean, pvar, SEED, off, s)
        np.testing.assert_array_equal(st["valid"], m["valid"].astype(np.int32))
        np.testing.assert_allclose(st["prop"], m["prop"], rtol=1e-14, atol=1e-14)
        ll_dev_inputs = sq.loglik("lgssm", st["prop"], y, N, pmean, pvar, sq.filter_seed(SEED), kd.chain_ids(C, off), ctr,
                                  F=LD)["ll"].astype(np.float64)
        np.testing.assert_allclose(st["out4"], ll_dev_inputs, rtol=TOL_LL, atol=TOL_LL)
        want, margin = pm.accept("lgssm", prior, before["theta"], st["prop"], st["valid"], before["ll"], st["out4"], useed, off, ctr)
        sure = margin >= 1e-9
        np.testing.assert_array_equal(acc[sure], want[sure])
        np.testing.assert_array_equal(st["theta"][acc], st["prop"][acc])
        np.testing.assert_array_equal(st["ll"][acc], st["out4"][acc])
        np.testing.assert_array_equal(st["theta"][~acc], before["theta"][~acc])
        np.testing.assert_array_equal(st["ll"][~acc], before["ll"][~acc])
        accepted, rejected, skipped = accepted + int(acc.sum()), rejected + int((~acc).sum()), skipped + int((~sure).sum())
    assert skipped <= 0.01 * 3 * C and accepted > 0 and rejected > 0, (accepted, rejected, skipped)
    np.testing.assert_array_equal(e.acceptance_rate(), st["n"] / 3.0)
    np.testing.assert_array_equal(e.loglik(), st["ll"])


def test_ensemble_eager_graph_resume_partition():
    """C = 70: 8 eager steps = 8 steps through graph_steps = 4 = 4 steps, a state_dict loaded into a fresh ensemble, 4 more = two
    ensembles of 35 chains with chain_offset 0 and 35 -- bitwise.  The checkpoint is PMMH's plus 'sqmc'; either kind of
    ensemble refuses the other's; sqmc = False is plain PMMH, bit for bit."""
    C = 70
    a = _ensemble(C)
    a.step(8)
    ref = _state(a)
    assert 0 < ref["n"].sum() < 8 * C and ref["ctr"] == 9
    b = _ensemble(C)
    kept = b.run(8, thin=4, graph_steps=4)
    got = _state(b)
    for k in ("theta", "ll", "n", "ctr"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(kept[-1], ref["theta"][:, :kept.shape[2]])
    c = _ensemble(C)
    c.step(4)
    state = c.state_dict()
    assert set(state) == PLAIN_KEYS | {"sqmc"} and state["sqmc"] is True
    d = _ensemble(C)
    d.load_state_dict(state)
    d.step(4)
    got = _state(d)
    for k in ("theta", "ll", "n", "ctr"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    halves = []
    for off in (0, 35):
        h = _ensemble(35, chain_offset=off)
        h.step(8)
        halves.append(_state(h))
    for k in ("theta", "ll", "n"):
        np.testing.assert_array_equal(np.concatenate([halves[0][k], halves[1][k]]), ref[k], err_msg=k)
    plain = _ensemble(C, sqmc=False)
    assert set(plain.state_dict()) == PLAIN_KEYS and plain.sqmc is False
    assert not np.array_equal(_state(plain)["ll"], _state(_ensemble(C))["ll"])       # (another filter, another estimate)
    with pytest.raises(ValueError, match="checkpoint sqmc = True does not match the ensemble \\(False\\)"):
        plain.load_state_dict(state)
    with pytest.raises(ValueError, match="checkpoint sqmc = False does not match the ensemble \\(True\\)"):
        d.load_state_dict(plain.state_dict())
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    default = ChainEnsemble("lgssm", _series(), default_params("lgssm"), num_chains=C, sampler="pmmh", N=ENS["N"], seed=SEED,
                            proposal_scale=ENS["scale"], prior=_prior())
    plain.step(3)
    default.step(3)
    p, q = _state(plain), _state(default)
    for k in ("theta", "ll", "n", "ctr", "out4"):
        np.testing.assert_array_equal(p[k], q[k], err_msg=k)


EXACT = dict(C=2048, burn=400)


def test_sqmc_and_kalman_chains_sample_the_same_posterior():
    """LGSSM, T = 20, 2048 chains from the same start with the same proposal_scale, the data, prior and scale of
    tests/test_gpu_pmmh.py's exactness test: sampler='pmmh' with sqmc and N = 16 against kind='marginal' (plain
    Metropolis-Hastings on the Kalman likelihood).  After the burn-in, per free coordinate (A, LQinv, LRinv),
    |mean_sqmc - mean_kf| <= 5 sqrt((var_sqmc + var_kf) / C) over the chains' final states: the chains are independent, so the
    bound is the CLT's, not a tuned number.  The burn-in is that test's 400 steps (theta's own burn-in of 100 with a margin of
    4): an SQMC chain carries nothing beside theta and its estimate, so it needs no more than a PMMH chain."""
    C = EXACT["C"]
    final = {}
    for arm, kw in (("sqmc", dict(kind="pf", sqmc=True)), ("kf", dict(kind="marginal", sqmc=False))):
        e = _ensemble(C, **kw)
        e.run(EXACT["burn"], thin=EXACT["burn"], graph_steps=50)
        final[arm] = e.theta()[:, ENS["free"]]
        rate = e.acceptance_rate()
        print(arm, "mean", final[arm].mean(0), "var", final[arm].var(0, ddof=1), "acceptance", float(rate.mean()))
        assert 0.05 < rate.mean() < 0.9
    diff = np.abs(final["sqmc"].mean(0) - final["kf"].mean(0))
    bound = 5.0 * np.sqrt((final["sqmc"].var(0, ddof=1) + final["kf"].var(0, ddof=1)) / C)
    print("diff", diff, "bound", bound)
    assert np.all(diff <= bound), (diff, bound)
