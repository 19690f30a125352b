"""GPU: ChainEnsemble(sampler='pmmh') -- the propose and accept kernels draw for draw against the host restatement
(tests/helpers/pmmh_model.py), the device log-prior against Prior.logprior, the stale estimate, eager against hipGraph
against resume against the rank partition, the sequence-list path, the refusals, and the exactness of the chain: a
particle filter with N = 64 and the Kalman likelihood sample the same posterior."""
import os
import sys

import numpy as np
import pytest

from test_host_logic import DATA_SEED, GEN, PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pmmh_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000C0DE4321
SCALE = {"svm": [0.3, 0.3, 0.3], "lgssm": [0.2, 1.0, 0.4, 0.4], "garch": [0.2, 0.3, 0.3, 1.5]}


def _series(model, T):
    np.random.seed(DATA_SEED[model])
    return GEN[model](T=T, parameters=default_params(model))["observations"].reshape(-1)


def _prior(model, var=1.0):
    return PRIORS[model].generate_default_prior(var=var, n=1, m=1)


def _ensemble(model, y, C, **kw):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    kw.setdefault("proposal_scale", SCALE[model])
    kw.setdefault("seed", SEED)
    kw.setdefault("N", 64)
    kw.setdefault("prior", _prior(model))
    return ChainEnsemble(model, y, default_params(model), num_chains=C, sampler="pmmh", **kw)


def _state(e):
    e.synchronize()
    return dict(theta=e.theta_dev.cpu().numpy(), prop=e.theta_prop_dev.cpu().numpy(), valid=e.valid_dev.cpu().numpy(),
                out4=e.out_dev.cpu().numpy()[:, 4], ll=e.ll_dev.cpu().numpy(), n=e.accept_dev.cpu().numpy(),
                ctr=int(e.step_ctr.item()))


def _same(a, b, keys=("theta", "ll", "n", "ctr")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- 1. the update rule against the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_update_rule_matches_the_restatement(model):
    """C = 300 chains (five waves, three 128-lane blocks), N = 64, T = 12, six eager steps.  Proposals within
    TOL_ULPS of the mirror, valid exact, theta_prop == theta bitwise where invalid; the decisions recomputed on the host
    from the device's out[4] are exact wherever |log u - log alpha| >= 1e-9 (at most 1 % of chain-steps under it)."""
    from sgmcmc_ssm_amd import _capi
    C, T, off = 300, 12, 2 ** 32 - 150                  # the chain ids straddle 2^32: the high word takes part in the key
    prior = _prior(model)
    e = _ensemble(model, _series(model, T), C, chain_offset=off)
    P, scale, useed = _capi.THETA_DIM[model], SCALE[model], pm.update_seed(SEED)
    st = _state(e)
    assert st["ctr"] == 1 and np.all(np.isfinite(st["ll"])) and not st["n"].any()      # the init pass took counter 0
    np.testing.assert_array_equal(st["ll"], st["out4"])
    seen = dict(invalid=0, accepted=0, rejected=0, skipped=0)
    for s in range(6):
        before = st
        e.step(1)
        st = _state(e)
        ctr = pm.step_counter(s)
        assert before["ctr"] == ctr and st["ctr"] == ctr + 1
        pr = pm.propose(model, before["theta"], scale, useed, off, ctr)
        assert not pr.amb.any(), "a proposal within rounding of the support's edge: choose another seed"
        np.testing.assert_array_equal(st["valid"], pr.valid.astype(np.int32))
        inv = ~pr.valid
        np.testing.assert_array_equal(st["prop"][inv], before["theta"][inv])            # bitwise the current theta
        err = np.abs(st["prop"][:, :P].astype(pm.LD) - pr.theta_prop)
        assert np.all(err <= pr.tol), (model, s, float(np.max(err / pr.tol)))
        np.testing.assert_array_equal(st["prop"][:, P:], before["theta"][:, P:])
        if model == "lgssm":
            assert np.all(st["prop"][:, 1] == 1.0)
        # decisions, from the device's own proposals and estimates
        acc, margin = pm.accept(model, prior, before["theta"][:, :P], st["prop"][:, :P], st["valid"], before["ll"], st["out4"],
                                useed, off, ctr)
        sure = margin >= 1e-9
        got = (st["n"] - before["n"]).astype(np.int64)
        assert set(np.unique(got)) <= {0, 1}
        print(model, "step", s, "valid", int(pr.valid.sum()), "accepted", int(got.sum()), "min margin", float(margin.min()))
        np.testing.assert_array_equal(got[sure] == 1, acc[sure])
        a = got == 1
        np.testing.assert_array_equal(st["theta"][a], st["prop"][a])
        np.testing.assert_array_equal(st["ll"][a], st["out4"][a])
        np.testing.assert_array_equal(st["theta"][~a], before["theta"][~a])
        np.testing.assert_array_equal(st["ll"][~a], before["ll"][~a])
        assert not (a & inv).any()
        seen["invalid"] += int(inv.sum())
        seen["accepted"] += int(a.sum())
        seen["rejected"] += int((~a & pr.valid).sum())
        seen["skipped"] += int((~sure).sum())
    assert seen["skipped"] <= 0.01 * 6 * C, seen
    assert seen["invalid"] > 0 and seen["accepted"] > 0 and seen["rejected"] > 0, seen
    np.testing.assert_array_equal(e.acceptance_rate(), st["n"] / 6.0)
    np.testing.assert_array_equal(e.loglik(), st["ll"])
    g, ll = e.last_gradient_statistics()
    assert g is None
    np.testing.assert_array_equal(ll, st["out4"])


# ---- 2. the log-prior -----------------------------------------------------------------------------------------------------
def _prior_pairs(model, n=40):
    """n pairs of raw rows, the first ones at the support's edge: |A| = 0.9999, tiny and large Cholesky factors."""
    from sgmcmc_ssm_amd import _capi
    rs = np.random.RandomState(17)
    P = _capi.THETA_DIM[model]

    def rows():
        th = np.zeros((n, _capi.MAX_THETA))
        if model == "garch":
            th[:, 0] = rs.uniform(-3, 3, n)
            th[:, 1:3] = rs.uniform(-4, 4, (n, 2))
            th[:, 3] = np.exp(rs.uniform(-3, 3, n))
            th[:6, 3] = [1e-6, 1e-3, 50.0, 1e3, 1e-9, 7.0]
        else:
            th[:, 0] = rs.uniform(-0.9999, 0.9999, n)
            th[:4, 0] = [0.9999, -0.9999, 0.99989999, 0.0]
            th[:, P - 2:P] = np.exp(rs.uniform(-3, 3, (n, 2)))
            th[4:10, P - 2] = [1e-6, 1e-3, 50.0, 1e3, 1e-9, 7.0]
            th[10:14, P - 1] = [1e-6, 1e-3, 50.0, 1e3]
            if model == "lgssm":
                th[:, 1] = 1.0
        return th
    return rows(), rows()[::-1].copy()


@pytest.mark.parametrize("var", [1.0, 100.0])
@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_device_logprior_differences_match_the_host(model, var):
    """pfg_logprior_device against Prior.logprior on 40 pairs per model and prior: the device value drops the terms of the
    hyper-parameters alone, so DIFFERENCES are compared, at 1e-12 relative to the larger of the pair's two |log-prior|
    values (the host's own two values carry a few ulps of that size each; a difference smaller than that cannot be
    asked for more tightly than the reference itself delivers it)."""
    import torch
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.ensemble import prior_hyper
    prior = _prior(model, var)
    hy = prior_hyper(model, prior)
    a, b = _prior_pairs(model)
    ctx = _capi.default_context()
    dev = []
    for th in (a, b):
        t = torch.from_numpy(th).to("cuda")
        o = torch.full((len(th),), float("nan"), dtype=torch.float64, device="cuda")
        ctx.logprior_device(model, len(th), t.data_ptr(), hy, o.data_ptr())
        torch.cuda.synchronize()
        dev.append(o.cpu().numpy())
    ha, hb = pm.logprior(model, prior, a), pm.logprior(model, prior, b)
    assert np.all(np.isfinite(ha)) and np.all(np.isfinite(hb)) and np.all(np.isfinite(dev[0])) and np.all(np.isfinite(dev[1]))
    d_dev = dev[0].astype(pm.LD) - dev[1].astype(pm.LD)
    d_host = ha.astype(pm.LD) - hb.astype(pm.LD)
    rel = np.abs(d_dev - d_host) / np.maximum(np.abs(ha), np.abs(hb))
    print(model, var, "max relative error of the differences", float(rel.max()))
    assert np.all(rel <= 1e-12), (model, var, float(rel.max()), int(np.argmax(rel)))
    # and the constant it drops is one constant
    const = dev[0].astype(pm.LD) - ha.astype(pm.LD)
    assert float(np.max(np.abs(const - const[0]) / np.maximum(1.0, np.abs(ha)))) <= 1e-12


# ---- 3. the estimate is never refreshed --------------------------------------------------------------------------------
def test_estimate_changes_only_with_theta():
    e = _ensemble("svm", _series("svm", 12), 70, proposal_scale=0.1)
    st = _state(e)
    moved = kept = 0
    for _ in range(40):
        before = st
        e.step(1)
        st = _state(e)
        dth = np.any(st["theta"] != before["theta"], axis=1)
        dll = st["ll"] != before["ll"]
        np.testing.assert_array_equal(dll, dth)
        np.testing.assert_array_equal(dth, st["n"] != before["n"])
        assert np.any(st["out4"] != st["ll"])            # fresh estimates were there to be (wrongly) taken
        moved += int(dth.sum())
        kept += int((~dth).sum())
    assert moved > 0 and kept > 0
    assert e.steps_done == 40 and st["ctr"] == 41


# ---- 4. eager, graph, resume, partition, sequence lists ---------------------------------------------------------------------
CONFIGS = [("svm", {}), ("garch", dict(resampling="stratified")), ("lgssm", dict(kind="marginal")), ("lgssm", dict(ess_threshold=0.5))]
CONFIG_IDS = ["svm", "garch-stratified", "lgssm-marginal", "lgssm-adaptive"]


@pytest.mark.parametrize("model, kw", CONFIGS, ids=CONFIG_IDS)
def test_eager_graph_resume(model, kw):
    """C = 70, N = 64, T = 12, a single series: 8 eager steps = 8 steps through graph_steps = 4 = 4 steps, a state_dict
    loaded into a fresh ensemble, 4 more -- bitwise, the estimates and acceptance counts included."""
    C, y = 70, _series(model, 12)
    a = _ensemble(model, y, C, **kw)
    a.step(8)
    ref = _state(a)
    assert ref["n"].sum() > 0 and ref["ctr"] == 9
    b = _ensemble(model, y, C, **kw)
    kept = b.run(8, thin=4, graph_steps=4)
    _same(ref, _state(b))
    np.testing.assert_array_equal(kept[-1], ref["theta"][:, :kept.shape[2]])
    assert b.steps_done == 8
    c = _ensemble(model, y, C, **kw)
    c.step(4)
    state = c.state_dict()
    assert set(state) >= {"ll", "n_accept"}
    d = _ensemble(model, y, C, **kw)
    d.load_state_dict(state)
    d.step(4)
    _same(ref, _state(d))


@pytest.mark.parametrize("model, kw", [("svm", dict(N=1100)), ("lgssm", dict(kind="marginal"))], ids=["svm-N1100", "lgssm-marginal"])
def test_rank_partition(model, kw):
    """Chains [0, 70) as one ensemble = two ensembles with chain_offset 0 and 35, bitwise: every draw is keyed by the global
    chain id.  As for the other samplers this holds where both partitions' launches run the same kernel: the launch plan
    picks the one-wave units of N <= 256 (and wg256x4s over the latency unit up to N = 1024) only above 64 windows, and
    another unit lays the particles' draws out differently.  So the particle-filter case runs at N = 1100, where the plan
    does not look at the batch size; the kernels that ran are compared."""
    y = _series(model, 12)
    a = _ensemble(model, y, 70, **kw)
    a.step(8)
    ref, variant = _state(a), a.ctx.last_variant()
    assert ref["n"].sum() > 0
    halves = []
    for off in (0, 35):
        h = _ensemble(model, y, 35, chain_offset=off, **kw)
        h.step(8)
        halves.append(_state(h))
        assert h.ctx.last_variant() == variant
    for k in ("theta", "ll", "n"):
        np.testing.assert_array_equal(np.concatenate([halves[0][k], halves[1][k]]), ref[k], err_msg=k)


def test_other_samplers_state_dict_is_unchanged():
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    e = ChainEnsemble("svm", _series("svm", 12), default_params("svm"), num_chains=4, N=64)
    assert set(e.state_dict()) == {"theta", "momentum", "step_ctr", "steps_done", "seed", "chain_offset", "model", "N", "C",
                                   "ess_threshold"}
    with pytest.raises(ValueError, match="belongs to sampler='pmmh'"):
        e.loglik()


def test_sequence_list_sums_the_windows():
    """Three sequences (10, 14, 8), num_sequences = -1: the reduced out[4] is the windows' out[4] summed in the reduction's
    order ((0 + w0) + w1) + w2, and the chain accepts on it."""
    y = _series("svm", 32)
    segs = [y[:10], y[10:24], y[24:]]
    e = _ensemble("svm", segs, 70, num_sequences=-1, subsequence_length=-1, buffer_length=0, window_sampling="device",
                  proposal_scale=0.1)
    assert e._multi and e.W == 3 and not e._rescale
    for k in range(3):
        if k:
            e.run(2, thin=2, graph_steps=2)
        st = _state(e)
        win, seq_len = e.window_statistics()
        np.testing.assert_array_equal(seq_len, np.tile([10, 14, 8], (70, 1)))
        w = win[:, :, 4]
        np.testing.assert_array_equal(st["out4"], ((0.0 + w[:, 0]) + w[:, 1]) + w[:, 2])
        acc = st["ll"] == st["out4"]
        assert np.all(np.isfinite(st["ll"]))
        if k == 0:
            assert acc.all()                        # the init pass
    assert st["n"].sum() > 0 and st["ctr"] == 5


# ---- 5. exactness -------------------------------------------------------------------------------------------------------------
EXACT = dict(T=20, C=4096, N=64, burn=400, scale=[0.15, 1.0, 0.3, 0.3], free=(0, 2, 3))


def test_particle_filter_and_kalman_chains_sample_the_same_posterior():
    """LGSSM, T = 20, 4096 chains from the same start with the same proposal_scale: sampler='pmmh' with kind='pf', N = 64
    against kind='marginal' (plain Metropolis-Hastings on the Kalman likelihood).  After the burn-in, per free
    coordinate (A, LQinv, LRinv), |mean_pf - mean_kf| <= 5 sqrt((var_pf + var_kf) / C) over the chains' final states:
    the chains are independent, so the bound is the CLT's, not a tuned number.

    Burn-in and proposal_scale chosen on the CPU (tools/pmmh_burnin_cpu.py: the restatement with the oracle's filter,
    N = 64, 128 chains, and the Kalman model, 512 chains, 400 steps, scale (0.15, -, 0.3, 0.3)); its output is quoted
    under CPU_RUN below.  Both arms' means stay inside their standard errors from step 100 on, so the burn-in of 400
    steps has a margin of 4 in step count."""
    T, C = EXACT["T"], EXACT["C"]
    np.random.seed(333)
    y = GEN["lgssm"](T=T, parameters=default_params("lgssm"))["observations"].reshape(-1)
    prior = _prior("lgssm", 100.0)
    final = {}
    for arm, kw in (("pf", dict(kind="pf", N=EXACT["N"])), ("kf", dict(kind="marginal"))):
        e = _ensemble("lgssm", y, C, prior=prior, proposal_scale=EXACT["scale"], **kw)
        e.run(EXACT["burn"], thin=EXACT["burn"], graph_steps=50)
        final[arm] = e.theta()[:, EXACT["free"]]
        rate = e.acceptance_rate()
        print(arm, "mean", final[arm].mean(0), "var", final[arm].var(0, ddof=1), "acceptance", float(rate.mean()))
        assert 0.05 < rate.mean() < 0.9
    diff = np.abs(final["pf"].mean(0) - final["kf"].mean(0))
    bound = 5.0 * np.sqrt((final["pf"].var(0, ddof=1) + final["kf"].var(0, ddof=1)) / C)
    print("diff", diff, "bound", bound)
    assert np.all(diff <= bound), (diff, bound)


CPU_RUN = """
# scale [0.15, 1.0, 0.3, 0.3] T 20 N 64 steps 400          (python tools/pmmh_burnin_cpu.py; means of A, LQinv, LRinv)
kalman  C  512 step   25  mean [0.7721 1.1041 1.2404]  se [0.0062 0.0131 0.0148]  var [0.0199 0.0877 0.1116]
kalman  C  512 step   50  mean [0.7474 1.0618 1.2746]  se [0.007  0.0135 0.0155]  var [0.0252 0.0928 0.1228]
kalman  C  512 step  100  mean [0.7482 1.0582 1.2931]  se [0.0069 0.0133 0.0161]  var [0.0243 0.0907 0.1331]
kalman  C  512 step  200  mean [0.7503 1.0656 1.2986]  se [0.0073 0.0121 0.0154]  var [0.0269 0.0754 0.1211]
kalman  C  512 step  300  mean [0.7516 1.0522 1.2781]  se [0.0074 0.0123 0.0154]  var [0.0282 0.0776 0.1219]
kalman  C  512 step  400  mean [0.7524 1.0651 1.2847]  se [0.0074 0.0127 0.0151]  var [0.0283 0.0829 0.1161]
kalman  acceptance 0.394
pf      C  128 step   25  mean [0.7632 1.0792 1.2185]  se [0.0132 0.0232 0.028 ]  var [0.0223 0.069  0.1006]
pf      C  128 step   50  mean [0.7747 1.0769 1.2836]  se [0.0128 0.0247 0.0328]  var [0.0209 0.0781 0.1381]
pf      C  128 step  100  mean [0.7525 1.0653 1.2562]  se [0.0137 0.0239 0.0276]  var [0.0241 0.0729 0.0975]
pf      C  128 step  200  mean [0.7626 1.0546 1.2855]  se [0.0134 0.0216 0.0319]  var [0.0228 0.0597 0.1301]
pf      C  128 step  300  mean [0.7324 1.0618 1.2224]  se [0.0159 0.0234 0.0318]  var [0.0326 0.0698 0.1291]
pf      C  128 step  400  mean [0.7443 1.0801 1.3019]  se [0.0137 0.026  0.0309]  var [0.0242 0.0864 0.1218]
pf      acceptance 0.365
(the wider scale (0.3, -, 0.5, 0.5) reaches the same means with acceptance 0.18 / 0.17.  On the MI355X, 4096 chains, step
400: pf mean 0.7596 1.0752 1.2804, kalman 0.7609 1.0724 1.2798, acceptance 0.363 / 0.394; differences 0.0013 0.0027 0.0006
against bounds 0.0169 0.0318 0.0390.)
"""


# ---- 6. refusals on the device path ----------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble, prior_hyper
    y, p = _series("svm", 12), default_params("svm")
    with pytest.raises(ValueError, match="needs proposal_scale"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, sampler="pmmh")
    with pytest.raises(ValueError, match="proposal_scale is the random walk of sampler='pmmh'"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, proposal_scale=0.1)
    with pytest.raises(NotImplementedError, match="pmmh needs the whole series"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, sampler="pmmh", proposal_scale=0.1, subsequence_length=4, buffer_length=2)
    with pytest.raises(NotImplementedError, match="kind='complete' samples paths"):
        ChainEnsemble("lgssm", y, default_params("lgssm"), num_chains=4, sampler="pmmh", proposal_scale=0.1, kind="complete",
                      num_samples=4)
    with pytest.raises(NotImplementedError, match="smoothing of pf = 'paris'"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, sampler="pmmh", proposal_scale=0.1, pf="paris")
    # a chain whose initial log-likelihood is not finite is named (the Kalman launch: arithmetic only, a NaN observation)
    bad = _series("lgssm", 12).copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="initial log-likelihood of chain 5 is not finite"):
        _ensemble("lgssm", bad, 4, kind="marginal", chain_offset=5)
    # the C ABI
    ctx = _capi.default_context()
    hy = prior_hyper("svm", _prior("svm"))
    th = torch.ones((4, _capi.MAX_THETA), dtype=torch.float64, device="cuda")
    tp, out = th.clone(), torch.zeros((4, _capi.OUT_DOUBLES), dtype=torch.float64, device="cuda")
    valid = torch.ones(4, dtype=torch.int32, device="cuda")
    ll, n = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    sc = torch.ones(_capi.MAX_THETA, dtype=torch.float64, device="cuda")
    prop = lambda model=0, B=4, **k: ctx.pmmh_propose_device(      # noqa: E731
        model, B, k.get("theta", th.data_ptr()), tp.data_ptr(), k.get("valid", valid.data_ptr()), k.get("scale", sc.data_ptr()), 1)
    acc = lambda model=0, B=4, **k: ctx.pmmh_accept_device(        # noqa: E731
        model, B, th.data_ptr(), tp.data_ptr(), valid.data_ptr(), k.get("outs", out.data_ptr()), k.get("ll", ll.data_ptr()),
        k.get("n", n.data_ptr()), k.get("hyper", hy), 0, 1)
    lp = lambda model=0, B=4, **k: ctx.logprior_device(model, B, k.get("theta", th.data_ptr()), k.get("hyper", hy),  # noqa: E731
                                                       k.get("out", ll.data_ptr()))
    for call in (prop, acc, lp):
        for model in (-1, 3):
            with pytest.raises(ValueError, match="Unrecognized model id"):
                call(model=model)
        with pytest.raises(ValueError, match="B must be >= 0"):
            call(B=-1)
        call(B=0)                                                   # nothing to do
    for call, kws in ((prop, ("theta", "valid", "scale")), (acc, ("outs", "ll", "n", "hyper")), (lp, ("theta", "hyper", "out"))):
        for k in kws:
            with pytest.raises(ValueError, match="NULL argument"):
                call(**{k: None})
    torch.cuda.synchronize()
    np.testing.assert_array_equal(th.cpu().numpy(), 1.0)            # no refused call wrote anything
    assert not n.cpu().numpy().any()
