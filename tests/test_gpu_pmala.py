"""GPU: ChainEnsemble(sampler='pmala') -- the propose and accept kernels draw for draw against the host restatement
(tests/helpers/pmala_model.py), the estimates that move only with theta, eager against hipGraph against resume against the
rank partition, the sequence-list path, the refusals, and the exactness of the chain: with the Kalman score and
likelihood (plain MALA) and with a particle filter of N = 64 it samples the posterior the exact PMMH chain samples."""
import os
import sys

import numpy as np
import pytest

from test_host_logic import DATA_SEED, GEN, PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pmala_model as pa  # noqa: E402
import window_reduce  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000C0DE4321
# chosen on the CPU (the restatement with the oracle's filter, N = 64, T = 12, 100 chains, six steps) so that invalid,
# accepted and rejected chain-steps are each a sixth of the total or more
SCALE = {"svm": [0.3, 0.3, 0.3], "lgssm": [0.2, 1.0, 0.4, 0.4], "garch": [0.3, 0.5, 0.5, 1.0]}


def _series(model, T):
    np.random.seed(DATA_SEED[model])
    return GEN[model](T=T, parameters=default_params(model))["observations"].reshape(-1)


def _prior(model, var=1.0):
    return PRIORS[model].generate_default_prior(var=var, n=1, m=1)


def _ensemble(model, y, C, sampler="pmala", **kw):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    kw.setdefault("proposal_scale", SCALE[model])
    kw.setdefault("seed", SEED)
    kw.setdefault("N", 64)
    kw.setdefault("prior", _prior(model))
    return ChainEnsemble(model, y, default_params(model), num_chains=C, sampler=sampler, **kw)


def _state(e):
    e.synchronize()
    out = e.out_dev.cpu().numpy()
    return dict(theta=e.theta_dev.cpu().numpy(), prop=e.theta_prop_dev.cpu().numpy(), valid=e.valid_dev.cpu().numpy(),
                out4=out[:, 4], outg=out[:, :4].copy(), ll=e.ll_dev.cpu().numpy(), grad=e.grad_cur_dev.cpu().numpy(),
                n=e.accept_dev.cpu().numpy(), ctr=int(e.step_ctr.item()))


def _same(a, b, keys=("theta", "ll", "grad", "n", "ctr")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- 1. the update rule against the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_update_rule_matches_the_restatement(model):
    """C = 300 chains (five waves, three 128-lane blocks) with chain ids that straddle 2^32, N = 64, T = 12, six eager
    steps.  Proposals within TOL_ULPS of the mirror computed from the device's own theta and grad_cur, valid exact,
    theta_prop == theta bitwise where invalid; the decisions recomputed on the host from the device's records are exact
    wherever |log u - log alpha| >= 1e-9 (at most 1 % of chain-steps under it); an accepting chain takes the proposal's
    theta, out[4] and out[0..3] bitwise, a rejecting one keeps all three bitwise."""
    from sgmcmc_ssm_amd import _capi
    C, T, off = 300, 12, 2 ** 32 - 150                  # the high word takes part in the key
    prior = _prior(model)
    e = _ensemble(model, _series(model, T), C, chain_offset=off)
    hy = e.hyper
    P, scale, useed = _capi.THETA_DIM[model], SCALE[model], pa.update_seed(SEED)
    st = _state(e)
    assert st["ctr"] == 1 and np.all(np.isfinite(st["ll"])) and not st["n"].any()      # the init pass took counter 0
    np.testing.assert_array_equal(st["ll"], st["out4"])
    np.testing.assert_array_equal(st["grad"], st["outg"])
    assert np.all(np.isfinite(st["grad"][:, list(pa.USED_COLS[model])])) and np.any(st["grad"] != 0)
    seen = dict(invalid=0, accepted=0, rejected=0, skipped=0)
    for s in range(6):
        before = st
        e.step(1)
        st = _state(e)
        ctr = pa.step_counter(s)
        assert before["ctr"] == ctr and st["ctr"] == ctr + 1
        pr = pa.propose(model, before["theta"], before["grad"], scale, useed, off, ctr, hy)
        assert not pr.amb.any(), "a proposal within rounding of the support's edge: choose another seed"
        np.testing.assert_array_equal(st["valid"], pr.valid.astype(np.int32))
        inv = ~pr.valid
        np.testing.assert_array_equal(st["prop"][inv], before["theta"][inv])            # bitwise the current theta
        err = np.abs(st["prop"][:, :P].astype(pa.LD) - pr.theta_prop)
        assert np.all(err <= pr.tol), (model, s, float(np.max(err / pr.tol)))
        np.testing.assert_array_equal(st["prop"][:, P:], before["theta"][:, P:])
        if model == "lgssm":
            assert np.all(st["prop"][:, 1] == 1.0)
        # decisions, from the device's own proposals and estimates
        acc, margin = pa.accept(model, prior, hy, scale, before["theta"][:, :P], st["prop"][:, :P], st["valid"], before["ll"],
                                st["out4"], before["grad"], st["outg"], useed, off, ctr)
        sure = margin >= 1e-9
        got = (st["n"] - before["n"]).astype(np.int64)
        assert set(np.unique(got)) <= {0, 1}
        print(model, "step", s, "valid", int(pr.valid.sum()), "accepted", int(got.sum()), "min margin", float(margin.min()),
              "max proposal error / tol", float(np.max(err / np.maximum(pr.tol, 1e-300))))
        np.testing.assert_array_equal(got[sure] == 1, acc[sure])
        a = got == 1
        np.testing.assert_array_equal(st["theta"][a], st["prop"][a])
        np.testing.assert_array_equal(st["ll"][a], st["out4"][a])
        np.testing.assert_array_equal(st["grad"][a], st["outg"][a])
        np.testing.assert_array_equal(st["theta"][~a], before["theta"][~a])
        np.testing.assert_array_equal(st["ll"][~a], before["ll"][~a])
        np.testing.assert_array_equal(st["grad"][~a], before["grad"][~a])
        assert not (a & inv).any()
        seen["invalid"] += int(inv.sum())
        seen["accepted"] += int(a.sum())
        seen["rejected"] += int((~a & pr.valid).sum())
        seen["skipped"] += int((~sure).sum())
    print(model, seen)
    assert seen["skipped"] <= 0.01 * 6 * C, seen
    assert seen["invalid"] > 0 and seen["accepted"] > 0 and seen["rejected"] > 0, seen
    np.testing.assert_array_equal(e.acceptance_rate(), st["n"] / 6.0)
    np.testing.assert_array_equal(e.loglik(), st["ll"])
    h = _capi.STAT_DIM[model]
    np.testing.assert_array_equal(e.score(), st["grad"][:, :h])
    g, ll = e.last_gradient_statistics()                # the latest PROPOSALS' estimates
    np.testing.assert_array_equal(g, st["outg"][:, :h])
    np.testing.assert_array_equal(ll, st["out4"])


# ---- 2. the estimates are never refreshed ------------------------------------------------------------------------------
def test_estimates_change_only_with_theta():
    e = _ensemble("svm", _series("svm", 12), 70, proposal_scale=0.1)
    st = _state(e)
    moved = kept = 0
    for _ in range(20):
        before = st
        e.step(1)
        st = _state(e)
        dth = np.any(st["theta"] != before["theta"], axis=1)
        np.testing.assert_array_equal(st["ll"] != before["ll"], dth)
        np.testing.assert_array_equal(np.any(st["grad"] != before["grad"], axis=1), dth)
        np.testing.assert_array_equal(dth, st["n"] != before["n"])
        # fresh estimates were there to be (wrongly) taken
        assert np.any(st["out4"] != st["ll"]) and np.any(st["outg"] != st["grad"])
        moved += int(dth.sum())
        kept += int((~dth).sum())
    assert moved > 0 and kept > 0
    assert e.steps_done == 20 and st["ctr"] == 21


# ---- 3. eager, graph, resume ------------------------------------------------------------------------------------------
CONFIGS = [("svm", {}), ("garch", dict(resampling="stratified")), ("lgssm", dict(kind="marginal")), ("lgssm", dict(ess_threshold=0.5))]
CONFIG_IDS = ["svm", "garch-stratified", "lgssm-marginal", "lgssm-adaptive"]


@pytest.mark.parametrize("model, kw", CONFIGS, ids=CONFIG_IDS)
def test_eager_graph_resume(model, kw):
    """C = 70, N = 64, T = 12, a single series: 8 eager steps = 8 steps through graph_steps = 4 = 4 steps, a state_dict
    loaded into a fresh ensemble, 4 more -- bitwise: theta, both estimates, the acceptance counts and the counter."""
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
    assert set(state) >= {"ll", "grad", "n_accept"}
    d = _ensemble(model, y, C, **kw)
    d.load_state_dict(state)
    d.step(4)
    _same(ref, _state(d))


def test_other_samplers_state_dicts_are_unchanged():
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    base = {"theta", "momentum", "step_ctr", "steps_done", "seed", "chain_offset", "model", "N", "C", "ess_threshold"}
    y = _series("svm", 12)
    e = ChainEnsemble("svm", y, default_params("svm"), num_chains=4, N=64)
    assert set(e.state_dict()) == base
    with pytest.raises(ValueError, match="belongs to sampler='pmala'"):
        e.score()
    m = _ensemble("svm", y, 4, sampler="pmmh", proposal_scale=0.1)
    assert set(m.state_dict()) == base | {"ll", "n_accept"}
    with pytest.raises(ValueError, match="belongs to sampler='pmala'"):
        m.score()
    assert set(_ensemble("svm", y, 4).state_dict()) == base | {"ll", "grad", "n_accept"}


# ---- 4. the rank partition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model, kw", [("svm", dict(N=1100)), ("lgssm", dict(kind="marginal"))], ids=["svm-N1100", "lgssm-marginal"])
def test_rank_partition(model, kw):
    """Chains [0, 70) as one ensemble = two ensembles with chain_offset 0 and 35, bitwise: every draw is keyed by the global
    chain id.  As for the other samplers this holds where both partitions' launches run the same kernel, so the
    particle-filter case runs at N = 1100, where the launch plan does not look at the batch size; the kernels that ran
    are compared."""
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
    for k in ("theta", "ll", "grad", "n"):
        np.testing.assert_array_equal(np.concatenate([halves[0][k], halves[1][k]]), ref[k], err_msg=k)


# ---- 5. sequence lists ---------------------------------------------------------------------------------------------------
def test_sequence_list_sums_the_windows():
    """Three sequences (10, 14, 8), num_sequences = -1, no rescale: the reduced record's score columns and out[4] are the
    windows' summed in the reduction's order (tests/helpers/window_reduce.py: ((0 + w0) + w1) + w2 per column), and the
    chain holds and accepts on them."""
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
        want = window_reduce.reduce_windows(win, seq_len, 3, 1, False, 32.0)
        np.testing.assert_array_equal(st["out4"], want[:, 4])
        np.testing.assert_array_equal(st["outg"], want[:, :4])
        np.testing.assert_array_equal(st["out4"], ((0.0 + win[:, 0, 4]) + win[:, 1, 4]) + win[:, 2, 4])
        for j in range(3):
            np.testing.assert_array_equal(st["outg"][:, j], ((0.0 + win[:, 0, j]) + win[:, 1, j]) + win[:, 2, j])
        assert np.all(np.isfinite(st["ll"])) and np.all(np.isfinite(st["grad"][:, :3]))
        taken = st["ll"] == st["out4"]
        np.testing.assert_array_equal(st["grad"][taken], st["outg"][taken])
        if k == 0:
            assert taken.all()                      # the init pass
    assert st["n"].sum() > 0 and st["ctr"] == 5


# ---- 6. exactness --------------------------------------------------------------------------------------------------------
EXACT = dict(T=20, C=4096, N=64, burn=200, scale=[0.2, 1.0, 0.3, 0.3], free=(0, 2, 3),
             pmmh_burn=400, pmmh_scale=[0.15, 1.0, 0.3, 0.3])      # the PMMH arm: test_gpu_pmmh.py's EXACT


def test_pmala_chains_sample_the_posterior_of_the_exact_pmmh_chain():
    """LGSSM, T = 20, 4096 chains from the same start, prior var = 100, the series and start of
    test_particle_filter_and_kalman_chains_sample_the_same_posterior (test_gpu_pmmh.py).  Three arms: sampler='pmala' with
    kind='marginal' (plain MALA: the Kalman launch's score and likelihood are exact), sampler='pmala' with kind='pf',
    N = 64, and the reference, sampler='pmmh' with kind='marginal' at its committed scale and burn-in.  Per free coordinate
    (A, LQinv, LRinv), each pMALA arm against the PMMH arm: |mean_a - mean_b| <= 5 sqrt((var_a + var_b) / C) over the
    chains' final states -- the chains are independent, so the bound is the CLT's, not a tuned number.  Both pMALA arms'
    mean acceptance lies in (0.2, 0.8): there the q-ratio does work, so a wrong sign or a missing reverse term in it moves
    the means.

    proposal_scale and burn-in chosen on the CPU (tools/pmala_burnin_cpu.py: the restatement with the Kalman model, 512
    chains, and the oracle's filter, N = 64, 128 chains, 200 steps, scale (0.2, -, 0.3, 0.3)); its output is quoted under
    CPU_RUN below.  From the checkpoint at step 25 on both arms' means show no trend and lie within 2.5 of their
    standard errors of the posterior means the PMMH test measured on 4096 chains (0.7609, 1.0724, 1.2798); the burn-in is
    counted from the next checkpoint, step 50, with a margin of 4: 200 steps."""
    T, C = EXACT["T"], EXACT["C"]
    np.random.seed(333)
    y = GEN["lgssm"](T=T, parameters=default_params("lgssm"))["observations"].reshape(-1)
    prior = _prior("lgssm", 100.0)
    final = {}
    arms = (("pmmh-kf", "pmmh", EXACT["pmmh_burn"], dict(kind="marginal", proposal_scale=EXACT["pmmh_scale"])),
            ("pmala-kf", "pmala", EXACT["burn"], dict(kind="marginal", proposal_scale=EXACT["scale"])),
            ("pmala-pf", "pmala", EXACT["burn"], dict(kind="pf", N=EXACT["N"], proposal_scale=EXACT["scale"])))
    for arm, sampler, burn, kw in arms:
        e = _ensemble("lgssm", y, C, sampler=sampler, prior=prior, **kw)
        e.run(burn, thin=burn, graph_steps=50)
        final[arm] = e.theta()[:, EXACT["free"]]
        rate = float(e.acceptance_rate().mean())
        print(arm, "mean", final[arm].mean(0), "var", final[arm].var(0, ddof=1), "acceptance", rate)
        if sampler == "pmala":
            assert 0.2 < rate < 0.8, (arm, rate)
    ref = final["pmmh-kf"]
    for arm in ("pmala-kf", "pmala-pf"):
        diff = np.abs(final[arm].mean(0) - ref.mean(0))
        bound = 5.0 * np.sqrt((final[arm].var(0, ddof=1) + ref.var(0, ddof=1)) / C)
        print(arm, "diff", diff, "bound", bound)
        assert np.all(diff <= bound), (arm, diff, bound)


CPU_RUN = """
# scale [0.2, 1.0, 0.3, 0.3] T 20 N 64 steps 200          (python tools/pmala_burnin_cpu.py; means of A, LQinv, LRinv)
kalman  C  512 step   12  mean [0.7585 1.0591 1.2568]  se [0.0067 0.0119 0.0147]  var [0.0231 0.0722 0.11  ]
kalman  C  512 step   25  mean [0.7598 1.0869 1.2942]  se [0.0065 0.0129 0.0149]  var [0.0216 0.0857 0.1143]
kalman  C  512 step   50  mean [0.7556 1.0623 1.2991]  se [0.0066 0.012  0.0158]  var [0.022  0.0734 0.1278]
kalman  C  512 step  100  mean [0.7546 1.0826 1.2854]  se [0.0071 0.0128 0.0148]  var [0.0255 0.0841 0.1127]
kalman  C  512 step  150  mean [0.7572 1.0668 1.281 ]  se [0.0073 0.0118 0.0154]  var [0.0271 0.0708 0.1208]
kalman  C  512 step  200  mean [0.7479 1.044  1.2968]  se [0.007  0.0121 0.0153]  var [0.025  0.0746 0.1202]
kalman  acceptance 0.521
pf      C  128 step   12  mean [0.7596 1.0885 1.2423]  se [0.0131 0.0244 0.0257]  var [0.0219 0.0762 0.0845]
pf      C  128 step   25  mean [0.7617 1.093  1.3001]  se [0.0129 0.0237 0.0308]  var [0.0212 0.0718 0.1211]
pf      C  128 step   50  mean [0.7561 1.0762 1.2741]  se [0.0129 0.0247 0.0306]  var [0.0213 0.078  0.12  ]
pf      C  128 step  100  mean [0.7588 1.0545 1.266 ]  se [0.0134 0.0223 0.0276]  var [0.023  0.0638 0.0977]
pf      C  128 step  150  mean [0.7698 1.1208 1.2732]  se [0.0139 0.0277 0.0315]  var [0.0249 0.0983 0.1268]
pf      C  128 step  200  mean [0.74   1.0618 1.303 ]  se [0.0139 0.0227 0.0323]  var [0.0248 0.066  0.1334]
pf      acceptance 0.413
"""


# ---- 7. refusals on the device path ----------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble, prior_hyper
    y, p = _series("svm", 12), default_params("svm")
    with pytest.raises(ValueError, match="sampler='pmala' needs proposal_scale"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, sampler="pmala")
    with pytest.raises(ValueError, match="pmmh_stat belongs to sampler='pmmh'"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, sampler="pmala", proposal_scale=0.1, pmmh_stat="score")
    with pytest.raises(NotImplementedError, match="pmala needs the whole series"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, sampler="pmala", proposal_scale=0.1, subsequence_length=4, buffer_length=2)
    with pytest.raises(NotImplementedError, match="kind='complete' samples paths"):
        ChainEnsemble("lgssm", y, default_params("lgssm"), num_chains=4, sampler="pmala", proposal_scale=0.1, kind="complete",
                      num_samples=4)
    with pytest.raises(NotImplementedError, match="score of pf = 'paris'"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, sampler="pmala", proposal_scale=0.1, pf="paris")
    # a chain whose initial estimates are not finite is named (the Kalman launch: arithmetic only, a NaN observation)
    bad = _series("lgssm", 12).copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="pmala: the initial log-likelihood or score of chain 5 is not finite"):
        _ensemble("lgssm", bad, 4, kind="marginal", chain_offset=5)
    # the C ABI
    ctx = _capi.default_context()
    hy = prior_hyper("svm", _prior("svm"))
    th = torch.ones((4, _capi.MAX_THETA), dtype=torch.float64, device="cuda")
    tp, out = th.clone(), torch.zeros((4, _capi.OUT_DOUBLES), dtype=torch.float64, device="cuda")
    valid = torch.ones(4, dtype=torch.int32, device="cuda")
    ll, n = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    grad = torch.zeros((4, _capi.MAX_THETA), dtype=torch.float64, device="cuda")
    sc = torch.ones(_capi.MAX_THETA, dtype=torch.float64, device="cuda")
    prop = lambda model=0, B=4, **k: ctx.pmala_propose_device(      # noqa: E731
        model, B, k.get("theta", th.data_ptr()), k.get("grad", grad.data_ptr()), k.get("prop", tp.data_ptr()),
        k.get("valid", valid.data_ptr()), k.get("scale", sc.data_ptr()), k.get("hyper", hy), 1)
    acc = lambda model=0, B=4, **k: ctx.pmala_accept_device(        # noqa: E731
        model, B, k.get("theta", th.data_ptr()), k.get("prop", tp.data_ptr()), k.get("valid", valid.data_ptr()),
        k.get("outs", out.data_ptr()), k.get("ll", ll.data_ptr()), k.get("grad", grad.data_ptr()), k.get("n", n.data_ptr()),
        k.get("hyper", hy), k.get("scale", sc.data_ptr()), 0, 1)
    for call in (prop, acc):
        for model in (-1, 3):
            with pytest.raises(ValueError, match="Unrecognized model id"):
                call(model=model)
        with pytest.raises(ValueError, match="B must be >= 0"):
            call(B=-1)
        call(B=0)                                                   # nothing to do
    for call, kws in ((prop, ("theta", "grad", "prop", "valid", "scale", "hyper")),
                      (acc, ("theta", "prop", "valid", "outs", "ll", "grad", "n", "hyper", "scale"))):
        for k in kws:
            with pytest.raises(ValueError, match="NULL argument"):
                call(**{k: None})
    torch.cuda.synchronize()
    np.testing.assert_array_equal(th.cpu().numpy(), 1.0)            # no refused call wrote anything
    np.testing.assert_array_equal(tp.cpu().numpy(), 1.0)
    assert not n.cpu().numpy().any() and not grad.cpu().numpy().any() and not ll.cpu().numpy().any()
