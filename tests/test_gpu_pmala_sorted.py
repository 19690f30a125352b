"""GPU: ChainEnsemble(sampler='pmala_sorted') -- particle MALA along the score of the correlated or the sequential quasi-Monte
Carlo filter.  The init pass against correlated / SQMC PMMH at the same seed, whole steps draw for draw against the host
restatement (tests/helpers/sorted_score_model.py), eager against hipGraph against resume against the rank partition, the
accessors and the checkpoint, and the exactness of the chain: at N = 16 both arms sample the posterior plain MALA on the Kalman
score samples."""
import os
import sys

import numpy as np
import pytest

from test_host_logic import DATA_SEED, GEN, PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pmala_model as pa  # noqa: E402
import sorted_score_model as ss  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000C0DE4321
SCALE = {"svm": [0.3, 0.3, 0.3], "lgssm": [0.2, 1.0, 0.4, 0.4]}        # test_gpu_pmmh_correlated.py's
RHO = 0.9
# the step test: (model, filter, N, lambduh) -- both models under both filters, both launch shapes, both recursions.  STEP_SEED
# was chosen on the CPU (python tools/pmala_sorted_burnin_cpu.py --margins 0x5EED0000C0DE4321): with it the host chain's smallest
# |log u - log alpha| over the 18 chain-steps of every configuration is above 0.03, no proposal lies within rounding of the
# support's edge, and every configuration both accepts and rejects
STEP_CASES = [("svm", "cpm", 16, 1.0), ("lgssm", "cpm", 130, 0.95), ("svm", "sqmc", 16, 0.95), ("lgssm", "sqmc", 256, 1.0)]
STEP_C, STEP_T, STEP_STEPS, STEP_OFF = 6, 12, 3, 2 ** 32 - 3
STEP_SEED = SEED
PLAIN_KEYS = {"theta", "momentum", "step_ctr", "steps_done", "seed", "chain_offset", "model", "N", "C", "ess_threshold", "ll",
              "n_accept"}


def _series(model, T):
    np.random.seed(DATA_SEED[model])
    return GEN[model](T=T, parameters=default_params(model))["observations"].reshape(-1)


def _prior(model, var=1.0):
    return PRIORS[model].generate_default_prior(var=var, n=1, m=1)


def _ensemble(model, y, C, which="cpm", sampler="pmala_sorted", lam=None, **kw):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    kw.setdefault("proposal_scale", SCALE[model])
    kw.setdefault("seed", SEED)
    kw.setdefault("N", 16)
    kw.setdefault("prior", _prior(model))
    if which == "cpm":
        kw.setdefault("correlation", RHO)
    else:
        kw["sqmc"] = True
    if lam is not None and lam != 1.0:
        kw.update(pf="nemeth", lambduh=lam)
    return ChainEnsemble(model, y, default_params(model), num_chains=C, sampler=sampler, **kw)


def _state(e):
    e.synchronize()
    out = e.out_dev.cpu().numpy()
    st = dict(theta=e.theta_dev.cpu().numpy(), prop=e.theta_prop_dev.cpu().numpy(), valid=e.valid_dev.cpu().numpy(),
              out4=out[:, 4], outg=out[:, :4].copy(), ll=e.ll_dev.cpu().numpy(), n=e.accept_dev.cpu().numpy(),
              ctr=int(e.step_ctr.item()))
    if hasattr(e, "grad_cur_dev"):
        st["grad"] = e.grad_cur_dev.cpu().numpy()
    if e.correlation is not None:
        st.update(aux=e.aux(), which=e.which_dev.cpu().numpy(), seen=e.seen_dev.cpu().numpy())
    return st


def _other_buffer(e):
    """[C, T+1, N+1]: the buffer each chain does NOT read -- after a step, the U' its filter ran on, accepted or not."""
    import torch
    rows = torch.arange(e.C, device=e.device)
    other = e._aux_view()[1 - (e.which_dev.long() & 1), rows]
    return other[:, :(e.T + 1) * (e.N + 1)].reshape(e.C, e.T + 1, e.N + 1).cpu().numpy()


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k not in ("prop", "valid", "out4", "outg"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- 1. the init pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N", [("svm", 16), ("lgssm", 200)])
@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_init_pass_is_correlated_pmmhs(model, N, lam):
    """Under correlation the init pass leaves bitwise the ll and U of sampler='pmmh', correlation=rho at the same seed: the same
    filter seed, the same rho = 0 launch at counter 0, the same commit.  The score it leaves is the launch's out[0..3]."""
    y = _series(model, 12)
    a = _state(_ensemble(model, y, 40, "cpm", lam=lam, N=N, chain_offset=2 ** 32 - 20))
    b = _state(_ensemble(model, y, 40, "cpm", sampler="pmmh", N=N, chain_offset=2 ** 32 - 20))
    for k in ("ll", "aux", "which", "seen", "theta", "ctr"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(a["grad"], a["outg"])
    h = ss.H_DIM[model]
    assert np.all(np.isfinite(a["grad"])) and np.all(a["grad"][:, :h] != 0) and np.all(a["grad"][:, h:] == 0) and a["ctr"] == 1


@pytest.mark.parametrize("model,N", [("svm", 16), ("lgssm", 256)])
@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_init_pass_is_sqmc_pmmhs(model, N, lam):
    """Under sqmc=True the init loglik() equals that of sampler='pmmh', sqmc=True at the same seed, bitwise."""
    y = _series(model, 12)
    a = _ensemble(model, y, 40, "sqmc", lam=lam, N=N, chain_offset=2 ** 32 - 20)
    b = _ensemble(model, y, 40, "sqmc", sampler="pmmh", N=N, chain_offset=2 ** 32 - 20)
    np.testing.assert_array_equal(a.loglik(), b.loglik())
    st = _state(a)
    np.testing.assert_array_equal(st["grad"], st["outg"])
    assert np.all(np.isfinite(st["grad"])) and np.all(st["grad"][:, :ss.H_DIM[model]] != 0)


# ---- 2. whole steps against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,which,N,lam", STEP_CASES)
def test_steps_match_the_restatement(model, which, N, lam):
    """C = 6 chains whose ids straddle 2^32, T = 12, three eager steps.  Each step is recomputed on the host (chain_step) from the
    device's state before it and compared draw for draw: valid exact, theta' to 1e-14, U' to 1e-15 (tests/test_gpu_cpm.py), the
    proposal's ll to 1e-9 and its score to 1e-9 of the terms' magnitude, the decision exact -- no decision's margin may lie
    under 1e-9 on the chosen seed -- and what a chain keeps: an accepting chain takes theta', ll, the score and U' bitwise the
    device's, a rejecting one keeps all four bitwise."""
    from sgmcmc_ssm_amd import _capi
    C, T, off = STEP_C, STEP_T, STEP_OFF
    prior, y = _prior(model), _series(model, T)
    e = _ensemble(model, y, C, which, lam=lam, N=N, chain_offset=off, seed=STEP_SEED)
    hy, P, h = e.hyper, _capi.THETA_DIM[model], ss.H_DIM[model]
    rho = RHO if which == "cpm" else None
    desc = e._cpm_desc if which == "cpm" else e._sqmc_desc
    pmean, pvar = float(desc["prior_mean"][0]), float(desc["prior_var"][0])
    st = _state(e)
    ll0, g0, U0, mag0 = ss.chain_init(model, st["theta"][:, :P], y, N, pmean, pvar, STEP_SEED, off, lam, which == "cpm")
    np.testing.assert_allclose(st["ll"], ll0, rtol=1e-9, atol=1e-9)
    assert np.all(np.abs(st["grad"] - g0) <= 1e-9 * mag0)
    if which == "cpm":
        np.testing.assert_allclose(st["aux"], U0, rtol=0, atol=1e-14)
    seen = dict(accepted=0, rejected=0)
    for s in range(STEP_STEPS):
        before = st
        e.step(1)
        st = _state(e)
        acc = (st["n"] - before["n"]).astype(np.int64) == 1
        m = ss.chain_step(model, prior, hy, before["theta"][:, :P], before["ll"], before["grad"], before.get("aux"), SCALE[model], rho,
                          lam, y, N, pmean, pvar, STEP_SEED, off, s)
        assert not m["amb"].any(), "a proposal within rounding of the support's edge: choose another seed"
        print(model, which, "step", s, "accepted", int(acc.sum()), "min margin", float(m["margin"].min()),
              "score err / mag", float(np.max(np.abs(st["outg"] - m["grad_prop"])[:, :h] / m["mag_prop"][:, :h])))
        np.testing.assert_array_equal(st["valid"], m["valid"].astype(np.int32))
        np.testing.assert_allclose(st["prop"][:, :P], m["prop"], rtol=1e-14, atol=1e-14)
        if which == "cpm":
            u_prop = np.where(acc[:, None, None], st["aux"], _other_buffer(e))
            scale = np.maximum(1.0, np.abs(before["aux"]) + np.abs(m["U_prop"]))
            assert np.all(np.abs(u_prop - m["U_prop"]) <= 1e-15 * scale)
        np.testing.assert_allclose(st["out4"], m["ll_prop"], rtol=1e-9, atol=1e-9)
        assert np.all(np.abs(st["outg"] - m["grad_prop"]) <= 1e-9 * m["mag_prop"]) and np.all(st["outg"][:, h:] == 0)
        assert np.all(m["margin"] >= 1e-9), "a decision inside the model's tolerance: choose another seed"
        np.testing.assert_array_equal(acc, m["accepted"])
        np.testing.assert_allclose(st["theta"][:, :P], m["theta"], rtol=1e-14, atol=1e-14)
        np.testing.assert_allclose(st["ll"], m["ll"], rtol=1e-9, atol=1e-9)
        for k, new in (("theta", "prop"), ("ll", "out4"), ("grad", "outg")):
            np.testing.assert_array_equal(st[k][acc], st[new][acc], err_msg=k)
            np.testing.assert_array_equal(st[k][~acc], before[k][~acc], err_msg=k)
        if which == "cpm":
            np.testing.assert_array_equal(st["which"][acc], 1 - before["which"][acc])
            np.testing.assert_array_equal(st["which"][~acc], before["which"][~acc])
            np.testing.assert_array_equal(st["aux"][~acc], before["aux"][~acc])
            np.testing.assert_array_equal(st["seen"], st["n"])
        seen["accepted"] += int(acc.sum())
        seen["rejected"] += int((~acc).sum())
    assert seen["accepted"] > 0 and seen["rejected"] > 0, seen
    np.testing.assert_array_equal(e.acceptance_rate(), st["n"] / float(STEP_STEPS))
    np.testing.assert_array_equal(e.loglik(), st["ll"])
    np.testing.assert_array_equal(e.score(), st["grad"][:, :h])
    g, ll = e.last_gradient_statistics()                # the latest PROPOSALS' estimates
    np.testing.assert_array_equal(g, st["outg"][:, :h])
    np.testing.assert_array_equal(ll, st["out4"])


# ---- 3. eager, graph, resume, partition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,which,N,lam", [("svm", "cpm", 16, 0.95), ("lgssm", "cpm", 200, 1.0), ("lgssm", "sqmc", 16, 0.95),
                                               ("svm", "sqmc", 256, 1.0)])
def test_eager_graph_resume_partition(model, which, N, lam):
    """C = 70, T = 12: 6 eager steps = 6 steps through graph_steps = 3 = 3 steps, a state_dict loaded into a fresh ensemble, 3
    more = two ensembles of 35 chains with chain_offset 0 and 35 -- bitwise: theta, both estimates, the acceptance counts, the
    counter, and under correlation the normals and the selector's bookkeeping."""
    C, y = 70, _series(model, 12)
    kw = dict(lam=lam, N=N)
    a = _ensemble(model, y, C, which, **kw)
    a.step(6)
    ref = _state(a)
    assert 0 < ref["n"].sum() < 6 * C and ref["ctr"] == 7
    b = _ensemble(model, y, C, which, **kw)
    kept = b.run(6, thin=3, graph_steps=3)
    _same(ref, _state(b))
    np.testing.assert_array_equal(kept[-1], ref["theta"][:, :kept.shape[2]])
    assert b.steps_done == 6
    c = _ensemble(model, y, C, which, **kw)
    c.step(3)
    state = c.state_dict()
    extra = {"grad", "sampler", "lambduh"} | ({"aux", "correlation", "T", "which", "seen"} if which == "cpm" else {"sqmc"})
    assert set(state) == PLAIN_KEYS | extra and state["sampler"] == "pmala_sorted"
    d = _ensemble(model, y, C, which, **kw)
    d.load_state_dict(state)
    d.step(3)
    _same(ref, _state(d))
    halves = []
    for off in (0, 35):
        hf = _ensemble(model, y, 35, which, chain_offset=off, **kw)
        hf.step(6)
        halves.append(_state(hf))
    for k in ("theta", "ll", "grad", "n") + (("aux",) if which == "cpm" else ()):
        np.testing.assert_array_equal(np.concatenate([halves[0][k], halves[1][k]]), ref[k], err_msg=k)


def test_checkpoints_and_accessors_keep_to_their_sampler():
    """A 'pmala_sorted' checkpoint names its sampler and lambduh: neither a correlated PMMH ensemble nor one with another
    lambduh takes it, and it takes neither's; aux() belongs to the correlated arm; the PMMH checkpoints are what they were."""
    y = _series("lgssm", 12)
    a = _ensemble("lgssm", y, 4, "cpm", lam=0.95)
    a.step(2)
    state = a.state_dict()
    with pytest.raises(ValueError, match="checkpoint sampler = pmala_sorted does not match"):
        _ensemble("lgssm", y, 4, "cpm", sampler="pmmh").load_state_dict(state)
    with pytest.raises(ValueError, match="checkpoint lambduh = 0.95 does not match"):
        _ensemble("lgssm", y, 4, "cpm", lam=0.5).load_state_dict(state)
    with pytest.raises(ValueError, match="checkpoint correlation = 0.9 does not match"):
        _ensemble("lgssm", y, 4, "sqmc", lam=0.95).load_state_dict(state)
    m = _ensemble("lgssm", y, 4, "cpm", sampler="pmmh")
    assert set(m.state_dict()) == PLAIN_KEYS | {"aux", "correlation", "T", "which", "seen"}
    with pytest.raises(ValueError, match="checkpoint sampler = None does not match"):
        a.load_state_dict(m.state_dict())
    s = _ensemble("lgssm", y, 4, "sqmc")
    with pytest.raises(ValueError, match="aux\\(\\) belongs to sampler='pmmh' with correlation set"):
        s.aux()
    assert a.aux().shape == (4, 13, 17) and s.score().shape == (4, 4)
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    with pytest.raises(ValueError, match="takes exactly one of correlation=rho"):
        ChainEnsemble("lgssm", y, default_params("lgssm"), num_chains=4, N=16, sampler="pmala_sorted", proposal_scale=0.1)


# ---- 4. exactness ---------------------------------------------------------------------------------------------------------------
# scale, chains, series and the reference arm's burn-in: test_gpu_pmala.py's EXACT.  burn: the sorted arms at N = 16.  The host
# chain model shows that 200 steps do not suffice there (CPU_RUN below: under correlation = 0.99 the mean of LRinv is 8, 5 and 2.6
# standard errors under the posterior mean 1.2798 at steps 25, 50 and 100 -- theta waits for the normals, which move by
# sqrt(1 - rho^2) an accepted step -- and inside 2.5 from the checkpoint at step 200 on, as the SQMC arm is from step 25 on):
# four times that checkpoint, 800 steps
EXACT = dict(T=20, C=4096, N=16, rho=0.99, lam=0.95, scale=[0.2, 1.0, 0.3, 0.3], free=(0, 2, 3), ref_burn=200, burn=800)


def test_sorted_pmala_chains_sample_the_posterior_of_plain_mala():
    """LGSSM, T = 20, 4096 chains from the same start, prior var = 100, the series and start of test_gpu_pmala.py's exactness
    test.  Arms: sampler='pmala_sorted' with correlation = 0.99 and with sqmc=True, N = 16, pf='nemeth' (lambduh = 0.95), against
    the exact chain, sampler='pmala' with kind='marginal' (plain MALA on the Kalman score and likelihood).  Per free coordinate
    (A, LQinv, LRinv): |mean_a - mean_b| <= 5 sqrt((var_a + var_b) / C) over the chains' final states -- the chains are
    independent, so the bound is the CLT's, test_gpu_pmala.py's.  At N = 16 the score is biased (O(1 / N), self-normalised) and
    noisy; the chain is exact all the same, because the reverse proposal density uses the score of the launch at the proposal."""
    T, C = EXACT["T"], EXACT["C"]
    np.random.seed(333)
    y = GEN["lgssm"](T=T, parameters=default_params("lgssm"))["observations"].reshape(-1)
    prior = _prior("lgssm", 100.0)
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    final = {}
    ref = ChainEnsemble("lgssm", y, default_params("lgssm"), num_chains=C, sampler="pmala", kind="marginal", prior=prior, seed=SEED,
                        proposal_scale=EXACT["scale"])
    ref.run(EXACT["ref_burn"], thin=EXACT["ref_burn"], graph_steps=50)
    final["pmala-kf"] = ref.theta()[:, EXACT["free"]]
    print("pmala-kf", "mean", final["pmala-kf"].mean(0), "var", final["pmala-kf"].var(0, ddof=1), "acceptance",
          float(ref.acceptance_rate().mean()))
    for arm, which in (("sorted-cpm", "cpm"), ("sorted-sqmc", "sqmc")):
        e = _ensemble("lgssm", y, C, which, lam=EXACT["lam"], N=EXACT["N"], prior=prior, proposal_scale=EXACT["scale"],
                      **(dict(correlation=EXACT["rho"]) if which == "cpm" else {}))
        e.run(EXACT["burn"], thin=EXACT["burn"], graph_steps=50)
        final[arm] = e.theta()[:, EXACT["free"]]
        rate = float(e.acceptance_rate().mean())
        print(arm, "mean", final[arm].mean(0), "var", final[arm].var(0, ddof=1), "acceptance", rate)
        assert 0.05 < rate < 0.9, (arm, rate)
    for arm in ("sorted-cpm", "sorted-sqmc"):
        diff = np.abs(final[arm].mean(0) - final["pmala-kf"].mean(0))
        bound = 5.0 * np.sqrt((final[arm].var(0, ddof=1) + final["pmala-kf"].var(0, ddof=1)) / C)
        print(arm, "diff", diff, "bound", bound)
        assert np.all(diff <= bound), (arm, diff, bound)


CPU_RUN = """
# scale [0.2, 1.0, 0.3, 0.3] T 20 N 16 steps 400 rho 0.99 lambduh 0.95   (python tools/pmala_sorted_burnin_cpu.py --chains 512;
# means of A, LQinv, LRinv; the posterior means test_gpu_pmmh.py measured on 4096 chains: 0.7609, 1.0724, 1.2798)
cpm   C  512 step   25  mean [0.7562 1.079  1.1594]  se [0.0069 0.0138 0.0143]  var [0.0247 0.0973 0.1049]
cpm   C  512 step   50  mean [0.7531 1.0776 1.1999]  se [0.007  0.0136 0.0155]  var [0.0251 0.0942 0.1226]
cpm   C  512 step  100  mean [0.7527 1.0568 1.2387]  se [0.0077 0.0125 0.016 ]  var [0.0306 0.0803 0.1314]
cpm   C  512 step  200  mean [0.7492 1.0467 1.2803]  se [0.0071 0.012  0.0154]  var [0.0255 0.0738 0.1213]
cpm   C  512 step  300  mean [0.7511 1.0313 1.294 ]  se [0.0072 0.0125 0.0164]  var [0.0265 0.0805 0.1376]
cpm   C  512 step  400  mean [0.7576 1.077  1.2496]  se [0.007  0.0126 0.0148]  var [0.0252 0.0811 0.1124]
cpm   acceptance 0.310
sqmc  C  512 step   25  mean [0.7623 1.0697 1.2653]  se [0.0066 0.0118 0.0151]  var [0.022  0.0713 0.1169]
sqmc  C  512 step   50  mean [0.7491 1.0605 1.2973]  se [0.0067 0.012  0.0153]  var [0.0231 0.0734 0.1196]
sqmc  C  512 step  100  mean [0.7449 1.0666 1.2902]  se [0.0074 0.0121 0.0156]  var [0.0279 0.0754 0.1241]
sqmc  C  512 step  200  mean [0.7506 1.0665 1.2764]  se [0.0073 0.012  0.0146]  var [0.0273 0.0743 0.1086]
sqmc  C  512 step  300  mean [0.7534 1.0597 1.2741]  se [0.0068 0.0134 0.015 ]  var [0.0239 0.0923 0.1154]
sqmc  C  512 step  400  mean [0.7599 1.0599 1.3036]  se [0.0068 0.0121 0.0165]  var [0.0236 0.0749 0.1398]
sqmc  acceptance 0.328
"""
