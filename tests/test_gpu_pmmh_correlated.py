"""GPU: ChainEnsemble(sampler='pmmh', correlation=rho) -- whole steps against the host restatement (tests/helpers/cpm_model.py on
pmmh_model.py): the proposal of theta and of the normals, the estimate, the decision and what a chain keeps; eager against
hipGraph against resume against the rank partition; the checkpoint; and the exactness of the chain: with rho = 0.99 and N = 16
it samples the posterior that Metropolis-Hastings on the Kalman likelihood samples."""
import os
import sys

import numpy as np
import pytest

from test_host_logic import DATA_SEED, GEN, PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cpm_model as cp  # noqa: E402
import pmmh_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000C0DE4321
SCALE = {"svm": [0.3, 0.3, 0.3], "lgssm": [0.2, 1.0, 0.4, 0.4]}
PLAIN_KEYS = {"theta", "momentum", "step_ctr", "steps_done", "seed", "chain_offset", "model", "N", "C", "ess_threshold", "ll",
              "n_accept"}


def _series(model, T):
    np.random.seed(DATA_SEED[model])
    return GEN[model](T=T, parameters=default_params(model))["observations"].reshape(-1)


def _prior(model, var=1.0):
    return PRIORS[model].generate_default_prior(var=var, n=1, m=1)


def _ensemble(model, y, C, **kw):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    kw.setdefault("proposal_scale", SCALE[model])
    kw.setdefault("seed", SEED)
    kw.setdefault("N", 16)
    kw.setdefault("prior", _prior(model))
    kw.setdefault("correlation", 0.9)
    return ChainEnsemble(model, y, default_params(model), num_chains=C, sampler="pmmh", **kw)


def _state(e):
    e.synchronize()
    return dict(theta=e.theta_dev.cpu().numpy(), prop=e.theta_prop_dev.cpu().numpy(), valid=e.valid_dev.cpu().numpy(),
                out4=e.out_dev.cpu().numpy()[:, 4], ll=e.ll_dev.cpu().numpy(), n=e.accept_dev.cpu().numpy(),
                ctr=int(e.step_ctr.item()), aux=e.aux(), which=e.which_dev.cpu().numpy(), seen=e.seen_dev.cpu().numpy())


def _other_buffer(e):
    """[C, T+1, N+1]: the buffer each chain does NOT read -- after a step, the U' its filter ran on, accepted or not."""
    import torch
    rows = torch.arange(e.C, device=e.device)
    other = e._aux_view()[1 - (e.which_dev.long() & 1), rows]
    return other[:, :(e.T + 1) * (e.N + 1)].reshape(e.C, e.T + 1, e.N + 1).cpu().numpy()


def _same(a, b, keys=("theta", "ll", "n", "ctr", "aux", "seen")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- 1. whole steps against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,rho", [("svm", 16, 0.9), ("lgssm", 130, 0.5)])
def test_steps_match_the_restatement(model, N, rho):
    """C = 150 chains, T = 12, six eager steps, both launch shapes.  Each step is recomputed on the host from the device's state
    before it: the proposal of theta within TOL_ULPS, U' to 1e-15 (tests/test_gpu_cpm.py), the estimate on the device's own
    theta' and U' to 1e-9, the decision exact wherever |log u - log alpha| >= 1e-9.  A chain that accepts takes theta', the
    estimate and U', bitwise the device's; one that rejects keeps theta, ll AND U, bitwise -- no estimate is ever refreshed."""
    from sgmcmc_ssm_amd import _capi
    C, T, off = 150, 12, 2 ** 32 - 70
    prior, y = _prior(model), _series(model, 12)
    e = _ensemble(model, y, C, N=N, correlation=rho, chain_offset=off)
    P, useed = _capi.THETA_DIM[model], pm.update_seed(SEED)
    pmean, pvar = float(e._cpm_desc["prior_mean"][0]), float(e._cpm_desc["prior_var"][0])
    st = _state(e)
    # the init pass: rho = 0 at counter 0, every chain reads buffer 0 afterwards
    ll0, U0 = cp.chain_init(model, st["theta"][:, :P], y, T, N, pmean, pvar, SEED, off)
    assert st["ctr"] == 1 and not st["n"].any() and not st["which"].any() and not st["seen"].any()
    np.testing.assert_allclose(st["aux"], U0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(st["ll"], ll0, rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(st["ll"], st["out4"])
    seen = dict(accepted=0, rejected=0, skipped=0)
    for s in range(6):
        before = st
        e.step(1)
        st = _state(e)
        ran_on = _other_buffer(e)
        acc = (st["n"] - before["n"]).astype(np.int64) == 1
        # the U' every chain's filter ran on: where the chain accepted it is now current
        u_prop = np.where(acc[:, None, None], st["aux"], ran_on)
        ctr = pm.step_counter(s)
        assert before["ctr"] == ctr and st["ctr"] == ctr + 1
        m = cp.chain_step(model, prior, before["theta"][:, :P], before["ll"], before["aux"], SCALE[model], rho, y, pmean, pvar,
                          SEED, off, s)
        np.testing.assert_array_equal(st["valid"], m["valid"].astype(np.int32))
        np.testing.assert_allclose(st["prop"][:, :P], m["prop"], rtol=1e-14, atol=1e-14)
        scale = np.maximum(1.0, np.abs(before["aux"]) + np.abs(m["U_prop"]))
        assert np.all(np.abs(u_prop - m["U_prop"]) <= 1e-15 * scale)
        ll_dev_inputs = cp.loglik(model, st["prop"][:, :P], y, u_prop, pmean, pvar, F=np.longdouble)["ll"].astype(np.float64)
        np.testing.assert_allclose(st["out4"], ll_dev_inputs, rtol=1e-9, atol=1e-9)
        want, margin = pm.accept(model, prior, before["theta"][:, :P], st["prop"][:, :P], st["valid"], before["ll"], st["out4"],
                                 useed, off, ctr)
        sure = margin >= 1e-9
        np.testing.assert_array_equal(acc[sure], want[sure])
        np.testing.assert_array_equal(st["theta"][acc], st["prop"][acc])
        np.testing.assert_array_equal(st["ll"][acc], st["out4"][acc])
        np.testing.assert_array_equal(st["which"][acc], 1 - before["which"][acc])
        # a rejected step: the old theta, the old estimate, the old normals
        np.testing.assert_array_equal(st["theta"][~acc], before["theta"][~acc])
        np.testing.assert_array_equal(st["ll"][~acc], before["ll"][~acc])
        np.testing.assert_array_equal(st["aux"][~acc], before["aux"][~acc])
        np.testing.assert_array_equal(st["which"][~acc], before["which"][~acc])
        np.testing.assert_array_equal(st["seen"], st["n"])
        seen["accepted"] += int(acc.sum())
        seen["rejected"] += int((~acc).sum())
        seen["skipped"] += int((~sure).sum())
        print(model, "step", s, "accepted", int(acc.sum()), "min margin", float(margin.min()))
    assert seen["skipped"] <= 0.01 * 6 * C and seen["accepted"] > 0 and seen["rejected"] > 0, seen
    np.testing.assert_array_equal(e.acceptance_rate(), st["n"] / 6.0)
    np.testing.assert_array_equal(e.loglik(), st["ll"])


# ---- 2. eager, graph, resume, partition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N", [("svm", 16), ("lgssm", 200)])
def test_eager_graph_resume_partition(model, N):
    """C = 70, T = 12: 8 eager steps = 8 steps through graph_steps = 4 = 4 steps, a state_dict loaded into a fresh ensemble, 4
    more = two ensembles of 35 chains with chain_offset 0 and 35 -- bitwise, the normals, the estimates and the acceptance
    counts included (the launch shape depends on N alone, so both partitions run the same kernel)."""
    C, y = 70, _series(model, 12)
    a = _ensemble(model, y, C, N=N)
    a.step(8)
    ref = _state(a)
    assert 0 < ref["n"].sum() < 8 * C and ref["ctr"] == 9
    b = _ensemble(model, y, C, N=N)
    kept = b.run(8, thin=4, graph_steps=4)
    _same(ref, _state(b))
    np.testing.assert_array_equal(kept[-1], ref["theta"][:, :kept.shape[2]])
    assert b.steps_done == 8
    c = _ensemble(model, y, C, N=N)
    c.step(4)
    state = c.state_dict()
    d = _ensemble(model, y, C, N=N, seed=SEED)
    d.load_state_dict(state)
    np.testing.assert_array_equal(d.aux(), state["aux"])
    d.step(4)
    _same(ref, _state(d))
    halves = []
    for off in (0, 35):
        h = _ensemble(model, y, 35, N=N, chain_offset=off)
        h.step(8)
        halves.append(_state(h))
    for k in ("theta", "ll", "n", "aux"):
        np.testing.assert_array_equal(np.concatenate([halves[0][k], halves[1][k]]), ref[k], err_msg=k)


def test_rho_zero_is_a_pmmh_chain_with_fresh_normals():
    """correlation = 0: every step filters on eps alone, whatever the chain holds."""
    y = _series("svm", 12)
    e = _ensemble("svm", y, 40, correlation=0.0)
    e.step(3)
    st = _state(e)
    fresh, _ = cp.propose_u(None, 0.0, 12, 16, cp.filter_seed(SEED), list(range(40)), 3)
    acc_last = st["ll"] == st["out4"]
    np.testing.assert_allclose(_other_buffer(e)[~acc_last], fresh[~acc_last], rtol=0, atol=1e-14)
    np.testing.assert_allclose(st["aux"][acc_last], fresh[acc_last], rtol=0, atol=1e-14)


# ---- 3. the checkpoint -------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_refusals():
    y = _series("svm", 12)
    plain = _ensemble("svm", y, 4, correlation=None)
    assert set(plain.state_dict()) == PLAIN_KEYS and plain.correlation is None
    with pytest.raises(ValueError, match="correlation set"):
        plain.aux()
    e = _ensemble("svm", y, 4)
    e.step(2)
    state = e.state_dict()
    assert set(state) == PLAIN_KEYS | {"aux", "correlation", "T", "which", "seen"}
    assert state["aux"].shape == (4, 13, 17) and state["correlation"] == 0.9 and state["T"] == 12
    with pytest.raises(ValueError, match="checkpoint correlation = 0.9 does not match the ensemble \\(None\\)"):
        plain.load_state_dict(state)
    with pytest.raises(ValueError, match="checkpoint correlation = None does not match the ensemble \\(0.9\\)"):
        e.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="checkpoint correlation = 0.9 does not match the ensemble \\(0.5\\)"):
        _ensemble("svm", y, 4, correlation=0.5).load_state_dict(state)
    with pytest.raises(ValueError, match="checkpoint N = 16 does not match"):
        _ensemble("svm", y, 4, N=8).load_state_dict(state)
    with pytest.raises(ValueError, match="checkpoint T = 12"):
        _ensemble("svm", _series("svm", 9), 4).load_state_dict(state)
    with pytest.raises(NotImplementedError, match="pmmh_stat stays at its default"):      # refused before anything is allocated
        _ensemble("svm", y, 4, pmmh_stat="score")


# ---- 4. exactness -------------------------------------------------------------------------------------------------------------
EXACT = dict(T=20, C=4096, N=16, rho=0.99, burn=1000, scale=[0.15, 1.0, 0.3, 0.3], free=(0, 2, 3))


def test_correlated_and_kalman_chains_sample_the_same_posterior():
    """LGSSM, T = 20, 4096 chains from the same start with the same proposal_scale, the data, prior and scale of
    tests/test_gpu_pmmh.py's exactness test: sampler='pmmh' with correlation = 0.99 and N = 16 against kind='marginal' (plain
    Metropolis-Hastings on the Kalman likelihood).  After the burn-in, per free coordinate (A, LQinv, LRinv),
    |mean_cpm - mean_kf| <= 5 sqrt((var_cpm + var_kf) / C) over the chains' final states: the chains are independent, so the
    bound is the CLT's, not a tuned number.

    The burn-in, chosen before any run: theta's own burn-in is 100 steps with a margin of 4 in tests/test_gpu_pmmh.py (CPU_RUN
    there); the normals move by rho per ACCEPTED step, an autocorrelation time of 1 / (1 - rho) = 100 accepted steps, 250 to 300
    steps at the acceptance of 0.35 to 0.4 measured there -- 1000 steps are over three of those on top of theta's.  The normals
    start from N(0, I), which is their marginal under the extended target up to the weighting by the estimate's error."""
    T, C = EXACT["T"], EXACT["C"]
    np.random.seed(333)
    y = GEN["lgssm"](T=T, parameters=default_params("lgssm"))["observations"].reshape(-1)
    prior = _prior("lgssm", 100.0)
    final = {}
    for arm, kw in (("cpm", dict(kind="pf", N=EXACT["N"], correlation=EXACT["rho"])), ("kf", dict(kind="marginal", correlation=None))):
        e = _ensemble("lgssm", y, C, prior=prior, proposal_scale=EXACT["scale"], **kw)
        e.run(EXACT["burn"], thin=EXACT["burn"], graph_steps=50)
        final[arm] = e.theta()[:, EXACT["free"]]
        rate = e.acceptance_rate()
        print(arm, "mean", final[arm].mean(0), "var", final[arm].var(0, ddof=1), "acceptance", float(rate.mean()))
        assert 0.05 < rate.mean() < 0.9
    diff = np.abs(final["cpm"].mean(0) - final["kf"].mean(0))
    bound = 5.0 * np.sqrt((final["cpm"].var(0, ddof=1) + final["kf"].var(0, ddof=1)) / C)
    print("diff", diff, "bound", bound)
    assert np.all(diff <= bound), (diff, bound)
