"""GPU: density-tempered SMC over resident PMMH chains -- the population kernels (csrc/pfg_smc.hip) and the tempered accept
(csrc/pfg_chains.hip) against the long-double model (tests/helpers/smc_model.py), a stage and a run of TemperedPopulation
against that model driven with the device's own estimates, eager against resumed, and the exactness of the law on the device
against the quadrature of tests/test_smc_host.py."""
import os
import sys

import numpy as np
import pytest

from test_host_logic import DATA_SEED, GEN, PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pmmh_model as pm  # noqa: E402
import smc_model as sm  # noqa: E402

from test_smc_host import EXACT, quadrature  # noqa: E402

pytestmark = pytest.mark.gpu

LD = sm.LD
SEED = 0x5EED0000C0DE4321
SHAPES = [2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 4097, 70001]
PATTERNS = ("spread", "near_equal", "dominant", "minus_inf_block", "last_stage")
GAP = 1e-12          # a child whose target lies within GAP * W of a CDF entry may take either neighbour


def population_case(B, pattern):
    """(h [B], phi, tau) of one weight pattern.  spread: several stages' worth of spread at phi = 0; near_equal:
    ESS(1) >= tau B at phi = 0, a single stage; dominant: one chain 1000 above the others and tau = 0.9 / B, so the step is
    the whole distance and every child comes from that chain; minus_inf_block: a block of degenerate estimates; last_stage:
    phi already at 0.999."""
    rng = np.random.default_rng([B, PATTERNS.index(pattern)])
    h = rng.normal(scale=5.0, size=B) - 40.0
    phi, tau = 0.0, 0.5
    if pattern == "near_equal":
        h = rng.normal(scale=1e-3, size=B) + 3.0
    elif pattern == "dominant":
        h = rng.normal(size=B)
        h[(2 * B) // 3] += 1000.0
        tau = 0.9 / B
    elif pattern == "minus_inf_block":
        h[B // 3:max(B // 2, B // 3 + 1)] = -np.inf
    elif pattern == "last_stage":
        phi = 0.999
    return h, phi, tau


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def run_temper(h, phi, tau, seed, stage):
    """pfg_smc_temper_device on h -> dict(status, result [8], parent [B], cdf [B], phi); every output starts from a sentinel."""
    import torch
    from sgmcmc_ssm_amd import _capi
    B = len(h)
    dev = torch.device("cuda", 0)
    h_dev = torch.from_numpy(np.asarray(h, dtype=np.float64)).to(dev)
    phi_dev = torch.full((1,), float(phi), dtype=torch.float64, device=dev)
    result = torch.full((_capi.SMC_RESULT_DOUBLES,), -7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    parent = torch.full((B,), -1, dtype=torch.int32, device=dev)
    cdf = torch.full((max(_capi.smc_scratch_bytes(B), 8) // 8,), -7.0, dtype=torch.float64, device=dev)
    _ctx().smc_temper_device(B, h_dev.data_ptr(), phi_dev.data_ptr(), tau, seed, stage, result.data_ptr(), status.data_ptr(),
                             parent.data_ptr(), cdf.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return dict(status=int(status.item()), result=result.cpu().numpy(), parent=parent.cpu().numpy().astype(np.int64),
                cdf=cdf.cpu().numpy()[:B], phi=float(phi_dev.item()))


def _untouched(out, phi):
    return np.all(out["result"] == -7.0) and np.all(out["parent"] == -1) and np.all(out["cdf"] == -7.0) and out["phi"] == phi


# ---- 5. the population kernels on synthetic h -----------------------------------------------------------------------------
@pytest.mark.parametrize("B", SHAPES)
def test_temper_kernel_matches_the_model(B):
    """Every weight pattern at one population size: one chain per thread (B <= 1024), the 1 -> 2 chains-per-thread switch
    (1025), a ragged last thread and idle threads (2049 = 3 x 683, 4097, 70001 = 69 x 1014 + 35).  phi' and delta agree with the
    long-double model to 1e-10 relative, the evidence increment and the ESS to 1e-9, the uniform is the keyed one, every
    parent is the one the model's search selects on the model's CDF -- a child whose target lies within 1e-12 W of a CDF
    entry is exempt, at most 1 child in 1000 -- offspring counts are floor or ceil of B p_i and parents do not decrease.
    On the CPU the model alone leaves out no child at all in any of the 55 cases (the count is printed)."""
    for k, pattern in enumerate(PATTERNS):
        h, phi, tau = population_case(B, pattern)
        stage = 3 + k + (1 << 33) * (k % 2)                 # the high word of the stage takes part in the key
        u = sm.stage_uniform(SEED, stage)
        want = sm.temper(h, phi, tau, u)
        got = run_temper(h, phi, tau, SEED, stage)
        assert want["status"] == 0 and got["status"] == 0, (pattern, want["status"], got["status"])
        phi_new, delta, incr, ess, u_dev, W, hmax, _ = got["result"]
        assert got["phi"] == phi_new and u_dev == float(u) and hmax == float(want["hmax"])
        rel = lambda a, b: abs(LD(a) - b) / max(abs(b), LD(1e-300))
        print(B, pattern, "phi'", phi_new, "delta", delta, "ess", ess, "rel", float(rel(delta, want["delta"])),
              float(rel(ess, want["ess"])), "exempt", int((want["gap"] <= GAP).sum()))
        assert rel(phi_new, want["phi_new"]) <= 1e-10 and rel(delta, want["delta"]) <= 1e-10
        assert rel(incr, want["increment"]) <= 1e-9 and rel(ess, want["ess"]) <= 1e-9 and rel(W, want["W"]) <= 1e-12
        if want["last"]:
            assert phi_new == 1.0 and delta == 1.0 - phi
        else:
            assert ess >= tau * B * (1 - 1e-12)
        sure = want["gap"] > GAP
        assert (~sure).sum() <= B / 1000.0
        np.testing.assert_array_equal(got["parent"][sure], want["parent"][sure])
        assert np.all(np.diff(got["parent"]) >= 0) and got["parent"].min() >= 0 and got["parent"].max() < B
        w = sm.weights(h, want["hmax"], want["delta"])
        expect = (w / want["W"] * B).astype(float)
        counts = np.bincount(got["parent"], minlength=B)
        assert np.all(counts >= np.floor(expect - 1e-6)) and np.all(counts <= np.ceil(expect + 1e-6))
        assert np.max(np.abs(got["cdf"].astype(LD) - want["cdf"])) <= 1e-12 * want["W"]
        if pattern == "dominant":
            assert np.all(got["parent"] == (2 * B) // 3)
        if pattern == "minus_inf_block":
            assert not counts[np.isneginf(h)].any()
        if pattern == "near_equal":
            assert want["last"] and phi == 0.0          # ESS(1) >= tau B at phi = 0: a single stage


def test_temper_kernel_flags_and_errors():
    """All -inf, a NaN, +inf, phi = 1 and a population that admits no step set the status and store nothing else; B = 1 and
    B = 2^20 + 1 are an error status of the call and no launch."""
    for h, phi, flag in ((np.full(300, -np.inf), 0.0, sm.NO_FINITE), (np.r_[np.zeros(1500), np.nan], 0.0, sm.NOT_A_NUMBER),
                         (np.r_[np.inf, np.zeros(70)], 0.2, sm.NOT_A_NUMBER), (np.zeros(64), 1.0, sm.BAD_PHI),
                         (np.r_[0.0, np.full(1030, -np.inf)], 0.0, sm.ZERO_STEP)):
        assert sm.temper(h, phi, 0.5, 0.5)["status"] == flag
        got = run_temper(h, phi, 0.5, SEED, 0)
        assert got["status"] == flag and _untouched(got, phi), (flag, got)
    for B in (1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="2 <= B <= 2\\^20"):            # PFG_ERR_INVALID
            run_temper(np.zeros(B), 0.0, 0.5, SEED, 0)
    with pytest.raises(ValueError, match="ess_target"):
        run_temper(np.zeros(8), 0.0, 1.0, SEED, 0)


# ---- 6. gather and scale ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 257, 70001])
def test_gather_and_scale(B):
    """The gather equals theta[parent], ll[parent] bitwise -- identity, one parent for all, long runs, the parents of a real
    stage, an out-of-range entry (the chain stays) --; the scale equals the long-double two-pass value to 1e-12, a zero-sd
    slot keeps its scale and a slot outside the mask (LGSSM's C) is untouched."""
    import torch
    from sgmcmc_ssm_amd import _capi
    dev = torch.device("cuda", 0)
    ctx, st = _ctx(), torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(B)
    theta = rng.normal(size=(B, 4)) * [0.3, 1.0, 2.0, 1e-3] + [0.5, 1.0, -3.0, 1e6]
    ll = rng.normal(size=B) * 10
    ll[B // 2] = -np.inf
    runs = np.sort(rng.integers(0, B, size=max(B // 50, 1)))
    real = run_temper(*population_case(B, "spread"), SEED, 1)["parent"] if B > 2 else np.array([1, 1])
    for name, parent in (("identity", np.arange(B)), ("one", np.full(B, B - 1)), ("runs", np.sort(rng.choice(runs, size=B))),
                         ("stage", real), ("bad", np.r_[np.int64(-1), np.full(B - 1, B)])):
        th_dev, ll_dev = torch.from_numpy(theta).to(dev), torch.from_numpy(ll).to(dev)
        tmp, ll_tmp = torch.zeros_like(th_dev), torch.zeros_like(ll_dev)
        par = torch.from_numpy(parent.astype(np.int32)).to(dev)
        ctx.smc_gather_device(B, par.data_ptr(), th_dev.data_ptr(), ll_dev.data_ptr(), tmp.data_ptr(), ll_tmp.data_ptr(), st)
        torch.cuda.synchronize(dev)
        src = np.arange(B) if name == "bad" else parent
        np.testing.assert_array_equal(th_dev.cpu().numpy(), theta[src], err_msg=name)
        np.testing.assert_array_equal(ll_dev.cpu().numpy(), ll[src], err_msg=name)
    th = theta.copy()
    th[:, 0] = 0.25                                      # a slot with no spread at all
    th_dev = torch.from_numpy(th).to(dev)
    for model in ("svm", "lgssm", "garch"):
        prev = np.array([0.11, 0.22, 0.33, 0.44])
        sc = torch.from_numpy(prev.copy()).to(dev)
        ctx.smc_scale_device(B, th_dev.data_ptr(), _capi.PMMH_MOVING_SLOTS[model], 1.37, sc.data_ptr(), st)
        torch.cuda.synchronize(dev)
        got, want = sc.cpu().numpy(), sm.scale(th, "garch", 1.37, prev)       # (every slot; the mask picks below)
        for j in range(4):
            if j == 0 or j not in sm.MOVING[model]:
                assert got[j] == prev[j], (model, j)       # zero sd, or not a slot of the mask: bitwise the previous scale
            else:
                assert abs(LD(got[j]) - want[j]) <= 1e-12 * want[j], (model, j, got[j], float(want[j]))


# ---- 7. the tempered accept -------------------------------------------------------------------------------------------------
def _accept_case(model, C=300):
    """A synthetic PMMH state in the middle of a step: theta from q0, proposals from pfg_pmmh_propose_device at a scale that
    leaves some outside the support, estimates with NaN, +inf and -inf among them, counter value 5."""
    import torch
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.ensemble import prior_hyper
    dev = torch.device("cuda", 0)
    P = _capi.THETA_DIM[model]
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    mean = np.zeros(4)
    mean[:P] = default_params(model).theta()
    sd = np.array([0.3, 0.3, 0.3, 0.3])
    theta = np.zeros((C, 4))
    theta[:, :P] = sm.initial_population(model, C, 11, mean, sd)
    rng = np.random.default_rng(C + P)
    ll_cur = rng.normal(size=C) * 3 - 20
    out = np.zeros((C, _capi.OUT_DOUBLES))
    out[:, 4] = ll_cur + rng.normal(size=C) * 2
    out[3, 4], out[40, 4], out[77, 4], out[150, 4] = np.nan, np.inf, -np.inf, -np.inf
    ll_cur[200] = -np.inf
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    s = dict(model=model, C=C, P=P, prior=prior, hyper=prior_hyper(model, prior), hy=sm.hyper_of(model, prior), mean=mean, sd=sd,
             theta=theta, ll=ll_cur, out=out, ctr=5, useed=pm.update_seed(SEED), dev=dev)
    scale = t(np.array([0.6, 0.5, 0.9, 2.0]))
    s["theta_dev"], s["prop_dev"], s["valid_dev"] = t(theta), t(theta), torch.zeros(C, dtype=torch.int32, device=dev)
    s["ctr_dev"] = torch.full((1,), 5, dtype=torch.int64, device=dev)
    _ctx().pmmh_propose_device(model, C, s["theta_dev"].data_ptr(), s["prop_dev"].data_ptr(), s["valid_dev"].data_ptr(),
                               scale.data_ptr(), s["useed"], 0, s["ctr_dev"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    s["prop"], s["valid"] = s["prop_dev"].cpu().numpy(), s["valid_dev"].cpu().numpy()
    s["mean_dev"], s["sd_dev"] = t(mean), t(sd)
    return s


def _run_accept(s, phi):
    """(theta, ll, n_accept, counter, log_alpha) after pfg_smc_accept_device at phi (None: pfg_pmmh_accept_device)."""
    import torch
    dev, C = s["dev"], s["C"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    th, ll, out, n = t(s["theta"]), t(s["ll"]), t(s["out"]), torch.zeros(C, dtype=torch.int64, device=dev)
    ctr = torch.full((1,), s["ctr"], dtype=torch.int64, device=dev)
    la = torch.full((C,), -7.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    if phi is None:
        _ctx().pmmh_accept_device(s["model"], C, th.data_ptr(), s["prop_dev"].data_ptr(), s["valid_dev"].data_ptr(), out.data_ptr(),
                                  ll.data_ptr(), n.data_ptr(), s["hyper"], 0, s["useed"], 0, ctr.data_ptr(), st)
    else:
        phi_dev = torch.full((1,), float(phi), dtype=torch.float64, device=dev)
        _ctx().smc_accept_device(s["model"], C, th.data_ptr(), s["prop_dev"].data_ptr(), s["valid_dev"].data_ptr(), out.data_ptr(),
                                 ll.data_ptr(), n.data_ptr(), s["hyper"], s["mean_dev"].data_ptr(), s["sd_dev"].data_ptr(),
                                 phi_dev.data_ptr(), la.data_ptr(), s["useed"], 0, ctr.data_ptr(), st)
    torch.cuda.synchronize(dev)
    return th.cpu().numpy(), ll.cpu().numpy(), n.cpu().numpy(), int(ctr.item()), la.cpu().numpy()


@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_tempered_accept(model):
    """phi = 1: theta, the estimates, the counts and the counter are pfg_pmmh_accept_device's bit for bit, invalid proposals and
    non-finite estimates included.  phi in {0, 0.37}: log alpha agrees with the long-double model to 1e-12 and every decision
    is the model's; a decision within 1e-12 of log u is exempt, at most 1 in 1000 (expected: none)."""
    s = _accept_case(model)
    assert (s["valid"] == 0).sum() > 5 and (s["valid"] == 1).sum() > 100
    plain, hot = _run_accept(s, None), _run_accept(s, 1.0)
    for a, b, what in zip(plain[:4], hot[:4], ("theta", "ll", "n_accept", "counter")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    assert plain[3] == 6 and 0 < plain[2].sum() < s["C"]
    for phi in (0.0, 0.37):
        th, ll, n, ctr, la = _run_accept(s, phi)
        acc, margin, want = sm.accept(model, s["hy"], s["theta"][:, :s["P"]], s["prop"][:, :s["P"]], s["valid"], s["ll"], s["out"][:, 4],
                                      s["mean"], s["sd"], phi, s["useed"], 0, s["ctr"])
        nan = np.isnan(want.astype(float))
        np.testing.assert_array_equal(np.isnan(la), nan)
        inf = np.isinf(want.astype(float))
        np.testing.assert_array_equal(la[inf], want.astype(float)[inf])
        fin = ~nan & ~inf
        err = np.abs(la[fin].astype(LD) - want[fin])
        print(model, phi, "log alpha err", float(err.max()), "min margin", float(margin.min()), "accepted", int(n.sum()))
        assert err.max() <= 1e-12
        sure = margin >= 1e-12
        assert (~sure).sum() <= s["C"] / 1000.0
        np.testing.assert_array_equal((n == 1)[sure], acc[sure])
        a = n == 1
        assert set(np.unique(n)) <= {0, 1} and ctr == 6 and a.any() and (~a).any()
        np.testing.assert_array_equal(th[a], s["prop"][a])
        np.testing.assert_array_equal(ll[a], s["out"][a, 4])
        np.testing.assert_array_equal(th[~a], s["theta"][~a])
        np.testing.assert_array_equal(ll[~a], s["ll"][~a])
        assert not (a & (s["valid"] == 0)).any() and not (a & ~np.isfinite(s["out"][:, 4])).any()


# ---- 8. a stage and a run against the host model ------------------------------------------------------------------------------
CONFIGS = [("svm", dict()), ("garch", dict(resampling="stratified")), ("lgssm", dict(kind="marginal"))]


def _series(model, T):
    np.random.seed(DATA_SEED[model])
    return GEN[model](T=T, parameters=default_params(model))["observations"].reshape(-1)


def _population(model, kw, C=257, moves=1, **more):
    from sgmcmc_ssm_amd.tempering import TemperedPopulation
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    return TemperedPopulation(model, _series(model, 12), default_params(model), num_chains=C, N=16, seed=SEED, prior=prior,
                              moves=moves, **kw, **more), prior


def _snapshot(pop):
    e = pop.ensemble
    e.synchronize()
    return dict(theta=e.theta_dev.cpu().numpy(), ll=e.ll_dev.cpu().numpy(), ctr=int(e.step_ctr.item()),
                scale=e.scale_dev.cpu().numpy(), prop=e.theta_prop_dev.cpu().numpy(), valid=e.valid_dev.cpu().numpy(),
                out4=e.out_dev.cpu().numpy()[:, 4], n=pop.accept_dev.cpu().numpy(), parent=pop.parent_dev.cpu().numpy().astype(np.int64),
                h=pop.h_dev.cpu().numpy())


@pytest.mark.parametrize("model, kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_stages_match_the_host_model(model, kw):
    """C = 257, N = 16, T = 12, moves = 1, stage by stage to phi = 1: from the device's state before a stage the model gives h (to
    1e-12 relative), phi' and delta (1e-10), the parents (exempt: a target within 1e-12 W of a CDF entry), the scale (1e-12), the
    proposals (pmmh_model's tolerance) and, from the device's own proposals and estimates, every decision (exempt: within
    1e-12 of log u).  The ensemble's own accept counts and steps_done stay 0; the counter advances once per move."""
    pop, prior = _population(model, kw)
    e, P, hy, useed = pop.ensemble, pm.P_DIM[model], sm.hyper_of(model, prior), pm.update_seed(SEED)
    np.testing.assert_array_equal(e.theta()[:, :P], sm.initial_population(model, 257, SEED, pop.q0_mean, pop.q0_sd))
    st = _snapshot(pop)
    assert st["ctr"] == 1 and np.all(np.isfinite(st["ll"]))
    skipped = 0
    while pop.phi < 1.0:
        before, phi = st, pop.phi
        assert pop.stage(1) == 1 and pop.stage_index <= 60
        st = _snapshot(pop)
        h = sm.log_target(model, hy, before["theta"][:, :P], before["ll"], pop.q0_mean, pop.q0_sd)
        assert np.max(np.abs(st["h"].astype(LD) - h) / np.maximum(np.abs(h), 1)) <= 1e-12
        want = sm.temper(st["h"], phi, pop.ess_target, sm.stage_uniform(SEED, pop.stage_index - 1))
        sched = pop.schedule()
        assert abs(LD(pop.phi) - want["phi_new"]) <= 1e-10 * want["phi_new"] and sched["phi"][-1] == pop.phi
        assert abs(LD(sched["delta"][-1]) - want["delta"]) <= 1e-10 * want["delta"]
        assert abs(LD(sched["increment"][-1]) - want["increment"]) <= 1e-9 * abs(want["increment"])
        sure = want["gap"] > GAP
        np.testing.assert_array_equal(st["parent"][sure], want["parent"][sure])
        theta_g, ll_g = before["theta"][st["parent"]], before["ll"][st["parent"]]
        sc = sm.scale(theta_g[:, :P], model, pop.scale_factor, before["scale"][:P])
        assert np.all(np.abs(st["scale"][:P].astype(LD) - sc) <= 1e-12 * sc)
        np.testing.assert_array_equal(sched["scale"][-1], st["scale"][:P])
        ctr = before["ctr"]
        assert st["ctr"] == ctr + 1
        pr = pm.propose(model, theta_g, st["scale"], useed, 0, ctr)
        assert not pr.amb.any()
        np.testing.assert_array_equal(st["valid"], pr.valid.astype(np.int32))
        assert np.all(np.abs(st["prop"][:, :P].astype(LD) - pr.theta_prop) <= pr.tol)
        acc, margin, _ = sm.accept(model, hy, theta_g[:, :P], st["prop"][:, :P], st["valid"], ll_g, st["out4"], pop.q0_mean, pop.q0_sd,
                                   pop.phi, useed, 0, ctr)
        ok = margin >= 1e-12
        got = (st["n"] - before["n"]) == 1
        np.testing.assert_array_equal(got[ok], acc[ok])
        skipped += int((~ok).sum()) + int((~sure).sum())
        np.testing.assert_array_equal(st["theta"][got], st["prop"][got])
        np.testing.assert_array_equal(st["theta"][~got], theta_g[~got])
        np.testing.assert_array_equal(st["ll"][~got], ll_g[~got])
        assert abs(sched["acceptance"][-1] - got.mean()) < 1e-15
        print(model, "stage", pop.stage_index, "phi", pop.phi, "ess", sched["ess"][-1], "accepted", int(got.sum()))
    assert pop.phi == 1.0 and skipped == 0
    assert e.steps_done == 0 and not e.accept_dev.any().item()
    assert abs(pop.log_evidence() - (sum(pop.schedule()["increment"]) + sm.log_q0_mass(model, pop.q0_mean, pop.q0_sd))) < 1e-12


@pytest.mark.parametrize("model, kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_resumed_run_is_the_uninterrupted_one(model, kw):
    """moves = 2: a run to phi = 1 against one stopped after its first stage, checkpointed, loaded into a fresh population and
    continued -- theta, the estimates, the counter, the scale, the schedule and the evidence are bitwise equal; a checkpoint of
    another q0, tau or moves is refused."""
    whole, _ = _population(model, kw, moves=2)
    info = whole.temper()
    first, _ = _population(model, kw, moves=2)
    first.stage(1)
    state = first.state_dict()
    assert set(state) - {"tempering"} == set(first.ensemble.state_dict())
    resumed, _ = _population(model, kw, moves=2)
    resumed.load_state_dict(state)
    resumed.temper()
    a, b = _snapshot(whole), _snapshot(resumed)
    for k in ("theta", "ll", "ctr", "scale", "n"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    again = resumed.schedule()
    for k in info:
        np.testing.assert_array_equal(info[k], again[k], err_msg=k)
    assert whole.log_evidence() == resumed.log_evidence() and whole.stage_index == resumed.stage_index
    assert a["ctr"] == 1 + 2 * whole.stage_index
    for other in (dict(init_sd=0.4), dict(ess_target=0.6), dict(moves=3)):
        wrong, _ = _population(model, kw, **{**dict(moves=2), **other})
        with pytest.raises(ValueError, match="does not match the population"):
            wrong.load_state_dict(state)


# ---- 9. exactness on the device -------------------------------------------------------------------------------------------------
def _device_runs(C, **kw):
    from sgmcmc_ssm_amd.tempering import TemperedPopulation
    prior = PRIORS["lgssm"].generate_default_prior(var=EXACT["prior_var"], n=1, m=1)
    lz, means, pops = [], [], []
    for seed in range(EXACT["seeds"]):
        pop = TemperedPopulation("lgssm", np.array(EXACT["y"]), default_params("lgssm"), num_chains=C, seed=seed, prior=prior,
                                 init_mean=EXACT["q0_mean"], init_sd=EXACT["q0_sd"], ess_target=EXACT["tau"], moves=EXACT["moves"], **kw)
        pop.temper()
        lz.append(pop.log_evidence())
        means.append(pop.ensemble.theta()[:, list(EXACT["free"])].mean(0))
        pops.append(pop)
    return np.array(lz), np.array(means), pops


def _inside(values, truth, what):
    se = values.std(0, ddof=1) / np.sqrt(len(values))
    ratio = np.abs(values.mean(0) - truth) / (5.0 * se)
    print(what, values.mean(0), "+-", se, "against", truth, "ratio to the bound", ratio)
    assert np.all(ratio <= 1.0), (what, ratio)


def test_exactness_with_the_kalman_likelihood():
    """The CPU setup of test_smc_host.py (LGSSM, T = 8, the same series, prior and q0) with kind='marginal', C = 4096 and 16
    seeds: the mean of log Z-hat and the pooled posterior means lie within 5 standard errors, taken across the seeds, of the
    quadrature's.  Afterwards the ensemble is a plain PMMH ensemble: run(20, graph_steps=5) equals 20 eager steps of a twin
    bitwise, and acceptance_rate() counts those 20 steps alone.

    Observed on the MI355X: log Z-hat -17.0107 +- 0.0057 against -17.0094, 0.04 of the bound; the means of (A, LQinv, LRinv) at
    0.25, 0.20 and 0.37 of theirs."""
    logz, means, _ = quadrature(48)
    lz, m, pops = _device_runs(4096, kind="marginal")
    _inside(lz, logz, "log Z-hat")
    _inside(m, means, "means")
    from sgmcmc_ssm_amd.tempering import TemperedPopulation
    prior = PRIORS["lgssm"].generate_default_prior(var=EXACT["prior_var"], n=1, m=1)
    twin = TemperedPopulation("lgssm", np.array(EXACT["y"]), default_params("lgssm"), num_chains=4096, seed=0, prior=prior,
                              init_mean=EXACT["q0_mean"], init_sd=EXACT["q0_sd"], ess_target=EXACT["tau"], moves=EXACT["moves"],
                              kind="marginal")
    twin.temper()
    a, b = pops[0].ensemble, twin.ensemble
    np.testing.assert_array_equal(a.theta(), b.theta())
    np.testing.assert_array_equal(a.proposal_scale, a.scale_dev.cpu().numpy())
    a.run(20, thin=20, graph_steps=5)
    b.step(20)
    np.testing.assert_array_equal(a.theta(), b.theta())
    np.testing.assert_array_equal(a.loglik(), b.loglik())
    assert a.steps_done == 20
    np.testing.assert_array_equal(a.acceptance_rate(), a.accept_dev.cpu().numpy() / 20.0)
    np.testing.assert_array_equal(a.acceptance_rate(), b.acceptance_rate())
    assert 0.05 < a.acceptance_rate().mean() < 0.9


def test_exactness_with_a_particle_filter():
    """The same with kind='pf', N = 64 particles: the pooled posterior means inside their bounds.  log Z-hat of a noisy
    likelihood estimate is reported, not asserted: the estimate of Z is unbiased, so its logarithm carries a Jensen bias.

    Observed on the MI355X: the means at 0.07, 0.004 and 0.18 of their bounds; log Z-hat -17.0106 +- 0.0060 against -17.0094
    (at T = 8 and N = 64 the bias is below the spread)."""
    logz, means, _ = quadrature(48)
    lz, m, _ = _device_runs(4096, kind="pf", N=64)
    print("log Z-hat", lz.mean(), "+-", lz.std(ddof=1) / 4.0, "against", logz, "(reported only)")
    _inside(m, means, "means")
