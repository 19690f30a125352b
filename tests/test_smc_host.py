"""Host checks of density-tempered SMC over resident PMMH chains (no GPU): the header and the binding, the long-double model
(tests/helpers/smc_model.py) -- the temperature search, the flags, the resampling --, the exactness of the law on the CPU
against a quadrature, and the refusals of TemperedPopulation."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pmmh_model as pm  # noqa: E402
import smc_model as sm  # noqa: E402

from test_capi_symbols import declared_functions  # noqa: E402

LD = sm.LD
SMC_NAMES = ("pfg_smc_scratch_bytes", "pfg_smc_logtarget_device", "pfg_smc_temper_device", "pfg_smc_gather_device",
             "pfg_smc_scale_device", "pfg_smc_accept_device")


# ---- 1. header and binding ---------------------------------------------------------------------------------------------
def test_header_binding_and_library_export_the_smc_calls():
    from sgmcmc_ssm_amd import _build, _capi
    declared = declared_functions()
    for name in SMC_NAMES:
        assert name in declared and name in _capi.EXPORTS, name
    if _build.is_stale():
        _build.build_library()
    raw = ctypes.CDLL(_build.LIB_PATH)
    for name in SMC_NAMES:
        assert hasattr(raw, name), name
    lib = _capi.load_library()
    assert lib.pfg_version() == 126
    assert lib.pfg_struct_size(2) == 376 and lib.pfg_struct_size(5) == 88 and lib.pfg_struct_size(99) == -1
    assert _capi.smc_scratch_bytes(2) == 256 and _capi.smc_scratch_bytes(33) == 512 and _capi.smc_scratch_bytes(1 << 20) == 8 << 20
    assert _capi.smc_scratch_bytes(1) == -1 and _capi.smc_scratch_bytes((1 << 20) + 1) == -1
    from sgmcmc_ssm_amd import tempering
    for model, slots in sm.MOVING.items():          # the binding's mask, the wrapper's list and the model's tuple agree
        assert tuple(tempering.moving_slots(model)) == slots
        assert _capi.PMMH_MOVING_SLOTS[model] == sum(1 << j for j in slots)


# ---- 2. the host model ---------------------------------------------------------------------------------------------------
def _random_h(rng):
    # C = 2 .. 5000, log-uniform (every tenth case one of the ends)
    C = int(rng.choice([2, 5000])) if rng.random() < 0.1 else int(round(np.exp(rng.uniform(np.log(2.0), np.log(5000.0)))))
    h = rng.normal(scale=10.0 ** rng.uniform(-1.0, np.log10(50.0)), size=C) + rng.normal(scale=100.0)
    if rng.random() < 0.4 and C > 4:
        h[rng.random(C) < 0.2] = -np.inf
    if not np.isfinite(h).any():
        h[0] = 0.0
    return h


def test_ess_at_the_chosen_step_and_the_search_ends_at_one():
    """200 random h vectors (normal scale 0.1 .. 50, C = 2 .. 5000, some entries -inf), tau drawn in (0.1, 0.9): at the
    chosen delta the ESS lies in [tau C, tau C (1 + 1e-9)] unless delta = 1 - phi; repeating the search on the same h ends
    with phi = 1 exactly in finitely many stages.  A vector with fewer than tau C finite entries has no admissible step: the
    zero-step flag."""
    rng = np.random.default_rng(20260101)
    searched = 0
    for case in range(200):
        h = _random_h(rng)
        tau = float(rng.uniform(0.1, 0.9))
        C = h.shape[0]
        t = sm.temper(h, 0.0, tau, 0.5)
        if t["status"] == sm.ZERO_STEP:             # fewer than tau C chains have a weight at all
            assert np.isfinite(h).sum() < tau * C
            continue
        assert t["status"] == 0
        e = sm.ess(h.astype(LD), t["hmax"], t["delta"])
        assert e >= LD(tau) * C
        if not t["last"]:
            searched += 1
            assert e <= LD(tau) * C * (1 + LD(1e-9)), (case, float(e), tau * C)
            assert 0 < t["delta"] < 1
        # the schedule on a fixed h: phi reaches 1 exactly
        phi, stages = 0.0, 0
        while phi < 1.0:
            s = sm.temper(h, phi, tau, 0.5)
            assert s["status"] == 0 and s["phi_new"] > phi
            phi, stages = float(s["phi_new"]), stages + 1
            assert stages < 10000
        assert phi == 1.0
    assert searched > 50


def test_flags():
    inf = np.inf
    assert sm.temper(np.full(5, -inf), 0.0, 0.5, 0.5)["status"] == sm.NO_FINITE
    assert sm.temper(np.array([0.0, np.nan, 1.0]), 0.0, 0.5, 0.5)["status"] == sm.NOT_A_NUMBER
    assert sm.temper(np.array([0.0, inf, 1.0]), 0.0, 0.5, 0.5)["status"] == sm.NOT_A_NUMBER
    assert sm.temper(np.array([0.0, 1.0]), 1.0, 0.5, 0.5)["status"] == sm.BAD_PHI
    assert sm.temper(np.array([0.0] + [-inf] * 9), 0.0, 0.5, 0.5)["status"] == sm.ZERO_STEP       # ESS is 1 < 5 for every step
    ok = sm.temper(np.array([0.0, -inf, 0.1, 0.2]), 0.0, 0.5, 0.5)
    assert ok["status"] == 0 and ok["cdf"][1] == ok["cdf"][0] and 1 not in ok["parent"]            # -inf: a zero weight


def test_systematic_resampling_of_the_chains():
    """Offspring counts are floor(C p_i) or ceil(C p_i), parents do not decrease, equal weights give the identity, and the
    uniform is the keyed one (a pure function of (seed, stage))."""
    rng = np.random.default_rng(7)
    for case in range(60):
        C = int(rng.integers(2, 3000))
        w = rng.gamma(0.3, size=C).astype(LD)
        if case % 3 == 0:
            w[rng.random(C) < 0.3] = 0
            w[0] = 1
        cdf = np.cumsum(w)
        u = float(rng.random())
        parent, _ = sm.systematic_parents(cdf, u)
        assert np.all(np.diff(parent) >= 0)
        counts = np.bincount(parent, minlength=C)
        expect = (w / cdf[-1] * C).astype(float)
        assert np.all(counts >= np.floor(expect - 1e-9)) and np.all(counts <= np.ceil(expect + 1e-9))
        assert not counts[np.asarray(w == 0)].any()
    for C in (2, 3, 64, 1000):
        parent, _ = sm.systematic_parents(np.cumsum(np.ones(C, dtype=LD)), 0.37)
        np.testing.assert_array_equal(parent, np.arange(C))
    us = [float(sm.stage_uniform(12345, s)) for s in range(4)] + [float(sm.stage_uniform(12346, 0))]
    assert len(set(us)) == 5 and all(0.0 < v < 1.0 for v in us)
    assert float(sm.stage_uniform(12345, 2)) == us[2]


def test_logprior_value_is_the_hosts_logprior_up_to_a_constant():
    """The restatement of the device's logprior_value differs from Prior.logprior by a constant of the hyper-parameters."""
    from test_host_logic import PRIORS
    rng = np.random.default_rng(3)
    for model in ("svm", "lgssm", "garch"):
        prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
        th = sm.initial_population(model, 12, 5, {"svm": [0.5, 1, 1], "lgssm": [0.5, 1, 1, 1], "garch": [0, 1, 1, 1]}[model],
                                   [0.3] * pm.P_DIM[model])
        d = sm.logprior_value(model, sm.hyper_of(model, prior), th).astype(float) - pm.logprior(model, prior, th)
        assert np.ptp(d) <= 1e-10 * max(1.0, np.abs(d).max()), (model, d)


# ---- 3. exactness on the CPU -----------------------------------------------------------------------------------------------
EXACT = dict(y=[0.31, -0.87, -1.92, -0.55, 0.64, 1.38, 2.11, 0.73], prior_var=1.0, x_mean=0.0, x_var=10.0, L_max=6.0,
             q0_mean=[0.5, 1.0, 1.0, 1.0], q0_sd=[0.5, 1.0, 0.5, 0.5], C=2000, tau=0.5, moves=2, seeds=16, free=(0, 2, 3))


def exact_hyper():
    from test_host_logic import PRIORS
    return sm.hyper_of("lgssm", PRIORS["lgssm"].generate_default_prior(var=EXACT["prior_var"], n=1, m=1))


def quadrature(n, hy=None):
    """Gauss-Legendre, n nodes per axis, of exp(logprior_value + log-likelihood) over (A, LQinv, LRinv) in [-0.9999, 0.9999] x
    (0, L_max]^2 -> (log Z, the posterior means of (A, LQinv, LRinv), the integrand's largest value on the L_max faces
    relative to its peak)."""
    hy = exact_hyper() if hy is None else hy
    x, w = np.polynomial.legendre.leggauss(n)
    a, wa = pm.A_MAX * x, pm.A_MAX * w
    l, wl = 0.5 * EXACT["L_max"] * (x + 1.0), 0.5 * EXACT["L_max"] * w
    A, LQ, LR = np.meshgrid(a, l, l, indexing="ij")
    th = np.column_stack([A.ravel(), np.ones(A.size), LQ.ravel(), LR.ravel()])
    f = sm.logprior_value("lgssm", hy, th).astype(float) + sm.kalman_loglik(th, EXACT["y"], EXACT["x_mean"], EXACT["x_var"])
    W = (wa[:, None, None] * wl[None, :, None] * wl[None, None, :]).ravel()
    peak = f.max()
    e = np.exp(f - peak) * W
    Z = e.sum()
    # the nodes nearest L_max stand for the faces: the integrand falls monotonically towards them
    cube = f.reshape(n, n, n)
    face = np.exp(max(cube[:, -1, :].max(), cube[:, :, -1].max()) - peak)
    return peak + np.log(Z), (e[:, None] * th[:, list(EXACT["free"])]).sum(0) / Z, face


_RUNS = {}


def exact_runs():
    """The 16 replicates of the host model, computed once: (log Z-hat [16], means [16, 3])."""
    if not _RUNS:
        hy = exact_hyper()
        loglik = lambda th, ctr: sm.kalman_loglik(th, EXACT["y"], EXACT["x_mean"], EXACT["x_var"])
        lz, means, stages = [], [], []
        for seed in range(EXACT["seeds"]):
            p = sm.Population("lgssm", hy, loglik, EXACT["C"], seed, EXACT["q0_mean"], EXACT["q0_sd"], tau=EXACT["tau"],
                              moves=EXACT["moves"]).run()
            assert p.phi == 1.0
            lz.append(p.log_evidence())
            means.append(p.theta[:, list(EXACT["free"])].mean(0))
            stages.append(p.stage_index)
        _RUNS.update(lz=np.array(lz), means=np.array(means), stages=stages)
    return _RUNS


def test_kalman_loglik_is_the_scalar_models():
    from kalman_model import kalman_window
    th = sm.initial_population("lgssm", 6, 1, EXACT["q0_mean"], EXACT["q0_sd"])
    got = sm.kalman_loglik(th, EXACT["y"], EXACT["x_mean"], EXACT["x_var"])
    for row, g in zip(th, got):
        want = kalman_window(row, EXACT["y"], 0, len(EXACT["y"]), None, EXACT["x_mean"], EXACT["x_var"])[1]
        assert abs(g - want) <= 1e-12 * abs(want)


def test_quadrature_converges():
    """Two resolutions agree to 1e-6 in log and the integrand on the faces L = L_max is below 1e-12 of its peak.  The prior
    is the default one with var = 1: df = 3, scale = 1 / 3, var_col = 1, so exp(logprior_value) behaves as LQinv^2 LRinv^2
    at L -> 0 (a power df - 2 from each Wishart term, one more from each coefficient's log L) and as exp(-1.5 L^2) at
    L -> inf, while the likelihood is bounded: the integrand is integrable at both ends."""
    lo, hi = quadrature(32), quadrature(48)
    print("log Z", lo[0], hi[0], "means", hi[1], "face", hi[2])
    assert abs(lo[0] - hi[0]) <= 1e-6 and np.all(np.abs(lo[1] - hi[1]) <= 1e-6)
    assert hi[2] < 1e-12


def test_tempered_population_is_exact_on_the_cpu():
    """LGSSM, T = 8, the Kalman likelihood, C = 2000, tau = 0.5, moves = 2, 16 seeds; q0 = N((0.5, -, 1, 1), 0.5^2): centred in
    the support with a spread that covers it, fixed before any run.  The mean over the seeds of log Z-hat lies within 5
    standard errors (across seeds) of the quadrature's log Z, and so does every pooled posterior mean.

    Observed: log Z-hat -17.0156 +- 0.0081 against -17.0094, 0.15 of the bound; the means of (A, LQinv, LRinv) at 0.02, 0.09 and
    0.13 of theirs; 1 or 2 stages per run."""
    logz, means, _ = quadrature(48)
    r = exact_runs()
    n = EXACT["seeds"]
    se_z = r["lz"].std(ddof=1) / np.sqrt(n)
    print("log Z-hat", r["lz"].mean(), "+-", se_z, "against", logz, "ratio to the bound", abs(r["lz"].mean() - logz) / (5 * se_z),
          "stages", r["stages"])
    assert abs(r["lz"].mean() - logz) <= 5.0 * se_z
    se_m = r["means"].std(0, ddof=1) / np.sqrt(n)
    print("means", r["means"].mean(0), "+-", se_m, "against", means, "ratio", np.abs(r["means"].mean(0) - means) / (5 * se_m))
    assert np.all(np.abs(r["means"].mean(0) - means) <= 5.0 * se_m)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
def _resolve(**kw):
    from sgmcmc_ssm_amd.tempering import TemperedPopulation
    from test_host_logic import default_params
    model = kw.pop("model", "svm")
    kw.setdefault("num_chains", 16)
    return TemperedPopulation.resolve_settings(model, default_params(model), **kw)


def test_refusals(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ok = _resolve()
    assert ok.theta0.shape == (16, 3) and np.all(pm.in_support("svm", ok.theta0))
    with pytest.raises(NotImplementedError, match="correlation"):
        _resolve(correlation=0.9)
    with pytest.raises(NotImplementedError, match="sampler stays 'pmmh'"):
        _resolve(sampler="pmala")
    for C in (1, (1 << 20) + 1):
        with pytest.raises(NotImplementedError, match="2 <= num_chains <= 2\\^20"):
            _resolve(num_chains=C)
    for tau in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ess_target"):
            _resolve(ess_target=tau)
    with pytest.raises(ValueError, match="moves"):
        _resolve(moves=0)
    for sd in (0.0, [0.3, -0.1, 0.3]):
        with pytest.raises(ValueError, match="init_sd"):
            _resolve(init_sd=sd)
    _resolve(model="lgssm", init_sd=[0.3, 0.0, 0.3, 0.3])          # C's entry is not q0's: ignored
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one rank of several"):
        _resolve()
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(NotImplementedError, match="one rank of several"):
        _resolve(chain_offset=16)


def test_initial_population_is_a_function_of_the_seed():
    a, b, c = _resolve(seed=5, model="lgssm"), _resolve(seed=5, model="lgssm"), _resolve(seed=6, model="lgssm")
    np.testing.assert_array_equal(a.theta0, b.theta0)
    assert not np.array_equal(a.theta0, c.theta0)
    assert np.all(a.theta0[:, 1] == 1.0)
    np.testing.assert_array_equal(a.theta0, sm.initial_population("lgssm", 16, 5, a.q0_mean, a.q0_sd))
    assert abs(a.scale_factor - 2.38 / np.sqrt(3.0)) < 1e-15


def test_resolve_settings_of_the_ensemble_is_unchanged_by_the_wrapper():
    """The wrapper forwards to ChainEnsemble(sampler='pmmh'): the ensemble's _resolve_settings gives, for that call, the
    namespace it gives without the wrapper in the process -- the same fields with the same values."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    from test_host_logic import default_params
    y = np.linspace(-1.0, 1.0, 12)
    kw = dict(num_chains=8, N=64, sampler="pmmh", proposal_scale=0.1)
    start = default_params("svm")
    before = vars(ChainEnsemble._resolve_settings("svm", y, start, **kw))
    import sgmcmc_ssm_amd.tempering  # noqa: F401
    s = _resolve(num_chains=8)
    after = vars(ChainEnsemble._resolve_settings("svm", y, start, **kw))
    assert before.keys() == after.keys()
    for k in before:
        if k == "proto":
            assert before[k] is after[k] is start
        else:
            np.testing.assert_equal(before[k], after[k])
    # ... and what the wrapper passes on resolves as a PMMH call of per-chain rows
    mine = ChainEnsemble._resolve_settings("svm", y, s.theta0, N=64, sampler="pmmh", proposal_scale=s.scale0[:3])
    assert vars(mine).keys() == before.keys()
    np.testing.assert_array_equal(vars(mine)["theta0"], s.theta0)
