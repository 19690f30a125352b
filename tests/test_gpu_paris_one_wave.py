"""GPU: paris64x2, the one-wave PaRIS variant (64 threads x 2 particles per window, N <= 128).

The plan picks it for device-generator batches of more than 64 windows; PFGRAD_VARIANT=paris64x2 forces it wherever it
holds N, REPLAY included, so that it is pinned against the same oracle pools and reference fixtures as paris256x1
(tests/test_gpu_paris.py)."""
import numpy as np
import pytest

from oracle import pf_oracle as po
from test_host_logic import default_params, GEN, vec
from test_gpu_paris import CASES, RTOL, ATOL, _seed_cases, _helper_for, _params_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


@pytest.fixture
def force_one_wave(monkeypatch):
    monkeypatch.setenv("PFGRAD_VARIANT", "paris64x2")


def _pool_case(model, kernel, N, Ntilde, R, dtype="f64"):
    """The inputs of test_gpu_paris.py::test_paris_pool_parity and the oracle's window on them."""
    rs = np.random.RandomState(N * 7 + Ntilde)
    T, t1, tL = 7, 1, 6
    p = default_params(model)
    np.random.seed(3)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    w = rs.uniform(1.0, 5.0, size=tL - t1)
    z0, u, z = po.draw_streams(rs, N, T)
    idx_u = rs.random_sample((T, Ntilde, max(R, 1), N))[:, :, :R]
    acc_u = rs.random_sample((T, Ntilde, max(R, 1), N))[:, :, :R]
    man_u = rs.random_sample((T, Ntilde, N))
    pv = 1.3
    ref = po.pf_window(model, p.theta(), y, N, z0, u, z, kernel=kernel, pf="paris", stat="score", t1=t1, tL=tL,
                       weights=w, prior_mean=0.0, prior_var=pv, save_all=True, Ntilde=Ntilde,
                       max_accept_reject=R, manual_sample_threshold=0,
                       paris_draws=po.PoolDraws(idx_u, acc_u, man_u))
    q = dict(model=model, kernel=kernel, smoother="paris", stat="score", dtype=dtype, rng="replay", N=N, t1=t1,
             tL=tL, prior_mean=0.0, prior_var=pv, y=y, weights=w, theta=p.theta(), z0=z0, u=u, z=z,
             Ntilde=Ntilde, max_accept_reject=R, paris_idx_u=np.ascontiguousarray(idx_u),
             paris_acc_u=np.ascontiguousarray(acc_u), paris_man_u=man_u)
    return q, ref


@pytest.mark.parametrize("model,kernel", CASES)
@pytest.mark.parametrize("N,Ntilde,R", [(32, 2, 6), (100, 3, 2), (128, 2, 3), (65, 1, 70)])
def test_one_wave_pool_parity(ctx, force_one_wave, model, kernel, N, Ntilde, R):
    """REPLAY on identical uniform pools: trajectories, log-weights, statistics and log-likelihood as the oracle's,
    at test_paris_pool_parity's tolerances.  (128, 2, 3): every slot of the wave holds a particle; (65, 1, 70): one
    child left over a wave, long tails of accept-reject rounds."""
    q, ref = _pool_case(model, kernel, N, Ntilde, R)
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == "paris64x2"
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=RTOL, atol=ATOL)
    # the traced backward parents (REPLAY hands them back too): the oracle's, draw for draw
    assert np.array_equal(np.transpose(o["all_paris_J"], (0, 2, 1)), ref["all_paris_J"])
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=RTOL, atol=1e-8)
    assert abs(o["loglik"] - ref["loglikelihood_estimate"]) <= ATOL + RTOL * abs(ref["loglikelihood_estimate"])


def test_one_wave_pool_parity_f32(ctx, force_one_wave):
    """f32 particle state on the same pools, at the f32 tolerances of test_gpu_pf_parity.py::test_f32_teacher_forced."""
    q, ref = _pool_case("lgssm", "optimal", 32, 2, 6, dtype="f32")
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == "paris64x2"
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=2e-3, atol=2e-3)


def test_one_wave_helper_seed_for_seed(force_one_wave):
    """The reference fixture with N <= 128 (paris_seed.npz s8: LGSSM, N = 64) through the Helper in np.random's order,
    on paris64x2: gradient, log-likelihood and the generator's next draw are the reference's."""
    from sgmcmc_ssm_amd import _capi
    cases = [(g, m) for g, m in _seed_cases("helper") if m["N"] <= 128]
    assert [m["key"] for _, m in cases] == ["s8"]
    g, m = cases[0]
    key = m["key"]
    helper = _helper_for(g, m)
    p = _params_for(m["model"], g.get(key, "theta"))
    kw = dict(observations=g.get(key, "y").reshape(-1, 1), parameters=p, subsequence_start=m["t1"], subsequence_end=m["tL"],
              weights=g.get(key, "weights"), pf="paris", N=m["N"], kernel=m["kernel"], **m["kwargs"])
    np.random.seed(m["seed"])
    grad = helper.pf_gradient_estimate(**kw)
    nxt = np.random.random_sample()
    assert _capi.default_context().last_variant() == "paris64x2"
    ref = g.get(key, "grad")
    np.testing.assert_allclose(vec(m["model"], grad), ref, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(ref).max()), err_msg=str(m))
    assert nxt == float(g.get(key, "next_draw")), m
    np.random.seed(m["seed"])
    ll = helper.pf_loglikelihood_estimate(**kw)
    nxt = np.random.random_sample()
    assert abs(ll - float(g.get(key, "loglik"))) <= 1e-9 * abs(float(g.get(key, "loglik"))), m
    assert nxt == float(g.get(key, "next_draw_loglik")), m


def _device_problems(model, N, B, T=30, seed=11):
    from sgmcmc_ssm_amd.particle_filters import make_problem
    p = default_params(model)
    np.random.seed(seed)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    kernel = "prior" if model == "svm" else "optimal"
    pm, pv = (0.0, 10.0) if model == "svm" else (0.0, float(po.garch_prior_x(p.theta())[1][0]))
    probs = [make_problem(model, kernel, "paris", y, p.theta(), N, prior_mean=pm, prior_var=pv, seed=5, stream=b, rng="device")
             for b in range(B)]
    return probs, (p, y, kernel, pm, pv)


@pytest.mark.parametrize("model", ["svm", "garch"])
def test_one_wave_device_rng_statistics(ctx, model):
    """Device generator, N = 100, 256 windows (the plan's own choice): mean score and log-likelihood agree with the
    reference-order oracle within 5 standard errors, as test_paris_device_rng_statistics checks paris256x1."""
    N, B, R = 100, 256, 64
    probs, (p, y, kernel, pm, pv) = _device_problems(model, N, B)
    assert probs[0]["max_accept_reject"] == 64
    outs = ctx.run_batch(probs)
    assert ctx.last_variant() == "paris64x2"
    got = np.array([np.append(o["mean_stat"], o["loglik"]) for o in outs])
    assert np.all(np.isfinite(got))
    rs = np.random.RandomState(1)
    ref = []
    for _ in range(R):
        r = po.pf_window_paris_rng(model, p.theta(), y, N, rng=rs, kernel=kernel, stat="score",
                                   prior_mean=pm, prior_var=pv)
        ref.append(np.append(r["mean_statistic"], r["loglikelihood_estimate"]))
    ref = np.array(ref)
    se = np.sqrt(got.var(axis=0) / B + ref.var(axis=0) / R)
    zscore = np.abs(got.mean(axis=0) - ref.mean(axis=0)) / se
    assert np.all(zscore < 5.0), (zscore, got.mean(axis=0), ref.mean(axis=0))


def test_one_wave_selection(ctx, monkeypatch):
    """Which PaRIS variant the plan picks: paris64x2 for device-generator batches of more than 64 windows with
    N <= 128; paris256x1 for REPLAY, for 64 windows or fewer and for N = 129."""
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    probs, _ = _device_problems("svm", 100, 65, T=6)
    ctx.run_batch(probs)
    assert ctx.last_variant() == "paris64x2"
    ctx.run_batch(probs[:64])
    assert ctx.last_variant() == "paris256x1"
    probs129, _ = _device_problems("svm", 129, 65, T=6)
    ctx.run_batch(probs129)
    assert ctx.last_variant() == "paris256x1"
    q, _ = _pool_case("svm", "prior", 100, 3, 2)
    ctx.run_batch([dict(q) for _ in range(65)])
    assert ctx.last_variant() == "paris256x1"
    # forced: paris256x1 also where paris64x2 would be picked; paris64x2 does not hold N = 129
    monkeypatch.setenv("PFGRAD_VARIANT", "paris256x1")
    ctx.run_batch(probs)
    assert ctx.last_variant() == "paris256x1"
    monkeypatch.setenv("PFGRAD_VARIANT", "paris64x2")
    ctx.run_batch(probs129)
    assert ctx.last_variant() == "paris256x1"
