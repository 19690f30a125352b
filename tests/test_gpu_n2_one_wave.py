"""GPU: n2_64x2, the one-wave variant of the Poyiadjis O(N^2) smoother (64 threads x 2 particles per window, N <= 128).

The plan picks it for device-generator batches of more than 64 windows; PFGRAD_VARIANT=n2_64x2 forces it wherever it
holds N, REPLAY included, so that it is pinned against the same reference fixtures and oracle as n2_256x1
(tests/test_gpu_n2.py).  The backward sweep over all parents is skipped before t1 of a window that starts without
init_stats: the per-particle statistics of those steps are exactly zero, and nothing else may change."""
import numpy as np
import pytest

from conftest import Golden
from oracle import pf_oracle as po
from test_host_logic import default_params, GEN
from test_gpu_n2 import _problem, RTOL, ATOL

pytestmark = pytest.mark.gpu

CASES = [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal")]


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


@pytest.fixture
def force_one_wave(monkeypatch):
    monkeypatch.setenv("PFGRAD_VARIANT", "n2_64x2")


def test_one_wave_reference_fixtures_f64(ctx, force_one_wave):
    """The ten N = 24 reference windows of n2.npz (three models, both proposals, score and sufficient statistics, traced,
    T = 10, window [2, 8)) on n2_64x2, at test_n2_reference_fixtures_f64's tolerances; the statistics of the steps up to
    t1 are exactly zero (the skipped sweeps)."""
    g = Golden("n2.npz")
    cases = [m for m in g.meta if m["N"] <= 128]
    assert [m["key"] for m in cases] == ["n{0}".format(i) for i in range(10)] and {m["N"] for m in cases} == {24}
    for m in cases:
        o = ctx.run_batch([_problem(m, g)], want_trace=True)[0]
        assert ctx.last_variant() == "n2_64x2"
        key = m["key"]
        ll = float(g.get(key, "loglikelihood_estimate"))
        assert abs(o["loglik"] - ll) <= ATOL + RTOL * abs(ll), (m, o["loglik"], ll)
        np.testing.assert_allclose(o["x_t"], g.get(key, "x_t"), rtol=RTOL, atol=ATOL, err_msg=str(m))
        np.testing.assert_allclose(o["log_weights"], g.get(key, "log_weights"), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(o["statistics"], g.get(key, "statistics"), rtol=RTOL, atol=1e-8, err_msg=str(m))
        ref = g.get(key, "mean_statistic")
        assert np.linalg.norm(o["mean_stat"] - ref) <= 1e-8 * max(1.0, np.linalg.norm(ref)), (m, o["mean_stat"], ref)
        if m["traced"]:
            np.testing.assert_allclose(o["all_x_t"], g.get(key, "all_x_t"), rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(o["all_statistics"], g.get(key, "all_statistics"), rtol=RTOL, atol=1e-8)
            np.testing.assert_allclose(o["all_loglikelihood_estimate"], g.get(key, "all_loglikelihood_estimate"),
                                       rtol=RTOL, atol=ATOL)
        assert m["t1"] == 2
        assert np.all(o["all_statistics"][:m["t1"] + 1] == 0.0), m
        assert np.any(o["all_statistics"][m["t1"] + 1] != 0.0), m


def _replay_case(model, kernel, N, t1=1, tL=6, T=7, dtype="f64"):
    """A REPLAY window with weights and the oracle's O(N^2) smoother on the same streams."""
    rs = np.random.RandomState(N * 7 + t1)
    p = default_params(model)
    np.random.seed(3)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    w = rs.uniform(1.0, 5.0, size=tL - t1)
    z0, u, z = po.draw_streams(rs, N, T)
    pv = 1.3
    ref = po.pf_window(model, p.theta(), y, N, z0, u, z, kernel=kernel, pf="poyiadjis_N2", stat="score", t1=t1, tL=tL,
                       weights=w, prior_mean=0.0, prior_var=pv, save_all=True)
    q = dict(model=model, kernel=kernel, smoother="poyiadjis_n2", stat="score", dtype=dtype, rng="replay", N=N, t1=t1,
             tL=tL, lambduh=1.0, prior_mean=0.0, prior_var=pv, y=y, weights=w, theta=p.theta(), z0=z0, u=u, z=z)
    return q, ref


def _assert_matches_oracle(o, ref):
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(o["statistics"], ref["statistics"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=RTOL, atol=1e-8)
    assert abs(o["loglik"] - ref["loglikelihood_estimate"]) <= ATOL + RTOL * abs(ref["loglikelihood_estimate"])


@pytest.mark.parametrize("model,kernel", CASES)
@pytest.mark.parametrize("N", [64, 65, 100, 128])
def test_one_wave_oracle_parity(ctx, force_one_wave, model, kernel, N):
    """REPLAY against the oracle at the wave's edge sizes: a full first slot row (64), one child past it (65), the
    experiment row's N (100), every slot full (128); T = 7, window [1, 6) with weights."""
    q, ref = _replay_case(model, kernel, N)
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == "n2_64x2"
    _assert_matches_oracle(o, ref)
    assert np.all(o["all_statistics"][:2] == 0.0)


def test_one_wave_window_from_the_first_step(ctx, force_one_wave):
    """t1 = 0: no step is skipped."""
    q, ref = _replay_case("svm", "prior", 100, t1=0, tL=5)
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == "n2_64x2"
    _assert_matches_oracle(o, ref)
    assert np.any(o["all_statistics"][1] != 0.0)


@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "optimal")])
def test_one_wave_warm_start_keeps_every_sweep(ctx, monkeypatch, model, kernel):
    """A window continued from another's final particles, log-weights and statistics (init_x / init_logw / init_stats):
    the statistics are non-zero from the start, so the steps before t1 keep their sweeps.  The oracle has no warm start:
    the final statistics are compared with n2_256x1 on the same inputs at rtol 1e-9."""
    N = 100
    monkeypatch.setenv("PFGRAD_VARIANT", "n2_64x2")
    q0, _ = _replay_case(model, kernel, N)
    first = ctx.run_batch([q0], want_final=True)[0]
    assert np.any(first["statistics"] != 0.0)
    q, _ = _replay_case(model, kernel, N, t1=3, tL=6)
    q = dict(q, init_x=first["x_t"], init_logw=first["log_weights"], init_stats=first["statistics"])
    del q["z0"]
    outs = {}
    for variant in ("n2_64x2", "n2_256x1"):
        monkeypatch.setenv("PFGRAD_VARIANT", variant)
        outs[variant] = ctx.run_batch([dict(q)], want_trace=True)[0]
        assert ctx.last_variant() == variant
    a, b = outs["n2_64x2"], outs["n2_256x1"]
    np.testing.assert_array_equal(a["all_statistics"][0], first["statistics"])
    # the steps before t1 moved the statistics from parent to parent: not zero, not the start's
    assert np.all(np.any(a["all_statistics"][1:4] != 0.0, axis=(1, 2)))
    for name in ("statistics", "all_statistics", "x_t", "log_weights", "mean_stat"):
        np.testing.assert_allclose(a[name], b[name], rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(b[name]).max())), err_msg=name)
    assert abs(a["loglik"] - b["loglik"]) <= 1e-9 * max(1.0, abs(b["loglik"]))


def test_one_wave_oracle_parity_f32(ctx, force_one_wave):
    """f32 particle state on the same streams, at the f32 tolerances of test_one_wave_pool_parity_f32."""
    q, ref = _replay_case("lgssm", "optimal", 32, dtype="f32")
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == "n2_64x2"
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=2e-3, atol=2e-3)


def _prior_x(model, theta):
    return (0.0, 10.0) if model != "garch" else (0.0, float(np.asarray(po.garch_prior_x(theta)[1]).reshape(-1)[0]))


@pytest.mark.parametrize("model,kernel", CASES)
def test_one_wave_device_kernel_replayed_by_oracle(ctx, force_one_wave, model, kernel):
    """The device-generator instantiation writes out the normals it drew and the ancestors it chose; the oracle replays
    the window on them (tolerances of test_gpu_device_replay.py::test_device_kernel_replayed_by_oracle).  The same key
    without any recording returns the same gradient and log-likelihood bit for bit."""
    N, T, t1, tL = 100, 12, 3, 10
    p = default_params(model)
    theta = p.theta()
    np.random.seed(17)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    weights = np.linspace(20.0, 30.0, tL - t1)
    pm, pv = _prior_x(model, theta)
    q = dict(model=model, kernel=kernel, smoother="poyiadjis_n2", stat="score", dtype="f64", rng="device", N=N, t1=t1, tL=tL,
             lambduh=1.0, prior_mean=pm, prior_var=pv, y=y, weights=weights, theta=theta, seed=20241004 + N, stream=T)
    o = ctx.run_batch([q], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == "n2_64x2"
    z, z0, anc = o["rec_z"], o["rec_z0"], o["all_ancestors"]
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(z0)) and np.any(z != 0.0) and np.any(z0 != 0.0)
    assert anc.min() >= 0 and anc.max() < N
    ref = po.pf_window(model, theta, y, N, z0, None, z, kernel=kernel, pf="poyiadjis_N2", stat="score", t1=t1, tL=tL,
                       weights=weights, prior_mean=pm, prior_var=pv, save_all=True, resampler=lambda t, logw: anc[t])
    r, a = 1e-8, 1e-8
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"], ref["all_loglikelihood_estimate"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=r, atol=1e-7)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=r, atol=1e-7)
    assert np.linalg.norm(o["mean_stat"] - ref["mean_statistic"]) < 1e-6 * max(1.0, np.linalg.norm(ref["mean_statistic"]))
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=r, atol=a)
    assert np.all(o["all_statistics"][:t1 + 1] == 0.0)
    if np.any(o["rec_u"] != 0):
        # (the O(N^2) kernels search an fp64 CDF with u01 of the generator word and record no words today; a launch
        # that does record them chose its ancestors in the layout of the 64 x 2 plain unit)
        ref_anc = np.array([po.device_ancestors(ref["all_log_weights"][t], o["rec_u"][t], 64, 2, "fixed32") for t in range(T)])
        assert int(np.sum(anc != ref_anc)) == 0
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == "n2_64x2"
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]) and plain["loglik"] == o["loglik"]


def _device_problems(model, N, B, T=30, seed=11, y=None):
    from sgmcmc_ssm_amd.particle_filters import make_problem
    p = default_params(model)
    if y is None:
        np.random.seed(seed)
        y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    kernel = "prior" if model == "svm" else "optimal"
    pm, pv = _prior_x(model, p.theta())
    probs = [make_problem(model, kernel, "poyiadjis_N2", y, p.theta(), N, prior_mean=pm, prior_var=pv, seed=5, stream=b, rng="device")
             for b in range(B)]
    return probs, (p, y, kernel, pm, pv)


@pytest.mark.parametrize("model", ["svm", "garch"])
def test_one_wave_device_rng_statistics(ctx, monkeypatch, model):
    """Device generator, N = 100, T = 30, 256 windows (the plan's own choice): every score column and the log-likelihood
    agree with 64 runs of the O(N^2) oracle, po.pf_window_rng(pf='poyiadjis_N2'), within 5 standard errors.  The oracle's
    sample is stored (tests/golden/n2_oracle_rng.npz, written by make_n2_oracle_golden.py; its first rows are recomputed
    by tests/test_n2_oracle_fixture_host.py).  (The O(N^2) oracle, not the O(N) estimate: for GARCH the reference's
    backward kernel scores only the x component of the state, so the two differ systematically in the phi / lambda
    columns, see tests/test_gpu_n2.py.)"""
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    g = Golden("n2_oracle_rng.npz")
    m = [q for q in g.meta if q["model"] == model][0]
    N, B, R = 100, 256, 64
    assert (m["N"], m["T"], m["runs"], m["pf"]) == (N, 30, R, "poyiadjis_N2")
    probs, (p, y, kernel, pm, pv) = _device_problems(model, N, B, y=g.get(model, "y"))
    np.testing.assert_array_equal(p.theta(), g.get(model, "theta"))
    assert (kernel, pm, pv) == (m["kernel"], m["prior_mean"], m["prior_var"])
    assert probs[0]["smoother"] == "poyiadjis_n2" and probs[0]["lambduh"] == 1.0
    outs = ctx.run_batch(probs)
    assert ctx.last_variant() == "n2_64x2"
    got = np.array([np.append(o["mean_stat"], o["loglik"]) for o in outs])
    assert np.all(np.isfinite(got))
    ref = g.get(model, "runs")
    assert ref.shape == (R, got.shape[1])
    se = np.sqrt(got.var(axis=0) / B + ref.var(axis=0) / R)
    zscore = np.abs(got.mean(axis=0) - ref.mean(axis=0)) / se
    assert np.all(zscore < 5.0), (zscore, got.mean(axis=0), ref.mean(axis=0))


def test_one_wave_selection(ctx, monkeypatch):
    """Which O(N^2) variant the plan picks: n2_64x2 for device-generator batches of more than 64 windows with N <= 128;
    n2_256x1 for REPLAY, for 64 windows or fewer and for N = 129; a forced tag wins where it holds N."""
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    probs, _ = _device_problems("svm", 100, 65, T=6)
    ctx.run_batch(probs)
    assert ctx.last_variant() == "n2_64x2"
    ctx.run_batch(probs[:64])
    assert ctx.last_variant() == "n2_256x1"
    probs129, _ = _device_problems("svm", 129, 65, T=6)
    ctx.run_batch(probs129)
    assert ctx.last_variant() == "n2_256x1"
    q, _ = _replay_case("svm", "prior", 100)
    ctx.run_batch([dict(q) for _ in range(65)])
    assert ctx.last_variant() == "n2_256x1"
    for N in (100, 128, 1024):
        assert ctx.scratch_bytes_smoother("svm", "f64", "device", "poyiadjis_n2", N) == 0
    assert ctx.scratch_bytes_smoother("svm", "f64", "device", "poyiadjis_n2", 2000) > 0
    # forced: n2_256x1 also where n2_64x2 would be picked; n2_64x2 does not hold N = 129
    monkeypatch.setenv("PFGRAD_VARIANT", "n2_256x1")
    ctx.run_batch(probs)
    assert ctx.last_variant() == "n2_256x1"
    monkeypatch.setenv("PFGRAD_VARIANT", "n2_256x4")
    ctx.run_batch(probs[:2])
    assert ctx.last_variant() == "n2_256x4"
    monkeypatch.setenv("PFGRAD_VARIANT", "n2_64x2")
    ctx.run_batch(probs129)
    assert ctx.last_variant() == "n2_256x1"
