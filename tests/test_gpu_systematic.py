"""GPU: systematic resampling (PFG_SMOOTHER_NEMETH_SYSTEMATIC, resampling='systematic', variant systematic256x4, device
generator, N <= 1024) pinned to the CPU oracle from the draws its traced launch records.

The reference resamples multinomially, so there is no REPLAY stream to compare with.  What is pinned instead: the traced
launch records the uniform every child searched with (rec_ud) beside its normals (rec_z0, rec_z); the offset u0_t of step t
is ud[t][0] N, every child's uniform must be (r + u0_t) / N, u0_t must lie on the 32-bit grid, and the words behind the
offsets must follow one another in lane 0's keyed generator (tests/helpers/keyed_draws.LaneRng).  po.pf_window then replays
the launch on the recorded numbers with tests/helpers/systematic_model.device_ancestors as its resampler -- trajectories,
ancestors (zero flips), log-weights, running log-likelihood, statistics, record.  Independently of the recorded uniforms,
every parent's offspring count must be floor(N p_i) or ceil(N p_i), the defining property of a systematic draw.  One
trace-honouring instantiation serves traced and production launches, so the production launch of the same window must
return the traced launch's record bit for bit, log-likelihood included (RegTraits::TWINLESS_LL).

Then the sufficient and the empty statistic, the f32 (ping-pong) instantiation teacher-forced, offsets across the windows
of a batch, batch invariance with trace buffers, f32 state and mixed statistics, and ChainEnsemble against hand-built
launches."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from sgmcmc_ssm_amd import _capi
from test_host_logic import default_params
from test_gpu_device_replay import THETA, _series
from test_gpu_batch_invariance import batch, check_alone, window
from test_gpu_stratified import DATOL, DRTOL, DSTAT_ATOL, _ensemble_series, _prior, _three_steps_equal_hand_built
from test_gpu_device_replay_stats import ATOL as S_ATOL, RTOL as S_RTOL, STAT_ATOL as S_STAT_ATOL, _full_width

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import keyed_draws  # noqa: E402
import systematic_model  # noqa: E402

pytestmark = pytest.mark.gpu

SM = "nemeth_systematic"
VARIANT = "systematic256x4"


@pytest.fixture(scope="module")
def ctx():
    return _capi.default_context(0)


def _problem(model, kernel, lam, N, T=24, win=(4, 20), stat="score", dtype="f64"):
    y = _series(model, T, seed=N + T)
    t1, tL, weights = 0, T, None
    if win is not None:
        t1, tL = win
        weights = np.linspace(20.0, 30.0, tL - t1)
    pm, pv = _prior(model)
    return dict(model=model, kernel=kernel, smoother=SM, stat=stat, dtype=dtype, rng="device", N=N, t1=t1, tL=tL,
                lambduh=lam, prior_mean=pm, prior_var=pv, y=y, weights=weights, theta=THETA[model], seed=20261019 + N,
                stream=T)


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _launch_pair(ctx, q):
    """The traced launch and the production launch of q; the production record must be the traced one bit for bit."""
    o = ctx.run_batch([q], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == VARIANT
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == VARIANT
    print("loglik traced", repr(float(o["loglik"])), "production", repr(float(plain["loglik"])))
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]), (plain["mean_stat"], o["mean_stat"])
    assert plain["loglik"] == o["loglik"], (plain["loglik"], o["loglik"])
    return o


def _check_recorded_uniforms(q, o, report=True):
    """Bounds, formula, grid, generator and distinctness of the uniforms a traced launch recorded; returns the offsets."""
    ud = o["rec_ud"]
    T, N = ud.shape
    assert (T, N) == (q["y"].shape[0], q["N"])
    assert np.all(ud >= 0.0) and np.all(ud < 1.0)
    u0, words, dist = systematic_model.offsets(ud)
    # formula.  4 ulps, derived: one rounding of 1 / N and one of the product are at most 1.5 ulp from the division
    # (tests/test_systematic_host.py measures 1 against the helper); the margin covers a contracted form of
    # (r + u0) * invN in the -ffp-contract=fast units
    worst = 0.0
    for t in range(T):
        worst = max(worst, float(_ulps(ud[t], systematic_model.systematic_uniforms(u0[t], N)).max()))
    if report:
        print("N", N, "worst ulp distance", worst, "worst distance from an integer", float(dist.max()) if T else 0.0)
    assert worst <= 4.0, worst
    # grid: u0 = (w + 0.5) / 2^32.  The fp64 bound at r = 0 is about 1.5e-6 (an ulp of 2^32 u0 after two roundings)
    assert np.all(dist < 1e-3), dist.max()
    assert np.all((words >= 0) & (words < (1 << 32)))
    # generator: the T words follow one another in lane 0's keyed stream (a chance match is of the order T K / 2^32),
    # and no offset is used twice
    K = 16 * (T + 2) + 64
    g = keyed_draws.LaneRng(q["seed"], q["stream"], q.get("step", 0), [0])
    stream = [int(g.next()[0]) for _ in range(K)]
    assert systematic_model.in_order_subsequence(words, stream), (words[:4], stream[:24])
    assert len(set(int(w) for w in words)) == T
    return u0


def _check_offspring(o, allowed=0):
    """Every parent has floor(N p_i) or ceil(N p_i) children.  delta = 1e-6, derived: N = 1024 times the 3e-12 error of the
    kernel's exp, with margin; a real miscount is off by at least one."""
    T = o["rec_ud"].shape[0]
    bad = sum(systematic_model.offspring_violations(o["all_ancestors"][t], o["all_log_weights"][t], 1e-6) for t in range(T))
    assert bad <= allowed, (bad, allowed)
    assert np.all(np.diff(o["all_ancestors"], axis=1) >= 0)


def _replay(q, o, pf, lam, stat, rtol, atol, stat_atol):
    """po.pf_window on the recorded draws against the traced launch."""
    ud, N = o["rec_ud"], q["N"]
    ref = po.pf_window(q["model"], q["theta"], q["y"], N, o["rec_z0"], None, o["rec_z"], kernel=q["kernel"], pf=pf,
                       lambduh=lam, stat=stat, t1=q["t1"], tL=q["tL"], weights=q["weights"], prior_mean=q["prior_mean"],
                       prior_var=q["prior_var"], save_all=True,
                       resampler=lambda t, logw: systematic_model.device_ancestors(logw, ud[t]))
    nflip = int(np.sum(o["all_ancestors"] != ref["all_ancestors"]))
    assert nflip == 0, "{0} ancestor indices differ".format(nflip)
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"], ref["all_loglikelihood_estimate"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=rtol, atol=stat_atol)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=rtol, atol=stat_atol)
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=rtol, atol=atol)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# a. replay by the oracle, fp64, score
# ---------------------------------------------------------------------------------------------------------------------
REPLAY_CASES = [
    # model, kernel, lambduh, N, T, window
    ("svm", "prior", 1.0, 1, 24, (4, 20)),                  # one particle
    ("svm", "prior", 0.95, 64, 24, (4, 20)),                # one wave, full
    ("svm", "prior", 1.0, 65, 24, (4, 20)),
    ("garch", "optimal", 0.9, 255, 24, (4, 20)),            # the edges of k = 0 -> 1
    ("garch", "prior", 1.0, 256, 24, (4, 20)),
    ("lgssm", "optimal", 0.95, 257, 24, (4, 20)),
    ("svm", "prior", 1.0, 1000, 24, (4, 20)),               # a ragged last slot
    ("lgssm", "prior", 1.0, 1023, 24, (4, 20)),
    ("garch", "optimal", 1.0, 1024, 24, (4, 20)),           # every slot
    ("svm", "prior", 0.95, 1024, 24, None),                 # the whole series, no weights
    ("svm", "prior", 1.0, 100, 1, None),
    ("svm", "prior", 1.0, 100, 130, (3, 127)),              # two 64-step log-likelihood flushes and a tail
]
assert len(REPLAY_CASES) == 12


@pytest.mark.parametrize("case", REPLAY_CASES, ids=lambda c: "{0}-{1}-lam{2}-N{3}-T{4}".format(*c))
def test_device_kernel_replayed_by_oracle(ctx, case):
    """One traced and one production launch per case; in this order: production against traced record, the recorded
    uniforms (bounds, formula, grid, generator, distinct offsets), offspring counts, sorted ancestors, the oracle's replay
    at the tolerances of test_gpu_stratified.py::test_device_kernel_replayed_by_oracle."""
    model, kernel, lam, N, T, win = case
    q = _problem(model, kernel, lam, N, T, win)
    o = _launch_pair(ctx, q)
    assert np.all(np.isfinite(o["rec_z"])) and np.all(np.isfinite(o["rec_z0"])) and np.any(o["rec_z"] != 0.0)
    _check_recorded_uniforms(q, o)
    _check_offspring(o)
    _replay(q, o, "nemeth", lam, "score", DRTOL, DATOL, DSTAT_ATOL)


# ---------------------------------------------------------------------------------------------------------------------
# b. the sufficient and the empty statistic
# ---------------------------------------------------------------------------------------------------------------------
STAT_UNITS = [("svm", "prior", 1000), ("garch", "optimal", 600), ("lgssm", "optimal", 257)]
STAT_SPREAD = [("poyiadjis_N", 1.0, "suff"), ("nemeth", 0.9, "suff"), ("poyiadjis_N", 1.0, "none")]
STAT_CASES = [(m, k, N, pf, lam, stat) for m, k, N in STAT_UNITS for pf, lam, stat in STAT_SPREAD]


@pytest.mark.parametrize("case", STAT_CASES, ids=lambda c: "{0}-{1}-N{2}-{3}-{5}".format(*c))
def test_device_kernel_replayed_on_suff_and_none(ctx, case):
    """The method of test_device_kernel_replayed_by_oracle on stat='suff' (poyiadjis_N and nemeth with lambduh = 0.9) and
    stat='none', at the tolerances of test_gpu_device_replay_stats.py, with that module's checks of the record's width."""
    model, kernel, N, pf, lam, stat = case
    q = _problem(model, kernel, lam, N, stat=stat)
    o = _launch_pair(ctx, q)
    _check_recorded_uniforms(q, o)
    _check_offspring(o)
    ref = _replay(q, o, pf, lam, stat, S_RTOL, S_ATOL, S_STAT_ATOL)
    T = q["y"].shape[0]
    assert o["mean_stat"].shape == (3,) and ref["all_statistics"].shape == o["all_statistics"].shape == (T + 1, N, 3)
    np.testing.assert_allclose(o["statistics"], ref["statistics"], rtol=S_RTOL, atol=S_STAT_ATOL)
    if stat == "suff":
        assert np.all(_full_width(o["all_statistics"], model)[..., 3:] == 0.0)
        assert np.all(_full_width(o["statistics"], model)[..., 3:] == 0.0)
        t1 = q["t1"]
        assert np.all(o["all_statistics"][:t1 + 1] == 0.0) and np.all(o["all_statistics"][t1 + 1][:, 1] > 0.0)
        assert np.all(o["mean_stat"] != 0.0)
    else:
        assert np.all(o["mean_stat"] == 0.0)
        assert np.all(_full_width(o["all_statistics"], model) == 0.0) and np.all(_full_width(o["statistics"], model) == 0.0)
        assert o["loglik"] != 0.0 and np.isfinite(o["loglik"])


# ---------------------------------------------------------------------------------------------------------------------
# c. f32 state (the ping-pong instantiation), teacher-forced step by step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kernel,N", STAT_UNITS)
def test_f32_state_device_kernel_replayed(ctx, model, kernel, N):
    """dtype='f32', after test_gpu_stratified.py::test_f32_state_device_kernels_replayed and at its tolerances: particles
    rtol 2e-5, log-weights 2e-4, statistics 2e-4 of their scale, at most max(3, 2e-4 T N) ancestors off; the recorded
    uniforms are checked as in fp64, and at most as many parents as that cap may miss their offspring bracket (an f32
    weight moves a CDF entry by ~1e-6)."""
    T = 24
    q = _problem(model, kernel, 1.0, N, T, None, dtype="f32")
    o = _launch_pair(ctx, q)
    ud, z = o["rec_ud"], o["rec_z"]
    _check_recorded_uniforms(q, o)
    cap = max(3, int(2e-4 * T * N))
    _check_offspring(o, allowed=cap)
    d = po.derived(model, q["theta"])
    flips = 0
    for t in range(T):
        x, lw, st = o["all_x_t"][t], o["all_log_weights"][t], o["all_statistics"][t]
        got = o["all_ancestors"][t]
        flips += int(np.sum(systematic_model.device_ancestors(lw, ud[t]) != got))
        yt = np.array([q["y"][t]])
        xp = x[got]
        xn = po.kernel_rv(model, kernel, d, xp, yt, z[t])
        np.testing.assert_allclose(o["all_x_t"][t + 1], xn, rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(o["all_log_weights"][t + 1], po.kernel_reweight(model, kernel, d, xp, xn, yt), rtol=2e-4, atol=2e-4)
        ref_st = st[got] + po.score_statistic(model, d, xp, xn, yt)
        assert np.max(np.abs(o["all_statistics"][t + 1] - ref_st)) < 2e-4 * np.maximum(1.0, np.abs(ref_st).max())
    print("f32 ancestor flips", flips, "cap", cap)
    assert flips <= cap, flips


# ---------------------------------------------------------------------------------------------------------------------
# d. offsets across the windows of a batch
# ---------------------------------------------------------------------------------------------------------------------
def test_offsets_across_windows(ctx):
    """256 SVM windows (N = 64, T = 16) with one seed and distinct streams in one launch: the 4096 offsets have mean 1/2
    within 5 / sqrt(12 n) and variance 1/12 within 5 sqrt(1 / (180 n)) (the test test_gpu_stratified.py applies to its
    U_r), each window's offsets are those of its own stream, and no two windows share an offset sequence."""
    B, N, T = 256, 64, 16
    y = _series("svm", T, seed=N + T)
    pm, pv = _prior("svm")
    qs = [dict(model="svm", kernel="prior", smoother=SM, stat="score", dtype="f64", rng="device", N=N, t1=0, tL=T, lambduh=1.0,
               prior_mean=pm, prior_var=pv, y=y, weights=None, theta=THETA["svm"], seed=20261019, stream=1000 + b)
          for b in range(B)]
    outs = ctx.run_batch(qs, want_trace=True, want_draws=True)
    assert ctx.last_variant() == VARIANT
    u0 = np.stack([_check_recorded_uniforms(q, o, report=False) for q, o in zip(qs, outs)])
    n = u0.size
    assert n == 4096
    print("offsets: mean", u0.mean(), "variance", u0.var())
    assert abs(u0.mean() - 0.5) < 5 / np.sqrt(12 * n)
    assert abs(u0.var() - 1 / 12) < 5 * np.sqrt(1 / 180 / n)
    assert len({row.tobytes() for row in u0}) == B
    assert len(set(u0.reshape(-1).tolist())) > n - 8            # 4096 draws of 2^32 values: a repeat has probability 2e-3


# ---------------------------------------------------------------------------------------------------------------------
# e. batch invariance beyond test_gpu_batch_invariance.py::test_systematic_alone_equals_batched
# ---------------------------------------------------------------------------------------------------------------------
ALONE_NS = (1024, 100, 1, 700, 333)


@pytest.mark.parametrize("mode", ["traced", "f32", "mixed_stat"])
def test_systematic_alone_equals_batched_traced(ctx, mode):
    """The batch of test_systematic_alone_equals_batched with trace buffers: on f64, with f32 state, and with stat cycling
    score / suff / none over its windows -- every window's record, particles and traced trajectory are bitwise those of the
    reversed batch and of the window run alone."""
    if mode == "mixed_stat":
        qs = [window("garch", "prior", N, i, rng="device", smoother=SM, stat=("score", "suff", "none")[i % 3])
              for i, N in enumerate(ALONE_NS)]
    else:
        qs = batch("garch", "prior", ALONE_NS, rng="device", smoother=SM, dtype="f32" if mode == "f32" else "f64")
    check_alone(ctx, qs, VARIANT, trace=True)


# ---------------------------------------------------------------------------------------------------------------------
# f. ChainEnsemble against hand-built launches
# ---------------------------------------------------------------------------------------------------------------------
def test_ensemble_device_windows():
    """8 SVM chains, N = 300, S = 16 / B = 4, windows sampled on the device: three steps equal ctx.run_batch of the
    descriptors the ensemble ran, bitwise; a graph replay of three steps equals three eager steps."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("svm")
    y = _ensemble_series("svm", 120)
    kw = dict(num_chains=8, N=300, epsilon=1e-3, seed=23, chain_offset=3, subsequence_length=16, buffer_length=4,
              window_sampling="device", resampling="systematic")
    ens = ChainEnsemble("svm", y, p, **kw)
    assert ens._smoother == ens._launch_smoother == SM
    _three_steps_equal_hand_built(ens, y, "poyiadjis_N", 1.0, VARIANT, "systematic", SM)
    eager = ChainEnsemble("svm", y, p, **kw)
    eager.step(3)
    graph = ChainEnsemble("svm", y, p, **kw).run(3, thin=3, graph_steps=3)
    np.testing.assert_array_equal(graph[0], eager.theta())
    np.testing.assert_array_equal(ens.theta(), eager.theta())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ensemble_multi_window(dtype):
    """minibatch_size = 2, GARCH, N = 64, pf='nemeth' with lambduh = 0.9: the window records and the reduced records of
    three steps against hand-built launches, and graph replay against eager steps."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("garch")
    y = _ensemble_series("garch", 90)
    kw = dict(num_chains=12, N=64, pf="nemeth", lambduh=0.9, epsilon=1e-3, dtype=dtype, seed=31, chain_offset=2,
              subsequence_length=16, buffer_length=4, minibatch_size=2, window_sampling="device", resampling="systematic")
    ens = ChainEnsemble("garch", y, p, **kw)
    assert ens._multi and ens.W == 2 and ens._smoother == SM
    _three_steps_equal_hand_built(ens, y, "nemeth", 0.9, VARIANT, "systematic", SM)
    eager = ChainEnsemble("garch", y, p, **kw)
    eager.step(3)
    graph = ChainEnsemble("garch", y, p, **kw).run(3, thin=3, graph_steps=3)
    np.testing.assert_array_equal(graph[0], eager.theta())
