"""The SVM prior 256 x 4 kernel (wg256x4s, bench config c2) shifts exp(lw - s) by a value that is not this step's maximum:
the previous step's exact maximum in the default build (guard |m_t - s| <= 512), or, built with -DPFG_OPT_SUMSHIFT=1
(csrc/pfg_reg_traits.hpp), a value that follows the scan total, s_{t+1} = s_t + ln2 * exponent(W_t), with the guard on W_t
(2^-728 <= W_t < 2^728) -- else the cold retry with the exact block maximum.  Its score comes from the proposal's noise term
(PFG_OPT_SCOREDZ).  Any shift that keeps exp in range gives the same normalised weights and the same s + log(W/N) up to
rounding, so under either guard every launch must be what the oracle replays from its recorded draws -- criteria of
tests/test_gpu_device_replay.py: zero ancestor flips, RTOL / ATOL on trajectories, log-weights, statistics and
log-likelihood, the TRACE = false twin bitwise equal to the traced one.  The cases sit where either guard decides.

Every input is chosen, and every property of it asserted, from the ORACLE's log-weights on the CPU.  The generator's words
and normals depend on the key (seed, stream) alone, not on the observations: a first launch on an ordinary series records
them, the oracle scans candidate series on those draws, and the launch of the chosen series must have consumed the same
draws (asserted).  Below, lse_t = log sum_i exp(lw_t[i]) of the oracle's log-weights.

  * guard, both sides (T = 24, N = 1000 / 65): y[8] by bisection (lse_9 falls monotonically in |y[8]|) so that lse falls by
    400 ... 500 at that step -- no retry, weights near 1e-200 -- and by 520 ... 700 -- a retry on the way down and one on
    the way up;
  * one dominant particle (N = 65, warm start): one log-weight 600 above the rest, ln W ~ 0 while 64 weights vanish;
  * a level that travels (T = 70, N = 65): y_t chosen step by step so that lse goes down by 40 per step to about -1800 and
    comes back by 60 per step: more than 1500 in total, less than 100 per step -- the shift is absolute, not accumulated;
    T = 70 crosses one lazy log-likelihood flush (step 64);
  * a NaN observation: NaN score, no finite log-likelihood, no hang (the guard fails, the retry runs once per step, the filter recovers);
  * a retrying window beside an ordinary one in one launch: each bitwise as alone.
"""
import os

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_gpu_device_replay import ATOL, RTOL, THETA, _series
from test_gpu_stale_shift import NT, PPT, VARIANT, _assert_replayed, _launch_twins, _oracle, _problem, _stable_loglik

pytestmark = pytest.mark.gpu

T = 24
GUARD_SHAPES = [1000, 65]
BANDS = {"inside": (400.0, 500.0), "outside": (520.0, 700.0)}      # the fall of lse at step 9, as the issue of this kernel sets them


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def _lse(all_lw):
    mx = np.max(all_lw, axis=-1)
    return mx + np.log(np.sum(np.exp(all_lw - mx[..., None]), axis=-1))


def _record_draws(ctx, q):
    """The draws of q's key: one traced launch (the observations do not enter the generator)."""
    old = os.environ.get("PFGRAD_VARIANT")
    os.environ["PFGRAD_VARIANT"] = VARIANT
    try:
        o = ctx.run_batch([dict(q)], want_trace=True, want_draws=True)[0]
        assert ctx.last_variant() == VARIANT and ctx.last_traced()
    finally:
        if old is None:
            del os.environ["PFGRAD_VARIANT"]
        else:
            os.environ["PFGRAD_VARIANT"] = old
    return {k: np.array(o[k]) for k in ("rec_u", "rec_z0", "rec_z")}


def _same_draws(o, draws):
    return all(np.array_equal(o[k], draws[k]) for k in ("rec_u", "rec_z0", "rec_z"))


def _outlier_for(q, draws, band):
    """y[8] whose fall lse_8 - lse_9 lies in the middle third of `band`, by geometric bisection on the oracle."""
    lo, hi = band[0] + (band[1] - band[0]) / 3.0, band[1] - (band[1] - band[0]) / 3.0
    a, b = 1.0, 1.0e6
    for _ in range(60):
        mid = float(np.sqrt(a * b))
        y = np.array(q["y"])
        y[8] = mid
        lse = _lse(_oracle(dict(q, y=y), draws)["all_log_weights"])
        fall = float(lse[8] - lse[9])
        if fall < lo:
            a = mid
        elif fall > hi:
            b = mid
        else:
            return mid
    raise AssertionError("no y[8] found for a fall in {0}".format(band))


@pytest.fixture(scope="module")
def guard_inputs(ctx):
    """{(N, side): (problem, draws)}: chosen once on the CPU, shared by the guard tests and the mixed launch."""
    out = {}
    for N in GUARD_SHAPES:
        q = _problem(N, _series("svm", T, seed=N + T))
        draws = _record_draws(ctx, q)
        for side, band in BANDS.items():
            y = np.array(q["y"])
            y[8] = _outlier_for(q, draws, band)
            out[(N, side)] = (dict(q, y=y), draws)
    return out


@pytest.mark.parametrize("side", ["inside", "outside"])
@pytest.mark.parametrize("N", GUARD_SHAPES)
def test_guard_on_the_scan_total_both_sides(ctx, monkeypatch, guard_inputs, N, side):
    q, draws = guard_inputs[(N, side)]
    o = _launch_twins(ctx, monkeypatch, q)
    assert _same_draws(o, draws)                                # the series was chosen on the draws this launch consumed
    ref = _oracle(q, o)
    assert np.all(np.isfinite(ref["all_statistics"])) and np.all(np.isfinite(ref["mean_statistic"]))
    assert np.all(ref["all_ancestors"] >= 0) and np.all(ref["all_ancestors"] < N)
    lse = _lse(ref["all_log_weights"])
    fall, rise = float(lse[8] - lse[9]), float(lse[10] - lse[9])
    print("N", N, side, "y[8]", q["y"][8], "lse falls by", fall, "and comes back by", rise)
    lo, hi = BANDS[side]
    assert lo <= fall <= hi
    if side == "inside":
        assert rise < 500.0                                     # W of step 10 stays below 2^728 = e^504.6 too: no retry either way
    else:
        assert rise >= 520.0                                    # a retry on the way down and one on the way up
    _assert_replayed(o, ref, _stable_loglik(ref["all_log_weights"]))


def _replay_warm(o, y, x0, logw0):
    """The oracle's building blocks on the launch's recorded draws, from a warm start (pf_window has none)."""
    N, Tw = x0.shape[0], len(y)
    d = po.derived("svm", THETA["svm"])
    x, lw, st = x0, logw0, np.zeros((N, 3))
    np.testing.assert_array_equal(o["all_x_t"][0], x0)
    np.testing.assert_array_equal(o["all_log_weights"][0], logw0)
    all_lw = [lw]
    for t in range(Tw):
        anc = po.device_ancestors(lw, o["rec_u"][t], NT, PPT, "fixed32")
        assert int(np.sum(anc != o["all_ancestors"][t])) == 0, t
        yt = np.array([y[t]])
        xp = x[anc]
        xn = po.kernel_rv("svm", "prior", d, xp, yt, o["rec_z"][t])
        st = st[anc] + po.score_statistic("svm", d, xp, xn, yt)
        x, lw = xn, po.kernel_reweight("svm", "prior", d, xp, xn, yt)
        all_lw.append(lw)
        np.testing.assert_allclose(o["all_x_t"][t + 1], x, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(o["all_log_weights"][t + 1], lw, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(o["all_statistics"][t + 1], st, rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(o["mean_stat"], np.sum(st.T * po.log_normalize(lw), axis=1), rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(o["loglik"], _stable_loglik(np.array(all_lw)), rtol=RTOL, atol=ATOL)
    return np.array(all_lw)


def test_one_dominant_particle(ctx, monkeypatch):
    """ln W ~ 0 although all weights but one vanish: the scan total says where the level is, not how many carry it."""
    N, Tw, who = 65, 4, 17
    rs = np.random.RandomState(6)
    x0 = rs.normal(scale=2.0, size=(N, 1))
    logw0 = rs.normal(scale=1.5, size=N)
    logw0[who] = logw0.max() + 600.0
    rest = np.delete(logw0, who)
    assert logw0[who] - rest.max() == 600.0 and np.exp(rest.max() - logw0[who]) < 1e-260
    assert abs(_lse(logw0) - logw0[who]) < 1e-12                 # ln W = 0 to rounding with the exact maximum as the shift
    y = _series("svm", Tw, seed=N + Tw)
    o = _launch_twins(ctx, monkeypatch, _problem(N, y, init_x=x0, init_logw=logw0))
    assert np.all(o["all_ancestors"][0] == who)
    _replay_warm(o, y, x0, logw0)


def _travelling_series(q, draws, targets):
    """y_t, step by step on the CPU, so that the oracle's lse_{t+1} hits targets[t]: lse_{t+1} falls monotonically in |y_t|
    from its value at y_t = 0 (bisection on the log-weights the oracle forms from the recorded draws)."""
    N, Tn = q["N"], len(targets)
    d = po.derived("svm", q["theta"])
    x = po.sample_x0("svm", q["prior_mean"], q["prior_var"], draws["rec_z0"])
    lw = np.zeros(N)
    y = np.zeros(Tn)
    for t in range(Tn):
        xp = x[po.device_ancestors(lw, draws["rec_u"][t], NT, PPT, "fixed32")]
        xn = po.kernel_rv("svm", "prior", d, xp, np.array([0.0]), draws["rec_z"][t])        # the prior proposal does not read y
        level = lambda v: float(_lse(po.kernel_reweight("svm", "prior", d, xp, xn, np.array([v]))))
        assert level(0.0) > targets[t]
        a, b = 0.0, 1.0
        while level(b) > targets[t]:
            b *= 4.0
        for _ in range(200):
            mid = 0.5 * (a + b)
            if level(mid) > targets[t]:
                a = mid
            else:
                b = mid
        y[t] = 0.5 * (a + b)
        x, lw = xn, po.kernel_reweight("svm", "prior", d, xp, xn, np.array([y[t]]))
    return y


def test_level_that_travels(ctx, monkeypatch):
    N, Tn, turn = 65, 70, 45
    targets = np.array([-40.0 * (t + 1) if t < turn else -40.0 * turn + 60.0 * (t + 1 - turn) for t in range(Tn)])
    q = _problem(N, np.zeros(Tn))
    draws = _record_draws(ctx, q)
    q["y"] = _travelling_series(q, draws, targets)
    o = _launch_twins(ctx, monkeypatch, q)
    assert _same_draws(o, draws)
    ref = _oracle(q, o)
    lse = _lse(ref["all_log_weights"])
    steps = np.abs(np.diff(lse))
    print("lse from", float(lse.max()), "down to", float(lse.min()), "and back to", float(lse[-1]), "largest step", float(steps.max()))
    assert lse.max() - lse.min() > 1500.0 and lse[-1] - lse.min() > 1000.0 and steps.max() < 100.0
    np.testing.assert_allclose(lse[1:], targets, rtol=0, atol=1e-6)
    _assert_replayed(o, ref, _stable_loglik(ref["all_log_weights"]))


def test_nan_observation_gives_nan_and_goes_on(ctx, monkeypatch):
    """y[8] = NaN: the children of step 8 weigh NaN, W of step 9 is no normal number, the guard fails and the retry runs (an
    `if`, no loop); score component 0 is NaN and the log-likelihood is not finite.  The proposal does not read y: states stay finite, and so do the
    log-weights once the NaN shift has been replaced by a retry's exact maximum."""
    monkeypatch.setenv("PFGRAD_VARIANT", VARIANT)
    N = 65
    y = _series("svm", T, seed=N + T)
    y[8] = np.nan
    q = _problem(N, y)
    o = ctx.run_batch([dict(q)], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == VARIANT and ctx.last_traced()
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == VARIANT and not ctx.last_traced()
    assert np.array_equal(plain["mean_stat"], o["mean_stat"], equal_nan=True)
    # (the kernel's table exp maps NaN to 0: W of step 9 is 0 and its log-likelihood term log(0) = -inf, or NaN)
    assert not np.isfinite(plain["loglik"]) and not np.isfinite(o["loglik"]) and np.isnan(o["mean_stat"][0])
    assert np.all(np.isnan(o["all_log_weights"][9]))
    assert np.all(np.isfinite(o["all_x_t"]))
    assert np.all(np.isfinite(o["all_log_weights"][:9])) and np.all(np.isfinite(o["all_log_weights"][11:]))


def test_retrying_and_ordinary_window_in_one_launch(ctx, monkeypatch, guard_inputs):
    """The guard is decided per workgroup: a window that retries beside one that does not -- each as alone, bitwise."""
    monkeypatch.setenv("PFGRAD_VARIANT", VARIANT)
    N = 1000
    qa = _problem(N, _series("svm", T, seed=N + T), seed=77)
    qb = guard_inputs[(N, "outside")][0]
    both = ctx.run_batch([dict(qa), dict(qb)])
    assert ctx.last_variant() == VARIANT
    for q, got in zip((qa, qb), both):
        alone = ctx.run_batch([dict(q)])[0]
        assert np.array_equal(alone["mean_stat"], got["mean_stat"]) and alone["loglik"] == got["loglik"]
        assert np.all(np.isfinite(got["mean_stat"])) and np.isfinite(got["loglik"])
