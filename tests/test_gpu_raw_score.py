"""The SVM prior 256 x 4 kernel (wg256x4s, bench config c2) carries the Poyiadjis O(N) score of a plain window as raw sums
and scales them where a statistic leaves the kernel (PFG_OPT_RAWSCORE in csrc/pfg_reg_traits.hpp; the NumPy restatement
of the recursion: tests/test_raw_score_host.py).  The launch must still be what the oracle replays from its recorded draws:

  * a weighted buffered window (t1 = 4, tL = 20, weights in [0.5, 2]): the sum of the window weights with w_t != 1, the
    steps without a statistic on both sides of the window, the per-step conversion of the traced statistics;
  * an unweighted whole window (every w_t exactly 1);
  * a warm start carrying statistics: two launches of T = 12, the second from the first's final particles, log-weights
    and statistics, against the oracle's building blocks replayed over the 24 steps -- the conversion in and out with
    nonzero values;
  * a plain, a lambda = 0.9 and a filter window in one launch: each equals itself alone, bitwise, and each is what the
    oracle replays -- the general path stays in the original scale.

Helpers and criteria of tests/test_gpu_stale_shift.py / tests/test_gpu_device_replay.py: zero ancestor flips, RTOL / ATOL on
trajectories and log-weights, rtol 1e-8 / atol 1e-7 on all_statistics and mean_stat, the production twin bitwise equal to
the traced one.  Shapes: N = 1000 (the full kernel), 257 (slots beyond N in three of the four particle rows), 65 (one wave
nearly empty); T = 24."""
import numpy as np
import pytest

from oracle import pf_oracle as po
from test_gpu_device_replay import ATOL, RTOL, THETA, _series
from test_gpu_stale_shift import NT, PPT, SHAPES, T, VARIANT, _assert_replayed, _launch_twins, _problem, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

T1, TL = 4, 20


def _weights(n, seed):
    return np.random.RandomState(seed).uniform(0.5, 2.0, size=n)


def _oracle_window(q, o, pf="poyiadjis_N", lambduh=1.0):
    """test_gpu_stale_shift._oracle with the window (t1, tL, weights) and the smoother passed on to po.pf_window"""
    words = o["rec_u"]
    with np.errstate(divide="ignore"):
        return po.pf_window("svm", q["theta"], q["y"], q["N"], o["rec_z0"], None, o["rec_z"], kernel="prior", pf=pf, lambduh=lambduh,
                            stat="score", t1=q["t1"], tL=q["tL"], weights=q.get("weights"), prior_mean=q["prior_mean"],
                            prior_var=q["prior_var"], save_all=True,
                            resampler=lambda t, logw: po.device_ancestors(logw, words[t], NT, PPT, "fixed32"))


def _window_loglik(all_lw, t1, tL, weights):
    """sum over the window's steps of  w_t (max + log(mean(exp(lw - max))))"""
    lw = all_lw[1:]
    mx = lw.max(axis=1)
    wt = np.zeros(lw.shape[0])
    wt[t1:tL] = 1.0 if weights is None else weights[:tL - t1]
    return float(np.sum(wt * (mx + np.log(np.mean(np.exp(lw - mx[:, None]), axis=1)))))


@pytest.mark.parametrize("N", SHAPES)
def test_weighted_buffered_window_replayed_by_oracle(ctx, monkeypatch, N):
    q = _problem(N, _series("svm", T, seed=N + T), t1=T1, tL=TL, weights=_weights(TL - T1, N))
    o = _launch_twins(ctx, monkeypatch, q)
    ref = _oracle_window(q, o)
    assert np.all(ref["all_statistics"][:T1 + 1] == 0.0) and np.any(ref["all_statistics"][T1 + 1] != 0.0)
    _assert_replayed(o, ref, _window_loglik(ref["all_log_weights"], T1, TL, q["weights"]))
    assert np.all(o["all_statistics"][:T1 + 1] == 0.0)                   # nothing added before the window: exactly zero
    np.testing.assert_allclose(o["statistics"], ref["statistics"], rtol=RTOL, atol=1e-7)          # final_stats
    # behind the window the statistics are copied along the ancestors: the same values, resampled
    for t in range(TL, T):
        np.testing.assert_array_equal(o["all_statistics"][t + 1], o["all_statistics"][t][o["all_ancestors"][t]])


@pytest.mark.parametrize("N", SHAPES)
def test_unweighted_whole_window_replayed_by_oracle(ctx, monkeypatch, N):
    q = _problem(N, _series("svm", T, seed=N + T + 1), seed=424242)
    o = _launch_twins(ctx, monkeypatch, q)
    ref = _oracle_window(q, o)
    _assert_replayed(o, ref, _window_loglik(ref["all_log_weights"], 0, T, None))
    np.testing.assert_allclose(o["statistics"], ref["statistics"], rtol=RTOL, atol=1e-7)


@pytest.mark.parametrize("N", SHAPES)
def test_warm_start_carrying_statistics(ctx, monkeypatch, N):
    """Two launches of T = 12; the second starts from the first's final_x / final_logw / final_stats.  The oracle's window
    function has no warm start: the 24 steps are replayed from its building blocks on the two launches' recorded draws."""
    Th = T // 2
    y = _series("svm", T, seed=N + 3)
    w = _weights(T, N + 1)
    qa = _problem(N, y[:Th], weights=w[:Th])
    oa = _launch_twins(ctx, monkeypatch, qa)
    qb = _problem(N, y[Th:], weights=w[Th:], seed=99, init_x=oa["x_t"], init_logw=oa["log_weights"], init_stats=oa["statistics"])
    ob = _launch_twins(ctx, monkeypatch, qb)
    assert np.any(np.abs(oa["statistics"]) > 1.0)                          # the second launch starts from nonzero statistics
    np.testing.assert_array_equal(ob["all_x_t"][0], oa["x_t"])
    np.testing.assert_array_equal(ob["all_log_weights"][0], oa["log_weights"])
    np.testing.assert_array_equal(ob["all_statistics"][0], oa["statistics"])
    d = po.derived("svm", THETA["svm"])
    x = po.sample_x0("svm", qa["prior_mean"], qa["prior_var"], oa["rec_z0"])
    lw, st = np.zeros(N), np.zeros((N, 3))
    for t in range(T):
        o, tt = (oa, t) if t < Th else (ob, t - Th)
        anc = po.device_ancestors(lw, o["rec_u"][tt], NT, PPT, "fixed32")
        assert int(np.sum(anc != o["all_ancestors"][tt])) == 0, t
        yt = np.array([y[t]])
        xp = x[anc]
        xn = po.kernel_rv("svm", "prior", d, xp, yt, o["rec_z"][tt])
        st = st[anc] + w[t] * po.score_statistic("svm", d, xp, xn, yt)
        x, lw = xn, po.kernel_reweight("svm", "prior", d, xp, xn, yt)
        np.testing.assert_allclose(o["all_x_t"][tt + 1], x, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(o["all_log_weights"][tt + 1], lw, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(o["all_statistics"][tt + 1], st, rtol=RTOL, atol=1e-7)
        if t == Th - 1:
            np.testing.assert_allclose(oa["statistics"], st, rtol=RTOL, atol=1e-7)
            np.testing.assert_allclose(oa["mean_stat"], np.sum(st.T * po.log_normalize(lw), axis=1), rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(ob["statistics"], st, rtol=RTOL, atol=1e-7)
    np.testing.assert_allclose(ob["mean_stat"], np.sum(st.T * po.log_normalize(lw), axis=1), rtol=RTOL, atol=1e-7)


@pytest.mark.parametrize("N", SHAPES)
def test_plain_and_non_plain_windows_in_one_launch(ctx, monkeypatch, N):
    """A raw window beside a lambda = 0.9 and a filter window (general path, original scale): each as alone, bitwise, and each
    replayed by the oracle."""
    monkeypatch.setenv("PFGRAD_VARIANT", VARIANT)
    y = _series("svm", T, seed=N + 7)
    w = _weights(TL - T1, N + 2)
    qs = [(_problem(N, y, t1=T1, tL=TL, weights=w, seed=1), "poyiadjis_N", 1.0),
          (_problem(N, y, t1=T1, tL=TL, weights=w, seed=2, lambduh=0.9), "nemeth", 0.9),
          (_problem(N, y, t1=T1, tL=TL, weights=w, seed=3, smoother="filter"), "filter", 1.0)]
    both = ctx.run_batch([dict(q) for q, _, _ in qs], want_trace=True, want_draws=True)
    assert ctx.last_variant() == VARIANT and ctx.last_traced()
    production = ctx.run_batch([dict(q) for q, _, _ in qs])
    assert ctx.last_variant() == VARIANT and not ctx.last_traced()
    for (q, pf, lam), got, prod in zip(qs, both, production):
        alone = ctx.run_batch([dict(q)], want_trace=True, want_draws=True)[0]
        for k in ("mean_stat", "all_x_t", "all_log_weights", "all_ancestors") + (() if pf == "filter" else ("all_statistics", "statistics")):
            assert np.array_equal(alone[k], got[k]), (pf, k)
        assert alone["loglik"] == got["loglik"]
        assert np.array_equal(prod["mean_stat"], got["mean_stat"]), pf       # production twin, the three in one launch
        ref = _oracle_window(q, got, pf=pf, lambduh=lam)
        assert int(np.sum(got["all_ancestors"] != ref["all_ancestors"])) == 0, pf
        np.testing.assert_allclose(got["all_x_t"], ref["all_x_t"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got["all_log_weights"], ref["all_log_weights"], rtol=RTOL, atol=ATOL)
        if pf == "filter":
            np.testing.assert_allclose(got["mean_stat"], ref["statistics"], rtol=RTOL, atol=1e-7)
        else:
            np.testing.assert_allclose(got["all_statistics"], ref["all_statistics"], rtol=RTOL, atol=1e-7)
            np.testing.assert_allclose(got["mean_stat"], ref["mean_statistic"], rtol=RTOL, atol=1e-7)
        np.testing.assert_allclose(got["loglik"], _window_loglik(ref["all_log_weights"], T1, TL, w), rtol=RTOL, atol=ATOL)
