"""Recorded-draw replay of the DEVICE-generator kernels on the SUFFICIENT and the EMPTY statistic, and mixed-statistic batches.

tests/test_gpu_device_replay.py, test_gpu_grid.py and test_gpu_stratified.py replay the device-generator units on the
score only.  stat='suff' (pf_latent_var_distr) and stat='none' (pf_loglikelihood_estimate, noisy_logjoint) are other
instantiations of the whole timestep body -- slots(SUFF) in pf_reg_kernel, sweep(SUFF) in pf_big_kernel, propagate(SUFF) in
the whole-GPU timestep kernel, and the SVM 256 x 4 unit's particle_step_svm_tuned, whose sufficient-statistic branch no
other test enters -- and 'none' takes the "plain, no statistic" branch of `children` for every step.  The method is that of
test_device_kernel_replayed_by_oracle, unchanged: the traced launch records the words / uniforms it searched the CDF with
and its normals, po.pf_window(stat=...) replays the launch on them with the unit's CDF layout as its resampler, and
trajectories, ancestors (zero flips), log-weights, running log-likelihood, per-particle statistics, their weighted mean and
the log-likelihood must agree at that test's tolerances (rtol 1e-8, statistics atol 1e-7; the whole-GPU rows at those of
test_giant_device_launch_replayed_by_oracle).  They bound the same error sources -- fused multiply-adds, the cubic expm1
under 3e-12 --; the sufficient statistic adds only products of particle states.

Every case has t1 > 0, tL < T and importance weights linspace(20, 30), so steps before, inside and after the window run;
the estimator (a run-time branch) is spread over the table: poyiadjis_N (branches 0 / 1 of `children`), nemeth with
lambduh = 0.9 (branch 2) and the filter.  Then three f32 teacher-forced cases, and batches that mix score, suff and none
windows: pfg_run_batch must plan the general kernel for them (the score-only `_score1` twins answer any other window with
NaNs) and every window must equal itself run alone, bit for bit.

PaRIS on the device generator is in tests/test_gpu_paris_device_replay.py (replayed from the backward parents its traced
launch returns), the O(N^2) units are in tests/test_gpu_n2_device_replay.py."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_gpu_device_replay import THETA, _series, _assert_twin_statistics
from test_gpu_grid import grid_device_ancestors
from test_gpu_stratified import _prior

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import stratified_model  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL, STAT_ATOL = 1e-8, 1e-8, 1e-7       # test_gpu_device_replay.py::test_device_kernel_replayed_by_oracle
GRID_STAT_TOL = 1e-7                           # test_gpu_grid.py::test_giant_device_launch_replayed_by_oracle (rtol = atol)

# (threads, particles per thread) of the LDS-resident units: their CDF runs thread-major over NT * PPT slots of 32-bit words
REG_LAYOUT = {"wg256x4s": (256, 4), "wg256x4": (256, 4), "wg256x1": (256, 1), "wg64x2": (64, 2), "wg64x2s": (64, 2),
              "wg64x4": (64, 4), "wg64x4s": (64, 4), "wg512x2s": (512, 2), "wg1024x1": (1024, 1), "wg1024x4s": (1024, 4)}
BIG_SLOTS = {"big4096": 4096, "big16384": 16384}
STRATIFIED = ("stratified256x4", "big4096_stratified", "big16384_stratified")

P, NM, F = ("poyiadjis_N", 1.0), ("nemeth", 0.9), ("filter", 1.0)
# three estimators x {suff, none} spread so that every unit sees suff with two estimators and none with one
SPREAD = {"A": [(P, "suff"), (NM, "suff"), (F, "none")],
          "B": [(P, "suff"), (F, "suff"), (NM, "none")],
          "C": [(NM, "suff"), (F, "suff"), (P, "none")],
          # stratified resampling is built for the NEMETH recursion alone
          "S": [(P, "suff"), (NM, "suff"), (NM, "none")],
          "S2": [(P, "suff"), (NM, "suff"), (P, "none")]}

# unit, model, kernel, N, T, spread: N the smallest that needs the unit and leaves its last per-thread slot ragged, unless
# the row is there for another edge (1024: every slot of the 256 x 4 unit; 777 / 600: the bench unit's ragged sizes)
UNITS = [
    ("wg256x4s", "svm", "prior", 777, 24, "A"),              # the STALE / STEP_TUNE instantiation: particle_step_svm_tuned
    ("wg256x4s", "svm", "prior", 1024, 24, [(NM, "suff"), (P, "none")]),
    ("wg256x4s", "garch", "optimal", 600, 24, "B"),          # suff has an x^4 column
    ("wg256x4", "svm", "prior", 900, 24, "C"),
    ("wg256x1", "svm", "prior", 129, 24, "A"),
    ("wg64x2", "lgssm", "prior", 65, 24, "B"),
    ("wg64x2s", "lgssm", "optimal", 100, 24, "C"),
    ("wg64x4", "lgssm", "optimal", 200, 24, "A"),
    ("wg64x4s", "svm", "prior", 256, 24, "B"),
    ("wg512x2s", "garch", "prior", 1000, 24, "C"),
    ("wg1024x1", "svm", "prior", 1000, 24, "A"),
    ("wg1024x4s", "svm", "prior", 1025, 12, "B"),
    ("big4096", "garch", "optimal", 1500, 12, "C"),
    ("big16384", "svm", "prior", 4097, 12, "A"),
    ("grid1024", "svm", "prior", 20000, 5, "B"),
    ("grid1024", "lgssm", "optimal", 17000, 5, [(F, "suff")]),
    ("grid2048", "svm", "prior", 600000, 3, "B"),
    ("stratified256x4", "svm", "prior", 1000, 24, "S"),
    ("big4096_stratified", "garch", "optimal", 1500, 12, "S2"),
    ("big16384_stratified", "lgssm", "optimal", 4097, 12, "S"),
]
CASES = [(unit, model, kernel, N, T, pf, lam, stat)
         for unit, model, kernel, N, T, spread in UNITS
         for (pf, lam), stat in (SPREAD[spread] if isinstance(spread, str) else spread)]
assert len(CASES) < 60


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def _window(T):
    """t1 > 0 and tL < T: (4, 20) of 24, (2, 10) of 12, (1, 4) of 5, (1, 2) of 3."""
    edge = max(1, T // 6)
    return edge, T - edge


def _problem(unit, model, kernel, N, T, pf, lam, stat, dtype="f64", stream=None):
    t1, tL = _window(T)
    pm, pv = _prior(model)
    smoother = "filter" if pf == "filter" else "nemeth_stratified" if unit in STRATIFIED else "nemeth"
    return dict(model=model, kernel=kernel, smoother=smoother, stat=stat, dtype=dtype, rng="device", N=N, t1=t1, tL=tL,
                lambduh=lam, prior_mean=pm, prior_var=pv, y=_series(model, T, seed=N + T), weights=np.linspace(20.0, 30.0, tL - t1),
                theta=THETA[model], seed=20261018 + N, stream=T if stream is None else stream)


def _force(monkeypatch, unit):
    """PFGRAD_VARIANT for the unit: a tag of the LDS-resident table, 'big' for the large-N kernel also where wg1024x4s
    would fit, 'grid' for the whole-GPU window; the stratified twins are chosen by the smoother."""
    if unit in STRATIFIED:
        monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    else:
        monkeypatch.setenv("PFGRAD_VARIANT", "big" if unit in BIG_SLOTS else "grid" if unit.startswith("grid") else unit)


def _resampler(unit, o):
    """(t, logw) -> ancestors in the unit's CDF layout, on the resampling inputs the launch recorded; and the flip
    counter of the whole-GPU rows, which continue on the kernel's ancestors as test_giant_device_launch_replayed_by_oracle
    does (0 elsewhere: there the oracle's ancestors are compared afterwards)."""
    N = o["rec_z"].shape[1]
    flips = [0]
    if unit in REG_LAYOUT:
        NT, PPT = REG_LAYOUT[unit]
        words = o["rec_u"]
        assert np.any(words != 0)
        return (lambda t, logw: po.device_ancestors(logw, words[t], NT, PPT, "fixed32")), flips
    ud = o["rec_ud"]
    assert np.all((ud >= 0.0) & (ud < 1.0)) and np.any(ud != 0.0)
    if unit in BIG_SLOTS:
        assert np.all(np.diff(ud, axis=1) >= 0.0)              # sorted uniforms; PPT = 1: child index = rank
        return (lambda t, logw: po.device_ancestors(logw, ud[t], BIG_SLOTS[unit], 1, "f64_uniform")), flips
    if unit in STRATIFIED:
        r = np.arange(N)
        assert np.all(ud >= r / N) and np.all(ud < (r + 1) / N)
        return (lambda t, logw: stratified_model.device_ancestors(logw, ud[t], unit)), flips
    TILE = {"grid1024": 1024, "grid2048": 2048}[unit]
    assert np.all(np.diff(ud, axis=1) >= 0.0)

    def resampler(t, logw):
        flips[0] += int(np.sum(grid_device_ancestors(logw, ud[t], TILE) != o["all_ancestors"][t]))
        return o["all_ancestors"][t].astype(np.int64)
    return resampler, flips


def _full_width(a, model):
    """run_batch returns the statistics cut to the oracle's three columns: the array the kernel wrote, STAT_DIM wide
    (GARCH and LGSSM: four columns, so the check of the fourth is not empty; SVM has three)."""
    from sgmcmc_ssm_amd import _capi
    full = a.base if a.base is not None else a
    assert full.shape[:-1] == a.shape[:-1] and full.shape[-1] == _capi.STAT_DIM[model], (full.shape, a.shape, model)
    return full


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{0}-{1}-{2}-N{3}-{5}-{7}".format(*c))
def test_device_kernel_replayed_on_suff_and_none(ctx, monkeypatch, case):
    unit, model, kernel, N, T, pf, lam, stat = case
    grid = unit.startswith("grid")
    q = _problem(unit, model, kernel, N, T, pf, lam, stat)
    _force(monkeypatch, unit)
    o = ctx.run_batch([q], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == unit                # the unit under test ran, and no score-only twin of it
    # the production launch (same key, no trace buffers: what pf_latent_var_distr / pf_loglikelihood_estimate launch)
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == unit and not ctx.last_variant().endswith("_score1")
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]), (plain["mean_stat"], o["mean_stat"])
    assert abs(plain["loglik"] - o["loglik"]) <= 1e-12 * abs(o["loglik"])

    z, z0 = o["rec_z"], o["rec_z0"]
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(z0)) and np.any(z != 0.0) and np.any(z0 != 0.0)
    resampler, flips = _resampler(unit, o)
    ref = po.pf_window(model, q["theta"], q["y"], N, z0, None, z, kernel=kernel, pf=pf, lambduh=lam, stat=stat, t1=q["t1"],
                       tL=q["tL"], weights=q["weights"], prior_mean=q["prior_mean"], prior_var=q["prior_var"], save_all=True,
                       resampler=resampler)
    nflip = flips[0] + int(np.sum(o["all_ancestors"] != ref["all_ancestors"]))
    assert nflip == 0, "{0} ancestor indices differ".format(nflip)
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"], ref["all_loglikelihood_estimate"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=RTOL, atol=ATOL)
    srtol, satol = (GRID_STAT_TOL, GRID_STAT_TOL) if grid else (RTOL, STAT_ATOL)
    assert o["mean_stat"].shape == (3,)
    if pf != "filter":
        assert ref["all_statistics"].shape == o["all_statistics"].shape == (T + 1, N, 3)
        np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=srtol, atol=satol)
        np.testing.assert_allclose(o["statistics"], ref["statistics"], rtol=srtol, atol=satol)
        np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=srtol, atol=satol)
        if stat == "suff":
            # the record is STAT_DIM wide (GARCH and LGSSM carry a fourth slot): nothing beyond the three columns
            assert np.all(_full_width(o["all_statistics"], model)[..., 3:] == 0.0)
            assert np.all(_full_width(o["statistics"], model)[..., 3:] == 0.0)
            # before the window nothing is accumulated, inside it every particle's x^2 column is
            t1 = q["t1"]
            assert np.all(o["all_statistics"][:t1 + 1] == 0.0) and np.all(o["all_statistics"][t1 + 1][:, 1] > 0.0)
    else:
        np.testing.assert_allclose(o["mean_stat"], ref["statistics"], rtol=srtol, atol=satol)
    if stat == "none":
        assert np.all(o["mean_stat"] == 0.0) and np.all(plain["mean_stat"] == 0.0)
        if pf != "filter":
            assert np.all(_full_width(o["all_statistics"], model) == 0.0) and np.all(_full_width(o["statistics"], model) == 0.0)
        assert o["loglik"] != 0.0 and np.isfinite(o["loglik"])
    else:
        assert np.all(o["mean_stat"] != 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# f32 particle state, teacher-forced (after test_gpu_device_replay.py::test_f32_state_device_kernels_replayed)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kernel,N,T,variant", [("svm", "prior", 1000, 24, "wg256x4"),
                                                     ("garch", "optimal", 1000, 24, "wg256x4"),
                                                     ("svm", "prior", 4000, 16, "wg1024x4s")])
def test_f32_state_device_kernels_replayed_on_suff(ctx, monkeypatch, model, kernel, N, T, variant):
    """dtype='f32', stat='suff', at the tolerances of test_f32_state_device_kernels_replayed: from the kernel's own traced
    particles, log-weights and statistics of step t, the oracle's resampling (on the recorded words), proposal, weight and
    po.sufficient_statistic give step t + 1 -- particles 2e-5, log-weights 2e-4, statistics 2e-4 of their scale, at most
    max(3, 2e-4 T N) ancestors off."""
    NT, PPT = REG_LAYOUT[variant]
    theta = THETA[model]
    y = _series(model, T, seed=3 * N + T)
    pm, pv = _prior(model)
    q = dict(model=model, kernel=kernel, smoother="nemeth", stat="suff", dtype="f32", rng="device", N=N, t1=0, tL=T,
             lambduh=1.0, prior_mean=pm, prior_var=pv, y=y, theta=theta, seed=777 + N, stream=T)
    monkeypatch.setenv("PFGRAD_VARIANT", variant)
    o = ctx.run_batch([q], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == variant
    words, z = o["rec_u"], o["rec_z"]
    d = po.derived(model, theta)
    flips = 0
    for t in range(T):
        x, lw, st = o["all_x_t"][t], o["all_log_weights"][t], o["all_statistics"][t]
        anc = po.device_ancestors(lw, words[t], NT, PPT, "fixed32")
        got = o["all_ancestors"][t]
        flips += int(np.sum(anc != got))
        yt = np.array([y[t]])
        xp = x[got]
        xn = po.kernel_rv(model, kernel, d, xp, yt, z[t])
        np.testing.assert_allclose(o["all_x_t"][t + 1], xn, rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(o["all_log_weights"][t + 1], po.kernel_reweight(model, kernel, d, xp, xn, yt), rtol=2e-4, atol=2e-4)
        ref_st = st[got] + po.sufficient_statistic(model, xp, xn)
        scale = np.maximum(1.0, np.abs(ref_st).max())
        assert np.max(np.abs(o["all_statistics"][t + 1] - ref_st)) < 2e-4 * scale, t
    assert flips <= max(3, int(2e-4 * T * N)), flips
    assert np.all(_full_width(o["all_statistics"], model)[..., 3:] == 0.0)
    ref0 = pm + np.sqrt(pv) * o["rec_z0"]
    np.testing.assert_allclose(o["all_x_t"][0][:, 0], ref0, rtol=2e-6, atol=2e-6)


# ---------------------------------------------------------------------------------------------------------------------
# mixed-statistic batches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,force,general", [(1000, 24, None, "wg1024x1"), (1000, 24, "wg1024x4s", "wg1024x4s"),
                                               (20000, 4, None, "grid1024")])
def test_mixed_statistic_batch_runs_the_general_kernel(ctx, monkeypatch, N, T, force, general):
    """Nine device-generator windows in one pfg_run_batch (SVM prior, distinct streams): three score windows with
    lambduh = 1, three suff, three none.  The plan keeps a score-only twin only when EVERY window is (NEMETH, lambduh = 1,
    score); a twin answers any other window with NaNs, which a log-likelihood-only caller would not see.  So: the mixed
    batch runs the general kernel, and every window's mean_stat and loglik are bitwise those of the window run alone on
    that kernel (PFGRAD_NO_SCORE1=1 keeps a lone score window off its twin); so are the six score and suff windows as a
    batch of their own.  Control: the three score windows as their
    own batch do run a `_score1` variant -- the twin of the same unit -- and agree with the mixed batch at rtol 1e-13,
    what _assert_twin_statistics allows between a unit and its twin.  N = 1000 on the plan's own choice for a small batch
    (wg1024x1) and on the 1024 x 4 unit (forced; the SVM 256 x 4 device units have no score-only twin), N = 20000 on the whole-GPU window (grid1024 against
    grid1024_score1)."""
    if force is None:
        monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    else:
        monkeypatch.setenv("PFGRAD_VARIANT", force)
    monkeypatch.delenv("PFGRAD_NO_SCORE1", raising=False)
    stats = ["score", "suff", "none"] * 3
    qs = [_problem("plan", "svm", "prior", N, T, "poyiadjis_N", 1.0, stat, stream=100 + i) for i, stat in enumerate(stats)]
    mixed = ctx.run_batch([dict(q) for q in qs])
    variant = ctx.last_variant()
    assert not variant.endswith("_score1"), variant
    assert variant == general
    for o, stat in zip(mixed, stats):
        assert np.all(np.isfinite(o["mean_stat"])) and np.isfinite(o["loglik"]) and o["loglik"] != 0.0
        assert np.all(o["mean_stat"] == 0.0) == (stat == "none")
    # distinct streams: no two windows share a log-likelihood
    assert len({o["loglik"] for o in mixed}) == len(mixed)

    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    for i, q in enumerate(qs):
        alone = ctx.run_batch([dict(q)])[0]
        assert ctx.last_variant() == variant
        assert np.array_equal(alone["mean_stat"], mixed[i]["mean_stat"]), (i, stats[i], alone["mean_stat"], mixed[i]["mean_stat"])
        assert alone["loglik"] == mixed[i]["loglik"], (i, stats[i])
    monkeypatch.delenv("PFGRAD_NO_SCORE1")

    # score and suff windows alone (no `none` window that would also rule the twin out): still the general kernel
    pair = [i for i, stat in enumerate(stats) if stat != "none"]
    both = ctx.run_batch([dict(qs[i]) for i in pair])
    assert ctx.last_variant() == variant
    for o, i in zip(both, pair):
        assert np.array_equal(o["mean_stat"], mixed[i]["mean_stat"]) and o["loglik"] == mixed[i]["loglik"], (i, stats[i])

    idx = [i for i, stat in enumerate(stats) if stat == "score"]
    control = ctx.run_batch([dict(qs[i]) for i in idx])
    twin = ctx.last_variant()
    assert twin == variant + "_score1", (twin, variant)
    for o, i in zip(control, idx):
        _assert_twin_statistics(o["mean_stat"], mixed[i]["mean_stat"], twin, where=i)
        assert abs(o["loglik"] - mixed[i]["loglik"]) <= 1e-13 * abs(mixed[i]["loglik"])
