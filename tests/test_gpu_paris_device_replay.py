"""GPU: PaRIS on the device generator (pf='paris', rng='device': what ChainEnsemble(pf='paris') launches) against a
deterministic reference.

The device instantiations were checked statistically only (mean score and log-likelihood of 256 windows within 5 standard
errors, at 64 accept-reject rounds) and the REPLAY pool tests pin other translation units -- and other code: the exact
categorical fallback of pf_reg_kernel's paris_slots has a branch of its own for the device generator (parents enumerated
lane-major, per-lane running sums, one wave scan, the owner lane resolved by readlane; the block maximum in fp64, an exact
wave maximum in f32).  Here a traced launch hands back the normals it drew (rec_z0, rec_z), the ancestors and the
backward-sampled parents of every child and draw (all_paris_J), and

(a) po.pf_window(pf='paris') replays the SAME launch of the LDS-resident units on them -- trajectories, log-weights,
    running log-likelihood, statistics, their weighted mean -- at the tolerances of
    test_gpu_n2_device_replay.py::test_256_thread_device_kernels_replayed_by_oracle (these units are built with fused
    multiply-adds and the cubic expm1, like the units that test pins);
(b) paris_mem1024 (N > 1024) records them too, and the uniform every child searched the filter CDF with (rec_ud):
    test_large_n_device_kernel_replayed_by_oracle replays it as (a) -- proposal, x0 and parent records included -- on
    SVM, GARCH and LGSSM, both proposals, at every chunk edge (MEM_REPLAY_CASES), and DERIVES its ancestors (e).
    test_large_n_device_kernel_teacher_forced stays: N = 1100 from the unit's own trace (forced_window.forced_paris_steps),
    x_{t+1} taken as traced;
(c) the parents themselves cannot be replayed -- the backward uniforms are not recorded -- so their LAW is tested from
    the trace: every J is a draw from the exact backward law of its child, whether it left an accept-reject round or the
    fallback (forced_window.backward_law_scores, both scores below 5); likewise the ancestors of the LDS-resident units,
    which record no resampling uniform (ancestor_law_score).
    tests/test_forced_paris_host.py shows the scores passing on the oracle's own parents and failing on four wrong
    samplers at every (model, N, T, Ntilde) of REG_CASES, MEM_CASES and F32_CASES, and why T is what it is: 24 below
    N = 700 and 6 at N = 1100, and longer for three GARCH cases, whose backward law is close to the filter weights.  On
    MEM_REPLAY_CASES the scores run up to N = 2049 as a sanity check, with no claim of power;
(d) f32 state (the fallback's other maximum), teacher-forced at the f32 tolerances of test_one_wave_pool_parity_f32; on
    paris_mem1024 with the proposal checked on the recorded normals (test_large_n_f32_state_teacher_forced);
(e) paris_mem1024's filter ancestors are derived, not taken: po.particle_order_ancestors (the unit's CDF in particle order,
    pinned to np.random.choice by tests/test_mem_resampling_host.py) on the traced log-weights and rec_ud, exactly, but
    for children whose uniform sits within 1e-10 of a CDF entry.

Three regimes of the backward sampler: max_accept_reject = 64 (the default: accept-reject dominates), 2 (most children
queue for the fallback) and 0 (what accept_reject=False launches: every draw of every child goes through the device-only
categorical branch).  Every case: window [t1, tL) = [2, T - 1) ([1, T - 1) for paris_mem1024) with weights
linspace(20, 30); the production launch of the same key returns mean_stat and loglik bit for bit."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_host_logic import default_params, GEN
from test_gpu_n2_one_wave import _prior_x

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import forced_window  # noqa: E402

pytestmark = pytest.mark.gpu

# unit, model, kernel, N, T, Ntilde, max_accept_reject, stat.  N: 100 ragged second slot of the wave, 128 every slot full;
# 200 ragged single slot; 700 third slot ragged, fourth empty, 11 of 16 parent chunks live in the fallback.
# max_accept_reject = 0 at least once per unit, and once per model on paris256x4.  T: the smallest at which all four wrong
# samplers of tests/test_forced_paris_host.py fail the law test at this (model, N, Ntilde) -- that file reads these tables.
REG_CASES = [
    ("paris64x2", "svm", "prior", 100, 24, 3, 0, "score"),
    ("paris64x2", "lgssm", "optimal", 100, 24, 3, 2, "suff"),
    ("paris64x2", "garch", "optimal", 128, 96, 3, 64, "score"),
    ("paris64x2", "lgssm", "prior", 128, 24, 3, 0, "suff"),
    ("paris256x1", "svm", "prior", 200, 24, 2, 2, "score"),
    ("paris256x1", "garch", "prior", 200, 48, 3, 0, "suff"),
    ("paris256x1", "lgssm", "optimal", 200, 24, 2, 64, "score"),
    ("paris256x4", "svm", "prior", 700, 6, 3, 0, "score"),
    ("paris256x4", "garch", "optimal", 700, 12, 3, 0, "suff"),
    ("paris256x4", "lgssm", "optimal", 700, 6, 2, 0, "score"),
    ("paris256x4", "svm", "prior", 700, 6, 3, 2, "suff"),
    ("paris256x4", "garch", "prior", 700, 6, 2, 64, "score"),
]
# N = 1100: the smallest N the plan sends to the large-N kernel; SVM prior only
MEM_CASES = [(3, 0, "score"), (3, 2, "suff"), (2, 64, "score")]
F32_CASES = [("paris64x2", "svm", "prior", 100, 24, 3), ("paris256x4", "lgssm", "optimal", 700, 6, 2)]
# paris_mem1024 replayed on its recorded draws: model, kernel, N, T, Ntilde, max_accept_reject, stat.  The unit works in chunks
# of 1024 particles and pads its CDF to a power of two.  N = 1025: the second chunk holds one particle; 2048: every chunk
# full, N is the padded size (no sentinel entries), GARCH's two-component record; 2049: the third chunk holds one particle;
# 4097: five chunks, every draw through the fallback; 8193: nine chunks, a padded CDF of 16384.
MEM_REPLAY_CASES = [
    ("svm", "prior", 1025, 6, 3, 0, "score"),
    ("garch", "optimal", 2048, 6, 2, 2, "suff"),
    ("lgssm", "optimal", 2049, 6, 2, 64, "score"),
    ("garch", "prior", 4097, 4, 2, 0, "score"),
    ("svm", "prior", 8193, 3, 2, 64, "score"),
]
MEM_F32_CASES = [("svm", "prior", 1100), ("lgssm", "optimal", 2049)]


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def _device_problem(model, kernel, stat, N, T, t1, tL, Ntilde, R, dtype="f64"):
    p = default_params(model)
    theta = p.theta()
    np.random.seed(17)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    pm, pv = _prior_x(model, theta)
    return dict(model=model, kernel=kernel, smoother="paris", stat=stat, dtype=dtype, rng="device", N=N, t1=t1, tL=tL,
                lambduh=1.0, prior_mean=pm, prior_var=pv, y=y, weights=np.linspace(20.0, 30.0, tL - t1), theta=theta,
                Ntilde=Ntilde, max_accept_reject=R, seed=20261019 + N, stream=8 * T + Ntilde + R + (1000 if dtype == "f32" else 0))


def _traced_and_production(ctx, monkeypatch, unit, q, want_draws):
    """The traced launch of q on `unit`; the production launch of the same key returns the same record bit for bit."""
    if unit == "paris_mem1024":
        monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    else:
        monkeypatch.setenv("PFGRAD_VARIANT", unit)
    o = ctx.run_batch([q], want_trace=True, want_draws=want_draws)[0]
    assert ctx.last_variant() == unit
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == unit
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]) and plain["loglik"] == o["loglik"]
    N, T, Ntilde = q["N"], len(q["y"]), q["Ntilde"]
    J, anc = o["all_paris_J"], o["all_ancestors"]
    assert J.shape == (T, Ntilde, N) and J.dtype == np.int32
    assert J.min() >= 0 and J.max() < N and anc.min() >= 0 and anc.max() < N
    # the draws of a child are not copies of one another, nor of its filter ancestor
    assert np.any(J[:, 0] != J[:, 1]) and np.any(J[:, 0] != anc)
    return o


def _assert_laws(tag, q, o):
    """(c) the backward parents follow the exact backward law of the traced particles and weights, the ancestors the
    multinomial law of the traced weights."""
    N, T, Ntilde = q["N"], len(q["y"]), q["Ntilde"]
    J = np.transpose(o["all_paris_J"], (0, 2, 1))
    zp, zx, terms = forced_window.backward_law_scores(q["model"], po.derived(q["model"], q["theta"]), o["all_x_t"],
                                                      o["all_log_weights"], J)
    print("backward law", tag, "Z_p = {0:.3f} Z_x = {1:.3f} terms = {2}".format(zp, zx, terms))
    assert terms == T * N * Ntilde
    assert abs(zp) < 5.0 and abs(zx) < 5.0, (zp, zx, terms)
    score, steps = forced_window.ancestor_law_score(o["all_log_weights"], o["all_ancestors"])
    print("ancestor law", tag, score, steps)
    assert steps == T - 1 and score < 5.0, (score, steps)


@pytest.mark.parametrize("case", REG_CASES, ids=lambda c: "{0}-{1}-{2}-N{3}-Nt{5}-R{6}-{7}".format(*c))
def test_lds_resident_device_units_replayed_by_oracle(ctx, monkeypatch, case):
    """(a) + (c): the oracle replays the launch on its recorded normals, with the traced ancestors and the traced backward
    parents given.  Statistics at or before t1 are exactly 0 and non-zero behind it."""
    unit, model, kernel, N, T, Ntilde, R, stat = case
    t1, tL = 2, T - 1
    q = _device_problem(model, kernel, stat, N, T, t1, tL, Ntilde, R)
    o = _traced_and_production(ctx, monkeypatch, unit, q, want_draws=True)
    z, z0, anc, J = o["rec_z"], o["rec_z0"], o["all_ancestors"], o["all_paris_J"]
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(z0)) and np.all(np.any(z != 0.0, axis=1)) and np.any(z0 != 0.0)
    ref = po.pf_window(model, q["theta"], q["y"], N, z0, None, z, kernel=kernel, pf="paris", stat=stat, t1=t1, tL=tL,
                       weights=q["weights"], prior_mean=q["prior_mean"], prior_var=q["prior_var"], save_all=True, Ntilde=Ntilde,
                       resampler=lambda t, logw: anc[t], paris_parents=lambda t: J[t].T)
    r, a = 1e-8, 1e-8
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"], ref["all_loglikelihood_estimate"], rtol=r, atol=a)
    assert o["all_statistics"].shape == ref["all_statistics"].shape
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=r, atol=1e-7)
    np.testing.assert_allclose(o["statistics"], ref["statistics"], rtol=r, atol=1e-7)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=r, atol=1e-7)
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=r, atol=a)
    assert np.all(o["all_statistics"][:t1 + 1] == 0.0) and np.all(np.any(o["all_statistics"][t1 + 1:] != 0.0, axis=(1, 2)))
    _assert_laws("{0} {1} {2} N={3} Nt={4} R={5} {6}".format(unit, model, kernel, N, Ntilde, R, stat), q, o)


def _assert_teacher_forced(q, o, lw_tol, st_tol, ll_rtol, mean_tol):
    """Step t + 1 of the trace from its step t (forced_window.forced_paris_steps); the running log-likelihood, the final
    statistics and their weighted mean follow from the traced log-weights and statistics."""
    T, t1, tL = len(q["y"]), q["t1"], q["tL"]
    J = np.transpose(o["all_paris_J"], (0, 2, 1))
    lw, st, dll = forced_window.forced_paris_steps(q["model"], q["kernel"], q["theta"], q["y"], o["all_x_t"],
                                                   o["all_log_weights"], o["all_statistics"], o["all_ancestors"], J,
                                                   stat=q["stat"], t1=t1, tL=tL, weights=q["weights"])
    np.testing.assert_allclose(o["all_log_weights"][1:], lw, rtol=lw_tol[0], atol=lw_tol[1])
    np.testing.assert_allclose(o["all_statistics"][1:], st, rtol=st_tol[0], atol=st_tol[1])
    np.testing.assert_allclose(o["all_loglikelihood_estimate"][1:], np.cumsum(dll), rtol=ll_rtol, atol=0)
    assert np.all(o["all_statistics"][:t1 + 1] == 0.0) and np.all(np.any(o["all_statistics"][t1 + 1:] != 0.0, axis=(1, 2)))
    np.testing.assert_allclose(o["statistics"], o["all_statistics"][T], rtol=0, atol=0)
    mean = np.sum(o["all_statistics"][T].T * po.log_normalize(o["all_log_weights"][T]), axis=1)
    np.testing.assert_allclose(o["mean_stat"], mean, rtol=mean_tol[0], atol=mean_tol[1])
    np.testing.assert_allclose(o["loglik"], o["all_loglikelihood_estimate"][T], rtol=1e-12, atol=0)
    assert np.all(np.isfinite(o["all_x_t"])) and np.all(o["all_log_weights"][0] == 0.0)


@pytest.mark.parametrize("Ntilde,R,stat", MEM_CASES)
def test_large_n_device_kernel_teacher_forced(ctx, monkeypatch, Ntilde, R, stat):
    """(b) + (c): paris_mem1024, SVM prior, N = 1100, T = 6, window [1, 5) (T = 3 leaves two steps with power against a
    sampler that drops the weights: tests/test_forced_paris_host.py), teacher-forced from the unit's own trace: x_{t+1} and
    the ancestors are taken as traced here -- test_large_n_device_kernel_replayed_by_oracle checks the proposal on the
    recorded normals and derives the ancestors.  Log-weights at rtol 1e-8, statistics at rtol 1e-8 / atol 1e-7, as
    test_gpu_n2_device_replay.py::test_large_n_device_kernel_teacher_forced."""
    model, kernel, N, T = "svm", "prior", 1100, 6
    q = _device_problem(model, kernel, stat, N, T, 1, T - 1, Ntilde, R)
    o = _traced_and_production(ctx, monkeypatch, "paris_mem1024", q, want_draws=False)
    _assert_teacher_forced(q, o, (1e-8, 0), (1e-8, 1e-7), 1e-8, (1e-8, 1e-7))
    assert len(np.unique(o["all_x_t"][1][:, 0])) == N               # children are fresh draws, not copies
    _assert_laws("paris_mem1024 svm prior N={0} Nt={1} R={2} {3}".format(N, Ntilde, R, stat), q, o)


def _assert_ancestors_restated(tag, q, o):
    """(e) the filter ancestors DERIVED: po.particle_order_ancestors on the traced log-weights of step t and the uniforms
    the launch recorded.  A child whose uniform lies within 1e-10 of a CDF entry (30 times the bound of the device's fast
    exp) may take either neighbour; at most one such child per 10^4 draws -- a condition, not a measurement: a draw is
    exempt with probability about 2e-10 N."""
    N, T = q["N"], len(q["y"])
    wrong, exempt, flips = forced_window.ancestors_against_restatement(o["all_log_weights"], o["rec_ud"], o["all_ancestors"], 1e-10)
    print("ancestors restated", tag, "exempt = {0} flips = {1} of {2} draws".format(exempt, flips, T * N))
    assert wrong == 0 and exempt * 10 ** 4 <= T * N, (wrong, exempt, flips)


@pytest.mark.parametrize("case", MEM_REPLAY_CASES, ids=lambda c: "{0}-{1}-N{2}-Nt{4}-R{5}-{6}".format(*c))
def test_large_n_device_kernel_replayed_by_oracle(ctx, monkeypatch, case):
    """(a) + (e) (+ (c) up to N = 2049, a sanity check: its power is claimed for the tables of
    tests/test_forced_paris_host.py only): paris_mem1024 hands back the normals and the resampling uniforms of its launch.
    The ancestors follow from the uniforms; the oracle replays the window on rec_z0 / rec_z with the traced ancestors and
    backward parents, at the tolerances of test_lds_resident_device_units_replayed_by_oracle -- this unit is built with the
    same flags.  Statistics at or before t1 are exactly 0 and non-zero behind it."""
    model, kernel, N, T, Ntilde, R, stat = case
    t1, tL = 1, T - 1
    q = _device_problem(model, kernel, stat, N, T, t1, tL, Ntilde, R)
    o = _traced_and_production(ctx, monkeypatch, "paris_mem1024", q, want_draws=True)
    tag = "paris_mem1024 {0} {1} N={2} Nt={3} R={4} {5}".format(model, kernel, N, Ntilde, R, stat)
    assert forced_window.recorded_draws_are_sound(o, T, N)
    _assert_ancestors_restated(tag, q, o)
    z, z0, anc, J = o["rec_z"], o["rec_z0"], o["all_ancestors"], o["all_paris_J"]
    ref = po.pf_window(model, q["theta"], q["y"], N, z0, None, z, kernel=kernel, pf="paris", stat=stat, t1=t1, tL=tL,
                       weights=q["weights"], prior_mean=q["prior_mean"], prior_var=q["prior_var"], save_all=True, Ntilde=Ntilde,
                       resampler=lambda t, logw: anc[t], paris_parents=lambda t: J[t].T)
    r, a = 1e-8, 1e-8
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"], ref["all_loglikelihood_estimate"], rtol=r, atol=a)
    assert o["all_statistics"].shape == ref["all_statistics"].shape
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=r, atol=1e-7)
    np.testing.assert_allclose(o["statistics"], ref["statistics"], rtol=r, atol=1e-7)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=r, atol=1e-7)
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=r, atol=a)
    assert np.all(o["all_statistics"][:t1 + 1] == 0.0) and np.all(np.any(o["all_statistics"][t1 + 1:] != 0.0, axis=(1, 2)))
    if N <= 2049:
        _assert_laws(tag, q, o)


@pytest.mark.parametrize("case", MEM_F32_CASES, ids=lambda c: "{0}-{1}-N{2}".format(*c))
def test_large_n_f32_state_teacher_forced(ctx, monkeypatch, case):
    """(d) + (e) on paris_mem1024: dtype='f32', Ntilde = 2, max_accept_reject = 0, T = 6, window [1, 5).  From the traced
    step t the oracle's proposal on the recorded normals gives x_{t+1} (rtol / atol 2e-5), forced_paris_steps the
    log-weights (2e-4), the statistics and their mean (2e-3); x0 = prior_mean + sd rec_z0 at 2e-6 -- the f32 tolerances of
    test_f32_state_fallback_teacher_forced and test_gpu_device_replay.py::test_f32_state_device_kernels_replayed.  The f32
    log-weights go through an f32 exp before the f64 CDF, so an ancestor flips where a uniform lies within ~1e-7 of an
    entry: at most max(3, 2e-4 T N) flips against the restatement, as that test allows."""
    model, kernel, N = case
    T, Ntilde = 6, 2
    q = _device_problem(model, kernel, "score", N, T, 1, T - 1, Ntilde, 0, dtype="f32")
    o = _traced_and_production(ctx, monkeypatch, "paris_mem1024", q, want_draws=True)
    assert forced_window.recorded_draws_are_sound(o, T, N)
    _assert_teacher_forced(q, o, (2e-4, 2e-4), (2e-3, 2e-3), 2e-4, (2e-3, 2e-3))
    d = po.derived(model, q["theta"])
    for t in range(T):
        xn = po.kernel_rv(model, kernel, d, o["all_x_t"][t][o["all_ancestors"][t]], np.array([q["y"][t]]), o["rec_z"][t])
        np.testing.assert_allclose(o["all_x_t"][t + 1], xn, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(o["all_x_t"][0][:, 0], q["prior_mean"] + np.sqrt(q["prior_var"]) * o["rec_z0"], rtol=2e-6, atol=2e-6)
    wrong, exempt, flips = forced_window.ancestors_against_restatement(o["all_log_weights"], o["rec_ud"], o["all_ancestors"], 1e-10)
    print("ancestors restated paris_mem1024 f32", model, kernel, N, "flips = {0} of {1} draws".format(flips, T * N))
    assert flips <= max(3, int(2e-4 * T * N)), flips


@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: "{0}-{1}-{2}-N{3}".format(*c))
def test_f32_state_fallback_teacher_forced(ctx, monkeypatch, case):
    """(d) + (c): dtype='f32' with max_accept_reject = 0 -- the fallback shifts by the exact wave maximum -- teacher-forced
    at the f32 tolerances of test_one_wave_pool_parity_f32 (log-weights 2e-4, statistics and their mean 2e-3)."""
    unit, model, kernel, N, T, Ntilde = case
    q = _device_problem(model, kernel, "score", N, T, 2, T - 1, Ntilde, 0, dtype="f32")
    o = _traced_and_production(ctx, monkeypatch, unit, q, want_draws=True)
    _assert_teacher_forced(q, o, (2e-4, 2e-4), (2e-3, 2e-3), 2e-4, (2e-3, 2e-3))
    np.testing.assert_allclose(o["all_x_t"][0][:, 0], q["prior_mean"] + np.sqrt(q["prior_var"]) * o["rec_z0"], rtol=2e-6, atol=2e-6)
    _assert_laws("{0} f32 {1} {2} N={3} Nt={4} R=0".format(unit, model, kernel, N, Ntilde), q, o)
