"""GPU: the device-generator instantiations of the 256-thread and large-N Poyiadjis O(N^2) units against a deterministic
reference.

n2_256x1 and n2_256x4 were checked only statistically (test_gpu_n2.py::test_n2_device_rng_and_f32: within 6 sd + 5 % of
the O(N) estimate); only the one-wave n2_64x2 had a recorded-draw replay.  The 256-thread units write the same rec_z /
rec_z0 and the traced launch returns the ancestors, so the replay of test_one_wave_device_kernel_replayed_by_oracle applies
unchanged: po.pf_window(pf='poyiadjis_N2') on the recorded normals with the traced ancestors as its resampler, score and
sufficient statistic, at that test's tolerances.

These units record no resampling words, so the ancestors themselves enter the replay as given.  Their LAW is checked from
the trace instead (tests/helpers/forced_window.ancestor_law_score, shown to pass on the oracle's own multinomial ancestors
and to fail on shifted ones by tests/test_forced_window_host.py).

n2_mem1024 (N > 1024: the large-N kernel's O(N^2) sweep) records its normals and, unlike the 256-thread units, the uniform
every child searched the CDF with (rec_ud).  test_large_n_device_kernel_replayed_by_oracle DERIVES its ancestors from them
(po.particle_order_ancestors on the traced log-weights, pinned to np.random.choice by tests/test_mem_resampling_host.py;
exact but for children whose uniform sits within 1e-10 of a CDF entry) and replays the window as above -- x0, proposal and
parent records included -- on every model, at every chunk edge of the unit.  test_large_n_device_kernel_teacher_forced
stays: N = 1100 from the unit's own trace (tests/helpers/forced_window.forced_steps), x_{t+1} and ancestors as traced."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_host_logic import default_params, GEN
from test_gpu_n2_one_wave import _prior_x, CASES

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import forced_window  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def _device_problem(model, kernel, stat, N, T, t1, tL):
    p = default_params(model)
    theta = p.theta()
    np.random.seed(17)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    pm, pv = _prior_x(model, theta)
    return dict(model=model, kernel=kernel, smoother="poyiadjis_n2", stat=stat, dtype="f64", rng="device", N=N, t1=t1, tL=tL,
                lambduh=1.0, prior_mean=pm, prior_var=pv, y=y, weights=np.linspace(20.0, 30.0, tL - t1), theta=theta,
                seed=20241004 + N, stream=T)


@pytest.mark.parametrize("stat", ["score", "suff"])
@pytest.mark.parametrize("model,kernel", CASES)
@pytest.mark.parametrize("variant,N,T", [("n2_256x1", 200, 8), ("n2_256x4", 700, 5)])
def test_256_thread_device_kernels_replayed_by_oracle(ctx, monkeypatch, variant, N, T, model, kernel, stat):
    """n2_256x1 at N = 200 (ragged single slot), n2_256x4 at N = 700 (third slot ragged, fourth empty); window [2, T - 1)
    with weights.  Tolerances of test_one_wave_device_kernel_replayed_by_oracle; the production launch of the same key
    returns the same mean_stat and loglik bit for bit; the ancestors follow the multinomial law of the traced weights:
    |sum_t Z_t| / sqrt(#steps) < 5 over the steps whose weights vary (all but step 0)."""
    t1, tL = 2, T - 1
    q = _device_problem(model, kernel, stat, N, T, t1, tL)
    monkeypatch.setenv("PFGRAD_VARIANT", variant)
    o = ctx.run_batch([q], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == variant
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == variant
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]) and plain["loglik"] == o["loglik"]
    z, z0, anc = o["rec_z"], o["rec_z0"], o["all_ancestors"]
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(z0)) and np.any(z != 0.0) and np.any(z0 != 0.0)
    assert anc.min() >= 0 and anc.max() < N
    ref = po.pf_window(model, q["theta"], q["y"], N, z0, None, z, kernel=kernel, pf="poyiadjis_N2", stat=stat, t1=t1, tL=tL,
                       weights=q["weights"], prior_mean=q["prior_mean"], prior_var=q["prior_var"], save_all=True,
                       resampler=lambda t, logw: anc[t])
    r, a = 1e-8, 1e-8
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=r, atol=a)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"], ref["all_loglikelihood_estimate"], rtol=r, atol=a)
    assert o["all_statistics"].shape == ref["all_statistics"].shape
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=r, atol=1e-7)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=r, atol=1e-7)
    assert np.linalg.norm(o["mean_stat"] - ref["mean_statistic"]) < 1e-6 * max(1.0, np.linalg.norm(ref["mean_statistic"]))
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=r, atol=a)
    assert np.all(o["all_statistics"][:t1 + 1] == 0.0) and np.any(o["all_statistics"][t1 + 1] != 0.0)
    score, steps = forced_window.ancestor_law_score(o["all_log_weights"], anc)
    print("ancestor law", variant, model, stat, score, steps)
    assert steps == T - 1 and score < 5.0, (score, steps)


# n2_mem1024 replayed on its recorded draws: (N, T, model, kernel).  The unit works in chunks of 1024 particles and pads its
# CDF to a power of two.  N = 1025: the second chunk holds one particle (every model); 2048: every chunk full, N is the
# padded size (no sentinel entries), GARCH's two-component record; 2049: the third chunk holds one particle; 4097: five chunks.
MEM_REPLAY_CASES = [(1025, 4) + mk for mk in CASES] + [(2048, 4, "garch", "optimal"), (2049, 4, "lgssm", "prior"),
                                                        (4097, 3, "svm", "prior")]


@pytest.mark.parametrize("stat", ["score", "suff"])
@pytest.mark.parametrize("N,T,model,kernel", MEM_REPLAY_CASES)
def test_large_n_device_kernel_replayed_by_oracle(ctx, monkeypatch, N, T, model, kernel, stat):
    """n2_mem1024, window [1, T - 1) with weights.  The launch records rec_z0, rec_z and rec_ud; the production launch of
    the same key returns the same mean_stat and loglik bit for bit.  The traced ancestors are the restatement's on the
    traced log-weights and the recorded uniforms (a child whose uniform lies within 1e-10 of a CDF entry -- 30 times the
    bound of the device's fast exp -- may take either neighbour; at most one such child per 10^4 draws, a condition and
    not a measurement: a draw is exempt with probability about 2e-10 N).  po.pf_window(pf='poyiadjis_N2') replays the
    window on the recorded normals at the tolerances of test_256_thread_device_kernels_replayed_by_oracle: this unit is
    built with the same flags.  Up to N = 2049 the ancestors' law score runs as a sanity check."""
    t1, tL = 1, T - 1
    q = _device_problem(model, kernel, stat, N, T, t1, tL)
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    o = ctx.run_batch([q], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == "n2_mem1024"
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == "n2_mem1024"
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]) and plain["loglik"] == o["loglik"]
    assert forced_window.recorded_draws_are_sound(o, T, N)
    z, z0, anc = o["rec_z"], o["rec_z0"], o["all_ancestors"]
    assert anc.shape == (T, N) and anc.min() >= 0 and anc.max() < N
    wrong, exempt, flips = forced_window.ancestors_against_restatement(o["all_log_weights"], o["rec_ud"], anc, 1e-10)
    print("ancestors restated n2_mem1024", model, kernel, N, stat, "exempt = {0} flips = {1} of {2} draws".format(exempt, flips, T * N))
    assert wrong == 0 and exempt * 10 ** 4 <= T * N, (wrong, exempt, flips)
    ref = po.pf_window(model, q["theta"], q["y"], N, z0, None, z, kernel=kernel, pf="poyiadjis_N2", stat=stat, t1=t1, tL=tL,
                       weights=q["weights"], prior_mean=q["prior_mean"], prior_var=q["prior_var"], save_all=True,
                       resampler=lambda t, logw: anc[t])
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
        score, steps = forced_window.ancestor_law_score(o["all_log_weights"], anc)
        print("ancestor law n2_mem1024", model, kernel, N, stat, score, steps)
        assert steps == T - 1 and score < 5.0, (score, steps)


@pytest.mark.parametrize("stat", ["score", "suff"])
def test_large_n_device_kernel_teacher_forced(ctx, monkeypatch, stat):
    """n2_mem1024, SVM prior, N = 1100, T = 3, window [1, 2) with a weight, teacher-forced: x_{t+1} and the ancestors are
    taken from the trace here (test_large_n_device_kernel_replayed_by_oracle checks the proposal on the recorded normals
    and derives the ancestors).  Everything downstream of the proposal is recomputed: from the traced
    particles, log-weights, statistics and ancestors of step t, forced_window.forced_steps recomputes the log-weights of
    step t + 1 (po.kernel_reweight) and the O(N^2) statistic recursion in float64 NumPy -- log-weights at rtol 1e-8,
    statistics at rtol 1e-8 / atol 1e-7 --, the running log-likelihood and the weighted mean follow from the traced
    log-weights and statistics, the production launch returns the same record bit for bit, and the ancestors follow the
    multinomial law of the traced weights."""
    model, kernel, N, T, t1, tL = "svm", "prior", 1100, 3, 1, 2
    q = _device_problem(model, kernel, stat, N, T, t1, tL)
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == "n2_mem1024"
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == "n2_mem1024"
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]) and plain["loglik"] == o["loglik"]
    anc = o["all_ancestors"]
    assert anc.min() >= 0 and anc.max() < N
    assert np.all(np.isfinite(o["all_x_t"])) and np.all(o["all_log_weights"][0] == 0.0)
    assert len(np.unique(o["all_x_t"][1])) == N                  # children are fresh draws, not copies
    lw, st, dll = forced_window.forced_steps(model, kernel, q["theta"], q["y"], o["all_x_t"], o["all_log_weights"],
                                             o["all_statistics"], anc, stat=stat, t1=t1, tL=tL, weights=q["weights"])
    np.testing.assert_allclose(o["all_log_weights"][1:], lw, rtol=1e-8, atol=0)
    np.testing.assert_allclose(o["all_statistics"][1:], st, rtol=1e-8, atol=1e-7)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"][1:], np.cumsum(dll), rtol=1e-8, atol=0)
    assert np.all(o["all_statistics"][:t1 + 1] == 0.0) and np.all(np.any(o["all_statistics"][t1 + 1:] != 0.0, axis=(1, 2)))
    np.testing.assert_allclose(o["statistics"], o["all_statistics"][T], rtol=0, atol=0)
    mean = np.sum(o["all_statistics"][T].T * po.log_normalize(o["all_log_weights"][T]), axis=1)
    np.testing.assert_allclose(o["mean_stat"], mean, rtol=1e-8, atol=1e-7)
    np.testing.assert_allclose(o["loglik"], o["all_loglikelihood_estimate"][T], rtol=1e-12, atol=0)
    score, steps = forced_window.ancestor_law_score(o["all_log_weights"], anc)
    print("ancestor law n2_mem1024", stat, score, steps)
    assert steps == T - 1 and score < 5.0, (score, steps)
