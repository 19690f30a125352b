"""GPU: ESS-triggered (adaptive) resampling, ess_threshold=tau (PFG_FLAG_ADAPTIVE_RESAMPLING) on every kernel that serves it.

REPLAY: the restatement on the oracle's pieces (tests/helpers/adaptive_model.py; with base = 0 it IS po.pf_window, see
tests/test_adaptive_host.py) is the specification -- decisions, ancestors and trajectories -- at the tolerance of
test_gpu_stratified.py.  DEVICE: the traced launch records the uniform every child searched with and its normals and the
restatement replays the launch on them.  Then batch invariance, the refusals through the library, the unflagged
descriptor, ess_threshold = None / 0, ChainEnsemble against hand-built launches, the drop-in sampler and the variance the
carried-over genealogy buys."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from sgmcmc_ssm_amd import _capi, particle_filters
from test_host_logic import default_params, GEN, vec
from test_gpu_device_replay import THETA, _series
from test_gpu_batch_invariance import LAMBDAS, batch, check_alone, assert_same
from test_gpu_pf_parity import _refusal_batch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import adaptive_model  # noqa: E402
import device_windows  # noqa: E402
import window_reduce  # noqa: E402

pytestmark = pytest.mark.gpu

FLAG = _capi.FLAG_ADAPTIVE_RESAMPLING
TAU = 0.5


@pytest.fixture(scope="module")
def ctx():
    return _capi.default_context(0)


def _prior(model):
    if model == "garch":
        pm, pv = po.garch_prior_x(THETA[model])
        return pm, float(np.asarray(pv).reshape(-1)[0])
    return 0.0, 10.0


def _identity_steps(anc):
    return np.all(anc == np.arange(anc.shape[1]), axis=1)


def _two_kept_in_a_row(resampled):
    r = np.asarray(resampled, dtype=bool)
    return bool(np.any(~r[1:] & ~r[:-1]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. REPLAY parity against the restatement
# ---------------------------------------------------------------------------------------------------------------------
RTOL, ATOL = 1e-9, 1e-9         # test_gpu_stratified.py, REPLAY cases
T_REPLAY, WINDOW = 16, (2, 14)
# fixed inputs, picked on the CPU so that the conditions asserted in _replay_case hold for every case: the streams
# po.draw_streams(RandomState(STREAM_SEED), N, T) on the series _series(model, 16, SERIES_SEED[model]) (GARCH with the optimal
# proposal has nearly even weights: its series is one on which the effective sample size does fall below N / 2 once)
STREAM_SEED = 5
SERIES_SEED = {"svm": 0, "garch": 1, "lgssm": 0}


def _replay_inputs(model, kernel, lam, N, T=T_REPLAY, window=WINDOW):
    t1, tL = window
    pm, pv = _prior(model)
    z0, u, z = po.draw_streams(np.random.RandomState(STREAM_SEED), N, T)
    return dict(model=model, kernel=kernel, smoother="nemeth", stat="score", dtype="f64", rng="replay", N=N, t1=t1, tL=tL,
                lambduh=lam, prior_mean=pm, prior_var=pv, y=_series(model, T, seed=SERIES_SEED[model]),
                weights=np.linspace(20.0, 30.0, tL - t1), theta=THETA[model], z0=z0, u=u, z=z, flags=FLAG, ess_threshold=TAU)


def _replay_reference(q):
    return adaptive_model.pf_window(q["model"], q["theta"], q["y"], q["N"], q["z0"], q["u"], q["z"], q["ess_threshold"],
                                    kernel=q["kernel"], pf="nemeth", lambduh=q["lambduh"], stat=q["stat"], t1=q["t1"], tL=q["tL"],
                                    weights=q["weights"], prior_mean=q["prior_mean"], prior_var=q["prior_var"])


def _replay_case(ctx, model, kernel, lam, N, T=T_REPLAY, window=WINDOW):
    q = _replay_inputs(model, kernel, lam, N, T, window)
    ref = _replay_reference(q)
    # conditions on the inputs, from the restatement: no decision within rounding of the threshold, both branches run
    print("margin", model, kernel, lam, N, ref["margin"], "resampled", ref["resampled"].astype(int))
    assert ref["margin"] >= 1e-7, ref["margin"]
    assert 1 <= ref["resampled"].sum() <= T - 1 and _two_kept_in_a_row(ref["resampled"])
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == ("adaptive256x4" if N <= 1024 else "mem1024_adaptive")
    np.testing.assert_array_equal(~_identity_steps(o["all_ancestors"]), ref["resampled"])
    assert int(np.sum(o["all_ancestors"] != ref["all_ancestors"])) == 0
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"], ref["all_loglikelihood_estimate"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=RTOL, atol=ATOL)
    # the untraced launch of the same window returns the traced one's record
    plain = ctx.run_batch([dict(q)])[0]
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]) and plain["loglik"] == o["loglik"]


@pytest.mark.parametrize("N", [100, 1024, 1025, 4097])
@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal")])
def test_replay_parity(ctx, model, kernel, lam, N):
    """pfg_run_batch with the flag and tau = 0.5 on (z0, u, z) against the restatement: window [2, 14) of T = 16 with
    weights; N = 100 (ragged 256 x 4), 1024 (every slot), 1025 (first size of the large-N twin, log-weights in registers),
    4097 (log-weights in the scratch).  Step for step the launch resamples where the restatement does."""
    _replay_case(ctx, model, kernel, lam, N)


def test_replay_parity_at_the_maximum(ctx):
    _replay_case(ctx, "svm", "prior", 1.0, 16384)


@pytest.mark.parametrize("stat", ["suff", "none"])
def test_replay_parity_other_statistics(ctx, stat):
    q = dict(_replay_inputs("svm", "prior", 0.95, 300), stat=stat)
    ref = _replay_reference(q)
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == "adaptive256x4"
    np.testing.assert_array_equal(~_identity_steps(o["all_ancestors"]), ref["resampled"])
    assert 1 <= ref["resampled"].sum() <= T_REPLAY - 1 and ref["margin"] >= 1e-7
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------------
# 2. recorded-draw replay of the DEVICE instantiations
# ---------------------------------------------------------------------------------------------------------------------
DRTOL, DATOL = 1e-8, 1e-8       # test_gpu_device_replay.py
DEVICE_CASES = [
    # model, kernel, lambduh, N, T, window, variant
    ("svm", "prior", 0.95, 1000, 16, (2, 14), "adaptive256x4"),
    ("garch", "optimal", 1.0, 3000, 16, (2, 14), "big4096_adaptive"),
    ("lgssm", "optimal", 0.95, 4097, 16, (2, 14), "big16384_adaptive"),
]


def _device_problem(model, kernel, lam, N, T, window, dtype="f64"):
    t1, tL = window
    pm, pv = _prior(model)
    return dict(model=model, kernel=kernel, smoother="nemeth", stat="score", dtype=dtype, rng="device", N=N, t1=t1, tL=tL,
                lambduh=lam, prior_mean=pm, prior_var=pv, y=_series(model, T, seed=SERIES_SEED[model]),
                weights=np.linspace(20.0, 30.0, tL - t1), theta=THETA[model], seed=20261018 + N, stream=T, flags=FLAG,
                ess_threshold=TAU)


@pytest.mark.parametrize("case", DEVICE_CASES, ids=lambda c: "{0}-{1}-N{3}-{6}".format(*c))
def test_device_kernel_replayed(ctx, case):
    """The traced launch records, per step and child, the uniform it searched with (rec_ud; unspecified on a step that kept
    its particles) and its normal; the restatement on the recorded numbers -- the resampling of a step that resamples
    restated by adaptive_model.device_ancestors, the decisions its own -- gives the launch's trajectory at rtol 1e-8 with
    every decision and ancestor equal.  The same key without recording returns the record bit for bit."""
    model, kernel, lam, N, T, window, variant = case
    q = _device_problem(model, kernel, lam, N, T, window)
    o = ctx.run_batch([q], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == variant
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == variant
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]) and plain["loglik"] == o["loglik"]
    ud, z, z0 = o["rec_ud"], o["rec_z"], o["rec_z0"]
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(z0)) and np.any(z != 0.0)
    ref = adaptive_model.pf_window(model, q["theta"], q["y"], N, z0, None, z, TAU, kernel=kernel, pf="nemeth", lambduh=lam,
                                   t1=q["t1"], tL=q["tL"], weights=q["weights"], prior_mean=q["prior_mean"], prior_var=q["prior_var"],
                                   resampler=lambda t, logw: adaptive_model.device_ancestors(logw, ud[t], variant))
    print("margin", case, ref["margin"], "resampled", ref["resampled"].astype(int))
    assert ref["margin"] >= 1e-7 and 1 <= ref["resampled"].sum() <= T - 1
    np.testing.assert_array_equal(~_identity_steps(o["all_ancestors"]), ref["resampled"])
    assert np.all((ud[ref["resampled"]] > 0.0) & (ud[ref["resampled"]] < 1.0))
    assert int(np.sum(o["all_ancestors"] != ref["all_ancestors"])) == 0
    np.testing.assert_allclose(o["all_x_t"], ref["all_x_t"], rtol=DRTOL, atol=DATOL)
    np.testing.assert_allclose(o["all_log_weights"], ref["all_log_weights"], rtol=DRTOL, atol=DATOL)
    np.testing.assert_allclose(o["all_loglikelihood_estimate"], ref["all_loglikelihood_estimate"], rtol=DRTOL, atol=DATOL)
    np.testing.assert_allclose(o["all_statistics"], ref["all_statistics"], rtol=DRTOL, atol=1e-7)
    np.testing.assert_allclose(o["mean_stat"], ref["mean_statistic"], rtol=DRTOL, atol=1e-7)
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=DRTOL, atol=DATOL)


@pytest.mark.parametrize("model,kernel,N,T,variant", [("svm", "prior", 1000, 16, "adaptive256x4"),
                                                     ("garch", "optimal", 3000, 16, "big4096_adaptive"),
                                                     ("lgssm", "optimal", 4097, 16, "big16384_adaptive")])
def test_f32_state_device_kernels_replayed(ctx, model, kernel, N, T, variant):
    """dtype='f32', one case per unit, TEACHER-FORCED step by step on the launch's own decisions and ancestors at the
    tolerances of test_gpu_device_replay.py::test_f32_state_device_kernels_replayed: particles rtol 2e-5, log-weights 2e-4,
    statistics 2e-4 of their scale, at most max(3, 2e-4 T N) ancestors off on the steps that resampled; a decision may differ
    from the fp64 rule only where the ESS is within 1e-4 N of the threshold (f32 weights)."""
    q = _device_problem(model, kernel, 1.0, N, T, (0, T), dtype="f32")
    q["weights"] = None
    o = ctx.run_batch([q], want_trace=True, want_draws=True)[0]
    assert ctx.last_variant() == variant
    plain = ctx.run_batch([dict(q)])[0]
    assert np.array_equal(plain["mean_stat"], o["mean_stat"]) and plain["loglik"] == o["loglik"]
    ud, z = o["rec_ud"], o["rec_z"]
    d = po.derived(model, q["theta"])
    kept = _identity_steps(o["all_ancestors"])
    assert 1 <= kept.sum() <= T - 1
    flips = 0
    for t in range(T):
        x, lw, st = o["all_x_t"][t], o["all_log_weights"][t], o["all_statistics"][t]
        got = o["all_ancestors"][t]
        res, ess = adaptive_model.ess_decision(lw, TAU)
        assert res == (not kept[t]) or abs(ess - TAU * N) < 1e-4 * N, (t, ess)
        base = np.zeros(N)
        if kept[t]:
            base = adaptive_model.carried_base(lw)
        else:
            flips += int(np.sum(adaptive_model.device_ancestors(lw, ud[t], variant) != got))
        yt = np.array([q["y"][t]])
        xp = x[got]
        xn = po.kernel_rv(model, kernel, d, xp, yt, z[t])
        np.testing.assert_allclose(o["all_x_t"][t + 1], xn, rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(o["all_log_weights"][t + 1], base + po.kernel_reweight(model, kernel, d, xp, xn, yt),
                                   rtol=2e-4, atol=2e-4)
        ref_st = st[got] + po.score_statistic(model, d, xp, xn, yt)
        assert np.max(np.abs(o["all_statistics"][t + 1] - ref_st)) < 2e-4 * np.maximum(1.0, np.abs(ref_st).max())
    assert flips <= max(3, int(2e-4 * T * N)), flips


# ---------------------------------------------------------------------------------------------------------------------
# 3. batch invariance, refusals, the unflagged descriptor
# ---------------------------------------------------------------------------------------------------------------------
TAUS = (0.5, 0.25, 1.0, 0.75)


def _adaptive_batch(model, kernel, Ns, rng):
    qs = batch(model, kernel, Ns, rng=rng, smoother="nemeth", flags=FLAG)
    for i, q in enumerate(qs):
        q["lambduh"] = LAMBDAS[i % len(LAMBDAS)]
        q["ess_threshold"] = TAUS[i % len(TAUS)]
    return qs


@pytest.mark.parametrize("rng", ["device", "replay"])
def test_adaptive_alone_equals_batched(ctx, rng):
    """140 windows of mixed N, T (0 and 1 included), windows, theta, weights, lambduh and tau in one launch: every window's
    record, final particles and statistics are bitwise those of the reversed batch and of the window run alone."""
    Ns = [(1024, 100, 1, 700, 333, 1000, 257)[i % 7] for i in range(140)]
    check_alone(ctx, _adaptive_batch("garch", "prior", Ns, rng), "adaptive256x4", trace=False, every=23)


@pytest.mark.parametrize("rng,Ns,variant", [("device", (4096, 1025, 3000, 2048), "big4096_adaptive"),
                                            ("device", (16384, 4097, 9000), "big16384_adaptive"),
                                            ("replay", (4096, 1025, 3000, 2048), "mem1024_adaptive"),
                                            ("replay", (16384, 4097, 9000), "mem1024_adaptive")])
def test_adaptive_large_n_alone_equals_batched(ctx, rng, Ns, variant):
    """The large-N twins, one size class per batch (so batch and lone window run the same instantiation)."""
    check_alone(ctx, _adaptive_batch("lgssm", "optimal", Ns, rng), variant)


_INV, _UNS = _capi.PFG_ERR_INVALID, _capi.PFG_ERR_UNSUPPORTED
_AD = dict(flags=FLAG, reserved=_capi.ess_threshold_bits(0.5))
_DEV = dict(_AD, rng=1, z0=None, u=None, z=None)
REFUSALS = [
    ([_AD, dict()], _INV, "problem 1: adaptive resampling (PFG_FLAG_ADAPTIVE_RESAMPLING) cannot share a batch"),
    ([dict(), _AD], _INV, "problem 1: adaptive resampling (PFG_FLAG_ADAPTIVE_RESAMPLING) cannot share a batch"),
    ([_DEV, dict(_DEV, flags=0)], _INV, "problem 1: adaptive resampling (PFG_FLAG_ADAPTIVE_RESAMPLING) cannot share a batch"),
    ([_AD, dict(_AD, N=16385)], _UNS, "problem 1: adaptive resampling is built for N <= 16384"),
    ([_DEV, dict(_DEV, N=16385)], _UNS, "problem 1: adaptive resampling is built for N <= 16384"),
    ([_AD, dict(_AD, smoother=1)], _UNS, "problem 1: adaptive resampling is built for the NEMETH recursion, not pf = 'filter'"),
    ([_AD, dict(_AD, smoother=2, Ntilde=2, paris_man_u=32)], _UNS,
     "problem 1: adaptive resampling is built for the NEMETH recursion, not pf = 'paris'"),
    ([_AD, dict(_AD, smoother=4)], _UNS, "problem 1: adaptive resampling is built for the NEMETH recursion, not pf = 'poyiadjis_N2'"),
    ([_AD, dict(_AD, smoother=8)], _UNS, "problem 1: adaptive resampling is built for multinomial draws"),
    ([_DEV, dict(_DEV, smoother=3)], _UNS, "problem 1: adaptive resampling is built for multinomial draws"),
    ([dict(_AD, stat=3, num_steps_ahead=1, pred_z=32)] * 2, _UNS,
     "problem 0: adaptive resampling is not built for the predictive statistic"),
    ([_AD, dict(_AD, elementwise=1, ew_mean=6)], _UNS, "problem 1: adaptive resampling is not built for elementwise statistics"),
    ([_AD, dict(_AD, reserved=0)], _INV, "problem 1: ess_threshold must be in (0, 1]"),
    ([_AD, dict(_AD, reserved=_capi.ess_threshold_bits(1.5))], _INV, "problem 1: ess_threshold must be in (0, 1]"),
]


def test_refusals_through_the_library(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    for faults, code, text in REFUSALS:
        keep = []
        ps, rs = _refusal_batch(keep, "svm", None, faults)
        rc = lib.pfg_run_batch(h, len(ps), ps, rs)
        msg = lib.pfg_last_error(h).decode()
        assert (rc, text in msg) == (code, True), (faults, rc, msg)
    # the new launch refuses the same; the scratch is the large-N kernels' state, whatever the generator
    desc = torch.zeros(_capi.DEV_PROBLEM_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    for rng in ("replay", "device"):
        with pytest.raises(NotImplementedError, match="adaptive resampling is built for N <= 16384"):
            ctx.launch_device_adaptive("svm", "prior", "f64", rng, 16385, 1, desc.data_ptr())      # (never read)
    assert ctx.scratch_bytes_adaptive("svm", "f64", 1024) == 0 and ctx.scratch_bytes_adaptive("svm", "f64", 16385) == -1
    for N in (1025, 4097):
        assert ctx.scratch_bytes_adaptive("svm", "f64", N) == ctx.scratch_bytes_smoother("svm", "f64", "replay", "nemeth", N) > 0
    assert ctx.scratch_bytes_adaptive("svm", "f32", 4097) == ctx.scratch_bytes_smoother("svm", "f32", "device", "nemeth", 4097) > 0
    # the high-level path: the Helper's elementwise call
    from sgmcmc_ssm_amd.models.svm import SVMSampler
    y = _series("svm", 12, seed=1).reshape(-1, 1)
    sampler = SVMSampler(n=1, m=1, observations=y, parameters=default_params("svm"))
    with pytest.raises(NotImplementedError, match="not built for elementwise statistics"):
        sampler.message_helper.pf_latent_var_distr(observations=y, parameters=sampler.parameters, N=50, ess_threshold=0.5)


@pytest.mark.parametrize("rng,N,variant", [("replay", 300, "adaptive256x4"), ("device", 300, "adaptive256x4"),
                                           ("replay", 2000, "mem1024_adaptive"), ("replay", 5000, "mem1024_adaptive"),
                                           ("device", 2000, "big4096_adaptive"), ("device", 5000, "big16384_adaptive")])
def test_unflagged_descriptor_in_an_adaptive_launch_gets_nans(ctx, rng, N, variant):
    """pfg_launch_device_adaptive does not read descriptors: one without the flag (here beside a flagged one) gets NaNs in
    out[0..7], never another estimator's numbers, and its neighbour is computed."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(dev)
    T = 6
    th = np.zeros(_capi.MAX_THETA)
    th[:3] = THETA["svm"]
    z0, u, z = po.draw_streams(np.random.RandomState(3), N, T)
    bufs = dict(y=t(_series("svm", T, seed=2)), theta=t(th), z0=t(z0), u=t(u), z=t(z))
    out = torch.zeros((2, _capi.OUT_DOUBLES), dtype=torch.float64, device=dev)
    sb = ctx.scratch_bytes_adaptive("svm", "f64", N)
    assert (sb > 0) == (N > 1024)
    scratch = torch.zeros(2 * max(sb, 1), dtype=torch.uint8, device=dev)
    d = np.zeros(2, dtype=_capi.DEV_PROBLEM_DTYPE)
    for k, v in bufs.items():
        if rng == "replay" or k in ("y", "theta"):
            d[k] = v.data_ptr()
    d["out"] = out.data_ptr() + np.arange(2, dtype=np.uint64) * np.uint64(8 * _capi.OUT_DOUBLES)
    if sb > 0:
        d["scratch"] = scratch.data_ptr() + np.arange(2, dtype=np.uint64) * np.uint64(sb)
    d["prior_var"], d["lambduh"], d["seed"], d["stream"] = 10.0, 1.0, 9, [1, 2]
    d["T"], d["t1"], d["tL"], d["N"] = T, 0, T, N
    d["smoother"], d["stat"] = _capi.SMOOTHER["nemeth"], _capi.STAT["score"]
    d["flags"], d["reserved"] = [FLAG, 0], [_capi.ess_threshold_bits(0.5), 0]
    desc = torch.from_numpy(d.view(np.uint8).reshape(2, -1)).to(dev)
    ctx.launch_device_adaptive("svm", "prior", "f64", rng, N, 2, desc.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert ctx.last_variant() == variant
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got[0, :5])) and np.any(got[0, :3] != 0.0), got
    assert np.all(np.isnan(got[1])), got


# ---------------------------------------------------------------------------------------------------------------------
# 4. ess_threshold = None / 0: the plain call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng,N", [("replay", 300), ("device", 300), ("device", 2000)])
def test_off_is_the_plain_call_bitwise(ctx, rng, N):
    y, th = _series("svm", 12, seed=4), THETA["svm"]
    outs, names = [], []
    for kw in ({}, dict(ess_threshold=None), dict(ess_threshold=0)):
        q = particle_filters.make_problem("svm", "prior", "nemeth", y, th, N, t1=2, tL=10, rng=rng, seed=11, stream=3,
                                          lambduh=0.9, random_state=np.random.RandomState(8), **kw)
        assert "ess_threshold" not in q and q["flags"] == 0
        outs.append(ctx.run_batch([q], want_final=True)[0])
        names.append(ctx.last_variant())
    assert names[0] == names[1] == names[2] and "adaptive" not in names[0]
    for o in outs[1:]:
        assert_same(outs[0], o, "off")
    on = particle_filters.make_problem("svm", "prior", "nemeth", y, th, N, t1=2, tL=10, rng=rng, seed=11, stream=3,
                                       lambduh=0.9, random_state=np.random.RandomState(8), ess_threshold=0.5)
    o = ctx.run_batch([on], want_final=True)[0]
    assert "adaptive" in ctx.last_variant() and not np.array_equal(o["mean_stat"], outs[0]["mean_stat"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. ChainEnsemble
# ---------------------------------------------------------------------------------------------------------------------
def _ensemble_series(model, T, seed=5):
    np.random.seed(seed)
    return GEN[model](T=T, parameters=default_params(model))["observations"].reshape(-1)


def _hand_built(ens, y_host, theta_rows, step, pf, lam):
    """ctx.run_batch of the descriptors the ensemble's latest step ran: the windows the device wrote, the chains'
    parameters before the step, (seed, stream, step) as the resident launch keys its generator."""
    d, yoff, woff, seq_len = device_windows.ensemble_windows(ens) if ens._multi else \
        device_windows.decode(ens.desc_dev, ens.y_dev.data_ptr(), ens.weights_dev.data_ptr()) + (None,)
    wtab = ens.weights_dev.cpu().numpy().reshape(-1)
    per = ens.W if ens._multi else 1
    probs = []
    for i in range(ens._nd):
        T, t1, tL = int(d["T"][i]), int(d["t1"][i]), int(d["tL"][i])
        w = None if woff[i] < 0 else wtab[woff[i]:woff[i] + (tL - t1)]
        kw = dict(lambduh=lam) if pf == "nemeth" else {}
        assert int(d["flags"][i]) & FLAG and _capi.ess_threshold_from_bits(d["reserved"][i]) == ens.ess_threshold and int(d["smoother"][i]) == 0
        q = particle_filters.make_problem(ens.model, ens.kernel, pf, y_host[yoff[i]:yoff[i] + T], theta_rows[i // per], ens.N,
                                          t1=t1, tL=tL, weights=w, prior_mean=float(d["prior_mean"][i]),
                                          prior_var=float(d["prior_var"][i]), flags=int(d["flags"][i]) & ~FLAG, dtype=ens.dtype,
                                          rng="device", seed=ens.seed, stream=int(d["stream"][i]),
                                          ess_threshold=ens.ess_threshold, **kw)
        assert q["flags"] == int(d["flags"][i])
        q["step"] = step
        probs.append(q)
    outs = ens.ctx.run_batch(probs)
    recs = np.zeros((len(probs), 8))
    h = _capi.STAT_DIM[ens.model]
    recs[:, :h] = [o["mean_stat"] for o in outs]
    recs[:, 4] = [o["loglik"] for o in outs]
    return recs, seq_len


def _three_steps_equal_hand_built(ens, y_host, pf, lam, variant):
    h = _capi.STAT_DIM[ens.model]
    for step in range(3):
        before = ens.theta()
        ens.step(1)
        ens.synchronize()
        assert ens.ctx.last_variant() == variant
        g, ll = ens.last_gradient_statistics()
        recs, seq_len = _hand_built(ens, y_host, before, step, pf, lam)
        assert ens.ctx.last_variant() == variant
        if ens._multi:
            win, _ = ens.window_statistics()
            np.testing.assert_array_equal(win.reshape(-1, 8)[:, :5], recs[:, :5])
            recs = window_reduce.reduce_windows(recs, seq_len, ens.K_eff, ens.M, ens._rescale, ens.T)
        assert g.tobytes() == np.ascontiguousarray(recs[:, :h]).tobytes() and ll.tobytes() == np.ascontiguousarray(recs[:, 4]).tobytes()
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(ll))
        assert not np.array_equal(before, ens.theta())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ensemble_single_window(dtype):
    """N = 2000 (the large-N twin), 8 chains, S = 16 / B = 4, windows sampled on the device: three steps equal hand-built
    launches of the same descriptors bitwise; a graph replay of three steps equals three eager steps bitwise; SGHMC and a
    state_dict resume run on it, and a checkpoint of another threshold is refused."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("svm")
    y = _ensemble_series("svm", 120)
    kw = dict(num_chains=8, N=2000, epsilon=1e-3, seed=23, chain_offset=3, subsequence_length=16, buffer_length=4,
              window_sampling="device", dtype=dtype, ess_threshold=0.5)
    ens = ChainEnsemble("svm", y, p, **kw)
    assert ens._smoother == "nemeth" and ens.ess_threshold == 0.5
    assert ens.scratch_dev.numel() == 8 * ens.ctx.scratch_bytes_adaptive("svm", dtype, 2000) > 0
    _three_steps_equal_hand_built(ens, y, "poyiadjis_N", 1.0, "big4096_adaptive")
    eager = ChainEnsemble("svm", y, p, **kw)
    eager.step(3)
    graph = ChainEnsemble("svm", y, p, **kw).run(3, thin=3, graph_steps=3)
    np.testing.assert_array_equal(graph[0], eager.theta())
    np.testing.assert_array_equal(ens.theta(), eager.theta())
    plain = ChainEnsemble("svm", y, p, **dict(kw, ess_threshold=None))
    plain.step(3)
    assert "adaptive" not in plain.ctx.last_variant() and not np.array_equal(plain.theta(), eager.theta())
    if dtype == "f64":
        full = ChainEnsemble("svm", y, p, sampler="sghmc", **kw)
        full.step(1)
        state = full.state_dict()
        assert state["ess_threshold"] == 0.5
        full.step(2)
        again = ChainEnsemble("svm", y, p, sampler="sghmc", **kw)
        again.load_state_dict(state)
        again.step(2)
        np.testing.assert_array_equal(full.theta(), again.theta())
        assert np.all(np.isfinite(full.theta()))
        with pytest.raises(ValueError, match="checkpoint ess_threshold"):
            plain.load_state_dict(state)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ensemble_multi_window(dtype):
    """minibatch_size = 2, N = 64, pf='nemeth': the same checks on the multi-window path (window records and the reduced
    records)."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("garch")
    y = _ensemble_series("garch", 90)
    kw = dict(num_chains=12, N=64, pf="nemeth", lambduh=0.9, epsilon=1e-3, dtype=dtype, seed=31, chain_offset=2,
              subsequence_length=16, buffer_length=4, minibatch_size=2, window_sampling="device", ess_threshold=0.75)
    ens = ChainEnsemble("garch", y, p, **kw)
    assert ens._multi and ens.W == 2 and ens.ess_threshold == 0.75
    _three_steps_equal_hand_built(ens, y, "nemeth", 0.9, "adaptive256x4")
    eager = ChainEnsemble("garch", y, p, **kw)
    eager.step(3)
    graph = ChainEnsemble("garch", y, p, **kw).run(3, thin=3, graph_steps=3)
    np.testing.assert_array_equal(graph[0], eager.theta())


def test_ensemble_host_windows_and_sgrld():
    """Host window sampling (single-window path) and the SGRLD update run adaptive chains; the host-sampled chains do not
    depend on the partition into ensembles."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("lgssm")
    y = _ensemble_series("lgssm", 80)
    kw = dict(N=100, epsilon=1e-3, seed=7, subsequence_length=16, buffer_length=4, sampler="sgrld", ess_threshold=0.5)
    whole = ChainEnsemble("lgssm", y, p, num_chains=10, **kw)
    whole.step(3)
    lo = ChainEnsemble("lgssm", y, p, num_chains=4, chain_offset=0, **kw)
    hi = ChainEnsemble("lgssm", y, p, num_chains=6, chain_offset=4, **kw)
    lo.step(3)
    hi.step(3)
    assert whole.ctx.last_variant() == "adaptive256x4"
    np.testing.assert_array_equal(np.concatenate([lo.theta(), hi.theta()]), whole.theta())
    assert np.all(np.isfinite(whole.theta()))


def test_resident_fit_passes_the_threshold_on():
    """fit(iter_type='SGLD', pf_kwargs=dict(rng='device', ess_threshold=0.5)) runs resident on a one-chain adaptive
    ensemble: reproducible under np.random.seed, another trajectory than always-resampling."""
    from sgmcmc_ssm_amd.models.svm import SVMSampler
    p = default_params("svm")
    y = _ensemble_series("svm", 100).reshape(-1, 1)

    def fit(**pf_kwargs):
        sampler = SVMSampler(n=1, m=1, observations=y, parameters=p.copy())
        np.random.seed(4)
        plist = sampler.fit(iter_type="SGLD", num_iters=4, output_all=True, epsilon=0.01, subsequence_length=16,
                            buffer_length=4, kind="pf", pf_kwargs=dict(pf="poyiadjis_N", N=200, rng="device", **pf_kwargs))
        return np.array([q.theta() for q in plist]), _capi.default_context().last_variant()

    a, va = fit(ess_threshold=0.5)
    b, _ = fit(ess_threshold=0.5)
    m, vm = fit()
    assert va == "adaptive256x4" and vm != va
    assert a.shape == (5, 3) and np.all(np.isfinite(a))
    np.testing.assert_array_equal(a, b)
    assert np.all(a[1] != m[1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. drop-in sampler
# ---------------------------------------------------------------------------------------------------------------------
def test_drop_in_noisy_gradient(monkeypatch):
    """np.random.seed(3); noisy_gradient(..., N=1000, ess_threshold=0.5) equals the same call on the stand-in at rtol 1e-9,
    and np.random stands afterwards where the multinomial call leaves it."""
    from sgmcmc_ssm_amd.models.svm import SVMSampler
    p = default_params("svm")
    y = _ensemble_series("svm", 60).reshape(-1, 1)
    sampler = SVMSampler(n=1, m=1, observations=y, parameters=p)
    kw = dict(kind="pf", pf="poyiadjis_N", N=1000)
    np.random.seed(3)
    got = vec("svm", sampler.noisy_gradient(ess_threshold=0.5, **kw))
    after = np.random.random()
    assert _capi.default_context().last_variant() == "adaptive256x4"
    np.random.seed(3)
    mult = vec("svm", sampler.noisy_gradient(**kw))
    assert np.random.random() == after
    assert np.all(got != mult)
    monkeypatch.setattr(particle_filters, "run_windows", adaptive_model.run_windows)
    np.random.seed(3)
    ref = vec("svm", sampler.noisy_gradient(ess_threshold=0.5, **kw))
    assert np.random.random() == after
    np.testing.assert_allclose(got, ref, rtol=1e-9)
    monkeypatch.undo()
    # N above the LDS-resident size and a buffered window go the same way (the large-N twin)
    kw2 = dict(kind="pf", pf="nemeth", lambduh=0.9, N=1500, subsequence_length=16, buffer_length=4)
    np.random.seed(8)
    got2 = vec("svm", sampler.noisy_gradient(ess_threshold=0.5, **kw2))
    assert _capi.default_context().last_variant() == "mem1024_adaptive"
    monkeypatch.setattr(particle_filters, "run_windows", adaptive_model.run_windows)
    np.random.seed(8)
    np.testing.assert_allclose(got2, vec("svm", sampler.noisy_gradient(ess_threshold=0.5, **kw2)), rtol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# 7. variance
# ---------------------------------------------------------------------------------------------------------------------
def test_adaptive_resampling_cuts_the_score_variance():
    """1024 chains at one theta, SVM, N = 100, T = 24, window [2, 22) on _series('svm', 24, seed=48): one launch that
    resamples at every step and one with tau = 0.5.  Per score component var_adaptive / var_always < 0.8 -- the reference
    arithmetic on the CPU (300 seeds of po.draw_streams) gives 0.52 / 0.44 / 0.51 at this shape and with 1024 draws the
    ratio's standard error is about 6 % of itself, so 0.8 is more than five standard errors above the measured worst case and
    still fails when the carry-over is lost --, and the two means agree within five standard errors.  The log-likelihood's
    ratio (CPU: 0.93) is printed, not asserted."""
    import torch
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    C = 1024
    p = default_params("svm")
    y = _series("svm", 24, seed=48)
    res = {}
    for tau in (None, TAU):
        ens = ChainEnsemble("svm", y, p, num_chains=C, N=100, epsilon=1e-3, seed=21, ess_threshold=tau)
        ens._desc["t1"], ens._desc["tL"] = 2, 22            # the full series as the buffered window [2, 22)
        ens.desc_dev.copy_(torch.from_numpy(ens._desc.view(np.uint8).reshape(ens._nd, -1)))
        ens.launch_pf()
        ens.synchronize()
        assert (ens.ctx.last_variant() == "adaptive256x4") == (tau is not None)
        g, ll = ens.last_gradient_statistics()
        res[tau] = np.column_stack([g, ll])
    a, b = res[None], res[TAU]
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    ratio = b.var(axis=0) / a.var(axis=0)
    se = np.sqrt(a.var(axis=0) / C + b.var(axis=0) / C)
    zs = np.abs(a.mean(axis=0) - b.mean(axis=0)) / se
    print("variance ratios (score components, log-likelihood)", ratio, "z", zs)
    assert np.all(ratio[:3] < 0.8), ratio
    assert np.all(zs[:3] < 5.0), zs
