"""GPU parity: the HIP particle-filter kernels (through the C ABI) against the CPU oracle and
the golden fixtures generated from the reference.

Tolerances.  REPLAY + f64 runs the reference's operation order in fp64; the only rounding
differences are exp/log (ocml vs NumPy) and the parallel weight sum / prefix scan, so results
agree to ~1e-12 relative unless an ancestor index flips on a near tie (probability ~1e-9 per
run; the kernel reports the smallest |u - cdf| margin so a flip can be diagnosed).  We assert
rtol 1e-9 / atol 1e-9 on gradients and log-likelihoods -- five orders tighter than the
north-star bar (gradient L2 error < 1e-4).  f32 state is checked teacher-forced per step
(rtol 2e-4) and statistically, because one flipped ancestor changes a whole-run gradient by
O(1) (SURVEY.md finding 2).
"""
import numpy as np
import pytest

from oracle import pf_oracle as po
from sgmcmc_ssm_amd import _capi

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-9


@pytest.fixture(scope="module")
def ctx():
    return _capi.default_context(0)


def _problem(meta, g, dtype="f64", rng="replay"):
    key = meta["key"]
    y = g.get(key, "y")
    N, T = meta["N"], meta["T"]
    streams = po.draw_streams(np.random.RandomState(meta["seed"]), N, T)
    lam = 1.0 if meta["pf"] == "poyiadjis_N" else (meta["lambduh"] if meta["lambduh"] is not None else 0.95)
    q = dict(model=meta["model"], kernel=meta["kernel"],
             smoother="filter" if meta["pf"] == "filter" else "nemeth", stat=meta["stat"],
             dtype=dtype, rng=rng, N=N, t1=meta["t1"], tL=meta["tL"], lambduh=lam,
             prior_mean=meta["prior_mean"], prior_var=meta["prior_var"],
             y=y, weights=g.get(key, "weights"), theta=g.get(key, "theta"),
             z0=streams[0], u=streams[1], z=streams[2])
    return q


def test_trace_cases_f64(ctx, golden_trace):
    """Every traced reference case: full save_all trajectories, all models/kernels/smoothers."""
    g = golden_trace
    probs = [_problem(m, g) for m in g.meta]
    # batches must share model/kernel; group
    by = {}
    for m, q in zip(g.meta, probs):
        by.setdefault((m["model"], m["kernel"]), []).append((m, q))
    n = 0
    for (_, _), items in by.items():
        outs = ctx.run_batch([q for _, q in items], want_trace=True)
        for (m, _), o in zip(items, outs):
            key = m["key"]
            np.testing.assert_allclose(o["all_x_t"], g.get(key, "all_x_t"), rtol=RTOL, atol=ATOL, err_msg=str(m))
            np.testing.assert_allclose(o["all_log_weights"], g.get(key, "all_log_weights"), rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(o["all_loglikelihood_estimate"], g.get(key, "all_loglikelihood_estimate"),
                                       rtol=RTOL, atol=ATOL, err_msg=str(m))
            if m["pf"] != "filter":
                np.testing.assert_allclose(o["all_statistics"], g.get(key, "all_statistics"), rtol=RTOL, atol=1e-8)
                np.testing.assert_allclose(o["mean_stat"], g.get(key, "mean_statistic"), rtol=RTOL, atol=1e-8)
            else:
                ref = g.get(key, "all_statistics")[-1]
                np.testing.assert_allclose(o["mean_stat"], ref, rtol=RTOL, atol=1e-8, err_msg=str(m))
            n += 1
    assert n == len(g.meta)


def test_window_cases_f64(ctx, golden_window):
    """Window-level reference outputs incl. the SURVEY known answer (SVM T=1000 N=1000), the
    BASELINE configs' shapes (N=4000 LDS-resident), ragged N and a single-step window."""
    g = golden_window
    n = 0
    for m in g.meta:
        q = _problem(m, g)
        o = ctx.run_batch([q], want_final=True)[0]
        key = m["key"]
        ll = float(g.get(key, "loglikelihood_estimate"))
        assert abs(o["loglik"] - ll) <= ATOL + RTOL * abs(ll), (m, o["loglik"], ll)
        if m["pf"] != "filter":
            ref = g.get(key, "mean_statistic")
        else:
            ref = g.get(key, "statistics")
        l2 = np.linalg.norm(o["mean_stat"] - ref)
        assert l2 <= 1e-7 * max(1.0, np.linalg.norm(ref)), (m, o["mean_stat"], ref)
        assert l2 < 1e-4          # the north-star bar, stated explicitly
        if g.get(key, "x_t") is not None:
            np.testing.assert_allclose(o["x_t"], g.get(key, "x_t"), rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(o["log_weights"], g.get(key, "log_weights"), rtol=RTOL, atol=ATOL)
        n += 1
    assert n >= 30


@pytest.fixture
def force_mem_kernel(monkeypatch):
    """Route every launch to the large-N kernel (state in HBM scratch) whatever N is."""
    monkeypatch.setenv("PFGRAD_VARIANT", "mem1024")


def test_trace_cases_f64_large_n_kernel(ctx, golden_trace, force_mem_kernel):
    """The large-N kernel on the fully traced reference cases (all models / smoothers)."""
    test_trace_cases_f64(ctx, golden_trace)


def test_window_cases_f64_large_n_kernel(ctx, golden_window, force_mem_kernel):
    test_window_cases_f64(ctx, golden_window)


@pytest.mark.parametrize("variant", ["wg256x4", "wg256x4s", "wg1024x1", "wg64x2"])
def test_reference_cases_on_every_lds_variant(ctx, golden_trace, golden_window, monkeypatch, variant):
    """Single windows with 256 < N <= 1024 are served by the latency variant (wg1024x1), large
    batches by the throughput variants; every variant must reproduce the reference fixtures, so
    each is forced in turn (PFGRAD_VARIANT applies where the variant can hold N)."""
    monkeypatch.setenv("PFGRAD_VARIANT", variant)
    test_trace_cases_f64(ctx, golden_trace)
    test_window_cases_f64(ctx, golden_window)


def test_large_n_vs_oracle(ctx):
    """N beyond the LDS-resident variants: GARCH fp64 N=4000 (112 B/particle), SVM N=10000
    (BASELINE config 5 shape), LGSSM N=16384 (maximum), Nemeth and filter smoothers."""
    rs = np.random.RandomState(77)
    cases = [("garch", "optimal", [0.0, 2.0, 2.0, 1.8], 4000, 12, "nemeth", 1.0),
             ("garch", "prior", [0.0, 2.0, 2.0, 1.8], 5000, 6, "nemeth", 0.9),
             ("svm", "prior", [0.95, 1.4, 1.4], 10000, 24, "nemeth", 1.0),
             ("lgssm", "optimal", [0.9, 1.0, 1.2, 1.0], 16384, 5, "nemeth", 0.95),
             ("svm", "prior", [0.9, 1.2, 1.1], 9000, 8, "filter", 1.0)]
    for model, kernel, theta, N, T, smoother, lam in cases:
        y = rs.normal(size=T)
        t1, tL = 1, T - 1
        w = rs.uniform(1.0, 40.0, size=tL - t1)
        z0, u, z = po.draw_streams(rs, N, T)
        q = dict(model=model, kernel=kernel, smoother=smoother, stat="score", dtype="f64", rng="replay", N=N,
                 t1=t1, tL=tL, lambduh=lam, prior_mean=0.0, prior_var=1.5, y=y, weights=w, theta=theta,
                 z0=z0, u=u, z=z)
        assert ctx.variant_name(model, kernel, "f64", "replay", N) == "mem1024"
        o = ctx.run_batch([q], want_final=True)[0]
        r = po.pf_window(model, theta, y, N, z0, u, z, kernel=kernel, pf="filter" if smoother == "filter" else "nemeth",
                         lambduh=lam, stat="score", t1=t1, tL=tL, weights=w, prior_mean=0.0, prior_var=1.5)
        np.testing.assert_allclose(o["x_t"], r["x_t"], rtol=RTOL, atol=ATOL, err_msg=model)
        np.testing.assert_allclose(o["log_weights"], r["log_weights"], rtol=RTOL, atol=ATOL)
        ref = r["statistics"] if smoother == "filter" else r["mean_statistic"]
        np.testing.assert_allclose(o["mean_stat"], ref, rtol=1e-8, atol=1e-8)
        assert abs(o["loglik"] - r["loglikelihood_estimate"]) <= 1e-8 * max(1.0, abs(r["loglikelihood_estimate"]))


def test_batch_heterogeneous_vs_oracle(ctx):
    """One launch, many windows with different N, T, theta, windows, weights (ragged batch)."""
    rs = np.random.RandomState(2024)
    probs, refs = [], []
    for b in range(24):
        N = int(rs.choice([1, 2, 63, 64, 65, 100, 255, 256, 257, 700, 1000, 1024]))
        T = int(rs.choice([0, 1, 2, 7, 24, 40]))
        t1 = int(rs.randint(0, T + 1))
        tL = int(rs.randint(t1, T + 1))
        theta = np.array([rs.uniform(-0.99, 0.99), rs.uniform(0.5, 2.0), rs.uniform(0.5, 2.0)])
        y = rs.normal(size=T) * 1.5
        w = rs.uniform(0.5, 30.0, size=tL - t1) if (b % 2 == 0) else None
        z0, u, z = po.draw_streams(rs, N, T)
        lam = float(rs.choice([1.0, 0.95, 0.5]))
        q = dict(model="svm", kernel="prior", smoother="nemeth", stat="score", dtype="f64", rng="replay",
                 N=N, t1=t1, tL=tL, lambduh=lam, prior_mean=0.3, prior_var=2.0, y=y, weights=w,
                 theta=theta, z0=z0, u=u, z=z)
        probs.append(q)
        refs.append(po.pf_window("svm", theta, y, N, z0, u, z, kernel="prior", pf="nemeth", lambduh=lam,
                                 stat="score", t1=t1, tL=tL, weights=w, prior_mean=0.3, prior_var=2.0))
    outs = ctx.run_batch(probs, want_final=True)
    for q, o, r in zip(probs, outs, refs):
        np.testing.assert_allclose(o["x_t"], r["x_t"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(o["log_weights"], r["log_weights"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(o["statistics"], r["statistics"], rtol=RTOL, atol=1e-8)
        np.testing.assert_allclose(o["mean_stat"], r["mean_statistic"], rtol=RTOL, atol=1e-8)
        assert abs(o["loglik"] - r["loglikelihood_estimate"]) <= ATOL + RTOL * abs(r["loglikelihood_estimate"])


@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "prior"), ("garch", "optimal"),
                                          ("lgssm", "prior"), ("lgssm", "optimal")])
def test_f32_teacher_forced(ctx, golden_trace, model, kernel):
    """f32 particle state, checked one step at a time from the reference's own state at t
    (warm start) so that ancestor flips cannot accumulate."""
    g = golden_trace
    m = [mm for mm in g.meta if mm["model"] == model and mm["kernel"] == kernel and mm["pf"] == "nemeth"
         and mm["lambduh"] is None][0]
    key = m["key"]
    N, T = m["N"], m["T"]
    streams = po.draw_streams(np.random.RandomState(m["seed"]), N, T)
    ax, alw, ast = g.get(key, "all_x_t"), g.get(key, "all_log_weights"), g.get(key, "all_statistics")
    w = g.get(key, "weights")
    probs = []
    for t in range(T):
        inside = m["t1"] <= t < m["tL"]
        probs.append(dict(model=model, kernel=kernel, smoother="nemeth", stat="score", dtype="f32", rng="replay",
                          N=N, t1=0 if inside else 1, tL=1 if inside else 1, lambduh=0.95,
                          y=g.get(key, "y")[t:t + 1], weights=(w[t - m["t1"]:t - m["t1"] + 1] if inside else None),
                          theta=g.get(key, "theta"), u=streams[1][t], z=streams[2][t],
                          init_x=ax[t], init_logw=alw[t], init_stats=ast[t]))
    outs = ctx.run_batch(probs, want_final=True)
    nflip = 0
    for t, o in enumerate(outs):
        # an f32 log-weight can move a CDF entry across u: tolerate (and count) rare flips
        ok = np.isclose(o["x_t"], ax[t + 1], rtol=2e-4, atol=2e-5).all(axis=1)
        nflip += int((~ok).sum())
        np.testing.assert_allclose(o["log_weights"][ok], alw[t + 1][ok], rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(o["statistics"][ok], ast[t + 1][ok], rtol=2e-3, atol=2e-3)
    assert nflip <= 2, nflip


def test_error_paths(ctx):
    base = dict(model="svm", kernel="prior", N=8, y=np.zeros(2), theta=[1.5, 1.0, 1.0],
                z0=np.zeros(8), u=np.zeros(16), z=np.zeros(16))
    with pytest.raises(ValueError, match="AR parameter"):
        ctx.run_batch([base])
    q = dict(base, theta=[0.5, 1.0, 1.0], kernel="optimal")
    with pytest.raises(NotImplementedError, match="optimal kernel not analytic"):
        ctx.run_batch([q])
    q = dict(base, theta=[0.5, 1.0, 1.0], t1=2, tL=1)
    with pytest.raises(ValueError):
        ctx.run_batch([q])
    assert ctx.run_batch([]) == []
    # every refusal of pfg_run_batch itself, on ctypes arrays (Context.run_batch refuses some of these in Python first)
    lib, h = ctx.lib, ctx.handle
    assert lib.pfg_run_batch(h, -1, None, None) == _capi.PFG_ERR_INVALID
    assert "NULL problems/results" in lib.pfg_last_error(h).decode()
    for row in _REFUSALS:
        base, which, fault, code, text = row
        keep = []
        ps, rs = _refusal_batch(keep, base, which, fault)
        rc = lib.pfg_run_batch(h, len(ps), ps, rs)
        msg = lib.pfg_last_error(h).decode()
        assert (rc, text in msg) == (code, True), (row, rc, msg)


_INV, _UNS, _NUM = _capi.PFG_ERR_INVALID, _capi.PFG_ERR_UNSUPPORTED, _capi.PFG_ERR_NUMERIC
_RAW, _CARRY = _capi.FLAG_PARIS_RAW_STREAM, _capi.FLAG_PARIS_RAW_CARRY
_NO_STREAMS = dict(z0=None, u=None, z=None)
# valid two-window batches (SVM, REPLAY, N = 8, T = 2 unless stated); a row changes one of them
_BASES = {
    "svm": {},
    "device": dict(rng=1, **_NO_STREAMS),
    "kalman": dict(model=2, smoother=6, theta=[0.5, 1.0, 1.0, 1.0], **_NO_STREAMS),
    "ffbs": dict(model=2, smoother=7, theta=[0.5, 1.0, 1.0, 1.0], z0=None, u=None),
    "n2": dict(smoother=4),
    "n2_ew": dict(smoother=4, elementwise=1, ew_mean=6),
    "paris": dict(smoother=2, Ntilde=2, paris_man_u=32),
    "paris_device": dict(smoother=2, Ntilde=2, rng=1, **_NO_STREAMS),
    "paris_stream": dict(smoother=2, Ntilde=2, paris_stream=64, paris_stream_len=64),
    "predictive": dict(smoother=1, stat=3, num_steps_ahead=1, pred_z=32),
    "systematic": dict(smoother=3, rng=1, **_NO_STREAMS),
    "elementwise": dict(elementwise=1, ew_mean=6),
}
# (base, window the fault goes into (None: both), fault, code, message substring).  Not here, because no input reaches
# them: elementwise with the predictive statistic (elementwise needs a smoother the predictive statistic refuses), and
# the whole-GPU smoother refusal (only NEMETH / FILTER batches are planned as whole-GPU windows).
_REFUSALS = [
    ("svm", None, dict(model=3), _INV, "Unrecognized model id"),
    ("svm", None, dict(kernel=2), _INV, "Unrecoginized kernel id"),
    ("svm", None, dict(kernel=1), _UNS, "SVM optimal kernel not analytic"),
    ("svm", None, dict(dtype=2), _INV, "bad dtype"),
    ("svm", None, dict(rng=2), _INV, "bad rng mode"),
    ("kalman", None, dict(model=1), _UNS, "the exact Kalman score (kind = 'marginal') is built for LGSSM only"),
    ("kalman", None, dict(dtype=1), _UNS, "the exact Kalman score (kind = 'marginal') is built for dtype f64 only"),
    ("ffbs", None, dict(model=0), _UNS, "FFBS latent paths (kind = 'complete') are built for LGSSM only"),
    ("ffbs", None, dict(dtype=1), _UNS, "FFBS latent paths (kind = 'complete') are built for dtype f64 only"),
    ("ffbs", None, dict(rng=2), _INV, "bad rng mode"),
    ("svm", 1, dict(model=1), _INV, "problem 1: model/kernel/dtype/rng must match across a batch"),
    ("svm", 1, dict(rng=1), _INV, "problem 1: model/kernel/dtype/rng must match across a batch"),
    ("svm", 1, dict(N=0), _INV, "problem 1: N must be >= 1"),
    ("svm", 1, dict(T=-1), _INV, "problem 1: T must be >= 0"),
    ("svm", 1, dict(t1=2, tL=1), _INV, "problem 1: need 0 <= t1 <= tL"),
    ("svm", 1, dict(smoother=5), _INV, "problem 1: Unrecognized pf (smoother id)"),
    ("ffbs", 1, dict(smoother=6), _INV, "problem 1: FFBS latent paths cannot share a batch with other smoothers"),
    ("ffbs", 1, dict(t1=3, tL=3), _INV, "problem 1: need t1 <= T"),
    ("ffbs", 1, dict(prior_var=0.0), _INV, "problem 1: the forward message needs a finite precision > 0"),
    ("ffbs", 1, dict(prior_mean=np.inf), _INV, "problem 1: the forward message needs a finite precision > 0"),
    ("ffbs", 1, dict(stat=1), _INV, "problem 1: FFBS latent paths take no warm start or elementwise statistic"),
    ("ffbs", 1, dict(init_x=8), _INV, "problem 1: FFBS latent paths take no warm start or elementwise statistic"),
    ("ffbs", 1, dict(x_T=8), _INV, "problem 1: FFBS latent paths have no particles"),
    ("ffbs", 1, dict(z=None), _INV, "problem 1: REPLAY FFBS needs z"),
    ("kalman", 1, dict(smoother=0), _INV, "problem 1: the exact Kalman score cannot share a batch with particle filters"),
    ("svm", 1, dict(smoother=6), _INV, "problem 1: the exact Kalman score cannot share a batch with particle filters"),
    ("kalman", 1, dict(t1=3, tL=3), _INV, "problem 1: need t1 <= T"),
    ("kalman", 1, dict(prior_var=np.nan), _INV, "problem 1: the forward message needs a finite precision > 0"),
    ("kalman", 1, dict(stat=3), _INV, "problem 1: the exact Kalman score takes no warm start, elementwise or predictive"),
    ("kalman", 1, dict(trace_x=16), _INV, "problem 1: the exact Kalman score has no particles"),
    ("n2", 1, dict(smoother=0), _INV, "problem 1: pf = 'poyiadjis_N2' cannot share a batch with other smoothers"),
    ("n2", 1, dict(N=16385), _UNS, "problem 1: pf = 'poyiadjis_N2' is implemented for N <= 16384"),
    ("n2_ew", 1, dict(N=5000), _UNS, "problem 1: elementwise statistics with pf = 'poyiadjis_N2' are implemented for N <= 4096"),
    # the edge: ews_n2_step_kernel holds bw[4096] in LDS
    ("n2_ew", 1, dict(N=4097), _UNS, "problem 1: elementwise statistics with pf = 'poyiadjis_N2' are implemented for N <= 4096"),
    ("n2", 1, dict(stat=3), _INV, "problem 1: Only can use pf = 'filter' since we are filtering"),
    ("paris", 1, dict(smoother=0), _INV, "problem 1: pf = 'paris' cannot share a batch with other smoothers"),
    ("paris", 1, dict(Ntilde=0), _INV, "problem 1: Ntilde must be in [1, 64]"),
    ("paris", 1, dict(max_accept_reject=-1), _INV, "problem 1: max_accept_reject must be >= 0"),
    ("paris_stream", None, dict(rng=1), _INV, "problem 0: paris_stream is a REPLAY input"),
    ("paris_stream", 1, dict(paris_man_u=32), _INV, "problem 1: paris_stream replaces the addressed pools"),
    ("paris_stream", 1, dict(paris_stream_len=-1), _INV, "problem 1: paris_stream_len and paris_manual_threshold must be >= 0"),
    ("paris_stream", 1, dict(paris_manual_threshold=-1), _INV, "problem 1: paris_stream_len and paris_manual_threshold must be >= 0"),
    ("paris_stream", 1, dict(N=16385), _UNS, "problem 1: pf = 'paris' is implemented for N <= 16384"),
    ("paris_stream", None, dict(dtype=1, flags=_RAW, **_NO_STREAMS), _UNS, "problem 0: PFG_FLAG_PARIS_RAW_STREAM is built for dtype f64"),
    ("paris_stream", 1, dict(flags=_RAW), _INV, "problem 1: PFG_FLAG_PARIS_RAW_STREAM draws z0 / u / z from paris_stream"),
    ("paris_stream", 1, dict(flags=_CARRY), _INV, "problem 1: PFG_FLAG_PARIS_RAW_CARRY needs PFG_FLAG_PARIS_RAW_STREAM"),
    ("paris_stream", 1, dict(flags=_RAW | _CARRY, paris_stream_len=0, **_NO_STREAMS), _INV,
     "problem 1: PFG_FLAG_PARIS_RAW_CARRY needs PFG_FLAG_PARIS_RAW_STREAM"),
    ("paris_stream", 1, dict(flags=_RAW | _CARRY, init_x=8, init_logw=8, T=0, tL=0, **_NO_STREAMS), _INV,
     "problem 1: PFG_FLAG_PARIS_RAW_CARRY with a warm start and T = 0"),
    ("paris", 1, dict(paris_man_u=None), _INV, "problem 1: REPLAY paris needs the paris_* uniform pools or paris_stream"),
    ("paris", 1, dict(max_accept_reject=1), _INV, "problem 1: REPLAY paris needs the paris_* uniform pools or paris_stream"),
    ("paris_device", 1, dict(flags=_RAW), _INV, "problem 1: PFG_FLAG_PARIS_RAW_STREAM needs paris_stream"),
    ("paris_device", 1, dict(flags=_CARRY), _INV, "problem 1: PFG_FLAG_PARIS_RAW_STREAM needs paris_stream"),
    ("paris_device", 1, dict(flags=_capi.FLAG_PARIS_NO_ACCEPT_REJECT), _UNS,
     "problem 1: PaRIS with accept_reject = False is built for the REPLAY stream order"),
    ("svm", 1, dict(paris_stream=8, paris_stream_len=8), _INV, "problem 1: paris_stream needs pf = 'paris'"),
    ("svm", 1, dict(stat=4), _INV, "problem 1: bad stat id"),
    ("predictive", 1, dict(stat=0), _INV, "problem 1: the predictive statistic cannot share a batch with others"),
    ("predictive", 1, dict(smoother=0), _INV, "problem 1: Only can use pf = 'filter' since we are filtering"),
    ("predictive", 1, dict(num_steps_ahead=16), _INV, "problem 1: num_steps_ahead must be in [0, 15]"),
    ("predictive", 1, dict(N=16385), _UNS, "problem 1: N exceeds the supported maximum of 16384"),
    ("predictive", 1, dict(pred_z=None), _INV, "problem 1: REPLAY predictive needs the pred_z pool"),
    ("svm", 1, dict(theta=None), _INV, "problem 1: theta is NULL"),
    ("svm", 1, dict(y=None), _INV, "problem 1: observations are NULL"),
    ("svm", 1, dict(z0=None), _INV, "problem 1: REPLAY needs z0"),
    ("svm", 1, dict(u=None), _INV, "problem 1: REPLAY needs u and z"),
    ("svm", 1, dict(init_x=8), _INV, "problem 1: init_x needs init_logw"),
    ("systematic", 1, dict(smoother=0), _INV, "problem 1: systematic resampling cannot share a batch with other smoothers"),
    ("systematic", 1, dict(N=1025), _UNS, "problem 1: systematic resampling needs the DEVICE rng and N <= 1024"),
    ("svm", 1, dict(prior_var=-1.0), _INV, "problem 1: prior_var must be >= 0"),
    ("svm", 1, dict(theta=[1.5, 1.0, 1.0]), _NUM, "Current AR parameter is |A| = 1.5 > 1\nTry calling project_parameters?"),
    ("elementwise", 1, dict(smoother=1), _UNS, "problem 1: elementwise statistics are built for pf = 'poyiadjis_N'"),
    ("elementwise", 1, dict(ew_mean=None), _INV, "problem 1: elementwise needs ew_mean"),
    ("elementwise", 1, dict(rec_z=16), _INV, "problem 1: elementwise statistics cannot be combined with trace outputs"),
    ("elementwise", 1, dict(t1=2), _INV, "problem 1: elementwise needs a non-empty window [t1, tL)"),
    ("svm", 1, dict(ew_stats=48), _INV, "problem 1: ew_mean / ew_stats need pfg_problem.elementwise"),
    ("svm", 1, dict(rec_u=16), _INV, "problem 1: rec_u / rec_z / rec_z0 record the DEVICE generator's draws and need trace_x"),
    ("device", 1, dict(rec_z0=8), _INV, "problem 1: rec_u / rec_z / rec_z0 record the DEVICE generator's draws and need trace_x"),
    ("svm", 1, dict(trace_anc=16), _INV, "problem 1: trace_anc needs trace_x"),
    # the traced backward parents [T][Ntilde][N]: with trace_x, of a PaRIS window, and not beside the elementwise pass
    # (which owns the buffer as a work piece)
    ("paris_device", 1, dict(trace_paris_J=32), _INV, "problem 1: trace_paris_J needs trace_x and pf = 'paris'"),
    ("svm", 1, dict(trace_x=24, trace_logw=24, trace_paris_J=32), _INV, "problem 1: trace_paris_J needs trace_x and pf = 'paris'"),
    ("paris_device", 1, dict(elementwise=1, ew_mean=6, trace_paris_J=32), _INV,
     "problem 1: elementwise statistics cannot be combined with trace outputs"),
    ("kalman", 1, dict(trace_paris_J=32), _INV, "problem 1: the exact Kalman score has no particles"),
    ("svm", 1, dict(stats_T=24), _INV, "problem 1: logw_T/stats_T need x_T"),
    ("svm", 1, dict(trace_x=24), _INV, "problem 1: trace_x and trace_logw go together"),
    ("svm", 1, dict(trace_stats=72), _INV, "problem 1: trace_stats needs trace_x"),
    ("device", None, dict(N=20000, elementwise=1, ew_mean=6), _UNS, "problem 0: elementwise statistics are built for N <= 16384"),
    ("device", None, [dict(N=20000), dict(N=600000)], _INV, "problem 0: whole-GPU windows of one batch must all have N <= 524288 or all N > 524288"),
]


def _refusal_batch(keep, base, which, fault):
    """Two windows of _BASES[base] as ctypes arrays, `fault` applied to window `which` (None: both; a list: one fault per
    window).  Pointer fields take
    an entry count (a zero buffer of the field's type), a list (those doubles) or None (NULL)."""
    ps, rs = (_capi.Problem * 2)(), (_capi.Result * 2)()
    for b in range(2):
        fields = dict(model=0, kernel=0, smoother=0, stat=0, dtype=0, rng=0, N=8, T=2, t1=0, tL=2, lambduh=1.0,
                      prior_var=1.0, y=2, theta=[0.5, 1.0, 1.0], z0=8, u=16, z=16)
        fields.update(_BASES[base])
        if isinstance(fault, list):
            fields.update(fault[b])
        elif which is None or which == b:
            fields.update(fault)
        for name, v in fields.items():
            rec = ps[b] if hasattr(_capi.Problem, name) else rs[b]
            ftype = dict(type(rec)._fields_)[name]
            if hasattr(ftype, "contents"):
                if v is not None:
                    a = np.asarray(v, dtype=np.float64) if isinstance(v, list) else np.zeros(v, dtype=ftype._type_)
                    keep.append(a)
                    v = a.ctypes.data_as(ftype)
            setattr(rec, name, v)
    return ps, rs


@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal")])
def test_f32_teacher_forced_large_n_kernel(ctx, golden_trace, force_mem_kernel, model, kernel):
    """f32 state in the large-N kernel (HBM scratch is f32 too), one reference step at a time."""
    test_f32_teacher_forced(ctx, golden_trace, model, kernel)


def test_edge_shapes(ctx):
    """N = 1, T = 0, a window that accumulates nothing (t1 == tL) and a huge observation."""
    rs = np.random.RandomState(5)
    for N, T, t1, tL in [(1, 5, 0, 5), (1, 0, 0, 0), (64, 6, 3, 3), (65, 4, 0, 4)]:
        y = rs.normal(size=T)
        if T > 2:
            y[1] = 40.0                      # extreme observation: weights collapse onto few particles
        theta = [0.9, 1.3, 0.8]
        z0, u, z = po.draw_streams(rs, N, T)
        q = dict(model="svm", kernel="prior", smoother="nemeth", stat="score", dtype="f64", rng="replay", N=N,
                 t1=t1, tL=tL, lambduh=1.0, prior_mean=0.0, prior_var=1.0, y=y, theta=theta, z0=z0, u=u, z=z)
        o = ctx.run_batch([q], want_final=True)[0]
        r = po.pf_window("svm", theta, y, N, z0, u, z, kernel="prior", pf="poyiadjis_N", stat="score", t1=t1, tL=tL,
                         prior_mean=0.0, prior_var=1.0)
        np.testing.assert_allclose(o["x_t"], r["x_t"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(o["mean_stat"], r["mean_statistic"], rtol=1e-8, atol=1e-8)
        assert abs(o["loglik"] - r["loglikelihood_estimate"]) <= 1e-8 * max(1.0, abs(r["loglikelihood_estimate"]))
        if t1 == tL:
            assert o["loglik"] == 0.0 and np.all(o["mean_stat"] == 0.0)


def test_f32_whole_run_statistics(ctx):
    """f32 state, device RNG, whole runs: mean score / log-likelihood agree with f64 runs within
    5 standard errors (f32 cannot be compared seed by seed over long runs, SURVEY finding 2)."""
    rs = np.random.RandomState(9)
    T, N, B = 100, 500, 384
    y = rs.normal(size=T) * 1.2
    theta = [0.95, 1.4142, 1.4142]
    def run(dtype, seed):
        probs = [dict(model="svm", kernel="prior", dtype=dtype, rng="device", N=N, y=y, theta=theta, seed=seed,
                      stream=b, prior_var=5.0) for b in range(B)]
        outs = ctx.run_batch(probs)
        return np.array([np.append(o["mean_stat"], o["loglik"]) for o in outs])
    a, b = run("f64", 1), run("f32", 2)
    se = np.sqrt(a.var(axis=0) / B + b.var(axis=0) / B)
    zs = np.abs(a.mean(axis=0) - b.mean(axis=0)) / se
    assert np.all(zs < 5.0), zs


@pytest.mark.parametrize("model,kernel,theta", [("svm", "prior", [0.95, 1.4, 1.4]),
                                                ("garch", "optimal", [0.0, 2.0, 2.0, 1.8]),
                                                ("lgssm", "optimal", [0.9, 1.0, 1.2, 1.0])])
@pytest.mark.parametrize("N,dtype", [(1500, "f64"), (4000, "f64"), (5000, "f64"), (16384, "f64"), (4000, "f32")])
def test_large_n_device_rng_fast_kernel(ctx, monkeypatch, model, kernel, theta, N, dtype):
    """N > 1024 with the device generator runs pf_big_kernel (thread-major CDF, unrolled search,
    two chunks in flight; NP2 = 4096 / 16384, odd chunk counts included).  Same estimator as the
    general large-N kernel (which is pinned to the reference in REPLAY mode): means of score,
    log-likelihood and filtered state over independent windows agree within Monte-Carlo error,
    for the Poyiadjis, Nemeth and filter smoothers."""
    rs = np.random.RandomState(N)
    T, B = 12, 48
    y = rs.normal(size=T)
    w = rs.uniform(1.0, 3.0, size=T - 3)
    res = {}
    for variant in ("big", "mem1024"):
        if variant == "mem1024":
            monkeypatch.setenv("PFGRAD_VARIANT", "mem1024")
        else:
            monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
        name = ctx.variant_name(model, kernel, dtype, "device", N)
        if variant == "mem1024":
            assert name == "mem1024"
        else:       # N <= 4096 stays LDS-resident when the state fits (SVM fp64, every model in f32)
            assert name in (("wg1024x4s", "big4096") if N <= 4096 else ("big16384",))
        for smoother, lam in (("nemeth", 1.0), ("nemeth", 0.9), ("filter", 1.0)):
            probs = [dict(model=model, kernel=kernel, smoother=smoother, stat="score", dtype=dtype, rng="device",
                          N=N, t1=2, tL=T - 1, lambduh=lam, prior_mean=0.0, prior_var=1.5, y=y, weights=w,
                          theta=theta, seed=7 + (variant == "big"), stream=b) for b in range(B)]
            outs = ctx.run_batch(probs, want_final=True)
            rows = []
            for o in outs:
                p = np.exp(o["log_weights"] - o["log_weights"].max())
                rows.append(np.concatenate([o["mean_stat"], [o["loglik"], np.sum(p * o["x_t"][:, 0]) / p.sum()]]))
            res[(variant, smoother, lam)] = np.array(rows)
            assert np.all(np.isfinite(res[(variant, smoother, lam)]))
    for smoother, lam in (("nemeth", 1.0), ("nemeth", 0.9), ("filter", 1.0)):
        a, b = res[("big", smoother, lam)], res[("mem1024", smoother, lam)]
        se = np.sqrt(a.var(axis=0) / B + b.var(axis=0) / B) + 1e-6 * (1 + np.abs(b.mean(axis=0)))
        zs = np.abs(a.mean(axis=0) - b.mean(axis=0)) / se
        assert np.all(zs < 5.5), (smoother, lam, zs, a.mean(axis=0), b.mean(axis=0))
    # the same window gives the same answer twice (reproducible streams)
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    q = dict(model=model, kernel=kernel, smoother="nemeth", stat="score", dtype=dtype, rng="device", N=N, t1=0, tL=T,
             lambduh=1.0, prior_mean=0.0, prior_var=1.5, y=y, theta=theta, seed=3, stream=9)
    o1, o2 = ctx.run_batch([q])[0], ctx.run_batch([q])[0]
    assert np.array_equal(o1["mean_stat"], o2["mean_stat"]) and o1["loglik"] == o2["loglik"]


@pytest.mark.parametrize("variant", ["auto", "wg256x4", "wg256x4s", "wg1024x1", "wg64x2", "mem1024"])
@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "prior"), ("garch", "optimal"),
                                          ("lgssm", "prior"), ("lgssm", "optimal")])
def test_randomised_windows_every_variant(ctx, monkeypatch, model, kernel, variant):
    """Randomised ragged batches (N, T, window, weights, lambda, smoother, statistic drawn at
    random) for every model / proposal on every kernel variant, REPLAY fp64 vs the oracle."""
    if variant == "auto":
        monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    else:
        monkeypatch.setenv("PFGRAD_VARIANT", variant)
    rs = np.random.RandomState(sum(map(ord, model + kernel + variant)))
    from test_host_logic import default_params
    theta = default_params(model).theta()
    probs, refs = [], []
    for b in range(10):
        N = int(rs.choice([1, 3, 64, 65, 200, 257, 999, 1000, 1024]))
        T = int(rs.choice([0, 1, 3, 9, 20]))
        t1 = int(rs.randint(0, T + 1))
        tL = int(rs.randint(t1, T + 1))
        y = rs.normal(size=T) * (1.5 if model != "garch" else 0.6)
        w = rs.uniform(0.5, 10.0, size=tL - t1) if rs.rand() < 0.5 else None
        z0, u, z = po.draw_streams(rs, N, T)
        smoother, lam = [("nemeth", 1.0), ("nemeth", 0.9), ("filter", 1.0)][int(rs.randint(3))]
        stat = "score" if rs.rand() < 0.7 else "suff"
        probs.append(dict(model=model, kernel=kernel, smoother=smoother, stat=stat, dtype="f64", rng="replay", N=N,
                          t1=t1, tL=tL, lambduh=lam, prior_mean=-0.2, prior_var=1.3, y=y, weights=w, theta=theta,
                          z0=z0, u=u, z=z))
        refs.append(po.pf_window(model, theta, y, N, z0, u, z, kernel=kernel,
                                 pf="filter" if smoother == "filter" else "nemeth", lambduh=lam, stat=stat,
                                 t1=t1, tL=tL, weights=w, prior_mean=-0.2, prior_var=1.3))
    # one launch per statistic / smoother family is not required: a batch may mix them
    outs = ctx.run_batch(probs, want_final=True)
    for q, o, r in zip(probs, outs, refs):
        tag = str((model, kernel, variant, q["N"], q["y"].shape[0], q["t1"], q["tL"], q["smoother"], q["lambduh"], q["stat"]))
        np.testing.assert_allclose(o["x_t"], r["x_t"], rtol=RTOL, atol=ATOL, err_msg=tag)
        np.testing.assert_allclose(o["log_weights"], r["log_weights"], rtol=RTOL, atol=ATOL, err_msg=tag)
        ref = r["statistics"] if q["smoother"] == "filter" else r["mean_statistic"]
        np.testing.assert_allclose(o["mean_stat"], ref, rtol=RTOL, atol=1e-8, err_msg=tag)
        assert abs(o["loglik"] - r["loglikelihood_estimate"]) <= ATOL + RTOL * abs(r["loglikelihood_estimate"]), tag


@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "optimal"), ("garch", "prior"), ("lgssm", "optimal")])
def test_degenerate_weights_and_outliers(ctx, monkeypatch, model, kernel):
    """Observations with 40-sigma outliers and exact zeros: log-weights hundreds of units below
    zero, one particle carrying (almost) all the weight.  REPLAY fp64 stays on the oracle; the
    device-generator variants (32-bit CDF, thread-major order, f32-unit normals) stay finite and
    agree with each other on the log-likelihood within Monte-Carlo error."""
    from test_host_logic import default_params
    theta = default_params(model).theta()
    rs = np.random.RandomState(12)
    T = 14
    y = rs.normal(size=T) * 0.5
    y[3], y[4], y[9] = 40.0, 0.0, -35.0
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    for N in (100, 1000, 3000):
        z0, u, z = po.draw_streams(rs, N, T)
        q = dict(model=model, kernel=kernel, smoother="nemeth", stat="score", dtype="f64", rng="replay", N=N, t1=0,
                 tL=T, lambduh=1.0, prior_mean=0.0, prior_var=1.0, y=y, theta=theta, z0=z0, u=u, z=z)
        o = ctx.run_batch([q])[0]
        r = po.pf_window(model, theta, y, N, z0, u, z, kernel=kernel, pf="poyiadjis_N", stat="score",
                         prior_mean=0.0, prior_var=1.0)
        assert np.all(np.isfinite(r["mean_statistic"]))
        np.testing.assert_allclose(o["mean_stat"], r["mean_statistic"], rtol=1e-7, atol=1e-7)
        # the reference's log(mean(exp(logw))) is not max-stabilised and underflows to -inf on the
        # outlier steps of the GARCH prior kernel; the kernel's m + log(W/N) stays finite
        # (deviation (i))
        ref_ll = r["loglikelihood_estimate"]
        assert np.isfinite(o["loglik"])
        if np.isfinite(ref_ll):
            assert abs(o["loglik"] - ref_ll) <= 1e-8 * abs(ref_ll)
        lls = {}
        for dtype in ("f64", "f32"):
            probs = [dict(q, rng="device", dtype=dtype, seed=4, stream=b) for b in range(64 if N < 2000 else 80)]
            for p_ in probs:
                for k in ("z0", "u", "z"):
                    p_.pop(k)
            outs = ctx.run_batch(probs)
            ll = np.array([o_["loglik"] for o_ in outs])
            ms = np.array([o_["mean_stat"] for o_ in outs])
            assert np.all(np.isfinite(ll)) and np.all(np.isfinite(ms)), (model, N, dtype)
            lls[dtype] = ll
        se = np.sqrt(lls["f64"].var() / len(lls["f64"]) + lls["f32"].var() / len(lls["f32"])) + 1e-6
        assert abs(lls["f64"].mean() - lls["f32"].mean()) < 6 * se + 2e-4 * abs(lls["f64"].mean())
        assert abs(lls["f64"].mean() - o["loglik"]) < 8 * lls["f64"].std() + 1.0


@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal"), ("lgssm", "prior")])
def test_one_wave_variant_replay_parity(ctx, monkeypatch, model, kernel):
    """wg64x2 (N <= 128, one wave per window) is what launches of more than 64 small windows run
    on: 70 ragged windows in one launch, REPLAY fp64 vs the oracle, plus the fully traced
    reference fixtures (N = 32) forced onto it."""
    from test_host_logic import default_params
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)
    theta = default_params(model).theta()
    rs = np.random.RandomState(31)
    probs, refs = [], []
    for b in range(70):
        N = int(rs.choice([1, 2, 5, 63, 64, 65, 100, 127, 128]))
        T = int(rs.choice([0, 1, 4, 11]))
        t1 = int(rs.randint(0, T + 1))
        tL = int(rs.randint(t1, T + 1))
        y = rs.normal(size=T) * (1.2 if model != "garch" else 0.6)
        w = rs.uniform(0.5, 5.0, size=tL - t1) if b % 3 == 0 else None
        z0, u, z = po.draw_streams(rs, N, T)
        smoother, lam = [("nemeth", 1.0), ("nemeth", 0.8), ("filter", 1.0)][b % 3]
        probs.append(dict(model=model, kernel=kernel, smoother=smoother, stat="score", dtype="f64", rng="replay", N=N,
                          t1=t1, tL=tL, lambduh=lam, prior_mean=0.2, prior_var=0.9, y=y, weights=w, theta=theta,
                          z0=z0, u=u, z=z))
        refs.append(po.pf_window(model, theta, y, N, z0, u, z, kernel=kernel,
                                 pf="filter" if smoother == "filter" else "nemeth", lambduh=lam, stat="score",
                                 t1=t1, tL=tL, weights=w, prior_mean=0.2, prior_var=0.9))
    assert ctx.variant_name(model, kernel, "f64", "replay", 128) == "wg64x2"
    outs = ctx.run_batch(probs, want_final=True)
    for q, o, r in zip(probs, outs, refs):
        np.testing.assert_allclose(o["x_t"], r["x_t"], rtol=RTOL, atol=ATOL)
        ref = r["statistics"] if q["smoother"] == "filter" else r["mean_statistic"]
        np.testing.assert_allclose(o["mean_stat"], ref, rtol=RTOL, atol=1e-8)
        assert abs(o["loglik"] - r["loglikelihood_estimate"]) <= ATOL + RTOL * abs(r["loglikelihood_estimate"])


def test_theta_grid_replay_f64(ctx):
    """Round 3: the reference over a GRID of parameters (tests/golden/theta_grid.npz: LGSSM C = 0.3 / 1.7 -- the
    optimal kernel's weight "assumes C = 1", lgssm/kernels.py:117-120 --, |A| = 0.9999, Cholesky factors 0.1 / 10,
    GARCH phi = 0.999, lambduh = 0.01 / 0.99).  REPLAY fp64, every traced step and the N = 1000 windows, rtol 1e-9.
    Where the reference's own log-likelihood underflows to -inf (one Nemeth trace with log-weights of -3.6e5; it is
    not max-stabilised, buffered_smoother.py:124-126) the kernel's must be finite (DESIGN deviation (i))."""
    from conftest import Golden
    g = Golden("theta_grid.npz")
    by = {}
    for m in g.meta:
        by.setdefault((m["model"], m["kernel"], m["traced"]), []).append((m, _problem(m, g)))
    n = 0
    for (_, _, traced), items in by.items():
        outs = ctx.run_batch([q for _, q in items], want_trace=traced, want_final=not traced)
        for (m, _), o in zip(items, outs):
            key = m["key"]
            if traced:
                np.testing.assert_allclose(o["all_x_t"], g.get(key, "all_x_t"), rtol=RTOL, atol=ATOL, err_msg=str(m))
                np.testing.assert_allclose(o["all_log_weights"], g.get(key, "all_log_weights"), rtol=RTOL, atol=ATOL, err_msg=str(m))
                ref_ll = g.get(key, "all_loglikelihood_estimate")
                ok = np.isfinite(ref_ll)
                np.testing.assert_allclose(o["all_loglikelihood_estimate"][ok], ref_ll[ok], rtol=RTOL, atol=ATOL, err_msg=str(m))
                assert np.all(np.isfinite(o["all_loglikelihood_estimate"]))
                if m["pf"] != "filter":
                    ref = g.get(key, "all_statistics")
                    scale = max(1.0, np.abs(ref).max())
                    np.testing.assert_allclose(o["all_statistics"], ref, rtol=RTOL, atol=1e-9 * scale, err_msg=str(m))
                    np.testing.assert_allclose(o["mean_stat"], g.get(key, "mean_statistic"), rtol=RTOL, atol=1e-9 * scale)
                else:
                    ref = g.get(key, "all_statistics")[-1]
                    np.testing.assert_allclose(o["mean_stat"], ref, rtol=RTOL, atol=1e-9 * max(1.0, np.abs(ref).max()), err_msg=str(m))
            else:
                ll = float(g.get(key, "loglikelihood_estimate"))
                assert abs(o["loglik"] - ll) <= ATOL + RTOL * abs(ll), (m, o["loglik"], ll)
                ref = g.get(key, "mean_statistic")
                l2 = np.linalg.norm(o["mean_stat"] - ref)
                assert l2 <= 1e-7 * max(1.0, np.linalg.norm(ref)), (m, o["mean_stat"], ref)
                np.testing.assert_allclose(o["log_weights"], g.get(key, "log_weights"), rtol=RTOL, atol=ATOL, err_msg=str(m))
            n += 1
    assert n == len(g.meta) == 76


@pytest.mark.parametrize("variant", ["wg256x4s", "wg1024x1", "wg64x2", "wg256x4"])
@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal")])
def test_replay_production_twin_equals_traced_twin(ctx, monkeypatch, model, kernel, variant):
    """The REPLAY kernels have a twin with the trace instrumentation compiled out (what the drop-in Sampler launches, r3);
    asked for traces the same windows run on the instrumented twin.  Same arithmetic: gradients bitwise equal,
    log-likelihoods to rounding (flushed per step when traced), and `last_traced` says which one ran."""
    monkeypatch.setenv("PFGRAD_VARIANT", variant)
    from test_host_logic import default_params
    rs = np.random.RandomState(11)
    theta = default_params(model).theta()
    N = 100 if variant == "wg64x2" else 1000
    probs = []
    for b in range(6):
        T = 40 + b
        z0, u, z = po.draw_streams(rs, N, T)
        probs.append(dict(model=model, kernel=kernel, smoother="nemeth", stat="score", dtype="f64", rng="replay", N=N,
                          t1=3, tL=T - 2, lambduh=1.0 if b % 2 else 0.9, prior_mean=0.0, prior_var=2.0,
                          y=rs.normal(size=T) * (1.5 if model != "garch" else 0.6), weights=rs.uniform(0.5, 3.0, size=T - 5),
                          theta=theta, z0=z0, u=u, z=z))
    a = ctx.run_batch([dict(q) for q in probs], want_final=True)
    assert ctx.last_variant() == variant and not ctx.last_traced()
    b = ctx.run_batch([dict(q) for q in probs], want_final=True, want_trace=True)
    assert ctx.last_variant() == variant and ctx.last_traced()
    for x, y_ in zip(a, b):
        assert np.array_equal(x["mean_stat"], y_["mean_stat"]) and np.array_equal(x["x_t"], y_["x_t"])
        assert np.array_equal(x["log_weights"], y_["log_weights"])
        assert abs(x["loglik"] - y_["loglik"]) <= 1e-12 * abs(y_["loglik"])


@pytest.mark.parametrize("model,kernel,N,variant", [("svm", "prior", 1000, "wg256x4s"), ("svm", "prior", 1000, "wg256x4"),
                                                    ("lgssm", "optimal", 100, "wg64x2"), ("lgssm", "prior", 777, "wg256x4s"),
                                                    ("svm", "prior", 1000, "wg1024x1"), ("svm", "prior", 4000, "mem1024"),
                                                    ("lgssm", "optimal", 2500, "mem1024")])
def test_replay_score_only_twin_is_bitwise_the_general_kernel(ctx, monkeypatch, model, kernel, N, variant):
    """A batch whose windows are all the Poyiadjis O(N) score (NEMETH, lambduh = 1, score) runs the seed-compatible units'
    twin with the filter / lambda != 1 / other statistics compiled out (PFG_SMOOTHER_POYIADJIS_N, chosen by pfg_run_batch).
    The REPLAY units are built without floating-point contraction, so the twin is the general kernel's arithmetic operation
    for operation: BITWISE the same result record and final particles.  PFGRAD_NO_SCORE1=1 launches the general kernel."""
    rs = np.random.RandomState(N)
    theta = {"svm": [0.95, 1.2, 1.3], "lgssm": [0.9, 1.0, 1.2, 1.0]}[model]
    probs = []
    for b in range(4):
        T = 30 + b
        z0, u, z = po.draw_streams(rs, N, T)
        probs.append(dict(model=model, kernel=kernel, smoother="nemeth", stat="score", dtype="f64", rng="replay", N=N, t1=2, tL=T - 3,
                          lambduh=1.0, prior_mean=0.0, prior_var=2.0, y=rs.normal(size=T), weights=rs.uniform(0.5, 3.0, size=T - 5),
                          theta=theta, z0=z0, u=u, z=z))
    monkeypatch.setenv("PFGRAD_VARIANT", variant)
    twin = ctx.run_batch([dict(q) for q in probs], want_final=True)
    assert ctx.last_variant() == variant + "_score1"
    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    general = ctx.run_batch([dict(q) for q in probs], want_final=True)
    assert ctx.last_variant() == variant
    for a, g in zip(twin, general):
        assert np.array_equal(a["mean_stat"], g["mean_stat"]) and a["loglik"] == g["loglik"]
        assert np.array_equal(a["x_t"], g["x_t"]) and np.array_equal(a["log_weights"], g["log_weights"]) and np.array_equal(a["statistics"], g["statistics"])
    # one window with lambduh = 0.9 in the batch: pfg_run_batch does not state POYIADJIS_N, the general kernel runs
    monkeypatch.delenv("PFGRAD_NO_SCORE1")
    mixed = [dict(q) for q in probs]
    mixed[1]["lambduh"] = 0.9
    out = ctx.run_batch(mixed, want_final=True)
    assert ctx.last_variant() == variant
    assert np.array_equal(out[0]["mean_stat"], general[0]["mean_stat"]) and not np.array_equal(out[1]["mean_stat"], general[1]["mean_stat"])
