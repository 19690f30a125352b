"""GPU tests: a window's result does not depend on the batch it runs in.

Every launch path sizes what a batch shares (dynamic LDS, the per-window scratch stride, unroll bounds) once, from the
batch's largest window, and each workgroup then lays out its own window from its own N.  The property pinned here:
when the batch and the lone window run the SAME kernel (ctx.last_variant() equal; PFGRAD_VARIANT forces it where the
plan depends on B or n_max), every window's mean_stat, loglik, x_t, log_weights, final statistics and traced
trajectory / ancestors are BITWISE those of the same descriptor run alone, and the same again with the batch reversed
(so every window also changes its position).  The batches mix N, T (0 and 1 included), t1 / tL, theta, weights
present and absent, lambduh and the smoother.

Device-generator windows are run with PFGRAD_NO_SCORE1=1 where the batch mixes estimators: the score-only twins fuse
multiply-adds differently from the general kernels, so which one a launch picks (from the whole batch) would change
the last bits.  The twins themselves are covered by batches in which every window is the Poyiadjis O(N) score.

Where the plan legitimately runs a different instantiation for the lone window, agreement is asserted at 1e-13
relative instead, and the docstring names the cause.  The Kalman / FFBS "alone" tests live with those kernels.
"""
import numpy as np
import pytest

from oracle import pf_oracle as po

pytestmark = pytest.mark.gpu

THETAS = {
    "svm": ([0.95, 1.4, 1.4], [0.6, 1.1, 0.8], [-0.3, 0.9, 1.7]),
    "garch": ([0.0, 2.0, 2.0, 1.8], [0.2, 1.5, 1.8, 1.2], [-0.1, 2.2, 2.2, 2.0]),
    "lgssm": ([0.9, 1.0, 1.2, 1.0], [0.5, 0.7, 0.8, 1.5], [-0.7, 1.3, 1.0, 0.6]),
}
# (T, t1, tL) of the windows, cycled: the empty series, one step, an empty accumulation window, buffers on both sides
SHAPES = ((5, 1, 4), (0, 0, 0), (1, 0, 1), (3, 0, 3), (6, 2, 2), (4, 0, 3), (2, 1, 2))
LAMBDAS = (1.0, 0.9, 0.95)


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def window(model, kernel, N, i, rng="replay", smoother=None, stat="score", dtype="f64", shape=None, **extra):
    """The i-th window of a mixed batch: shape, theta, weights and lambduh all cycle with i."""
    rs = np.random.RandomState(1000 * i + N % 997)
    T, t1, tL = shape if shape is not None else SHAPES[i % len(SHAPES)]
    smoother = smoother or ("filter" if i % 5 == 3 else "nemeth")
    q = dict(model=model, kernel=kernel, smoother=smoother, stat=stat, dtype=dtype, rng=rng, N=N, t1=t1, tL=tL,
             lambduh=LAMBDAS[i % len(LAMBDAS)] if smoother == "nemeth" else 1.0, prior_mean=0.1 * (i % 3),
             prior_var=1.5, y=rs.normal(size=T), theta=THETAS[model][i % len(THETAS[model])])
    if i % 2 == 0 and tL > t1:
        q["weights"] = rs.uniform(1.0, 40.0, size=tL - t1)
    if rng == "replay":
        q["z0"], q["u"], q["z"] = po.draw_streams(rs, N, T)
    else:
        q["seed"], q["stream"] = 77, 5 * i + 3
    q.update(extra)
    return q


def batch(model, kernel, Ns, **kw):
    return [window(model, kernel, N, i, **kw) for i, N in enumerate(Ns)]


KEYS = ("mean_stat", "loglik", "x_t", "log_weights", "statistics", "predictive", "all_x_t", "all_log_weights",
        "all_statistics", "all_loglikelihood_estimate", "all_ancestors")


def assert_same(a, b, where, rtol=0.0):
    for k in KEYS:
        if k not in a and k not in b:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (where, k, x.shape, y.shape)
        if rtol == 0.0 or x.dtype.kind != "f":
            if x.dtype.kind == "f":
                x, y = x.astype(np.float64).view(np.uint64), y.astype(np.float64).view(np.uint64)
            bad = np.flatnonzero(x.reshape(-1) != y.reshape(-1))
            assert bad.size == 0, (where, k, bad[:8], np.asarray(a[k]).reshape(-1)[bad[:4]], np.asarray(b[k]).reshape(-1)[bad[:4]])
        else:
            np.testing.assert_allclose(x, y, rtol=rtol, atol=rtol, err_msg="{0} {1}".format(where, k))


def check_alone(ctx, qs, expect, trace=True, rtol=0.0, lone_variant=None, every=1):
    """Run qs as one batch, reversed, and window by window; assert the kernel and the results."""
    outs = ctx.run_batch(qs, want_final=True, want_trace=trace)
    assert ctx.last_variant() == expect, (ctx.last_variant(), expect)
    rev = ctx.run_batch(qs[::-1], want_final=True, want_trace=trace)[::-1]
    assert ctx.last_variant() == expect
    for b in range(len(qs)):
        assert_same(outs[b], rev[b], ("reversed", b))
        assert np.all(np.isfinite(outs[b]["mean_stat"])) and np.isfinite(outs[b]["loglik"]), (b, outs[b]["mean_stat"])
    for b in range(0, len(qs), every):
        o1 = ctx.run_batch([qs[b]], want_final=True, want_trace=trace)[0]
        assert ctx.last_variant() == (lone_variant or expect), (b, ctx.last_variant())
        assert_same(outs[b], o1, ("alone", b, qs[b]["N"]), rtol=rtol)
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# the LDS-resident kernels
# ---------------------------------------------------------------------------------------------------------------------
REG = [
    # variant, rng, model, kernel, Ns
    ("wg64x2", "replay", "svm", "prior", (128, 1, 77, 100, 64, 3)),
    ("wg256x4s", "replay", "garch", "optimal", (1000, 17, 1024, 513, 256, 999, 5)),
    ("wg1024x1", "replay", "lgssm", "optimal", (700, 1024, 3, 1000, 257)),
    ("wg64x2s", "device", "lgssm", "prior", (128, 100, 1, 65, 33)),
    ("wg256x4s", "device", "svm", "prior", (1024, 300, 1, 1000, 64, 777)),
    ("wg1024x1", "device", "garch", "prior", (1024, 257, 900, 2)),
]


@pytest.mark.parametrize("trace", [True, False])
@pytest.mark.parametrize("case", REG, ids=lambda c: "{0}-{1}-{2}".format(*c))
def test_reg_variants_alone_equals_batched(ctx, monkeypatch, case, trace):
    """The plain LDS-resident kernels, traced (the trace-honouring build) and not (the production twin)."""
    variant, rng, model, kernel, Ns = case
    monkeypatch.setenv("PFGRAD_VARIANT", variant)
    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    check_alone(ctx, batch(model, kernel, Ns, rng=rng), variant, trace=trace)


def test_reg_f32_alone_equals_batched(ctx, monkeypatch):
    monkeypatch.setenv("PFGRAD_VARIANT", "wg256x4")
    check_alone(ctx, batch("lgssm", "prior", (1000, 31, 1024, 400), rng="replay", dtype="f32"), "wg256x4")


@pytest.mark.parametrize("rng", ["replay", "device"])
def test_score1_twins_alone_equal_batched(ctx, monkeypatch, rng):
    """Every window the Poyiadjis O(N) score (nemeth, lambduh = 1, score, untraced): batch and lone windows both run
    the score-only twin of the forced unit."""
    monkeypatch.delenv("PFGRAD_NO_SCORE1", raising=False)
    variant = "wg256x4s" if rng == "replay" else "wg64x2s"
    Ns = (1000, 256, 1, 1024, 77) if rng == "replay" else (128, 1, 100, 64)
    monkeypatch.setenv("PFGRAD_VARIANT", variant)
    qs = batch("svm", "prior", Ns, rng=rng, smoother="nemeth", lambduh=1.0)
    check_alone(ctx, qs, variant + "_score1", trace=False)


def test_batches_across_the_latency_batch_size(ctx, monkeypatch):
    """B = 63, 64, 65 and 80 windows around kLatencyBatch: the plan would switch variants with B, so the variant is
    forced; each window equals itself alone and in every other batch size."""
    monkeypatch.setenv("PFGRAD_VARIANT", "wg256x4s")
    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    Ns = [int(n) for n in np.random.RandomState(3).randint(1, 1025, size=80)]
    full = batch("svm", "prior", Ns, rng="device")
    ref = check_alone(ctx, full, "wg256x4s", trace=False, every=9)
    for B in (63, 64, 65):
        outs = ctx.run_batch(full[:B], want_final=True)
        assert ctx.last_variant() == "wg256x4s"
        for b in range(B):
            assert_same(outs[b], ref[b], ("B", B, b))


# ---------------------------------------------------------------------------------------------------------------------
# the large-N kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns", [(4096, 1025, 3000, 1, 2048), (16384, 4097, 9000, 12000)], ids=["lw4", "general"])
def test_mem1024_alone_equals_batched(ctx, monkeypatch, Ns):
    """The general large-N kernel, REPLAY: its LW4 instantiation for batches with N <= 4096, the general one above
    (the name is the same: each batch stays on one side of 4096, so batch and lone window run the same code)."""
    monkeypatch.setenv("PFGRAD_VARIANT", "mem1024")
    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    check_alone(ctx, batch("svm", "prior", Ns, rng="replay"), "mem1024")
    check_alone(ctx, batch("garch", "optimal", Ns[:3], rng="replay"), "mem1024", trace=False)


@pytest.mark.parametrize("Ns,variant", [((4096, 1025, 3000, 2048), "big4096"), ((16384, 4097, 9000, 5000), "big16384")])
def test_big_alone_equals_batched(ctx, monkeypatch, Ns, variant):
    """The fast large-N kernel (device generator, sorted uniforms): one np2 class per batch.  PFGRAD_VARIANT=big keeps
    the lone windows whose state would fit an LDS-resident unit on it."""
    monkeypatch.setenv("PFGRAD_VARIANT", "big")
    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    check_alone(ctx, batch("lgssm", "optimal", Ns, rng="device"), variant)
    check_alone(ctx, batch("garch", "prior", Ns[:3], rng="device"), variant, trace=False)


def test_predictive_alone_equals_batched(ctx):
    """The predictive statistic (general large-N kernel, any N): pred_z, its own scratch after the window's."""
    qs = []
    for i, N in enumerate((3000, 200, 1025, 5000)):
        q = window("svm", "prior", N, i, rng="replay", smoother="filter", stat="predictive", shape=(4 + i % 2, 0, 4 + i % 2),
                   num_steps_ahead=2 + i % 2)
        T = q["y"].shape[0]
        q["pred_z"] = np.random.RandomState(i).normal(size=T * (q["num_steps_ahead"] + 1) * N)
        qs.append(q)
    outs = ctx.run_batch(qs, want_final=True)
    assert ctx.last_variant() == "mem1024"
    for b, q in enumerate(qs):
        o1 = ctx.run_batch([q], want_final=True)[0]
        assert ctx.last_variant() == "mem1024"
        assert_same(outs[b], o1, ("predictive", b))


# ---------------------------------------------------------------------------------------------------------------------
# the smoothers with kernels of their own
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,Ns", [("paris64x2", (128, 1, 100, 50)), ("paris256x4", (1024, 300, 17, 900)),
                                        ("paris_mem1024", (3000, 1025, 2000))])
def test_paris_alone_equals_batched(ctx, monkeypatch, variant, Ns):
    """PaRIS (device generator): the one-wave unit, an LDS-resident unit, the large-N kernel's PaRIS instantiation."""
    if variant != "paris_mem1024":
        monkeypatch.setenv("PFGRAD_VARIANT", variant)
    qs = batch("svm", "prior", Ns, rng="device", smoother="paris", Ntilde=2, max_accept_reject=8)
    check_alone(ctx, qs, variant, trace=False)


def test_n2_mem1024_alone_equals_batched(ctx):
    qs = batch("lgssm", "prior", (1500, 1100, 2000), rng="replay", smoother="poyiadjis_n2")
    check_alone(ctx, qs, "n2_mem1024", trace=False)


def test_systematic_alone_equals_batched(ctx):
    qs = batch("garch", "prior", (1024, 100, 1, 700, 333), rng="device", smoother="nemeth_systematic")
    check_alone(ctx, qs, "systematic256x4", trace=False)


# ---------------------------------------------------------------------------------------------------------------------
# the whole-GPU window
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", ["replay", "device"])
def test_grid_alone_equals_batched(ctx, monkeypatch, rng):
    """Whole-GPU windows of the 1024-particle tile class (REPLAY: PFGRAD_VARIANT=grid also brings N <= 16384 in)."""
    monkeypatch.setenv("PFGRAD_VARIANT", "grid")
    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    Ns = (40000, 1000, 16385, 3, 100003) if rng == "replay" else (40000, 16385, 100003, 20000)
    qs = batch("svm", "prior", Ns, rng=rng, smoother="nemeth")
    check_alone(ctx, qs, "grid1024", trace=(rng == "replay"))


def test_grid_device_across_two_to_the_20(ctx, monkeypatch):
    """Device generator, 2048-particle tiles, a batch straddling 2^20: the batch's step kernel is unrolled for the
    8 tile partials per thread of n_max > 2^20 (kmax = 8), a lone window with N <= 2^20 runs the kmax = 2 build.  The
    two reduce the same partials in the same order; asserted at 1e-13 relative."""
    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    qs = batch("svm", "prior", ((1 << 20) + 1, 600000, 1 << 20), rng="device", smoother="nemeth",
               shape=(2, 0, 2))
    check_alone(ctx, qs, "grid2048", trace=False, rtol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# the predictive statistic through pfg_launch_device
# ---------------------------------------------------------------------------------------------------------------------
def test_predictive_descriptor_on_the_device_path_gets_nans(ctx):
    """pfg_launch_device plans without seeing the descriptors: with REPLAY and 1024 < N <= 4096 it runs the LW4
    instantiation of the large-N kernel, which has no predictive branch.  A PFG_STAT_PREDICTIVE descriptor must get
    NaNs there (as the score-only twins refuse foreign windows), never another statistic's numbers; the same window
    through pfg_run_batch takes the general kernel and matches the predictive oracle."""
    import torch
    from sgmcmc_ssm_amd import _capi
    model, N, T, K = "svm", 2000, 6, 2
    theta = [0.9, 1.2, 1.1]
    rs = np.random.RandomState(41)
    y = rs.normal(size=T)
    z0, u, z = po.draw_streams(rs, N, T)
    pz = rs.normal(size=(T, K + 1, N))
    q = dict(model=model, kernel="prior", smoother="filter", stat="predictive", dtype="f64", rng="replay", N=N, t1=0,
             tL=T, prior_mean=0.0, prior_var=2.0, y=y, theta=theta, z0=z0, u=u, z=z, pred_z=pz, num_steps_ahead=K)
    o = ctx.run_batch([q])[0]
    assert ctx.last_variant() == "mem1024"
    r = po.pf_window(model, theta, y, N, z0, u, z, kernel="prior", pf="filter", stat="predictive", num_steps_ahead=K,
                     pred_normals=lambda t, k: pz[t, k], prior_mean=0.0, prior_var=2.0)
    np.testing.assert_allclose(o["predictive"], r["statistics"], rtol=1e-9, atol=1e-9)
    assert abs(o["loglik"] - r["loglikelihood_estimate"]) <= 1e-9 * max(1.0, abs(r["loglikelihood_estimate"]))

    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(dev)
    yd, thd, z0d, ud, zd, pzd = t(y), t(theta + [0.0]), t(z0), t(u), t(z), t(pz)
    out = torch.zeros(_capi.OUT_DOUBLES, dtype=torch.float64, device=dev)
    pred = torch.zeros(_capi.MAX_PRED, dtype=torch.float64, device=dev)
    scratch = torch.zeros(ctx.scratch_bytes(model, "f64", "replay", N), dtype=torch.uint8, device=dev)
    pscratch = torch.zeros(N * _capi.MAX_PRED * 8, dtype=torch.uint8, device=dev)
    d = np.zeros(1, dtype=_capi.DEV_PROBLEM_DTYPE)
    d["y"], d["theta"], d["z0"], d["u"], d["z"] = yd.data_ptr(), thd.data_ptr(), z0d.data_ptr(), ud.data_ptr(), zd.data_ptr()
    d["out"], d["scratch"] = out.data_ptr(), scratch.data_ptr()
    d["pred_z"], d["pred_out"], d["pred_scratch"] = pzd.data_ptr(), pred.data_ptr(), pscratch.data_ptr()
    d["num_steps_ahead"] = K
    d["prior_var"], d["lambduh"] = 2.0, 1.0
    d["T"], d["t1"], d["tL"], d["N"] = T, 0, T, N
    d["smoother"], d["stat"] = _capi.SMOOTHER["filter"], _capi.STAT["predictive"]
    desc = torch.from_numpy(d.view(np.uint8).reshape(1, -1)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ctx.launch_device(model, "prior", "f64", "replay", N, 1, desc.data_ptr(), st)
    torch.cuda.synchronize(dev)
    assert ctx.last_variant() == "mem1024"
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[:_capi.MAX_STAT + 1])), got
