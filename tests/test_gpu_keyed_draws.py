"""GPU: the kernels driven by counter-keyed Philox4x32-10 draws outside the particle filters, draw for draw against the
host mirror (tests/helpers/keyed_draws.py): the resident chain updates (SGLD, SGHMC, SGRLD, Gibbs) against a
long-double evaluation of the formulas include/pfgrad.h states, the window samplers bitwise, and the device-generator
FFBS against the mirrored lane generator.  The statistical tests elsewhere check the law of the draws; these check the
values, so a drift term, a score column or a key word that is off shows up in every chain.  Each case is one launch
through the C ABI on device tensors."""
import os
import sys

import numpy as np
import pytest

from test_host_logic import PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import device_windows  # noqa: E402
import ffbs_model  # noqa: E402
import keyed_draws as kd  # noqa: E402
import lgssm_chain_rules as rules  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096
EPS, TSCALE, SEED = 0.02, 50.0, 0x5EED0000C0DE1234
# (chain_offset, *step_ctr or None): the high words of the chain id and of the counter both take part in the key
KEYS = [(0, None), (0, 0), (2 ** 32 - 100, 7), (2 ** 32 + 5, 2 ** 32 - 1), (2 ** 32 - 100, 2 ** 32 + 3), (2 ** 32 + 5, 0)]
KEY_IDS = ["off0-null", "off0-ctr0", "straddle-ctr7", "hi-ctr2^32-1", "straddle-ctr2^32+3", "hi-ctr0"]


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context()


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda") if dtype is None else torch.tensor(a, dtype=dtype,
                                                                                                   device="cuda")


def _sync():
    import torch
    torch.cuda.synchronize()


def _counter(step):
    import torch
    return None if step is None else torch.tensor([step], dtype=torch.int64, device="cuda")


def _hyper(model, var=1.0):
    from sgmcmc_ssm_amd.ensemble import prior_hyper
    return prior_hyper(model, PRIORS[model].generate_default_prior(var=var, n=1, m=1))


def _chain_inputs(model, n=C, seed=1):
    """theta around the defaults with edge rows -- |A| on both sides of 0.9999, negative Cholesky factors -- and ghat
    mostly O(1), a few +-1e3, some zeros.  Returns the device theta [n, MAX_THETA] and outs [n, OUT_DOUBLES] as numpy."""
    from sgmcmc_ssm_amd import _capi
    rs = np.random.RandomState(seed)
    P = _capi.THETA_DIM[model]
    th = np.zeros((n, _capi.MAX_THETA))
    th[:, :P] = default_params(model).theta() * rs.uniform(0.8, 1.2, size=(n, P))
    if model == "lgssm":
        th[:, 1] = 1.0
    if model != "garch":
        edge = np.array([0.99995, 0.99991, 0.9999, 0.99989, 0.9998, 0.9995, 0.999, 1.5])
        k = min(n, 64)
        th[:k, 0] = np.resize(np.concatenate([edge, -edge]), k)
        th[k // 4: k // 2, P - 1] *= -1.0
        th[k // 2: 3 * k // 4, P - 2] *= -1.0
    else:
        th[: min(n, 32), 3] *= -1.0
    g = np.zeros((n, _capi.OUT_DOUBLES))
    g[:, :4] = rs.standard_normal((n, 4))
    big = rs.uniform(size=n) < 0.03
    g[big, :4] = rs.choice([-1e3, 1e3], size=(big.sum(), 4))
    g[rs.uniform(size=n) < 0.03, :4] = 0.0
    g[:, 4:] = rs.standard_normal((n, _capi.OUT_DOUBLES - 4))           # columns the updates must not read
    return th, g


def _assert_matches(exp, got, what, cols=None):
    bad = exp.mismatch(got, cols)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("{0}: {1} components off, first chain {2} slot {3}: kernel {4!r}, mirror {5!r}, tol {6:.3g}"
                             .format(what, int(bad.sum()), i, j, float(got[i, j]), float(exp.theta[i, j]),
                                     float(exp.tol[i, j])))


# ---- a. SGLD and SGHMC ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_sgld_update_matches_the_mirror(model, key):
    from sgmcmc_ssm_amd import _capi
    off, step = key
    th0, g = _chain_inputs(model)
    hy = _hyper(model)
    theta, outs, ctr = _dev(th0), _dev(g), _counter(step)
    _ctx().sgld_update_device(model, C, theta.data_ptr(), outs.data_ptr(), hy, EPS, TSCALE, SEED, off,
                              None if ctr is None else ctr.data_ptr())
    _sync()
    got = theta.cpu().numpy()
    exp = kd.sgld_expected(model, th0, g, hy, EPS, TSCALE, SEED, off, step)
    _assert_matches(exp, got, "sgld " + model)
    P = _capi.THETA_DIM[model]
    np.testing.assert_array_equal(got[:, P:], th0[:, P:])                 # slots past the model's are untouched
    if ctr is not None:
        assert int(ctr.item()) == step + 1
    assert exp.amb.sum() <= 8                                            # the ambiguity band is a few ulps wide
    if model != "garch":
        assert (np.abs(th0[:, 0] + 0.0) > 0.9999).any() and (np.abs(got[:, 0]) <= 0.9999 * (1 + 1e-15)).all()


@pytest.mark.parametrize("alpha", [0.1, 1.0])
@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_sghmc_three_steps_match_the_mirror(model, alpha):
    """Three SGHMC steps with the counter bump and the momentum carried, each against the mirror from the kernel's
    state before it; at alpha = 1 the first step is the SGLD step bit for bit (include/pfgrad.h)."""
    import torch
    from sgmcmc_ssm_amd import _capi
    th0, g = _chain_inputs(model, seed=2)
    hy = _hyper(model)
    off, step0 = 2 ** 32 - 100, 2 ** 32 - 2                 # the counter crosses 2^32 on the way
    theta, outs, ctr = _dev(th0), _dev(g), _counter(step0)
    mom = torch.zeros((C, _capi.MAX_THETA), dtype=torch.float64, device="cuda")
    P = _capi.THETA_DIM[model]
    for k in range(3):
        before, m_before = theta.cpu().numpy(), mom.cpu().numpy()
        _ctx().sghmc_update_device(model, C, theta.data_ptr(), mom.data_ptr(), outs.data_ptr(), hy, EPS, alpha, TSCALE,
                                   SEED, off, ctr.data_ptr())
        _sync()
        got, m_got = theta.cpu().numpy(), mom.cpu().numpy()
        exp = kd.sgld_expected(model, before, g, hy, EPS, TSCALE, SEED, off, step0 + k, momentum=m_before, alpha=alpha)
        _assert_matches(exp, got, "sghmc {0} step {1}".format(model, k))
        dm = np.abs(m_got[:, :P].astype(np.longdouble) - exp.momentum)
        assert np.all(dm <= exp.mom_tol), ("momentum", k, float(np.max(dm / exp.mom_tol)))
        assert int(ctr.item()) == step0 + k + 1
        if k == 0 and alpha == 1.0:
            sg, c2 = _dev(th0), _counter(step0)
            _ctx().sgld_update_device(model, C, sg.data_ptr(), outs.data_ptr(), hy, EPS, TSCALE, SEED, off, c2.data_ptr())
            _sync()
            np.testing.assert_array_equal(sg.cpu().numpy(), got)


# ---- b. SGRLD ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("n", [C, 1])
def test_sgrld_update_matches_the_mirror(n, key):
    off, step = key
    th0, g = _chain_inputs("lgssm", n=n, seed=3)
    if n == 1:
        th0[0, :4] = [0.99993, 1.0, -1.3, 0.7]
    hy = _hyper("lgssm")
    theta, outs, ctr = _dev(th0), _dev(g), _counter(step)
    _ctx().sgrld_update_device("lgssm", n, theta.data_ptr(), outs.data_ptr(), hy, EPS, TSCALE, SEED, off,
                               None if ctr is None else ctr.data_ptr())
    _sync()
    got = theta.cpu().numpy()
    exp = kd.sgrld_expected(th0, g, hy, EPS, TSCALE, SEED, off, step)
    _assert_matches(exp, got, "sgrld")
    np.testing.assert_array_equal(got[:, 4:], th0[:, 4:])
    if ctr is not None:
        assert int(ctr.item()) == step + 1


# ---- c. Gibbs ------------------------------------------------------------------------------------------------------
def _gibbs_stats(case, n=C, seed=4):
    rs = np.random.RandomState(seed)
    if case == "paths":
        out = np.zeros((n, 8))
        for c in range(n):
            T = int(rs.randint(2, 120))
            x = np.zeros(T)
            a, q = rs.uniform(-0.95, 0.95), rs.uniform(0.05, 2.0)
            for t in range(1, T):
                x[t] = a * x[t - 1] + np.sqrt(q) * rs.standard_normal()
            out[c] = rules.gibbs_stats(x, x + rs.standard_normal(T) * rs.uniform(0.3, 2.0))
        return out
    if case == "short_small_df":
        return np.tile(rules.gibbs_stats([0.8], [1.3]), (n, 1))
    return np.zeros((n, 8))                                    # T = 0


def _gibbs_hyper(case):
    from sgmcmc_ssm_amd.ensemble import prior_hyper
    prior = PRIORS["lgssm"].generate_default_prior(var=100.0, n=1, m=1)
    if case == "short_small_df":
        prior.hyperparams["df_Qinv"] = 1.2      # shape 0.6 for Qinv, 0.7 for Rinv: the boosted branch
        prior.hyperparams["df_Rinv"] = 0.4
    return prior_hyper("lgssm", prior)


@pytest.mark.parametrize("key", KEYS[1:4], ids=KEY_IDS[1:4])
@pytest.mark.parametrize("case", ["paths", "short_small_df"])
def test_gibbs_update_matches_the_mirror(case, key):
    off, step = key
    stats = _gibbs_stats(case)
    hy = _gibbs_hyper(case)
    from sgmcmc_ssm_amd import _capi
    th0 = np.tile([0.5, 1.0, 1.0, 1.0], (C, 1))
    assert _capi.MAX_THETA == 4 and _capi.OUT_DOUBLES == 8
    theta, outs, ctr = _dev(th0), _dev(stats), _counter(step)
    _ctx().gibbs_update_device("lgssm", C, theta.data_ptr(), outs.data_ptr(), hy, SEED, off,
                               None if ctr is None else ctr.data_ptr())
    _sync()
    got = theta.cpu().numpy()
    exp, tie, shq, shr = kd.gibbs_expected(stats, hy, SEED, off, step)
    assert tie.sum() <= 2, int(tie.sum())
    keep = ~tie
    bad = exp.mismatch(got)[keep]
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:3])
    assert np.all(got[:, 1] == 1.0) and np.all(np.isfinite(got[:, :4]))
    if case == "short_small_df":
        assert np.all(shq < 1) and np.all(shr < 1)
    else:
        assert np.all(shq > 1)


@pytest.mark.parametrize("df_Qinv", [0.6, 1.0, 1.5, 3.0])
def test_gibbs_update_without_transitions(df_Qinv):
    """T = 0 statistics: Qinv's degrees of freedom drop to df0 - 1; A and LQinv are NaN exactly where the mirror's shape
    is <= 0, and otherwise equal the mirror."""
    stats = _gibbs_stats("empty", n=256)
    hy = _gibbs_hyper("long")
    hy.df_Qinv = df_Qinv
    theta, outs = _dev(np.zeros((256, 4))), _dev(stats)
    _ctx().gibbs_update_device("lgssm", 256, theta.data_ptr(), outs.data_ptr(), hy, SEED, 7, None)
    _sync()
    got = theta.cpu().numpy()
    exp, tie, shq, _ = kd.gibbs_expected(stats, hy, SEED, 7, None)
    nan_expected = bool(shq[0] <= 0)
    assert np.all(np.isnan(got[:, 0]) == nan_expected) and np.all(np.isnan(got[:, 2]) == nan_expected)
    assert np.all(np.isfinite(got[:, 3]))
    assert not exp.mismatch(got)[~tie].any()


# ---- d. window samplers -------------------------------------------------------------------------------------------
def _probs(n):
    import torch
    from sgmcmc_ssm_amd import _capi
    return torch.zeros(n * _capi.DEV_PROBLEM_DTYPE.itemsize, dtype=torch.uint8, device="cuda")


ONE = [  # T, S, buffer, strict
    (1000, 16, 4, False), (1000, 16, 4, True), (1000, 7, 0, True), (1000, 1000, 0, False), (1000, 999, 3, True),
    (997, 10, 5000, False), (1000, 16, 2 ** 31 - 1, False), (1000, 16, 2 ** 31 - 1, True),
]


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("T,S,buffer,strict", ONE)
def test_one_window_sampler_matches_the_mirror(T, S, buffer, strict, key):
    """sample_windows_kernel, bitwise: y offset, T, t1, tL and weights offset of every chain (buffer = 2^31 - 1 needs
    the bounds in 64 bits)."""
    import torch
    off, step = key
    y = torch.zeros(T, dtype=torch.float64, device="cuda")
    w = torch.zeros(T * S, dtype=torch.float64, device="cuda")
    desc, ctr = _probs(C), _counter(step)
    _ctx().sample_windows_device(C, desc.data_ptr(), y.data_ptr(), w.data_ptr(), T, S, buffer, strict, SEED, off,
                                 None if ctr is None else ctr.data_ptr())
    _sync()
    d, yoff, woff = device_windows.decode(desc, y.data_ptr(), w.data_ptr())
    ref = kd.windows_one(C, T, S, buffer, strict, SEED, off, step)
    for name, got in (("yoff", yoff), ("T", d["T"]), ("t1", d["t1"]), ("tL", d["tL"]), ("woff", woff)):
        np.testing.assert_array_equal(got, ref[name], err_msg=name)
    if ctr is not None:
        assert int(ctr.item()) == step                      # the sampler reads the counter, the update bumps it


MULTI = [  # lengths, S, buffer, strict, K, M, chains
    ([50, 8, 120, 33, 16, 200, 5], 16, 3, False, -1, 3, 512),
    ([50, 8, 120, 33, 16, 200, 5], 16, 0, True, 1, 5, 1024),
    ([50, 8, 120, 33, 16, 200, 5], 33, 2 ** 31 - 1, False, 7, 2, 512),
    ([50, 8, 120, 33, 16, 200, 5], 20, 500, True, 3, 1, 2048),
    (list(np.random.RandomState(9).randint(10, 300, size=40)), 24, 6, False, -1, 100, 8),
    (list(np.random.RandomState(9).randint(10, 300, size=40)), 24, 2 ** 31 - 1, True, 12, 250, 4),
]


@pytest.mark.parametrize("key", KEYS[1:5], ids=KEY_IDS[1:5])
@pytest.mark.parametrize("case", range(len(MULTI)))
def test_multi_window_sampler_matches_the_mirror(case, key):
    """sample_windows_multi_kernel, bitwise: every window's y offset, T, t1, tL, weights offset and sequence length,
    for all-sequence (K = -1), one-sequence and every-sequence draws, several windows per sequence, W in the thousands."""
    import torch
    lengths, S, buffer, strict, K, M, nc = MULTI[case]
    off, step = key
    bounds = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n_seq = len(lengths)
    woffs = np.concatenate([[0], np.cumsum(np.asarray(lengths) * S)])[:-1].astype(np.int64)
    W = (n_seq if K == -1 else K) * M
    y = torch.zeros(int(bounds[-1]), dtype=torch.float64, device="cuda")
    wt = torch.zeros(int(np.sum(np.asarray(lengths) * S)), dtype=torch.float64, device="cuda")
    b_dev, w_dev = _dev(bounds), _dev(woffs)
    desc = _probs(nc * W)
    seq_len = torch.zeros(nc * W, dtype=torch.int32, device="cuda")
    ctr = _counter(step)
    _ctx().sample_windows_multi_device(nc, n_seq, b_dev.data_ptr(), w_dev.data_ptr(), K, M, desc.data_ptr(),
                                       seq_len.data_ptr(), y.data_ptr(), wt.data_ptr(), S, buffer, strict, SEED, off,
                                       ctr.data_ptr())
    _sync()
    d, yoff, woff = device_windows.decode(desc, y.data_ptr(), wt.data_ptr())
    ref, _ = kd.windows_multi(nc, bounds, K, M, S, buffer, strict, SEED, off, step, weight_offsets=woffs)
    for name, got in (("yoff", yoff), ("T", d["T"]), ("t1", d["t1"]), ("tL", d["tL"]), ("woff", woff),
                      ("seq_len", seq_len.cpu().numpy())):
        np.testing.assert_array_equal(got, ref[name], err_msg=name)


# ---- e. FFBS with the device generator ------------------------------------------------------------------------------
FM = dict(log_constant=0.0, mean_precision=np.zeros(1), precision=np.eye(1) / 10)
# The normals the kernel used, recovered from its traced paths, against the mirror's: what is left is the error of the
# f32 transcendental units (v_log_f32, v_sqrt_f32, v_sin_f32 / v_cos_f32) in normal_pair_f32, which nothing else in
# this repository bounds.  Measured on an MI355X over the four cases below (9.6e4 normals): max |z_kernel - z_mirror|
# = 5.1e-7 (per case 3.8e-7, 4.6e-7, 5.1e-7, 3.5e-7).  The tolerance is about 4x that; a keying error gives O(1).
Z_TOL = 2e-6
FFBS = [  # T, N, t1, tL, stat, stream, step
    (150, 1, 0, 150, "score", 0, 0), (200, 64, 40, 150, "score", 3, 2 ** 32 + 5), (90, 300, 10, 80, "score", 2 ** 32 + 1, 7),
    (120, 1, 0, 120, "gibbs", 11, 2 ** 32 - 1),
]


def test_ffbs_device_generator_matches_the_mirror():
    """FFBS windows with rng='device' (N = 1, 64 and 300 paths -- lanes loop past the workgroup --, t1 > 0, and the
    Gibbs statistic): the traced paths are the mirror's backward recursion driven by the mirrored jsf32 words, and the
    score / statistic is the complete-data one of those paths.  Tolerance: Z_TOL, the measured f32-unit Box-Muller
    error (max |z_kernel - z_mirror| = 5.1e-7 on an MI355X) times about 4."""
    from sgmcmc_ssm_amd.models.lgssm import LGSSMHelper, LGSSMParameters
    helper = LGSSMHelper(n=1, m=1)
    rs = np.random.RandomState(21)
    theta = [0.8, 1.0, 1.5, 1.2]
    p = LGSSMParameters(A=np.eye(1) * theta[0], C=np.eye(1) * theta[1], LQinv=np.eye(1) * theta[2],
                        LRinv=np.eye(1) * theta[3])
    qs, ys = [], []
    for T, N, t1, tL, stat, stream, step in FFBS:
        y = rs.standard_normal(T) * 1.5
        w = rs.uniform(0.5, 2.0, size=tL - t1) if stat == "score" and t1 > 0 else None
        qs.append(helper.ffbs_problem(y, p, N, t1, tL, weights=w, forward_message=FM, stat=stat, rng="device",
                                      seed=SEED, stream=stream, step=step))
        ys.append(y)
    outs = _ctx().run_batch(qs, want_trace=True)
    zerr = []
    for (T, N, t1, tL, stat, stream, step), q, y, o in zip(FFBS, qs, ys, outs):
        z = kd.ffbs_normals(SEED, stream, step, N, T)
        paths = np.asarray(o["paths"]).reshape(T, N)
        # the normals the kernel used, recovered from its paths through the same backward recursion
        msgs = ffbs_model.forward_messages(theta, y, q["prior_mean"], q["prior_var"])
        AtQinv = theta[0] * theta[2] ** 2
        zk = np.zeros((T, N))
        m, P = msgs[-1]
        zk[T - 1] = (paths[T - 1] - m / P) / np.sqrt(1.0 / P)
        for t in range(T - 2, -1, -1):
            m, P = msgs[t]
            c = 1.0 / (P + AtQinv * theta[0])
            zk[t] = (paths[t] - c * (m + AtQinv * paths[t + 1])) / np.sqrt(c)
        zm = z.reshape(T, N)[::-1].astype(float)            # z[k N + s]: time T - 1 - k
        zerr.append(float(np.max(np.abs(zk - zm))))
        mirror = np.array(ffbs_model.sample_paths(theta, y, z.astype(float), N, q["prior_mean"], q["prior_var"]))
        assert np.max(np.abs(paths - mirror)) <= 20 * Z_TOL * max(1.0, np.max(np.abs(mirror))), (T, N, stat)
        g = np.asarray(o["mean_stat"])
        if stat == "gibbs":
            want = rules.gibbs_stats(paths[:, 0], y)
            np.testing.assert_allclose(g[:7], want[:7], rtol=1e-12, atol=1e-12)
        else:
            want = ffbs_model.complete_score(theta, y, paths[t1:tL], t1, tL, q["weights"],
                                             paths[t1 - 1] if t1 > 0 else None)
            scale = max(1.0, np.max(np.abs(want)))
            np.testing.assert_allclose(g[:4], want, rtol=0, atol=1e-12 * (tL - t1) * scale)
            np.testing.assert_array_equal(g[4:8], 0.0)
    print("max |z_kernel - z_mirror| per case:", zerr)
    assert max(zerr) <= Z_TOL, zerr
