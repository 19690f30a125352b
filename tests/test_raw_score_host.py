"""The raw-sum form of the SVM Poyiadjis O(N) score (PFG_OPT_RAWSCORE, csrc/pfg_reg_traits.hpp), restated in NumPy.

The kernel carries along the genealogy, instead of the score s[0..2] itself, the three sums
    r0 += (w y^2) e,   r1 += (w z) z,   r2 += (w z) xp          (e = exp(-x'), z = the proposal's normal, w = the window weight)
and Cw += w, and maps them where a statistic leaves the kernel:
    s0 = iLRinv Cw - LRinv r0,   s1 = iLQinv (Cw - r1),   s2 = (Qinv iLQinv) r2.
Here that recursion runs beside `oracle.pf_oracle.score_statistic` accumulated per step along the SAME ancestors: SVM,
N = 65, T = 24, a window t1 = 4, tL = 20 with non-unit weights, from zero statistics and from given ones (the
init-statistics conversion  r0 = -s0 / LRinv, r1 = -s1 / iLQinv, r2 = s2 / (Qinv iLQinv)  with Cw = 0, there and back).

Agreement: 1e-12 relative, element by element (no absolute floor)."""
import numpy as np
import pytest

from oracle import pf_oracle as po

N, T, T1, TL = 65, 24, 4, 20
THETAS = [np.array([0.95, 2.0 ** 0.5, 2.0 ** 0.5]), np.array([0.6, 2.5, 0.7])]


def raw_in(d, s):
    LRinv, LQinv, Qinv = d["LRinv"].item(), d["LQinv"].item(), d["Qinv"].item()
    iLQinv = 1.0 / LQinv
    return np.stack([-s[:, 0] / LRinv, -s[:, 1] / iLQinv, s[:, 2] / (Qinv * iLQinv)], axis=1)


def raw_out(d, Cw, r):
    LRinv, LQinv, Qinv = d["LRinv"].item(), d["LQinv"].item(), d["Qinv"].item()
    iLRinv, iLQinv = 1.0 / LRinv, 1.0 / LQinv
    return np.stack([iLRinv * Cw - LRinv * r[:, 0], iLQinv * (Cw - r[:, 1]), (Qinv * iLQinv) * r[:, 2]], axis=1)


def _run(theta, seed, init_stats):
    """-> [(per-step score, raw form mapped back)] for every t, and the two weighted means at the end."""
    rs = np.random.RandomState(seed)
    d = po.derived("svm", theta)
    y = rs.normal(size=T) * 0.8
    weights = rs.uniform(0.5, 2.0, size=TL - T1)
    x = po.sample_x0("svm", 0.0, 10.0, rs.normal(size=N).astype(np.float32).astype(np.float64))
    logw = np.zeros(N)
    st = np.zeros((N, 3)) if init_stats is None else init_stats.copy()
    r, Cw = (st.copy() if init_stats is None else raw_in(d, st)), 0.0
    steps = [(st, raw_out(d, Cw, r))]
    for t in range(T):
        anc = po.multinomial_ancestors(po.log_normalize(logw), rs.uniform(size=N))
        z = rs.normal(size=N).astype(np.float32).astype(np.float64)         # f32-born normals, as the device generator's
        yt = np.array([y[t]])
        xp = x[anc]
        xn = po.kernel_rv("svm", "prior", d, xp, yt, z)
        st, r = st[anc], r[anc]
        if T1 <= t < TL:
            w = float(weights[t - T1])
            st = st + w * po.score_statistic("svm", d, xp, xn, yt)
            e = np.exp(-xn[:, 0])
            zw = w * z
            r = r + np.stack([(w * yt[0] ** 2) * e, zw * z, zw * xp[:, 0]], axis=1)
            Cw += w
        x, logw = xn, po.kernel_reweight("svm", "prior", d, xp, xn, yt)
        steps.append((st, raw_out(d, Cw, r)))
    W = po.log_normalize(logw)
    mean_ref = np.sum(st.T * W, axis=1)
    mean_raw = raw_out(d, Cw, np.sum(r.T * W, axis=1)[None, :])[0]         # the affine map commutes with the weighted mean
    return steps, mean_ref, mean_raw, Cw


def _close(got, ref):
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("theta", THETAS, ids=["A0.95", "A0.6"])
@pytest.mark.parametrize("warm", [False, True], ids=["zero_stats", "init_stats"])
def test_raw_recursion_matches_per_step_score(theta, warm):
    init = np.random.RandomState(3).normal(scale=5.0, size=(N, 3)) if warm else None
    steps, mean_ref, mean_raw, Cw = _run(theta, 11, init)
    assert Cw > 0.0 and abs(Cw - (TL - T1)) > 0.5                        # non-unit weights really entered
    assert np.all(np.max(np.abs(np.array([s for s, _ in steps])), axis=(0, 1)) > 1.0)
    for ref, got in steps:
        _close(got, ref)
    if not warm:                                                          # before the window: nothing added, exactly zero
        assert all(np.all(got == 0.0) for _, got in steps[:T1 + 1])
    _close(mean_raw, mean_ref)


@pytest.mark.parametrize("theta", THETAS, ids=["A0.95", "A0.6"])
def test_init_statistics_conversion_there_and_back(theta):
    d = po.derived("svm", theta)
    s = np.random.RandomState(5).normal(scale=30.0, size=(N, 3))
    s[0] = 0.0                                                              # zero statistics stay zero
    back = raw_out(d, 0.0, raw_in(d, s))
    np.testing.assert_allclose(back, s, rtol=1e-12, atol=0.0)
    assert np.all(back[0] == 0.0)
    # and with a statistic added on top: Cw = w
    w = 1.7
    r = raw_in(d, s)
    r[:, 1] += w * 0.25
    np.testing.assert_allclose(raw_out(d, w, r)[:, 1], s[:, 1] + w * (1.0 / d["LQinv"].item()) * (1.0 - 0.25), rtol=1e-12, atol=0.0)
