"""CPU: the host mirror of the counter-keyed draws (tests/helpers/keyed_draws.py) that tests/test_gpu_keyed_draws.py
holds the kernels to.  Philox4x32-10 against Random123's known answers; the mirror's update formulas against the host
samplers' own step (the code the reference fixtures pin), with the mirrored normals and a fixed gradient injected;
the mirror's Gamma and sequence draws against their documented laws; its long-double transforms against mpmath."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import scipy.stats

from test_host_logic import PRIORS, SAMPLERS, from_theta

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import keyed_draws as kd  # noqa: E402
import lgssm_chain_rules as rules  # noqa: E402


# ---- Philox4x32-10 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = kd.philox4x32_10(ctr, key)
    assert tuple(int(v) for v in got) == want
    # vectorised: the same block in every lane of a broadcast batch
    many = kd.philox4x32_10((np.full(5, ctr[0], np.uint64),) + ctr[1:], key)
    assert all(np.all(m == w) for m, w in zip(many, want))


def test_umul64hi_and_uniform53_are_exact():
    rs = np.random.RandomState(3)
    bits = [int(v) * 2 + 1 for v in rs.randint(0, 2 ** 63, size=200, dtype=np.int64)] + [0, 2 ** 64 - 1]
    for rng in (1, 2, 7, 2 ** 31 - 1, 2 ** 32 - 1):
        got = kd.umul64hi(np.array(bits, dtype=object), rng)
        assert [int(v) for v in got] == [(b * rng) >> 64 for b in bits]
        assert np.all((got >= 0) & (got < rng))
    u = kd.uniform53(np.array([0, 0xFFFFFFFF], np.uint32), np.array([0, 0xFFFFFFFF], np.uint32))
    assert u[0] == np.longdouble(0.5) / np.longdouble(2.0 ** 53) and u[1] == 1 - u[0]


# ---- the update formulas against the host samplers' step -----------------------------------------------------------
def _inject(monkeypatch, sampler, model, ghat, z, T):
    """The host step with ghat as its log-likelihood gradient and the mirrored normals (times the requested scale) as
    its np.random.normal draws, in the order it asks for them."""
    import oracle.pf_oracle as po
    names = po.SCORE_NAMES[model]
    grad = {n: np.full(np.shape(sampler.parameters.var_dict[n]), float(ghat[j])) for j, n in enumerate(names)}
    monkeypatch.setattr(sampler, "_noisy_grad_loglikelihood", lambda **kw: {k: v.copy() for k, v in grad.items()})
    monkeypatch.setattr(sampler, "_get_T", lambda **kw: T)
    queue = [float(v) for v in z]

    def normal(loc=0.0, scale=1.0, size=None):
        return loc + np.full(size if size is not None else (), queue.pop(0)) * scale
    monkeypatch.setattr(np.random, "normal", normal)
    return queue


THETAS = {"svm": [[0.93, 1.3, 1.6], [-0.4, 0.7, 2.2]],
          "lgssm": [[0.81, 1.0, 1.2, 0.9], [-0.3, 1.0, 2.5, 1.7]],
          "garch": [[-2.1, 1.4, -0.8, 1.9], [-0.9, 2.6, 0.3, 1.1]]}


@pytest.mark.parametrize("model", ["svm", "lgssm", "garch"])
@pytest.mark.parametrize("row", [0, 1])
def test_sgld_reference_is_the_host_step(monkeypatch, model, row):
    """sampler.sample_sgld at one theta with a fixed gradient and the mirrored normals is the mirror's long-double
    update to about 1e-13 relative (no projection triggers at these theta)."""
    from sgmcmc_ssm_amd.ensemble import prior_hyper
    eps, T, seed, off, step = 0.02, 50.0, 0x1234ABCD9876, 2 ** 32 - 3, 2 ** 32 + 1
    theta = np.array([THETAS[model][row]])
    ghat = np.zeros((1, 8))
    ghat[0, :4] = [0.7, -1.3, 2.1, -0.4]
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    exp = kd.sgld_expected(model, theta, ghat, prior_hyper(model, prior), eps, T, seed, off, step)
    z = kd.chain_normals(1, seed, off, step)[0]
    sampler = SAMPLERS[model][0](n=1, m=1, observations=np.zeros((10, 1)), prior=prior,
                                 parameters=from_theta(model, theta[0]))
    left = _inject(monkeypatch, sampler, model, ghat[0], z, T)
    host = sampler.sample_sgld(eps).theta()
    assert len(left) == 4 - theta.shape[1]                  # one normal per variable, in the mirror's order
    cols = [0, 2, 3] if model == "lgssm" else list(range(theta.shape[1]))      # LGSSM's C is pinned by the kernel
    ref = exp.theta[0, cols].astype(float)
    np.testing.assert_allclose(host[cols], ref, rtol=1e-13, atol=0)
    assert not np.array_equal(host, theta[0])


@pytest.mark.parametrize("row", [0, 1])
def test_sgrld_reference_is_the_host_step(monkeypatch, row):
    from sgmcmc_ssm_amd.models.lgssm import LGSSMPreconditioner
    eps, T, seed, off, step = 0.02, 50.0, 99, 5, 7
    theta = np.array([THETAS["lgssm"][row]])
    ghat = np.zeros((1, 8))
    ghat[0, :4] = [-0.6, 1.1, 0.3, 2.4]
    prior = PRIORS["lgssm"].generate_default_prior(var=1.0, n=1, m=1)
    exp = kd.sgrld_expected(theta, ghat, rules.hyper_of(prior), eps, T, seed, off, step)
    z = kd.chain_normals(1, seed, off, step)[0]
    sampler = SAMPLERS["lgssm"][0](n=1, m=1, observations=np.zeros((10, 1)), prior=prior,
                                   parameters=from_theta("lgssm", theta[0]))
    left = _inject(monkeypatch, sampler, "lgssm", ghat[0], z, T)
    host = sampler.sample_sgrld(eps, preconditioner=LGSSMPreconditioner()).theta()
    assert left == []
    np.testing.assert_allclose(host[[0, 2, 3]], exp.theta[0, [0, 2, 3]].astype(float), rtol=1e-13, atol=0)


def test_sghmc_with_full_friction_is_sgld():
    """alpha = 1: (1 - 1) v + d = d, the SGLD step (include/pfgrad.h), whatever the momentum was."""
    from sgmcmc_ssm_amd.ensemble import prior_hyper
    prior = PRIORS["svm"].generate_default_prior(var=1.0, n=1, m=1)
    th = np.array(THETAS["svm"])
    g = np.ones((2, 8))
    a = kd.sgld_expected("svm", th, g, prior_hyper("svm", prior), 0.02, 50.0, 3, 0, 1)
    b = kd.sgld_expected("svm", th, g, prior_hyper("svm", prior), 0.02, 50.0, 3, 0, 1, momentum=np.full((2, 3), 5.0),
                         alpha=1.0)
    np.testing.assert_array_equal(a.theta, b.theta)


# ---- the mirror's own laws -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [0.3, 0.6, 1.0, 2.5, 100.0])
def test_gamma_mirror_is_gamma(shape):
    """20000 keyed Marsaglia-Tsang draws (boost below shape 1) pass KS against Gamma(shape, 1)."""
    keys = kd.ChainKeys(range(7, 20007), seed=0xC0FFEE, step=3)
    x, tie, _ = kd.gamma_draw(keys, 0, shape)
    assert np.all(np.isfinite(x)) and np.all(x > 0) and tie.sum() <= 2
    assert scipy.stats.kstest(x.astype(float), scipy.stats.gamma(shape).cdf).pvalue > 1e-4


def test_gamma_mirror_refuses_non_positive_shapes():
    keys = kd.ChainKeys(range(4), seed=1, step=0)
    x, _, _ = kd.gamma_draw(keys, 0, np.array([0.0, -0.5, np.inf, np.nan]))
    assert np.all(np.isnan(x))
    # T = 0 statistics: Qinv's degrees of freedom drop to df0 - 1, NaN exactly when that shape is <= 0
    hy = dict(df_Qinv=1.0, scale_Qinv=1.0, df_Rinv=3.0, scale_Rinv=1.0, mean_A=0.0, var_col_A=1.0, mean_C=1.0,
              var_col_C=1.0)
    exp, _, shq, shr = kd.gibbs_expected(np.zeros((3, 8)), hy, 5, 0, 0)
    assert np.all(shq == 0) and np.all(shr == 1.5)
    assert np.all(np.isnan(exp.theta[:, [0, 2]].astype(float))) and np.all(np.isfinite(exp.theta[:, 3].astype(float)))


def test_sequence_choice_mirror_has_the_law_of_choice_without_replacement():
    """The ordered K-tuples the multi-window walk draws are uniform over the n! / (n - K)! arrangements, the law of
    np.random.choice(n, K, replace=False); every chain's tuple is distinct and in range."""
    n, K, C = 5, 3, 24000
    bounds = np.concatenate([[0], np.cumsum([30, 40, 50, 60, 70])])
    rec, chosen = kd.windows_multi(C, bounds, K, 1, 8, 2, False, seed=0xABCDEF0123, chain_offset=2 ** 32 - 7, step=11)
    assert all(len(set(r)) == K for r in chosen.tolist()) and chosen.min() >= 0 and chosen.max() < n
    tuples = list(itertools.permutations(range(n), K))
    index = {t: i for i, t in enumerate(tuples)}
    counts = np.bincount([index[tuple(r)] for r in chosen.tolist()], minlength=len(tuples))
    assert scipy.stats.chisquare(counts).pvalue > 1e-4
    # the windows lie in their sequences, S long, buffered by 2
    seq = np.repeat(chosen.reshape(-1), 1)
    lo, Tk = bounds[seq], np.diff(bounds)[seq]
    assert np.all(rec["seq_len"] == Tk) and np.all(rec["tL"] - rec["t1"] == 8)
    start = rec["yoff"] - lo + rec["t1"]
    assert np.all((start >= 0) & (start <= Tk - 8)) and np.all(rec["t1"] == np.minimum(start, 2))


def test_one_window_mirror_is_uniform_and_in_range():
    rec = kd.windows_one(20000, 100, 10, 3, False, seed=7, chain_offset=2 ** 32 - 100, step=2 ** 32 + 3)
    start = rec["yoff"] + rec["t1"]
    assert np.all((start >= 0) & (start <= 90)) and np.all(rec["tL"] - rec["t1"] == 10)
    assert scipy.stats.chisquare(np.bincount(start, minlength=91)).pvalue > 1e-4
    strict = kd.windows_one(20000, 100, 10, 0, True, seed=7, chain_offset=0, step=None)
    assert np.all(strict["yoff"] % 10 == 0) and scipy.stats.chisquare(np.bincount(strict["yoff"] // 10)).pvalue > 1e-4


def test_lane_generator_normals_are_standard():
    z = kd.ffbs_normals(seed=12345, stream=3, step=2, N=512, T=64).astype(float)
    assert abs(z.mean()) < 5 / math.sqrt(z.size) and abs(z.std() - 1) < 0.02
    assert scipy.stats.kstest(z, "norm").pvalue > 1e-4


# ---- the long-double transforms against mpmath ----------------------------------------------------------------------
def test_long_double_transforms_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    words = [0, 1, 2, 3, 0x7FFFFFFF, 0x80000000, 0x40000000, 0xC0000000, 0xFFFFFFFE, 0xFFFFFFFF]
    rs = np.random.RandomState(5)
    a = np.array(words + list(rs.randint(0, 2 ** 32, size=300, dtype=np.uint64)), dtype=np.uint32)
    b = np.array(words[::-1] + list(rs.randint(0, 2 ** 32, size=300, dtype=np.uint64)), dtype=np.uint32)
    z0, z1 = kd.normal_pair(a, b)
    for i in range(len(a)):
        u1 = (mpmath.mpf(int(a[i])) + mpmath.mpf(0.5)) / 2 ** 32
        r = mpmath.sqrt(-2 * mpmath.log(u1))
        ang = mpmath.pi * mpmath.mpf(int(b[i])) / 2 ** 31
        for got, want in ((z0[i], r * mpmath.cos(ang)), (z1[i], r * mpmath.sin(ang))):
            assert abs(mpmath.mpf(float(got)) + mpmath.mpf(float(got - np.longdouble(float(got)))) - want) <= 1e-17 * r
    # the Gamma acceptance test's two sides: the long-double error is far below the tie margin
    keys = kd.ChainKeys(range(200), seed=77, step=0)
    r = keys.draw(0, 0)
    zz, _ = kd.normal_pair(r[0], r[1])
    u = kd.uniform53(r[2], r[3])
    for shape in (0.6 + 1.0, 2.5, 100.0):
        d = np.longdouble(shape) - np.longdouble(1) / 3
        c = 1 / np.sqrt(9 * d)
        t = 1 + c * zz
        ok = t > 0
        v = t ** 3
        rhs = 0.5 * zz * zz + d - d * v + d * np.log(np.where(ok, v, 1))
        lhs = np.log(u)
        for i in np.nonzero(ok)[0][:60]:
            mz = mpmath.mpf(float(zz[i])) + mpmath.mpf(float(zz[i] - np.longdouble(float(zz[i]))))
            md = mpmath.mpf(shape) - mpmath.mpf(1) / 3
            mv = (1 + mz / mpmath.sqrt(9 * md)) ** 3
            mrhs = mz * mz / 2 + md - md * mv + md * mpmath.log(mv)
            mu = (mpmath.mpf(int(r[2][i]) >> 5) * 2 ** 26 + (int(r[3][i]) >> 6) + mpmath.mpf(0.5)) / 2 ** 53
            scale = max(1.0, abs(float(mrhs)), abs(float(md * mv)))
            assert abs(_mp(mpmath, rhs[i]) - mrhs) <= 1e-15 * scale
            assert abs(_mp(mpmath, lhs[i]) - mpmath.log(mu)) <= 1e-17 * max(1.0, abs(float(mpmath.log(mu))))


def _mp(mpmath, x):
    """a long double as an mpf, exactly (two doubles)."""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - np.longdouble(hi)))
