"""CPU: tests/helpers/systematic_model.py on the oracle alone -- what tests/test_gpu_systematic.py then asks of the kernel.

Systematic resampling searches the CDF with (r + u0) / N, one u0 per step on the 32-bit grid (w + 0.5) / 2^32.  On
po.device_ancestors (the index-order fp64 CDF over 1024 slots) the helper's uniforms give sorted ancestors whose offspring
counts are floor(N p_i) or ceil(N p_i) for every parent; the uniforms stay below 1 and within one ulp of the IEEE
division; and the generator word comes back exactly from the recorded uniform of child 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import keyed_draws  # noqa: E402
import systematic_model  # noqa: E402

NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024)
SCALES = (0.1, 1.0, 5.0, 30.0)
DRAWS = 200


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("N", NS)
def test_helper_on_the_oracle(N):
    rs = np.random.RandomState(100 + N)
    r = np.arange(N)
    worst_ulp, worst_dist = 0.0, 0.0
    for scale in SCALES:
        logw = scale * rs.normal(size=N)
        words = rs.randint(0, 1 << 32, size=DRAWS, dtype=np.uint64).astype(np.int64)
        words[:2] = 0, (1 << 32) - 1                    # both ends of the grid
        u0s = (words + 0.5) / 4294967296.0
        assert np.all((u0s > 0.0) & (u0s < 1.0))
        ud = np.stack([systematic_model.systematic_uniforms(u0, N) for u0 in u0s])
        assert ud.shape == (DRAWS, N) and np.all(ud >= 0.0) and np.all(ud < 1.0)
        exact = (r[None, :] + u0s[:, None]) / N
        worst_ulp = max(worst_ulp, float(_ulps(ud, exact).max()))
        assert _ulps(ud, exact).max() <= 1.0
        for t in range(DRAWS):
            anc = systematic_model.device_ancestors(logw, ud[t])
            assert anc.shape == (N,) and anc.min() >= 0 and anc.max() < N
            assert np.all(np.diff(anc) >= 0)
            assert systematic_model.offspring_violations(anc, logw, 1e-9) == 0, (N, scale, t)
        u0_back, w_back, dist = systematic_model.offsets(ud)
        assert np.array_equal(w_back, words)
        worst_dist = max(worst_dist, float(dist.max()))
        assert dist.max() < 1e-3
        np.testing.assert_allclose(u0_back, u0s, rtol=0, atol=2.0 ** -40)
    print("N", N, "worst ulp", worst_ulp, "worst distance from an integer", worst_dist)


def test_offspring_violations_sees_a_miscount():
    """N p_i = 1/2 and 3/2 in turn, so the brackets are [0, 1] and [1, 2] (an integer N p_i would have delta open its
    bracket by one on either side): one child moved between two parents of the first kind that had one child each leaves
    one of them with two, a violation; the other, with none, stays inside its bracket."""
    N = 64
    Np = np.where(np.arange(N) % 2 == 0, 0.5, 1.5)
    logw = np.log(Np)
    anc = systematic_model.device_ancestors(logw, systematic_model.systematic_uniforms(0.25, N))
    assert systematic_model.offspring_violations(anc, logw, 1e-9) == 0
    n = np.bincount(anc, minlength=N)
    assert np.all(n[1::2] >= 1) and n.sum() == N
    lone = np.flatnonzero((Np == 0.5) & (n == 1))
    assert lone.size >= 2
    anc[anc == lone[0]] = lone[1]
    assert systematic_model.offspring_violations(anc, logw, 1e-9) == 1
    # multinomial ancestors of uneven weights are no systematic draw
    rs = np.random.RandomState(3)
    logw = rs.normal(size=N)
    p = np.exp(logw - logw.max())
    multinomial = np.sort(rs.choice(N, size=N, p=p / p.sum()))
    assert systematic_model.offspring_violations(multinomial, logw, 1e-9) > 0


def test_in_order_subsequence_on_lane_words():
    g = keyed_draws.LaneRng(20261019, 7, 0, [0])
    stream = [int(g.next()[0]) for _ in range(200)]
    assert len(set(stream)) == 200
    pick = [stream[i] for i in (0, 3, 10, 11, 150, 199)]
    assert systematic_model.in_order_subsequence(pick, stream)
    assert systematic_model.in_order_subsequence([], stream)
    assert systematic_model.in_order_subsequence(stream, stream)
    assert not systematic_model.in_order_subsequence(pick[::-1], stream)
    assert not systematic_model.in_order_subsequence([stream[5], stream[5]], stream)      # one occurrence serves one word
    assert not systematic_model.in_order_subsequence(pick, stream[:199])
    other = keyed_draws.LaneRng(20261019, 8, 0, [0])
    assert not systematic_model.in_order_subsequence([int(other.next()[0]) for _ in range(4)], stream)
    # numpy words as the GPU test passes them
    assert systematic_model.in_order_subsequence(np.array(pick, dtype=np.int64), np.array(stream, dtype=np.uint32))
