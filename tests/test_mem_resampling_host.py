"""CPU: po.particle_order_ancestors -- the host restatement of pf_mem_kernel's device-generator resampling (CDF in particle
order, f64, searched with the child's own uniform) -- against the reference's np.random.choice semantics, and the counting
of tests/helpers/forced_window.ancestors_against_restatement that the GPU replays of paris_mem1024 / n2_mem1024 rely on.

The log-weights are the oracle's own (po.pf_window, SVM, save_all) at N = 1025 and 2049: one particle in the last chunk of
1024.  The uniforms are of the device's form, (word + 0.5) / 2^32."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_host_logic import default_params, GEN

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import forced_window  # noqa: E402

GAP_TOL = 1e-10


def _oracle_window(N, T=4):
    p = default_params("svm")
    np.random.seed(17)
    y = GEN["svm"](T=T, parameters=p)["observations"].reshape(-1)
    z0, u, z = po.draw_streams(np.random.RandomState(1000 + N), N, T)
    return po.pf_window("svm", p.theta(), y, N, z0, u, z, kernel="prior", pf="poyiadjis_N", prior_var=10.0, save_all=True)


def test_hand_made_cdf():
    """Weights 1 : 2 : 1 -> CDF 0.25, 0.75, 1: a uniform ON an entry goes to the next particle (entries <= u are counted),
    the count is clamped to N - 1, and the gap is the distance to the nearest entry on either side."""
    logw = np.log(np.array([1.0, 2.0, 1.0])) - 7.0
    u = np.array([0.1, 0.25, 0.5, 0.75, 0.875, 1.0])
    anc, gap = po.particle_order_ancestors(logw, u)
    assert anc.tolist() == [0, 1, 1, 2, 2, 2]
    np.testing.assert_allclose(gap, [0.15, 0.0, 0.25, 0.0, 0.125, 0.0], rtol=0, atol=1e-15)


@pytest.mark.parametrize("N", [1025, 2049])
def test_restatement_is_np_random_choice_on_the_same_uniforms(N):
    """Every step of the oracle's window: the restatement returns po.multinomial_ancestors of the normalised weights on the
    same uniforms, and RandomState(s).choice(N, size=N, p=w) on the uniforms RandomState(s) hands out.  No child is exempt
    at these inputs, so the agreement is exact."""
    ref = _oracle_window(N)
    rs = np.random.RandomState(5 * N)
    exempt = 0
    for t, logw in enumerate(ref["all_log_weights"]):
        w = po.log_normalize(logw)
        ud = (rs.randint(0, 2 ** 32, size=N, dtype=np.uint64).astype(np.float64) + 0.5) / 4294967296.0
        anc, gap = po.particle_order_ancestors(logw, ud)
        exempt += int(np.sum(gap < GAP_TOL))
        assert anc.min() >= 0 and anc.max() <= N - 1
        assert np.array_equal(anc, po.multinomial_ancestors(w, ud))
        un = np.random.RandomState(77 + t).random_sample(N)
        assert np.array_equal(po.particle_order_ancestors(logw, un)[0], np.random.RandomState(77 + t).choice(N, size=N, replace=True, p=w))
        assert np.all(gap >= 0.0) and np.all(gap < 1.0)
    assert exempt == 0
    assert t > 0 and len(np.unique(ref["all_log_weights"][t])) > N // 2         # the weights do vary


def test_counting_of_differing_children():
    """ancestors_against_restatement on the restatement's own ancestors: nothing wrong, nothing exempt.  A child moved by one
    particle counts as wrong unless its uniform sits on a CDF entry; moved by two it counts as wrong even there."""
    N = 1025
    ref = _oracle_window(N)
    all_logw = ref["all_log_weights"][:3]
    rs = np.random.RandomState(3)
    ud = (rs.randint(0, 2 ** 32, size=(3, N), dtype=np.uint64).astype(np.float64) + 0.5) / 4294967296.0
    # child 7 of step 1 searches with a CDF entry itself (an exact tie), child 8 with a uniform 1e-11 above one
    cs = np.cumsum(np.exp(all_logw[1] - np.max(all_logw[1])))
    cdf = cs * (1.0 / cs[-1])
    ud[1, 7], ud[1, 8] = cdf[300], cdf[500] + 1e-11
    anc = np.array([po.particle_order_ancestors(all_logw[t], ud[t])[0] for t in range(3)])
    assert anc[1, 7] == 301 and anc[1, 8] == 501
    assert forced_window.ancestors_against_restatement(all_logw, ud, anc, GAP_TOL) == (0, 2, 0)
    moved = anc.copy()
    moved[1, 7], moved[1, 8] = 300, 500                  # the other neighbour of an exempt child: allowed
    assert forced_window.ancestors_against_restatement(all_logw, ud, moved, GAP_TOL) == (0, 2, 2)
    moved[1, 8] = 499                                    # two away: wrong even where exempt
    assert forced_window.ancestors_against_restatement(all_logw, ud, moved, GAP_TOL) == (1, 2, 2)
    moved = anc.copy()
    moved[2, 11] = (moved[2, 11] + 1) % N                # an ordinary child on the wrong parent
    assert forced_window.ancestors_against_restatement(all_logw, ud, moved, GAP_TOL) == (1, 2, 1)
