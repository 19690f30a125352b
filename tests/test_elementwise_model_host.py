"""CPU: the trace-driven longdouble reference of the elementwise pass (tests/helpers/elementwise_model.py) equals
the oracle's elementwise run when it is fed the oracle's own saved particles, log-weights and ancestors -- the
tie between the reference (oracle, bit-exact to it: test_oracle_elementwise_matches_reference) and what
tests/test_gpu_elementwise_shapes.py compares the kernels with at shapes the oracle is too slow for."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_host_logic import default_params, GEN

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import elementwise_model as em      # noqa: E402

_MK = [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal")]
_CASES = [mk + (pf, lam, N, T, t1, tL)
          for mk in _MK
          for pf, lam, N, T, t1, tL in (("nemeth", 0.9, 64, 12, 2, 10), ("poyiadjis_N", None, 51, 11, 0, 11),
                                        ("poyiadjis_N2", None, 33, 9, 1, 8))] + \
         [("garch", "optimal", "poyiadjis_N", None, 37, 93, 2, 92)]        # wide: L = 90


@pytest.mark.parametrize("model,kernel,pf,lam,N,T,t1,tL", _CASES)
def test_helper_equals_oracle_on_its_own_trace(model, kernel, pf, lam, N, T, t1, tL):
    rs = np.random.RandomState(N + T)
    p = default_params(model)
    np.random.seed(6)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    w = rs.uniform(1.0, 3.0, size=tL - t1)
    z0, u, z = po.draw_streams(rs, N, T)
    ref = po.pf_window(model, p.theta(), y, N, z0, u, z, kernel=kernel, pf=pf, lambduh=lam, stat="suff", t1=t1, tL=tL,
                       weights=w, prior_mean=0.0, prior_var=1.3, elementwise_statistic=True, save_all=True)
    tx, tlw, ta = ref["all_x_t"], ref["all_log_weights"], ref["all_ancestors"]
    assert tx.shape[:2] == (T + 1, N) and tlw.shape == (T + 1, N) and ta.shape == (T, N)
    if pf == "poyiadjis_N2":
        stats, mean = em.ew_reference_n2(model, p.theta(), tx, tlw, t1, tL, w, chunk=16)      # three chunks, one ragged
    else:
        stats, mean = em.ew_reference(model, tx, tlw, ta, t1, tL, w, 1.0 if lam is None else lam)
    assert stats.dtype == np.longdouble and stats.shape == (N, 3 * (tL - t1)) and mean.shape == (3 * (tL - t1),)
    assert np.all(ref["statistics"][:, 0::3] != 0.0)          # every block was written
    np.testing.assert_allclose(stats.astype(np.float64), ref["statistics"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(mean.astype(np.float64), ref["mean_statistic"], rtol=1e-12, atol=0)
    # the float64 evaluation the tolerance floor is measured with is the same function
    s64, m64 = (em.ew_reference_n2(model, p.theta(), tx, tlw, t1, tL, w, dtype=np.float64) if pf == "poyiadjis_N2"
                else em.ew_reference(model, tx, tlw, ta, t1, tL, w, 1.0 if lam is None else lam, dtype=np.float64))
    assert s64.dtype == np.float64
    np.testing.assert_allclose(s64, ref["statistics"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(m64, ref["mean_statistic"], rtol=1e-11, atol=0)


def test_case_tables_reach_what_they_name():
    """The shape tables the GPU test walks: column widths on both sides of the 256-column block, all four N mod 4
    tails per model, and the O(N^2) sizes on both sides of each stride and of the LDS-resident kernel."""
    wd = sorted({3 * (c[5] - c[4]) for c in em.CASES_ON})
    assert wd == [255, 258, 513]
    for mk in _MK:
        assert {c[2] % 4 for c in em.CASES_ON if c[:2] == mk and c[2] < 100} == {0, 1, 2, 3}
        assert {c[6] for c in em.CASES_ON if c[:2] == mk} == {0.9, 1.0}
        assert {c[2] for c in em.CASES_N2 if c[:2] == mk} >= {257, 515, 1025}
    assert any(c[2] == 1100 and c[5] - c[4] == 86 for c in em.CASES_ON)
    assert any(c[2] == 4096 for c in em.CASES_N2) and any(3 * (c[5] - c[4]) == 270 for c in em.CASES_N2)
    assert any(c[4] > 0 and c[5] < c[3] for c in em.CASES_ON)
