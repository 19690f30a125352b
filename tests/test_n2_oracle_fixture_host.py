"""CPU: tests/golden/n2_oracle_rng.npz is what the oracle computes -- the first runs of each model's sample of the
Poyiadjis O(N^2) smoother, recomputed with oracle/pf_oracle.py from the stored series and parameters."""
import os
import sys

import numpy as np

from conftest import Golden
from oracle import pf_oracle as po

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_n2_oracle_golden as maker  # noqa: E402


def test_stored_runs_are_the_oracles():
    g = Golden("n2_oracle_rng.npz")
    assert [m["model"] for m in g.meta] == ["svm", "garch"]
    for m in g.meta:
        model = m["model"]
        theta, y, kernel, pm, pv = maker.case(model)
        np.testing.assert_array_equal(theta, g.get(model, "theta"))
        np.testing.assert_array_equal(y, g.get(model, "y"))
        assert (kernel, pm, pv, maker.N, maker.T, maker.RUNS) == (m["kernel"], m["prior_mean"], m["prior_var"], m["N"], m["T"], m["runs"])
        stored = g.get(model, "runs")
        assert stored.shape == (64, len(theta) + 1) and np.all(np.isfinite(stored))
        rs = np.random.RandomState(m["oracle_seed"])
        for row in stored[:2]:
            r = po.pf_window_rng(model, theta, y, m["N"], rng=rs, kernel=kernel, pf="poyiadjis_N2", stat="score",
                                 prior_mean=pm, prior_var=pv)
            np.testing.assert_allclose(np.append(r["mean_statistic"], r["loglikelihood_estimate"]), row, rtol=1e-12, atol=1e-12)
