"""Writes tests/golden/n2_oracle_rng.npz: 64 runs of the CPU oracle's Poyiadjis O(N^2) smoother (oracle/pf_oracle.py,
pf_window_rng(pf='poyiadjis_N2')) per model on one series -- N = 100, T = 30, RandomState(1) -- the reference sample the
device-generator test of n2_64x2 compares with (tests/test_gpu_n2_one_wave.py).  Each run costs 0.15 s on a CPU; the
fixture keeps the 20 s out of the GPU suite, and tests/test_n2_oracle_fixture_host.py recomputes its first rows.

    python tests/golden/make_n2_oracle_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd")]

from oracle import pf_oracle as po                      # noqa: E402
from test_host_logic import default_params, GEN         # noqa: E402

N, T, RUNS, SERIES_SEED, ORACLE_SEED = 100, 30, 64, 11, 1


def case(model):
    """(theta, y, kernel, prior_mean, prior_var) of the model's window."""
    p = default_params(model)
    np.random.seed(SERIES_SEED)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    kernel = "prior" if model == "svm" else "optimal"
    pv = 10.0 if model != "garch" else float(np.asarray(po.garch_prior_x(p.theta())[1]).reshape(-1)[0])
    return p.theta(), y, kernel, 0.0, pv


def oracle_runs(model, runs):
    theta, y, kernel, pm, pv = case(model)
    rs = np.random.RandomState(ORACLE_SEED)
    rows = []
    for _ in range(runs):
        r = po.pf_window_rng(model, theta, y, N, rng=rs, kernel=kernel, pf="poyiadjis_N2", stat="score",
                             prior_mean=pm, prior_var=pv)
        rows.append(np.append(r["mean_statistic"], r["loglikelihood_estimate"]))
    return np.array(rows)


if __name__ == "__main__":
    arrays, meta = {}, []
    for model in ("svm", "garch"):
        theta, y, kernel, pm, pv = case(model)
        arrays[model + "/theta"], arrays[model + "/y"] = theta, y
        arrays[model + "/runs"] = oracle_runs(model, RUNS)
        meta.append(dict(key=model, model=model, kernel=kernel, pf="poyiadjis_N2", stat="score", N=N, T=T, runs=RUNS,
                         prior_mean=pm, prior_var=pv, oracle_seed=ORACLE_SEED))
    np.savez_compressed(os.path.join(HERE, "n2_oracle_rng.npz"), meta=np.array(json.dumps(meta)), **arrays)
    print("wrote n2_oracle_rng.npz", {k: v.shape for k, v in arrays.items()})
