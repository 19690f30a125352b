"""Timings of the SVM and GARCH experiments' POYIADJIS_N2_100 row as ChainEnsemble(pf='poyiadjis_N2') runs: N = 100,
S = 40, buffer = -1, T = 1000, SGLD (eps 0.1 / 0.01 as the demos, divided by T as tools/kalman_time.py does),
12288 chains, device window sampling, K steps per hipGraph replay -- on n2_64x2 (the plan's choice) and on n2_256x1
(forced with PFGRAD_VARIANT=n2_256x1, the baseline).  Reports ms per step, steps / s, chain-steps / s and the smoother
kernel's time (torch events around launch_pf: median, min and max of 8, which is the run-to-run spread quoted with it).
The library is the one PFGRAD_LIB selects: a build with -DPFG_OPT_N2SKIP=0 (python -m sgmcmc_ssm_amd._build noskip
-DPFG_OPT_N2SKIP=0) prices the skipped sweeps.
usage: python tools/n2_ensemble_time.py [--chains 12288] [--steps 8] [--graph-steps 2] [--variants n2_64x2,n2_256x1] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sgmcmc_ssm_amd.ensemble import ChainEnsemble  # noqa: E402
from sgmcmc_ssm_amd.models.svm import SVMParameters, generate_svm_data  # noqa: E402
from sgmcmc_ssm_amd.models.garch import GARCHParameters, generate_garch_data  # noqa: E402

T = 1000


def row(model, seed=8080):
    """The demos' parameters (nonlinear_ssm_pf_experiment_scripts/{svm,garch}/demo_setup.py) and a T = 1000 series."""
    np.random.seed(seed)
    if model == "svm":
        p = SVMParameters(A=np.eye(1) * 0.95, Q=np.eye(1) * 0.5, R=np.eye(1) * 0.5)
        p.project_parameters()
        return p, generate_svm_data(T=T, parameters=p)["observations"], 0.1
    lm, lp, ll = GARCHParameters.convert_alpha_beta_gamma(0.1, 0.8, 0.05)
    p = GARCHParameters(log_mu=lm, logit_phi=lp, logit_lambduh=ll, LRinv=np.eye(1) * 0.3 ** -0.5)
    p.project_parameters()
    return p, generate_garch_data(T=T, parameters=p)["observations"], 0.01


def ensemble(model, variant, C, steps, K):
    if variant != "n2_64x2":                    # n2_64x2 is the plan's own choice for this row
        os.environ["PFGRAD_VARIANT"] = variant
    else:
        os.environ.pop("PFGRAD_VARIANT", None)
    try:
        p, y, eps = row(model)
        ens = ChainEnsemble(model, y, p, num_chains=C, N=100, pf="poyiadjis_N2", epsilon=eps / T,
                            subsequence_length=40, buffer_length=-1, window_sampling="device", seed=5)
        ens.run(K, thin=K, graph_steps=K)           # capture + first replay
        ens.synchronize()
        ran = ens.ctx.last_variant()
        t = time.perf_counter()
        ens.run(steps, thin=steps, graph_steps=K)
        ens.synchronize()
        dt = time.perf_counter() - t
        st = torch.cuda.current_stream()
        ms = []
        for _ in range(8):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            ens.launch_pf(st)
            b.record(st)
            ens.synchronize()
            ms.append(a.elapsed_time(b))
        assert ens.ctx.last_variant() == ran == variant, (ran, variant)
        step_ms = 1e3 * dt / steps
        pf_ms = float(np.median(ms))
        return dict(lib=os.path.basename(os.environ.get("PFGRAD_LIB", "libpfgrad.so")), model=model, variant=variant, chains=C,
                    steps=steps, graph_steps=K, ms_per_step=step_ms, steps_per_s=steps / dt, chain_steps_per_s=steps * C / dt,
                    launch_pf_ms_median=pf_ms, launch_pf_ms_min=float(np.min(ms)), launch_pf_ms_max=float(np.max(ms)),
                    pf_share=pf_ms / step_ms, finite=bool(np.all(np.isfinite(ens.theta()))))
    finally:
        os.environ.pop("PFGRAD_VARIANT", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=12288)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--graph-steps", type=int, default=2)
    ap.add_argument("--variants", default="n2_64x2,n2_256x1")
    ap.add_argument("--models", default="svm,garch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(workload="POYIADJIS_N2_100 row: N=100 S=40 buffer=-1 T=1000 SGLD, device windows, graph replay",
               runs=[ensemble(m, v, a.chains, a.steps, a.graph_steps)
                     for m in a.models.split(",") for v in a.variants.split(",")])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
