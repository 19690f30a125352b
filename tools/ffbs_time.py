"""Timings of kind='complete' (FFBS paths, PFG_SMOOTHER_KALMAN_FFBS) and Gibbs on the LGSSM experiment's MC_100 row
(T = 1000, A = .9, Q = .1, R = 1, S = 40, buffer = -1, eps = .1, num_samples = 100):
  * the drop-in sampler: sample_sgrld(kind='complete', num_samples=100) + project_parameters steps per second
    (host normals in the reference's order, one window per step);
  * the drop-in Gibbs step (sample_gibbs + project_parameters: one FFBS path of the whole series, conjugate draws);
  * ChainEnsemble(kind='complete', num_samples=100), device window sampling, SGLD, K = 16 steps per hipGraph replay:
    steps / s and chain-steps / s for C chains, and the kernel alone (torch events around launch_pf).
Kernel times for the record come from a separate profiler run of this script (--kernel-only):
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/ffbs_time.py --kernel-only
usage: python tools/ffbs_time.py [--kernel-only] [--chains 1024,12288] [--out FILE]"""
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
from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, LGSSMSampler, generate_lgssm_data  # noqa: E402


def mc_row(T=1000, seed=8181):
    p = LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1), Q=np.eye(1) * 0.1, R=np.eye(1))
    p.project_parameters()
    np.random.seed(seed)
    return p, generate_lgssm_data(T=T, parameters=p)["observations"]


def dropin(y, kw, steps, warmup=10):
    start = LGSSMParameters(A=np.eye(1) * 0.5, C=np.eye(1), Q=np.eye(1) * 0.5, R=np.eye(1) * 0.5)
    sampler = LGSSMSampler(n=1, m=1, observations=y, parameters=start)
    np.random.seed(1)
    sampler.fit(num_iters=warmup, **kw)
    t = time.perf_counter()
    sampler.fit(num_iters=steps, **kw)
    dt = time.perf_counter() - t
    return dict(steps=steps, seconds=dt, steps_per_s=steps / dt, ms_per_step=1e3 * dt / steps)


def ensemble(p, y, C, steps=160, K=16):
    ens = ChainEnsemble("lgssm", y, p, num_chains=C, kind="complete", num_samples=100, epsilon=0.1 / 1000,
                        subsequence_length=40, buffer_length=-1, window_sampling="device", seed=5)
    ens.run(K, thin=K, graph_steps=K)           # capture + first replay
    ens.synchronize()
    t = time.perf_counter()
    ens.run(steps, thin=steps, graph_steps=K)
    ens.synchronize()
    dt = time.perf_counter() - t
    st = torch.cuda.current_stream()
    ms = []
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        ens.launch_pf(st)
        b.record(st)
        ens.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(chains=C, steps=steps, graph_steps=K, seconds=dt, steps_per_s=steps / dt,
                chain_steps_per_s=steps * C / dt, launch_pf_ms_median=float(np.median(ms)),
                variant=ens.ctx.last_variant(), finite=bool(np.all(np.isfinite(ens.theta()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true", help="only the ensemble runs (for a profiler)")
    ap.add_argument("--chains", default="1024,12288")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p, y = mc_row()
    res = dict(workload="LGSSM MC_100 row: T=1000 A=.9 Q=.1 R=1 S=40 buffer=-1 num_samples=100")
    if not a.kernel_only:
        res["dropin_sgrld_mc100"] = dropin(y, dict(iter_type="SGRLD", epsilon=0.1, subsequence_length=40,
                                                   buffer_length=-1, kind="complete", num_samples=100), steps=200)
        res["dropin_gibbs"] = dropin(y, dict(iter_type="Gibbs"), steps=200)
    res["ensemble"] = [ensemble(p, y, int(C)) for C in a.chains.split(",")]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
