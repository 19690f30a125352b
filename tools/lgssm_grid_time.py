"""Time the four rows of the reference's LGSSM experiment (lgssm/demo_setup.py: T = 1000, A = 0.9, Q = 0.1, R = 1) as
resident 12288-chain ensembles with graph replay, next to one drop-in LGSSMSampler chain per row:

    KF          kind='marginal'                      SGRLD, S = 40, B = -1, eps = 0.1
    MC_100      kind='complete', num_samples = 100   SGRLD
    NEMETH_100  kind='pf', pf='nemeth', N = 100      SGRLD
    Gibbs       one FFBS path, then a conjugate draw  Gibbs

    python tools/lgssm_grid_time.py --out DIR [--chains 12288] [--steps 40] [--row-timeout 600]

Every row runs in a fresh child process under `timeout -k 10 <row-timeout>` (the parent never opens the GPU); the
first child that fails ends the run.  Writes DIR/lgssm_grid_time.json: per row the ensemble's chain-steps/s and ms per
step and the drop-in's ms per step."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"))

ROWS = {
    "KF": dict(sampler="sgrld", kind="marginal"),
    "MC_100": dict(sampler="sgrld", kind="complete", num_samples=100),
    "NEMETH_100": dict(sampler="sgrld", kind="pf", pf="nemeth", N=100),
    "Gibbs": dict(sampler="gibbs"),
}
DROP_IN = {
    "KF": ("SGRLD", dict(kind="marginal")),
    "MC_100": ("SGRLD", dict(kind="complete", num_samples=100)),
    "NEMETH_100": ("SGRLD", dict(kind="pf", pf_kwargs=dict(pf="nemeth", N=100))),
    "Gibbs": ("Gibbs", {}),
}


def _series():
    import numpy as np
    from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, generate_lgssm_data
    np.random.seed(12345)
    p = LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1), Q=np.eye(1) * 0.1, R=np.eye(1))
    return generate_lgssm_data(T=1000, parameters=p)["observations"], p


def run_row(name, chains, steps, drop_steps):
    import numpy as np
    import torch
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    from sgmcmc_ssm_amd.models.lgssm import LGSSMPrior, LGSSMSampler
    y, p = _series()
    prior = LGSSMPrior.generate_default_prior(var=100.0, n=1, m=1)
    fm = dict(log_constant=0.0, mean_precision=np.zeros(1), precision=np.eye(1) / 10)
    kw = dict(ROWS[name])
    if kw["sampler"] == "sgrld":
        kw.update(epsilon=0.1, subsequence_length=40, buffer_length=-1, window_sampling="device")
    ens = ChainEnsemble("lgssm", y[:, 0], p, num_chains=chains, prior=prior, seed=1, forward_message=fm, **kw)
    K = 10
    ens.run(K, thin=K, graph_steps=K)              # capture + one replay: code objects loaded, caches warm
    torch.cuda.synchronize()
    reps = max(1, steps // K)
    t0 = time.perf_counter()
    ens.run(reps * K, thin=reps * K, graph_steps=K)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    ok = bool(np.all(np.isfinite(ens.theta())))
    # one drop-in chain on the host loop
    it, dkw = DROP_IN[name]
    if it == "SGRLD":
        dkw = dict(dkw, epsilon=0.1, subsequence_length=40, buffer_length=-1)
    s = LGSSMSampler(n=1, m=1, observations=y, prior=prior, parameters=p.copy())
    np.random.seed(3)
    s.fit(it, 3, **dkw)
    t1 = time.perf_counter()
    s.fit(it, drop_steps, **dkw)
    dsec = time.perf_counter() - t1
    return dict(row=name, chains=chains, steps=reps * K, graph_steps=K, finite=ok,
                ensemble_ms_per_step=1e3 * sec / (reps * K),
                ensemble_chain_steps_per_s=chains * reps * K / sec,
                dropin_steps=drop_steps, dropin_ms_per_step=1e3 * dsec / drop_steps,
                dropin_chain_steps_per_s=drop_steps / dsec, variant=ens.ctx.last_variant())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--chains", type=int, default=12288)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--dropin-steps", type=int, default=100)
    ap.add_argument("--row-timeout", type=int, default=600)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help=argparse.SUPPRESS)           # child: run this row, print its JSON
    a = ap.parse_args()
    if a.row:
        print(json.dumps(run_row(a.row, a.chains, a.steps, a.dropin_steps)), flush=True)
        return 0
    os.makedirs(a.out, exist_ok=True)
    results = []
    for name in a.rows.split(","):
        cmd = ["timeout", "-k", "10", str(a.row_timeout), sys.executable, os.path.abspath(__file__), "--out", a.out,
               "--row", name, "--chains", str(a.chains), "--steps", str(a.steps), "--dropin-steps", str(a.dropin_steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            results.append(dict(row=name, failed=r.returncode))
            print("row {0}: exit {1}; stopping".format(name, r.returncode), flush=True)
            break
        res = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(res)
        print(json.dumps(res), flush=True)
    with open(os.path.join(a.out, "lgssm_grid_time.json"), "w") as f:
        json.dump(results, f, indent=1)
    return 0 if all("failed" not in r for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
