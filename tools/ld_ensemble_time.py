"""Timings of the exchange-rate demos' LD row -- full-data Langevin dynamics,
    fit_timed(iter_type='SGLD', epsilon=0.1, subsequence_length=-1, num_sequences=-1, buffer_length=0,
              kind='pf', pf_kwargs=dict(pf='paris', N=...))
(demo/exchange_rate/exchange_rate_full_demo.py:108-113 with N = 1000; save_{svm,garch}_params.py:85-88 with N = 10000)
-- on the 49 EUR/USD segments of tests/golden/eurus.npz (5907 points), SVM and GARCH:

  ensemble  ChainEnsemble(num_sequences=-1, subsequence_length=-1, buffer_length=0, pf='paris'): W = 49 whole-segment
            windows per chain, one PaRIS launch of C * 49 windows + the reduction + the SGLD update per step, K steps per
            hipGraph replay, after a warm-up replay, synchronised; C in {1, 4, 16, 64}
  drop-in   Seq{SVM,GARCH}Sampler.sample_sgld(num_sequences=-1, pf='paris', rng='device'): one chain, the host loop
            (49 windows in one pfg_run_batch per step, the gradient combined on the host)

Both use max_accept_reject = 64 accept-reject rounds (the ensemble's default).  Reports chain-steps / s, ms per step,
the kernel variant the PaRIS launch ran (pfg_last_variant) and the scratch bytes per chain (49 windows x
pfg_scratch_bytes_smoother); a size whose scratch does not fit half of the free device memory is skipped and says so.
usage: python tools/ld_ensemble_time.py [--chains 1 4 16 64] [--N 1000 10000] [--models svm garch] [--out FILE]"""
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
from sgmcmc_ssm_amd.models.svm import SVMParameters, SeqSVMSampler  # noqa: E402
from sgmcmc_ssm_amd.models.garch import GARCHParameters, SeqGARCHSampler  # noqa: E402

EPS = 0.1
ROUNDS = 64


def segments():
    g = np.load(os.path.join(ROOT, "tests", "golden", "eurus.npz"))
    b = np.concatenate([[0], np.cumsum(g["segment_lengths"])])
    return [g["segments"][b[k]:b[k + 1]].astype(np.float64) for k in range(len(b) - 1)]


def params(model):
    """The demos' starting points (nonlinear_ssm_pf_experiment_scripts/{svm,garch}/demo_setup.py)."""
    if model == "svm":
        p = SVMParameters(A=np.eye(1) * 0.95, Q=np.eye(1) * 0.5, R=np.eye(1) * 0.5)
    else:
        lm, lp, ll = GARCHParameters.convert_alpha_beta_gamma(0.1, 0.8, 0.05)
        p = GARCHParameters(log_mu=lm, logit_phi=lp, logit_lambduh=ll, LRinv=np.eye(1) * 0.3 ** -0.5)
    p.project_parameters()
    return p


def time_ensemble(model, segs, N, C, steps, K):
    ens = ChainEnsemble(model, segs, params(model), num_chains=C, N=N, pf="paris", epsilon=EPS, subsequence_length=-1,
                        buffer_length=0, num_sequences=-1, max_accept_reject=ROUNDS, seed=11)
    ens.run(K, thin=K, graph_steps=K)           # capture + one replay (warm-up)
    ens.synchronize()
    t = time.perf_counter()
    ens.run(steps, thin=steps, graph_steps=K)
    ens.synchronize()
    dt = time.perf_counter() - t
    ok = bool(np.all(np.isfinite(ens.theta())))
    return dict(path="ensemble", model=model, N=N, chains=C, windows_per_chain=ens.W, steps=steps, graph_steps=K,
                ms_per_step=1e3 * dt / steps, chain_steps_per_s=C * steps / dt, variant=ens.ctx.last_variant(),
                scratch_bytes_per_chain=ens.W * ens.scratch_bytes_per_window, finite=ok)


def time_dropin(model, segs, N, steps):
    Sampler = SeqSVMSampler if model == "svm" else SeqGARCHSampler
    s = Sampler(n=1, m=1, observations=[x.reshape(-1, 1) for x in segs], parameters=params(model))
    kw = dict(epsilon=EPS, num_sequences=-1, subsequence_length=-1, buffer_length=0, kind="pf", pf="paris", N=N,
              rng="device", max_accept_reject=ROUNDS)
    np.random.seed(1)
    s.sample_sgld(**kw)                         # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        s.sample_sgld(**kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    from sgmcmc_ssm_amd import _capi
    return dict(path="drop-in", model=model, N=N, chains=1, windows_per_chain=len(segs), steps=steps,
                ms_per_step=1e3 * dt / steps, chain_steps_per_s=steps / dt, variant=_capi.default_context().last_variant(),
                finite=bool(np.all(np.isfinite(s.parameters.theta()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--N", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--models", nargs="+", default=["svm", "garch"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    segs = segments()
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
    for model in a.models:
        for N in a.N:
            steps, K = (4, 2) if N <= 1000 else (2, 2)
            emit(time_dropin(model, segs, N, steps))
            probe = ChainEnsemble(model, segs, params(model), num_chains=1, N=N, pf="paris", epsilon=EPS,
                                  subsequence_length=-1, buffer_length=0, num_sequences=-1)
            per_chain = probe.W * probe.scratch_bytes_per_window
            del probe
            torch.cuda.empty_cache()
            for C in a.chains:
                free, _ = torch.cuda.mem_get_info()
                if C * per_chain > free // 2:
                    emit(dict(path="ensemble", model=model, N=N, chains=C, skipped="scratch {0} B > half the free {1} B".format(
                        C * per_chain, free)))
                    continue
                emit(time_ensemble(model, segs, N, C, steps, K))
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
