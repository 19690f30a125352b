"""CPU: burn-in and proposal scale of the pMALA exactness test (tests/test_gpu_pmala.py), chosen without a GPU.

The update rule is the host restatement (tests/helpers/pmala_model.py); the log-likelihoods and scores are the Kalman model
(tests/helpers/kalman_model.py: exact, so that arm is plain MALA) and the CPU oracle's particle filter (oracle/pf_oracle.py,
N particles, multinomial resampling, the Poyiadjis O(N) score), both under the ensemble's forward message (mean 0, variance
10).  LGSSM, the series of the test (T observations from the default parameters, np.random.seed(333)), every chain started
at the default parameters, the prior with var = 100 -- the setting of tools/pmmh_burnin_cpu.py, whose Kalman arm is the
exact reference the GPU test compares against.  Printed per arm and checkpoint: the mean over the chains of each free
coordinate (A, LQinv, LRinv), its standard error and variance, and the acceptance rate.  The burn-in of the test is at
least four times the step count of the first checkpoint from which both arms' means stay inside their standard errors.

    python tools/pmala_burnin_cpu.py [--chains-pf 128] [--chains-kf 512] [--steps 200] [--scale 0.2 1 0.3 0.3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"),
          os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import kalman_model  # noqa: E402
import pmala_model  # noqa: E402
from oracle import pf_oracle  # noqa: E402
from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, LGSSMPrior, generate_lgssm_data  # noqa: E402

FREE = (0, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains-pf", type=int, default=128)
    ap.add_argument("--chains-kf", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--scale", type=float, nargs=4, default=[0.2, 1.0, 0.3, 0.3])
    ap.add_argument("--seed", type=int, default=2025)
    args = ap.parse_args()
    p0 = LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1) * 1.0, Q=np.eye(1) * 0.7, R=np.eye(1) * 1.0)
    np.random.seed(333)
    y = generate_lgssm_data(T=args.T, parameters=p0)["observations"].reshape(-1)
    prior = LGSSMPrior.generate_default_prior(var=100.0, n=1, m=1)
    hy = dict(pmala_model.kd.rules.hyper_of(prior))

    def kf(th, ctr):
        res = [kalman_model.kalman_window(r, y, 0, args.T, None, 0.0, 10.0) for r in th]
        return np.array([r[1] for r in res]), np.array([r[0] for r in res])

    def pf(th, ctr):
        res = [pf_oracle.pf_window_rng("lgssm", r, y, args.N, rng=np.random.RandomState([args.seed, ctr, c]), stat="score",
                                       prior_mean=0.0, prior_var=10.0) for c, r in enumerate(th)]
        return np.array([r["loglikelihood_estimate"] for r in res]), np.array([r["mean_statistic"] for r in res])

    marks = sorted({max(1, args.steps // d) for d in (16, 8, 4, 2, 1)} | {max(1, 3 * args.steps // 4)})
    print("# scale", args.scale, "T", args.T, "N", args.N, "steps", args.steps)
    for name, fn, C in (("kalman", kf, args.chains_kf), ("pf", pf, args.chains_pf)):
        if C <= 0:
            continue
        th0 = np.tile(p0.theta(), (C, 1))
        th, ll, g, nacc, trace = pmala_model.run_chains("lgssm", prior, hy, th0, args.scale, fn, args.seed, 0, args.steps)
        for m in marks:
            x = trace[m - 1][:, FREE]
            print("{0:<7} C {1:>4} step {2:>4}  mean {3}  se {4}  var {5}".format(
                name, C, m, np.round(x.mean(0), 4), np.round(x.std(0, ddof=1) / np.sqrt(C), 4), np.round(x.var(0, ddof=1), 4)),
                flush=True)
        print("{0:<7} acceptance {1:.3f}".format(name, nacc.mean() / args.steps), flush=True)


if __name__ == "__main__":
    main()
