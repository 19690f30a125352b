"""CPU: the burn-in of the exactness test of sampler='pmala_sorted' (tests/test_gpu_pmala_sorted.py), and the margins of the
decisions of its step test, chosen without a GPU.

The chain is the host restatement (tests/helpers/sorted_score_model.py: pmala_model's proposal and decision around the sorted
filters with the score).  LGSSM, the series of the exactness tests (T observations from the default parameters,
np.random.seed(333)), every chain started at the default parameters, the prior with var = 100, x_{-1} ~ N(0, 10) -- the setting
of tools/pmala_burnin_cpu.py, whose Kalman arm is the reference the GPU test compares against.  Arms: correlation = rho and
sqmc, N particles, pf='nemeth' with lambduh.  Printed per arm and checkpoint: the mean over the chains of each free coordinate
(A, LQinv, LRinv), its standard error and variance, and the acceptance rate.  The burn-in of the test is at least four times
the step count of the first checkpoint from which both arms' means stay inside 2.5 standard errors of the reference means.

    python tools/pmala_sorted_burnin_cpu.py [--chains 256] [--steps 400] [--N 16] [--rho 0.99] [--lambduh 0.95]
    python tools/pmala_sorted_burnin_cpu.py --margins SEED      (the step test: smallest |log u - log alpha| per configuration)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"),
          os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import pmala_model  # noqa: E402
import sorted_score_model as ss  # noqa: E402
from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, LGSSMPrior, generate_lgssm_data  # noqa: E402

FREE = (0, 2, 3)


def run(model, prior, hy, th, y, N, pm, pv, scale, rho, lam, seed, off, steps, marks=(), name=""):
    """`steps` steps of the host chain from th [C, P]; returns (accepted [steps, C], margin [steps, C], amb [steps, C])."""
    ll, g, U, _ = ss.chain_init(model, th, y, N, pm, pv, seed, off, lam, rho is not None)
    acc, margin, amb = [], [], []
    for s in range(steps):
        m = ss.chain_step(model, prior, hy, th, ll, g, U, scale, rho, lam, y, N, pm, pv, seed, off, s)
        th, ll, g, U = m["theta"], m["ll"], m["grad"], m["U"]
        acc.append(m["accepted"]), margin.append(m["margin"]), amb.append(m["amb"])
        if s + 1 in marks:
            x = th[:, FREE]
            print("{0:<5} C {1:>4} step {2:>4}  mean {3}  se {4}  var {5}".format(
                name, len(th), s + 1, np.round(x.mean(0), 4), np.round(x.std(0, ddof=1) / np.sqrt(len(th)), 4),
                np.round(x.var(0, ddof=1), 4)), flush=True)
    return np.array(acc), np.array(margin), np.array(amb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--rho", type=float, default=0.99)
    ap.add_argument("--lambduh", type=float, default=0.95)
    ap.add_argument("--scale", type=float, nargs=4, default=[0.2, 1.0, 0.3, 0.3])
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--margins", type=lambda v: int(v, 0), default=None)
    args = ap.parse_args()
    if args.margins is not None:
        import test_gpu_pmala_sorted as t       # the step test's own configurations, series, priors and scales
        from sgmcmc_ssm_amd.ensemble import prior_hyper
        for model, which, N, lam in t.STEP_CASES:
            prior = t._prior(model)
            hy = prior_hyper(model, prior)
            th = np.tile(t.default_params(model).theta(), (t.STEP_C, 1))
            acc, margin, amb = run(model, prior, hy, th, t._series(model, t.STEP_T), N, 0.0, 10.0, t.SCALE[model],
                                   t.RHO if which == "cpm" else None, lam, args.margins, t.STEP_OFF, t.STEP_STEPS)
            print(model, which, "N", N, "lambduh", lam, "accepted", int(acc.sum()), "of", acc.size, "min margin",
                  float(margin.min()), "ambiguous proposals", int(amb.sum()))
        return
    p0 = LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1) * 1.0, Q=np.eye(1) * 0.7, R=np.eye(1) * 1.0)
    np.random.seed(333)
    y = generate_lgssm_data(T=args.T, parameters=p0)["observations"].reshape(-1)
    prior = LGSSMPrior.generate_default_prior(var=100.0, n=1, m=1)
    hy = dict(pmala_model.kd.rules.hyper_of(prior))
    marks = sorted({max(1, args.steps // d) for d in (16, 8, 4, 2, 1)} | {max(1, 3 * args.steps // 4)})
    print("# scale", args.scale, "T", args.T, "N", args.N, "steps", args.steps, "rho", args.rho, "lambduh", args.lambduh)
    for name, rho in (("cpm", args.rho), ("sqmc", None)):
        th0 = np.tile(p0.theta(), (args.chains, 1))
        acc, _, _ = run("lgssm", prior, hy, th0, y, args.N, 0.0, 10.0, args.scale, rho, args.lambduh, args.seed, 0, args.steps,
                        marks, name)
        print("{0:<5} acceptance {1:.3f}".format(name, acc.mean()), flush=True)


if __name__ == "__main__":
    main()
