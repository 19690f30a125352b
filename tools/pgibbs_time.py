"""Step time and movement of a particle Gibbs ensemble beside a PMMH ensemble of the same build and shape, and the posterior
means of 'pgibbs' beside 'gibbs' (LGSSM) and 'pmmh' (SVM) (needs the GPU).

Shape: the series of bench.py's c2 (SVM, T = 1000), N = 100 particles, 12288 chains, the whole series in every step.

  step time   two resident ensembles whose whole steps are timed alternately with HIP events (warm-up first; `reps` rounds):
                pmmh    propose + particle filter (stat 'none') + accept, at `--pmmh-scale`
                pgibbs  conditional SMC sweep with ancestor sampling + conjugate draw
              Reported per row: median, min, max and inter-quartile range of the step in ms, chain-steps per second.
  movement    after `--burn` steps, over `--steps` steps: E (theta_j(t + 1) - theta_j(t))^2 of (A, LQinv, LRinv) per step and
              per GPU-second; PMMH's acceptance rate, pgibbs's degenerate sweeps.
  means       (a measurement, not a test) the chain-and-time average of theta after a burn-in, with the standard error over
              the chains: LGSSM T = 20 'pgibbs' beside 'gibbs', SVM T = 100 'pgibbs' beside 'pmmh'.  They need not agree
              beyond O(1 / T): the conjugate draw leaves the theta-dependence of x_0's law out of the conditional, and with
              conditionals that are not those of one joint law the stationary law depends on the path kernel too.

There is no pass / fail ratio.

    python tools/pgibbs_time.py [--reps 9] [--out profiles/pgibbs_vs_pmmh.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from sgmcmc_ssm_amd import _capi  # noqa: E402
from sgmcmc_ssm_amd.ensemble import ChainEnsemble  # noqa: E402


def averaged(e, burn, steps, P, jacobian=False):
    """[C, P] time average of theta over `steps` steps after `burn`.  jacobian: the self-normalised average under the weights
    LQinv LRinv (SVM), which turn a density stated on the Cholesky factors without Jacobian terms into the one on (Qinv, Rinv)."""
    e.step(burn)
    acc = torch.zeros((e.C, P), dtype=torch.float64, device=e.device)
    wsum = torch.zeros((e.C, 1), dtype=torch.float64, device=e.device)
    for _ in range(steps):
        e.step(1)
        th = e.theta_dev[:, :P]
        w = (th[:, 1:2] * th[:, 2:3]) if jacobian else torch.ones_like(wsum)
        acc += th * w
        wsum += w
    e.synchronize()
    return (acc / wsum).cpu().numpy()


def means_row(name, avg):
    m, se = avg.mean(axis=0), avg.std(axis=0, ddof=1) / np.sqrt(len(avg))
    return "  {0:<22} ".format(name) + "  ".join("{0:>9.5f} +- {1:.5f}".format(a, b) for a, b in zip(m, se))


def posterior_means(args, lines, result):
    from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, generate_lgssm_data
    from sgmcmc_ssm_amd.models.svm import SVMParameters, generate_svm_data
    C = args.mean_chains
    lines.append("# posterior means (a measurement, not a test): time average over {0} steps after {1}, mean over {2} chains +- its "
                 "standard error; the samplers need not agree beyond O(1 / T) (x_0's term is left out of the conjugate draw)".format(
                     args.mean_steps, args.mean_burn, C))
    np.random.seed(3)
    p = LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1), Q=np.eye(1) * 0.1, R=np.eye(1))
    y = generate_lgssm_data(T=20, parameters=p)["observations"]
    lines.append("# LGSSM T = 20 (A, C, LQinv, LRinv)")
    for name, kw in (("gibbs (FFBS)", dict(sampler="gibbs")), ("pgibbs N = 16", dict(sampler="pgibbs", N=16)),
                     ("pgibbs N = 128", dict(sampler="pgibbs", N=128))):
        avg = averaged(ChainEnsemble("lgssm", y, p, num_chains=C, seed=11, **kw), args.mean_burn, args.mean_steps, 4)
        lines.append(means_row(name, avg))
        result["means_lgssm_" + name] = avg.mean(axis=0).tolist()
    np.random.seed(4)
    p = SVMParameters(A=np.eye(1) * 0.95, Q=np.eye(1) * 0.5, R=np.eye(1) * 0.5)
    y = generate_svm_data(T=100, parameters=p)["observations"]
    lines.append("# SVM T = 100 (A, LQinv, LRinv); pmmh: N = 256, scale {0}, {1} x the steps".format(args.mean_pmmh_scale, args.mean_pmmh_factor))
    lines.append("# pmmh's target is prior.logprior on the raw row WITHOUT the Jacobian of Qinv = LQinv^2, Rinv = LRinv^2, which the "
                 "Wishart draws of a Gibbs sampler include: 'pmmh x LQinv LRinv' reweights its samples by that factor")
    pmmh = dict(sampler="pmmh", N=256, proposal_scale=args.mean_pmmh_scale)
    for name, kw, f, jac in (("pmmh", pmmh, args.mean_pmmh_factor, False), ("pmmh x LQinv LRinv", pmmh, args.mean_pmmh_factor, True),
                             ("pgibbs N = 64", dict(sampler="pgibbs", N=64), 1, False)):
        avg = averaged(ChainEnsemble("svm", y, p, num_chains=C, seed=12, **kw), args.mean_burn * f, args.mean_steps * f, 3, jac)
        lines.append(means_row(name, avg))
        result["means_svm_" + name] = avg.mean(axis=0).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--chains", type=int, default=None)
    ap.add_argument("--pmmh-scale", type=float, default=0.02)
    ap.add_argument("--burn", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mean-chains", type=int, default=2048)
    ap.add_argument("--mean-burn", type=int, default=300)
    ap.add_argument("--mean-steps", type=int, default=700)
    ap.add_argument("--mean-pmmh-scale", type=float, default=0.08)
    ap.add_argument("--mean-pmmh-factor", type=int, default=5)
    ap.add_argument("--no-means", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pgibbs_time.py measures on the GPU: none is visible")
    st = torch.cuda.current_stream()
    w = bench.config_workload("c2")
    chains, P = args.chains or w["chains"], 3
    T = len(np.reshape(w["y"], -1))
    lines = ["# SVM T = {0} N = {1}, {2} chains, same build; pmmh at scale {3}; pgibbs scratch {4:.2f} GB".format(
        T, args.N, chains, args.pmmh_scale, chains * _capi.csmc_scratch_bytes(T, args.N) / 1e9)]
    common = dict(num_chains=chains, N=args.N, prior=w["prior"], seed=2024)
    ens = dict(pmmh=ChainEnsemble(w["model"], w["y"], w["p0"], sampler="pmmh", proposal_scale=args.pmmh_scale, **common),
               pgibbs=ChainEnsemble(w["model"], w["y"], w["p0"], sampler="pgibbs", **common))
    for e in ens.values():
        e.step(args.burn)
        e.synchronize()
    ms = {m: [] for m in ens}
    for _ in range(args.reps):
        for m, e in ens.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            e.step(1)
            b.record(st)
            e.synchronize()
            ms[m].append(a.elapsed_time(b))
    med = {m: float(np.median(v)) for m, v in ms.items()}
    lines += ["# whole steps alternated, HIP events, {0} rounds after {1} steps; ms".format(args.reps, args.burn),
              "# {0:<7} {1:>9} {2:>9} {3:>9} {4:>8} {5:>8} {6:>14}".format("mode", "median", "min", "max", "iqr", "/ pmmh", "chain-steps/s")]
    for m, v in ms.items():
        q1, q3 = np.percentile(v, [25, 75])
        assert np.all(np.isfinite(ens[m].theta()))
        lines.append("  {0:<7} {1:>9.4f} {2:>9.4f} {3:>9.4f} {4:>8.4f} {5:>8.3f} {6:>14.0f}".format(
            m, med[m], float(np.min(v)), float(np.max(v)), float(q3 - q1), med[m] / med["pmmh"], ens[m].C / (med[m] * 1e-3)))
    lines += ["# over {0} further steps: E (theta_j(t+1) - theta_j(t))^2 of (A, LQinv, LRinv) per step and per GPU-second".format(args.steps),
              "# {0:<7} {1:>36} {2:>36}  {3}".format("mode", "squared jump / step", "squared jump / GPU-second", "note")]
    result = dict(median_ms=med, reps=args.reps, N=args.N, chains=chains)
    for m, e in ens.items():
        n0 = e.accept_dev.cpu().numpy().astype(np.float64) if m == "pmmh" else e.n_degenerate().astype(np.float64)
        prev = e.theta_dev[:, :P].clone()
        sq = torch.zeros(P, dtype=torch.float64, device=prev.device)
        for _ in range(args.steps):
            e.step(1)
            cur = e.theta_dev[:, :P]
            sq += ((cur - prev) ** 2).mean(0)
            prev.copy_(cur)
        e.synchronize()
        esjd = sq.cpu().numpy() / args.steps
        per_s = esjd / (med[m] * 1e-3)
        if m == "pmmh":
            note = "accepted {0:.3f}".format(float(np.mean(e.accept_dev.cpu().numpy() - n0) / args.steps))
        else:
            note = "degenerate sweeps {0:.0f} of {1}".format(float(np.sum(e.n_degenerate() - n0)), args.steps * e.C)
        lines.append("  {0:<7} {1:>36} {2:>36}  {3}".format(m, " ".join("{0:.3e}".format(v) for v in esjd),
                                                         " ".join("{0:.3e}".format(v) for v in per_s), note))
        result[m] = dict(esjd=esjd.tolist(), esjd_per_gpu_second=per_s.tolist(), note=note)
    del ens
    torch.cuda.empty_cache()
    if not args.no_means:
        posterior_means(args, lines, result)
    print(json.dumps(result), flush=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
