"""Step time of a pMALA ensemble against the PMMH and SGLD ensembles of the same build and shape, and what the score buys
(needs the GPU).

Shape c2 of bench.py: SVM, T = N = 1000, 12288 chains, the whole series in every step.

  step time   three resident ensembles whose whole steps are timed alternately with HIP events (warm-up first; `reps`
              rounds), so all see the same clocks and neighbours:
                sgld   particle filter (score) + sgld update
                pmmh   propose + particle filter (stat 'none') + accept
                pmala  propose + particle filter (score) + accept
              Reported per row: the kernel the particle-filter launch ran (pfg_last_variant), median, min, max and
              inter-quartile range of the step in ms, the ratio of the medians to sgld's, chain-steps per second.
  the score   PMMH and pMALA each at the scale (one number for every coordinate) of a grid whose acceptance rate in a
              pilot (`--pilot-chains` chains, `--pilot-burn` steps discarded, `--pilot-steps` measured) comes nearest to
              `--target`; then, on the 12288 chains after `--burn` steps, over `--steps` steps: the acceptance rate, the
              expected squared jump distance E (theta_j(t + 1) - theta_j(t))^2 per coordinate and step, and the same per
              GPU-second (divided by the median step time above).

There is no pass / fail ratio: the table says what the Langevin proposal costs and moves beside the random walk.

    python tools/pmala_time.py [--reps 15] [--target 0.3] [--out profiles/pmala_vs_pmmh.txt]"""
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
from sgmcmc_ssm_amd.ensemble import ChainEnsemble  # noqa: E402

GRID = {"pmmh": (0.003, 0.005, 0.01, 0.02, 0.03, 0.05), "pmala": (0.005, 0.01, 0.02, 0.03, 0.05, 0.08)}


def ensemble(w, chains=None, **kw):
    return ChainEnsemble(w["model"], w["y"], w["p0"], num_chains=chains or w["chains"], N=w["N"], kernel=w["kernel"],
                         epsilon=w["epsilon"], prior=w["prior"], subsequence_length=w["S"], buffer_length=w["B"], seed=2024, **kw)


def pilot(w, sampler, args):
    """scale -> acceptance rate over the pilot's measured steps; the grid's scale nearest the target."""
    rates = {}
    for s in GRID[sampler]:
        e = ensemble(w, chains=args.pilot_chains, sampler=sampler, proposal_scale=s)
        e.step(args.pilot_burn)
        e.synchronize()
        n0 = e.accept_dev.cpu().numpy().astype(np.float64)
        e.step(args.pilot_steps)
        e.synchronize()
        rates[s] = float(np.mean(e.accept_dev.cpu().numpy() - n0) / args.pilot_steps)
        del e
        torch.cuda.empty_cache()
    return rates, min(rates, key=lambda s: abs(rates[s] - args.target))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--target", type=float, default=0.3)
    ap.add_argument("--pilot-chains", type=int, default=1024)
    ap.add_argument("--pilot-burn", type=int, default=30)
    ap.add_argument("--pilot-steps", type=int, default=30)
    ap.add_argument("--burn", type=int, default=40)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pmala_time.py measures on the GPU: none is visible")
    st = torch.cuda.current_stream()
    w = bench.config_workload("c2")
    if w["S"] != -1:
        raise SystemExit("pmala_time.py expects the full-series shape c2")
    P = 3
    lines = ["# SVM T = {0} N = {1}, {2} chains, same build; scales: the grid's nearest to acceptance {3} in a pilot of {4} "
             "chains ({5} steps after {6})".format(len(np.reshape(w["y"], -1)), w["N"], w["chains"], args.target,
                                                  args.pilot_chains, args.pilot_steps, args.pilot_burn)]
    scale, result = {}, {}
    for sampler in ("pmmh", "pmala"):
        rates, scale[sampler] = pilot(w, sampler, args)
        lines.append("# pilot {0:<6} ".format(sampler) + "  ".join("{0}: {1:.3f}".format(s, r) for s, r in rates.items()) +
                     "   -> scale {0}".format(scale[sampler]))
        result["pilot_" + sampler] = rates
    ens = dict(sgld=ensemble(w), pmmh=ensemble(w, sampler="pmmh", proposal_scale=scale["pmmh"]),
               pmala=ensemble(w, sampler="pmala", proposal_scale=scale["pmala"]))
    for e in ens.values():
        e.step(args.burn)           # burn-in (and warm-up: code objects, LDS attributes)
        e.synchronize()
    # ---- step time: whole steps alternated
    ms, variant = {m: [] for m in ens}, {}
    for _ in range(args.reps):
        for m, e in ens.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            e.step(1)
            b.record(st)
            e.synchronize()
            ms[m].append(a.elapsed_time(b))
            variant[m] = e.ctx.last_variant()
    med = {m: float(np.median(v)) for m, v in ms.items()}
    lines += ["# whole steps alternated, HIP events, {0} rounds; ms".format(args.reps),
              "# {0:<7} {1:<12} {2:>9} {3:>9} {4:>9} {5:>8} {6:>8} {7:>14}".format(
                  "mode", "pf kernel", "median", "min", "max", "iqr", "/ sgld", "chain-steps/s")]
    for m, v in ms.items():
        q1, q3 = np.percentile(v, [25, 75])
        assert np.all(np.isfinite(ens[m].theta()))
        lines.append("  {0:<7} {1:<12} {2:>9.4f} {3:>9.4f} {4:>9.4f} {5:>8.4f} {6:>8.3f} {7:>14.0f}".format(
            m, variant[m], med[m], float(np.min(v)), float(np.max(v)), float(q3 - q1), med[m] / med["sgld"],
            ens[m].C / (med[m] * 1e-3)))
    lines.append("  pmala / pmmh {0:.3f}".format(med["pmala"] / med["pmmh"]))
    # ---- what the score buys: acceptance and expected squared jump distance after the burn-in
    lines += ["# after {0} + {1} steps, over {2} steps and {3} chains: acceptance, E (theta_j(t+1) - theta_j(t))^2 of "
              "(A, LQinv, LRinv) per step and per GPU-second".format(args.burn, args.reps, args.steps, w["chains"]),
              "# {0:<7} {1:>7} {2:>9} {3:>36} {4:>36}".format("mode", "scale", "accepted", "esjd / step", "esjd / GPU-second")]
    for m in ("pmmh", "pmala"):
        e = ens[m]
        n0 = e.accept_dev.cpu().numpy().astype(np.float64)
        prev = e.theta_dev[:, :P].clone()
        sq = torch.zeros(P, dtype=torch.float64, device=prev.device)
        for _ in range(args.steps):
            e.step(1)
            cur = e.theta_dev[:, :P]
            sq += ((cur - prev) ** 2).mean(0)
            prev.copy_(cur)
        e.synchronize()
        esjd = sq.cpu().numpy() / args.steps
        acc = float(np.mean(e.accept_dev.cpu().numpy() - n0) / args.steps)
        per_s = esjd / (med[m] * 1e-3)
        lines.append("  {0:<7} {1:>7} {2:>9.3f} {3:>36} {4:>36}".format(
            m, scale[m], acc, " ".join("{0:.3e}".format(v) for v in esjd), " ".join("{0:.3e}".format(v) for v in per_s)))
        result[m] = dict(scale=scale[m], accepted=acc, esjd=esjd.tolist(), esjd_per_gpu_second=per_s.tolist())
    result.update(median_ms=med, variant=variant, reps=args.reps)
    print(json.dumps(result), flush=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
