"""Step time of a PMMH ensemble against the SGLD ensemble of the same build and shape (needs the GPU).

Shape c2 of bench.py: SVM, T = N = 1000, 12288 chains, the whole series in every step.  Two comparisons, each with two
resident ensembles whose whole steps are timed alternately with HIP events (warm-up first; `reps` pairs), so both see the
same clocks and neighbours:

  sgld        particle filter (score) + sgld update             against  pmmh        propose + particle filter + accept
  pmmh-none   the filter launched with stat 'none' (no score)    against  pmmh-score  the score launch, its score ignored

Reported per row: the kernel the particle-filter launch ran (pfg_last_variant), median, min, max and inter-quartile range
of the step in ms, the ratio of the medians to the row's partner, chain-steps per second, and for PMMH the acceptance rate
over the timed steps.  There is no pass / fail ratio: the table says what an exact step costs beside an SGLD step.

    python tools/pmmh_time.py [--reps 15] [--scale 0.02] [--out profiles/pmmh_vs_sgld.txt]"""
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


def ensemble(w, **kw):
    return ChainEnsemble(w["model"], w["y"], w["p0"], num_chains=w["chains"], N=w["N"], kernel=w["kernel"], epsilon=w["epsilon"],
                         prior=w["prior"], subsequence_length=w["S"], buffer_length=w["B"], seed=2024, **kw)


def timed_pairs(ens, reps, st):
    """ms per whole step of each ensemble of `ens` (name -> ensemble), steps alternated; and the kernels they ran."""
    for e in ens.values():
        e.step(2)           # warm up: code objects, LDS attributes
        e.synchronize()
    ms, variant = {m: [] for m in ens}, {}
    for _ in range(reps):
        for m, e in ens.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            e.step(1)
            b.record(st)
            e.synchronize()
            ms[m].append(a.elapsed_time(b))
            variant[m] = e.ctx.last_variant()
    return ms, variant


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--scale", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pmmh_time.py measures on the GPU: none is visible")
    st = torch.cuda.current_stream()
    w = bench.config_workload("c2")
    if w["S"] != -1:
        raise SystemExit("pmmh_time.py expects the full-series shape c2")
    lines = ["# whole steps, SVM T = {0} N = {1}, {2} chains, same build, steps alternated, HIP events; ms".format(
                 len(np.reshape(w["y"], -1)), w["N"], w["chains"]),
             "# {0:<11} {1:<12} {2:>9} {3:>9} {4:>9} {5:>8} {6:>7} {7:>14} {8:>10}".format(
                 "mode", "pf kernel", "median", "min", "max", "iqr", "ratio", "chain-steps/s", "accepted")]
    result = {}
    for first, second, make in (
            ("sgld", "pmmh", lambda: dict(sgld=ensemble(w), pmmh=ensemble(w, sampler="pmmh", proposal_scale=args.scale))),
            ("pmmh-none", "pmmh-score", lambda: {
                "pmmh-none": ensemble(w, sampler="pmmh", proposal_scale=args.scale, pmmh_stat="none"),
                "pmmh-score": ensemble(w, sampler="pmmh", proposal_scale=args.scale, pmmh_stat="score")})):
        ens = make()
        ms, variant = timed_pairs(ens, args.reps, st)
        med = {m: float(np.median(v)) for m, v in ms.items()}
        for m, v in ms.items():
            q1, q3 = np.percentile(v, [25, 75])
            e = ens[m]
            assert np.all(np.isfinite(e.theta()))
            acc = "{0:.3f}".format(float(np.mean(e.acceptance_rate()))) if e.sampler == "pmmh" else "-"
            lines.append("  {0:<11} {1:<12} {2:>9.4f} {3:>9.4f} {4:>9.4f} {5:>8.4f} {6:>7.3f} {7:>14.0f} {8:>10}".format(
                m, variant[m], med[m], float(np.min(v)), float(np.max(v)), float(q3 - q1), med[m] / med[first],
                e.C / (med[m] * 1e-3), acc))
        result[first + "/" + second] = dict(median_ms=med, variant=variant)
        del ens
        torch.cuda.empty_cache()
    print(json.dumps(dict(result, reps=args.reps)), flush=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
