"""Particle-filter launch time of adaptive (ESS-triggered) against always-resampling windows on the same build (needs the GPU).

Per shape two resident ensembles that differ in `ess_threshold` only; their PF launches are timed alternately with HIP
events (warm-up first; `reps` pairs), so both see the same clocks and neighbours.  Reported per shape: the kernels, median,
min, max and inter-quartile range of the launch in ms, the ratio of the medians, chain-steps per second of the PF launch, and
the share of timesteps that resampled -- counted on `--share-windows` traced windows of the same shape and parameters
(trace_anc is the identity on a step that kept its particles).

    python tools/adaptive_time.py [--reps 15] [--tau 0.5] [--shapes t1000 c5] [--out profiles/adaptive_vs_always.txt]

Shapes: t1000 = SVM T = N = 1000, 12288 chains (bench config c2: the LDS-resident 256 x 4 units); c5 = EURUS SVM N = 10000,
S = 16 / B = 4, 2048 chains (bench config c5: big16384 against big16384_adaptive)."""
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
from sgmcmc_ssm_amd import particle_filters  # noqa: E402
from sgmcmc_ssm_amd.ensemble import ChainEnsemble  # noqa: E402

SHAPES = {"t1000": "c2", "c5": "c5"}


def ensemble(w, tau):
    return ChainEnsemble(w["model"], w["y"], w["p0"], num_chains=w["chains"], N=w["N"], kernel=w["kernel"], epsilon=w["epsilon"],
                         prior=w["prior"], subsequence_length=w["S"], buffer_length=w["B"], seed=2024, ess_threshold=tau,
                         window_sampling=("device" if w["S"] != -1 and not isinstance(w["y"], list) else "host"))


def resampled_share(ens, w, tau, windows):
    """Share of the timesteps of `windows` traced windows of the shape (the chains' parameters) that resampled."""
    seqs = w["y"] if isinstance(w["y"], list) else [w["y"]]
    rs = np.random.RandomState(1)
    probs = []
    for k in range(windows):
        y = np.asarray(seqs[k % len(seqs)], dtype=float).reshape(-1)
        if w["S"] != -1 and y.shape[0] > w["window_T"]:
            s = int(rs.randint(0, y.shape[0] - w["window_T"] + 1))
            y = y[s:s + w["window_T"]]
        t1 = 0 if w["S"] == -1 else min(w["B"], y.shape[0] - 1)
        probs.append(particle_filters.make_problem(w["model"], ens.kernel, "poyiadjis_N", y, w["p0"].theta(), w["N"], t1=t1,
                                                   tL=y.shape[0] - t1, prior_mean=float(ens._desc["prior_mean"][0]),
                                                   prior_var=float(ens._desc["prior_var"][0]), rng="device", seed=77, stream=k,
                                                   ess_threshold=tau))
    kept = steps = 0
    for q in probs:
        anc = ens.ctx.run_batch([q], want_trace=True)[0]["all_ancestors"]
        kept += int(np.sum(np.all(anc == np.arange(anc.shape[1]), axis=1)))
        steps += anc.shape[0]
    return 1.0 - kept / max(steps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--share-windows", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_time.py measures on the GPU: none is visible")
    st = torch.cuda.current_stream()
    lines = ["# PF launch, adaptive (ess_threshold = {0}) against always-resampling, same build, launches alternated, HIP events; ms".format(args.tau),
             "# {0:<6} {1:<9} {2:<20} {3:>7} {4:>9} {5:>9} {6:>9} {7:>8} {8:>7} {9:>14} {10:>10}".format(
                 "shape", "mode", "kernel", "chains", "median", "min", "max", "iqr", "ratio", "chain-steps/s", "resampled")]
    for shape in args.shapes:
        w = bench.config_workload(SHAPES[shape])
        ens = {}
        for m, tau in (("always", None), ("adaptive", args.tau)):
            ens[m] = ensemble(w, tau)
            ens[m].step(2)          # warm up: code objects, LDS attributes, the windows of two steps
            ens[m].synchronize()
        ms, variant = {m: [] for m in ens}, {}
        for _ in range(args.reps):
            for m, e in ens.items():
                if e.window_sampling == "device":
                    e.launch_windows(st)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                e.launch_pf(st)
                b.record(st)
                e.launch_update(st)
                e.synchronize()
                ms[m].append(a.elapsed_time(b))
                variant[m] = e.ctx.last_variant()
        share = resampled_share(ens["adaptive"], w, args.tau, args.share_windows)
        med = {m: float(np.median(v)) for m, v in ms.items()}
        for m, v in ms.items():
            q1, q3 = np.percentile(v, [25, 75])
            g, _ = ens[m].last_gradient_statistics()
            assert np.all(np.isfinite(g))
            lines.append("  {0:<6} {1:<9} {2:<20} {3:>7} {4:>9.4f} {5:>9.4f} {6:>9.4f} {7:>8.4f} {8:>7.3f} {9:>14.0f} {10:>10}".format(
                shape, m, variant[m], ens[m].C, med[m], float(np.min(v)), float(np.max(v)), float(q3 - q1),
                med[m] / med["always"], ens[m].C / (med[m] * 1e-3), "{0:.3f}".format(share) if m == "adaptive" else "1.000"))
        print(json.dumps({"shape": shape, "median_ms": med, "variant": variant, "reps": args.reps, "resampled_share": share}), flush=True)
        del ens
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
