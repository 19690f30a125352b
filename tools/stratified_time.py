"""Particle-filter launch time of stratified against multinomial resampling on the same build (needs the GPU).

Per shape two resident ensembles that differ in `resampling` only; their PF launches are timed alternately with HIP events
(warm-up first; `reps` pairs), so both see the same clocks and neighbours.  Reported per shape and resampler: the kernel,
median, min, max and inter-quartile range of the launch in ms, and the ratio of the medians.

    python tools/stratified_time.py [--reps 15] [--shapes c5 c4 t1000] [--out profiles/stratified_vs_multinomial.txt]

Shapes: c5 = EURUS SVM N = 10000, S = 16 / B = 4, 2048 chains (bench config c5); c4 = SVM N = 4000, T = 1000, 512 chains
(c4: multinomial windows of SVM fp64 run LDS-resident there, wg1024x4s, so the large-N multinomial kernel, forced with
PFGRAD_VARIANT=big, is timed beside it as the stratified twin's own counterpart); t1000 = SVM T = N = 1000, 12288 chains
(c2's shape: the LDS-resident 256 x 4 units)."""
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

SHAPES = {"c5": "c5", "c4": "c4", "t1000": "c2"}


class forced:
    """PFGRAD_VARIANT for the plans made inside the block (the planner reads it at every query and launch)."""

    def __init__(self, variant):
        self.variant = variant

    def __enter__(self):
        if self.variant:
            os.environ["PFGRAD_VARIANT"] = self.variant

    def __exit__(self, *exc):
        os.environ.pop("PFGRAD_VARIANT", None)


def ensemble(cfg, resampling):
    w = bench.config_workload(cfg)
    return ChainEnsemble(w["model"], w["y"], w["p0"], num_chains=w["chains"], N=w["N"], kernel=w["kernel"], epsilon=w["epsilon"],
                         prior=w["prior"], subsequence_length=w["S"], buffer_length=w["B"], seed=2024, resampling=resampling,
                         window_sampling=("device" if w["S"] != -1 and not isinstance(w["y"], list) else "host"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stratified_time.py measures on the GPU: none is visible")
    st = torch.cuda.current_stream()
    lines = ["# PF launch, stratified against multinomial resampling, same build, launches alternated, HIP events; ms",
             "# {0:<6} {1:<12} {2:<22} {3:>7} {4:>9} {5:>9} {6:>9} {7:>8} {8:>7}".format(
                 "shape", "resampling", "kernel", "chains", "median", "min", "max", "iqr", "ratio")]
    for shape in args.shapes:
        modes = {"multinomial": ("multinomial", None), "stratified": ("stratified", None)}
        if shape == "c4":
            modes["multinom/big"] = ("multinomial", "big")
        ens = {}
        for m, (resampling, force) in modes.items():
            with forced(force):
                ens[m] = ensemble(SHAPES[shape], resampling)
                ens[m].step(2)          # warm up: code objects, LDS attributes, the windows of two steps
                ens[m].synchronize()
        ms, variant = {m: [] for m in ens}, {}
        for _ in range(args.reps):
            for m, e in ens.items():
                with forced(modes[m][1]):
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
        med = {m: float(np.median(v)) for m, v in ms.items()}
        for m, v in ms.items():
            q1, q3 = np.percentile(v, [25, 75])
            g, _ = ens[m].last_gradient_statistics()
            assert np.all(np.isfinite(g))
            lines.append("  {0:<6} {1:<12} {2:<22} {3:>7} {4:>9.4f} {5:>9.4f} {6:>9.4f} {7:>8.4f} {8:>7.3f}".format(
                shape, m, variant[m], ens[m].C, med[m], float(np.min(v)), float(np.max(v)), float(q3 - q1),
                med[m] / med["multinomial"]))
        print(json.dumps({"shape": shape, "median_ms": med, "variant": variant, "reps": args.reps}), flush=True)
        del ens
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
