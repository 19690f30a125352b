"""What a control-variate SGLD step costs and what it buys in the variance of the step's gradient (needs the GPU).

  cost       SVM T = N = 1000, 12288 chains (shape c2 of bench.py), buffered (S = 16, B = 4, device windows) and the full
             series.  Three resident ensembles whose whole steps are timed alternately with HIP events (warm-up first; `reps`
             rounds), so all see the same clocks and neighbours:
               sgld      one window per chain
               sgld_m2   minibatch_size = 2: two windows per chain, the equal-work comparison
               sgld_cv   every window at theta and at the centre, one launch of twice the descriptors
             Per row: the kernel the filter launch ran, median, min, max and inter-quartile range in ms, the ratio of the
             medians to sgld's.  Then the update and accumulate kernels alone.
             --sgld-only times the sgld ensemble alone, and --root DIR imports bench.py and the package from DIR: given a
             checkout of the parent commit with its library built, the two together give the parent's own sgld step, to be
             run in turns with --sgld-only on this tree (processes alternated).
  variance   per coordinate, the variance over 1024 chains of the step's raw gradient estimate (score columns, before the
             prior and the 1 / T scaling): plain (one window), M = 2 (minibatch_size = 2), and control variate, the latter
             split into the window part out - out_centre and the centre gradient's own error.  Offsets theta - centre of 0,
             0.25, 1 and 2 posterior standard deviations in every free coordinate at once; the standard deviations are the
             Laplace ones, 1 / sqrt of the diagonal observed information at the centre by central differences of the
             whole-series score (mean over the chains; SVM: at N = 1000 for both particle counts, the whole-series score at
             N = 100 is too poor to difference).  SVM (S = 16, B = 4, N = 1000 and 100) and LGSSM kind='marginal'.
             Then the error of centre_gradient() for centre_repeats 1 and 8: its root mean square over chains around the
             mean of the 8-repeat gradients.

None of the figures is a pass / fail bound.

    python tools/sgld_cv_stats.py [--reps 15] [--skip-variance] [--sgld-only [--root DIR]] [--out profiles/sgld_cv.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv[1:-1]:      # before the imports: which tree they come from
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from sgmcmc_ssm_amd.ensemble import ChainEnsemble  # noqa: E402

SCORE_COL = {"svm": (2, 1, 0), "lgssm": (3, 2, 1, 0)}       # the score column of each theta slot (include/pfgrad.h)
FREE = {"svm": (0, 1, 2), "lgssm": (0, 2, 3)}               # the theta slots that move (LGSSM's C stays 1)
NAMES = {"svm": ("LRinv", "LQinv", "A"), "lgssm": ("LRinv", "LQinv", "C", "A")}
OFFSETS = (0.0, 0.25, 1.0, 2.0)


def timed(st, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def row(name, variant, v, base):
    q1, q3 = np.percentile(v, [25, 75])
    med = float(np.median(v))
    return "  {0:<9} {1:<12} {2:>9.4f} {3:>9.4f} {4:>9.4f} {5:>8.4f} {6:>8.3f}".format(
        name, variant, med, float(np.min(v)), float(np.max(v)), float(q3 - q1), med / base if base else float("nan"))


def cost(args, lines):
    st = torch.cuda.current_stream()
    w = bench.config_workload("c2")
    for S, B, what in ((16, 4, "S = 16, B = 4, device windows"), (-1, -1, "full series")):
        kw = dict(num_chains=w["chains"], N=w["N"], kernel=w["kernel"], epsilon=1e-4, prior=w["prior"], subsequence_length=S,
                  buffer_length=B, seed=2024, window_sampling="device")
        make = dict(sgld=lambda: ChainEnsemble(w["model"], w["y"], w["p0"], **kw),
                    sgld_m2=lambda: ChainEnsemble(w["model"], w["y"], w["p0"], minibatch_size=2, **kw),
                    sgld_cv=lambda: ChainEnsemble(w["model"], w["y"], w["p0"], sampler="sgld_cv", **kw))
        ens = {m: f() for m, f in make.items() if m == "sgld" or not args.sgld_only}
        for e in ens.values():
            e.step(3)
            e.synchronize()
        ms, variant = {m: [] for m in ens}, {}
        for _ in range(args.reps):
            for m, e in ens.items():
                ms[m].append(timed(st, lambda: e.step(1)))
                variant[m] = e.ctx.last_variant()
        lines += ["# cost: SVM T = {0} N = {1}, {2} chains, {3}; whole steps alternated, HIP events, {4} rounds; ms".format(
            len(np.reshape(w["y"], -1)), w["N"], w["chains"], what, args.reps),
            "# {0:<9} {1:<12} {2:>9} {3:>9} {4:>9} {5:>8} {6:>8}".format("mode", "pf kernel", "median", "min", "max", "iqr", "/ sgld")]
        base = float(np.median(ms["sgld"]))
        for m, v in ms.items():
            assert np.all(np.isfinite(ens[m].theta()))
            lines.append(row(m, variant[m], v, base))
        if args.sgld_only:
            continue
        e = ens["sgld_cv"]
        upd = [timed(st, e.launch_update) for _ in range(args.reps)]
        acc = [timed(st, lambda: e.ctx.cv_accumulate_device(e.C, e.centre_out_dev.data_ptr(), e.centre_acc_dev.data_ptr(), 0, 1,
                                                            e.centre_ctr_dev.data_ptr(), e._stream(None)))
               for _ in range(args.reps)]
        med = float(np.median(ms["sgld_cv"]))
        lines.append("  alone (each with its counter bump): sgld_cv update {0:.4f} ms = {1:.2%} of the step, cv_accumulate {2:.4f} ms".format(
            float(np.median(upd)), float(np.median(upd)) / med, float(np.median(acc))))
        del ens
        torch.cuda.empty_cache()


def laplace_sd(e, model, hat, h, repeats):
    """1 / sqrt of the diagonal observed information at `hat`: central differences of the whole-series score."""
    sd = np.zeros(len(hat))
    for j in FREE[model]:
        g = []
        for s in (+1.0, -1.0):
            th = hat.copy()
            th[j] += s * h
            e.set_centre(th, repeats=repeats)
            g.append(e.centre_gradient().mean(axis=0)[SCORE_COL[model][j]])
        info = -(g[0] - g[1]) / (2.0 * h)
        sd[j] = 1.0 / np.sqrt(info) if info > 0 else np.nan
    return sd


def gradients(e, theta, multi=False):
    """The records of one launch at `theta` for every chain (no update); the counter is bumped by hand for fresh draws."""
    e.theta_dev[:, :theta.shape[0]] = torch.from_numpy(theta).to(e.device)
    e.step_ctr += 1
    e.launch_windows()
    e.launch_pf()
    if multi:
        e.launch_reduce()
    e.synchronize()


def fmt(v):
    return " ".join("{0:>10.4g}".format(x) for x in v)


def variance(args, lines):
    C = 1024
    cases = [("svm", "pf", 1000), ("svm", "pf", 100), ("lgssm", "marginal", 1)]
    sds = {}        # per model, from its first case: the whole-series score at N = 100 is too poor to difference
    for model, kind, N in cases:
        p, y, prior, cfg = bench.make_workload(model, 1000)
        hat = p.theta()
        h = len(NAMES[model])
        kw = dict(num_chains=C, N=N, kernel=cfg["kernel"], epsilon=1e-4, prior=prior, subsequence_length=16, buffer_length=4,
                  seed=77, window_sampling="device", kind=kind)
        cv = ChainEnsemble(model, y, p, sampler="sgld_cv", **kw)
        m2 = ChainEnsemble(model, y, p, minibatch_size=2, **kw) if kind == "pf" else None
        if model not in sds:
            sds[model] = laplace_sd(cv, model, hat, 0.02, 1 if kind == "marginal" else 4)
        sd = sds[model]
        title = "{0} kind='{1}'{2}, T = 1000, S = 16, B = 4, {3} chains".format(model, kind, " N = {0}".format(N) if kind == "pf" else "", C)
        lines += ["# variance: " + title, "#   Laplace sd of (" + ", ".join(["A", "LQinv", "LRinv"] if model == "svm" else ["A", "C", "LQinv", "LRinv"]) +
                  "): " + fmt(sd), "#   columns: " + ", ".join(NAMES[model])]
        if not np.all(np.isfinite(sd[list(FREE[model])])):
            lines.append("#   the observed information is not positive in some coordinate: no offsets")
            continue
        # the error of the centre gradient for 1 and 8 repeats
        grads = {}
        for R in (8, 1):
            cv.set_centre(hat, repeats=R)
            grads[R] = cv.centre_gradient()
        ref = grads[8].mean(axis=0)
        for R in (1, 8):
            lines.append("  centre_gradient() rms error over chains, centre_repeats = {0}: {1}".format(
                R, fmt(np.sqrt(((grads[R] - ref) ** 2).mean(axis=0)))))
        for k in OFFSETS:
            th = hat.copy()
            for j in FREE[model]:
                th[j] += k * sd[j]
            gradients(cv, th)
            cur, cen = cv.cv_statistics()
            cg = cv.centre_grad_dev.cpu().numpy()
            part = (cur - cen)[:, :h]
            g_cv, plain = cg[:, :h] + part, cur[:, :h]
            lines.append("  offset {0:>4} sd   plain      {1}".format(k, fmt(plain.var(axis=0))))
            if m2 is not None:
                gradients(m2, th, multi=True)
                two = m2.out_dev.cpu().numpy()[:, :h]
                lines.append("                   M = 2      {0}".format(fmt(two.var(axis=0))))
            lines.append("                   cv         {0}".format(fmt(g_cv.var(axis=0))))
            lines.append("                   cv window  {0}   (out - out_centre alone)".format(fmt(part.var(axis=0))))
            lines.append("                   cv / plain {0}".format(fmt(g_cv.var(axis=0) / plain.var(axis=0))))
            if m2 is not None:
                lines.append("                   cv / M = 2 {0}".format(fmt(g_cv.var(axis=0) / two.var(axis=0))))
        del cv, m2
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--skip-variance", action="store_true")
    ap.add_argument("--sgld-only", action="store_true", help="the cost rows of the sgld ensemble alone")
    ap.add_argument("--root", default=None, help="import bench.py and the package from this checkout (its library built)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgld_cv_stats.py measures on the GPU: none is visible")
    lines = ["# tree: " + ROOT] if args.sgld_only else []
    cost(args, lines)
    if not args.skip_variance and not args.sgld_only:
        variance(args, lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
