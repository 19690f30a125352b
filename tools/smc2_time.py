"""SMC^2 over resident PMMH chains (SequentialPopulation) at the shape of profiles/smc_tempering.txt (needs the GPU).

Shape: the series of bench.py's c2 (SVM, T = 1000), 12288 chains, N = 1000 particles, chunk = 50.

  run         one population per seed taken through the series one stage at a time, every stage timed with HIP events (the
              stage's host read included).  Reported per seed: stages, how many resampled, the total, log_evidence(); for the
              first seed every stage's t, ESS, whether it resampled, its acceptance and its time.
  kernels     on the last population: reweight, the row gather (also on GARCH's rows, N (NS + 1) = 3000 doubles, plain buffers),
              adopt (every chain adopting), scale and one filter launch on a chunk and on the whole prefix, HIP events, median
              (IQR) over `--reps` launches after 2.  The gather's rate is its traffic, 2 x C x row x 8 bytes, over its time,
              beside the 8.0 TB/s specification and the 6.29 TB/s a float4 copy reaches on this part.
  share       for the first seed the filter launches of every stage lie between HIP events of their own (the upload of their
              descriptors included): what is left of a stage is the population kernels, the torch bookkeeping and the host read.

There is no pass / fail ratio.

    python tools/smc2_time.py [--seeds 3] [--out profiles/smc2_timing.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from sgmcmc_ssm_amd.sequential import SequentialPopulation  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def med_iqr(v):
    q1, q2, q3 = np.percentile(v, [25, 50, 75])
    return "{0:.4f} ({1:.4f})".format(q2, q3 - q1)


def reps(stream, fn, n):
    for _ in range(2):
        fn()
    return [timed(stream, fn) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--chains", type=int, default=None)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--moves", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smc2_time.py measures on the GPU: none is visible")
    st = torch.cuda.current_stream()
    w = bench.config_workload("c2")
    chains = args.chains or w["chains"]
    T = len(np.reshape(w["y"], -1))
    lines = ["# SVM T = {0}, N = {1}, {2} chains, chunk {3}; q0 = N(start, 0.3^2), tau 0.5, {4} moves per resampling stage".format(
        T, args.N, chains, args.chunk, args.moves)]
    pop, evidence = None, []
    for seed in range(args.seeds):
        pop = SequentialPopulation(w["model"], w["y"], w["p0"], num_chains=chains, N=args.N, chunk=args.chunk, prior=w["prior"],
                                   seed=1000 + seed, moves=args.moves)
        ms, inside, pairs = [], [], []
        if seed == 0:           # the filter launches of every stage between events of their own (descriptor upload included)
            launch = pop.launch_filter

            def between_events(*a, **k):
                ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev[0].record(st)
                launch(*a, **k)
                ev[1].record(st)
                pairs.append(ev)
            pop.launch_filter = between_events
        while pop.t < pop.T:
            ms.append(timed(st, lambda: pop.step(1)))
            inside.append(sum(a.elapsed_time(b) for a, b in pairs))
            del pairs[:]
        if seed == 0:
            del pop.launch_filter
        s = pop.schedule()
        evidence.append(pop.log_evidence())
        lines.append("# seed {0}: {1} stages, {2} resampled, {3} filter launches, total {4:.1f} ms, log-evidence {5:.4f}".format(
            1000 + seed, len(ms), int(s["resampled"][1:].sum()), pop.launches, sum(ms), evidence[-1]))
        if seed == 0:
            lines.append("#   t, ESS before resampling, resampled, acceptance, increment, ms of the stage, ms of it in filter launches")
            for k, m in enumerate(ms):
                lines.append("  {0:5d} {1:9.1f} {2:d} {3:.3f} {4:10.4f} {5:9.3f} {6:9.3f}".format(
                    int(s["t"][k + 1]), s["ess"][k + 1], int(s["resampled"][k + 1]), s["acceptance"][k + 1], s["increment"][k + 1], m,
                    inside[k]))
            # (the first stage loads the code objects: it is listed above and left out here)
            for name, pick in (("resampled", 1), ("did not resample", 0)):
                ks = [k for k in range(1, len(ms)) if s["resampled"][k + 1] == pick]
                tot, fil = sum(ms[k] for k in ks), sum(inside[k] for k in ks)
                if ks:
                    lines.append("#   the {0} stages after the first that {1}: {2:.1f} ms, {3:.1f} ms of it in filter launches; the "
                                 "rest {4:.1f} ms = {5:.2f}% of those stages".format(len(ks), name, tot, fil, tot - fil,
                                                                                    100.0 * (tot - fil) / tot))
    lines.append("# log-evidence over {0} seeds: mean {1:.4f}, sd {2:.4f}".format(
        len(evidence), float(np.mean(evidence)), float(np.std(evidence, ddof=1)) if len(evidence) > 1 else float("nan")))

    # the kernels alone, on the last population (its state is no longer needed)
    e, C, row = pop.ensemble, pop.C, pop.row_doubles
    pop.parent_dev.copy_(torch.randint(0, C, (C,), device=e.device, dtype=torch.int32))
    lines.append("# the kernels alone, HIP events, {0} launches each after 2; median (IQR) ms".format(args.reps))

    def gather_rows():
        e.ctx.seq_gather_device(C, pop.parent_dev.data_ptr(), row, pop.state_dev[0].data_ptr(), pop.state_dev[1].data_ptr(),
                                e.theta_dev.data_ptr(), e.theta_prop_dev.data_ptr(), e.ll_dev.data_ptr(), pop.ll_tmp_dev.data_ptr(),
                                e._stream(None))
    g = reps(st, gather_rows, args.reps)
    rate = 2.0 * C * row * 8 / (np.median(g) * 1e-3)
    lines.append("  gather, SVM rows ({0} doubles, {1:.1f} MB each way)  {2}   {3:.2f} TB/s = {4:.0f}% of the 8.0 TB/s "
                 "specification, {5:.0f}% of a float4 copy's 6.29 TB/s".format(row, C * row * 8 / 1e6, med_iqr(g), rate / 1e12,
                                                                              100 * rate / HBM_SPEC, 100 * rate / HBM_COPY))
    grow = args.N * 3
    a = torch.randn((C, grow), dtype=torch.float64, device=e.device)
    b = torch.empty_like(a)

    def gather_garch():
        e.ctx.seq_gather_device(C, pop.parent_dev.data_ptr(), grow, a.data_ptr(), b.data_ptr(), e.theta_dev.data_ptr(),
                                e.theta_prop_dev.data_ptr(), e.ll_dev.data_ptr(), pop.ll_tmp_dev.data_ptr(), e._stream(None))
    g = reps(st, gather_garch, args.reps)
    rate = 2.0 * C * grow * 8 / (np.median(g) * 1e-3)
    lines.append("  gather, GARCH rows ({0} doubles, {1:.1f} MB each way)  {2}   {3:.2f} TB/s = {4:.0f}% of the specification, "
                 "{5:.0f}% of a float4 copy".format(grow, C * grow * 8 / 1e6, med_iqr(g), rate / 1e12, 100 * rate / HBM_SPEC,
                                                    100 * rate / HBM_COPY))
    del a, b
    counts = torch.ones(C, dtype=torch.int64, device=e.device)
    seen = torch.zeros(C, dtype=torch.int64, device=e.device)

    def adopt_all():
        seen.zero_()
        e.ctx.seq_adopt_device(C, counts.data_ptr(), seen.data_ptr(), row, pop.state_dev[0].data_ptr(),
                               pop.state_dev[1].data_ptr(), e._stream(None))
    zero = reps(st, seen.zero_, args.reps)
    g = reps(st, adopt_all, args.reps)
    lines.append("  adopt, every chain (with the {0:.4f} ms fill of `seen`)  {1}".format(float(np.median(zero)), med_iqr(g)))
    incr = torch.randn(C, dtype=torch.float64, device=e.device) * 3.0

    def reweight():
        pop.logw_dev.zero_()
        pop.launch_reweight(incr.data_ptr(), 1, 0.5)
    lines.append("  reweight (resampling)  " + med_iqr(reps(st, reweight, args.reps)))
    lines.append("  scale  " + med_iqr(reps(st, pop.launch_scale, args.reps)))
    chunk_ms = reps(st, lambda: pop.launch_filter(e.theta_dev, pop.T - args.chunk, args.chunk, 0, 1), args.reps)
    whole_ms = reps(st, lambda: pop.launch_filter(e.theta_dev, 0, pop.T, None, 1), args.reps)
    lines.append("  filter launch, warm-started, {0} observations (descriptor upload included)  {1}".format(args.chunk, med_iqr(chunk_ms)))
    lines.append("  filter launch, from scratch, {0} observations  {1}".format(pop.T, med_iqr(whole_ms)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
