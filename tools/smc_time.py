"""Density-tempered SMC over resident PMMH chains beside plain PMMH of the same build and shape (needs the GPU).

Shape: the series of bench.py's c2 (SVM, T = 1000), 12288 chains, N = 1000 particles, the whole series in every step.

  stages      `--seeds` populations (TemperedPopulation, q0 centred at the common start with sd 0.3, tau 0.5, 2 moves) are run to
              phi = 1 one stage at a time; every whole stage -- five population kernels, `moves` x (propose, filter, accept), the
              host read of phi -- is timed with HIP events and alternated with one plain PMMH step (proposal_scale 0.02 from
              the common start) of the same build.  The first stage of the first population is warm-up and not counted.
              Reported: the number of stages per seed, median (IQR) of a stage and of a plain step in ms, the acceptance per
              stage at the population's own scale against plain PMMH's, the log-evidence per seed with its mean and spread.
  kernels     afterwards, on the last population (its state is no longer needed): each population kernel and the tempered
              accept alone, HIP events, median (IQR) over `--reps` launches; the temperature kernel from phi = 0 on the final
              population's h, which makes it search (reported: the delta it finds).  Their sum against a stage is the share
              of a stage the population kernels take.
  burn-in     the plain ensemble goes on from the common start, `--check` steps at a time up to `--max-steps`: the first step
              count at which the across-chain mean of every coordinate is within two of its standard errors of the tempered
              populations' pooled mean -- what the burn-in of independent chains costs where the population starts there.

There is no pass / fail ratio.

    python tools/smc_time.py [--seeds 5] [--out profiles/smc_tempering.txt]"""
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
from sgmcmc_ssm_amd.tempering import TemperedPopulation  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--chains", type=int, default=None)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--moves", type=int, default=2)
    ap.add_argument("--scale", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--check", type=int, default=50)
    ap.add_argument("--max-steps", type=int, default=1500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smc_time.py measures on the GPU: none is visible")
    st = torch.cuda.current_stream()
    w = bench.config_workload("c2")
    chains, P = args.chains or w["chains"], 3
    T = len(np.reshape(w["y"], -1))
    lines = ["# SVM T = {0}, N = {1}, {2} chains; tempered: q0 = N(start, 0.3^2), tau 0.5, {3} moves per stage; plain PMMH: "
             "proposal_scale {4}".format(T, args.N, chains, args.moves, args.scale)]
    plain = ChainEnsemble(w["model"], w["y"], w["p0"], sampler="pmmh", proposal_scale=args.scale, num_chains=chains,
                          prior=w["prior"], seed=2024, N=args.N)
    plain.step(2)
    plain.synchronize()
    stage_ms, step_ms, evidence, pooled, n_stages = [], [], [], [], []
    pop = None
    for seed in range(args.seeds):
        pop = TemperedPopulation(w["model"], w["y"], w["p0"], num_chains=chains, N=args.N, prior=w["prior"], seed=1000 + seed,
                                 moves=args.moves)
        first = seed == 0
        while pop.phi < 1.0:
            ms = timed(st, lambda: pop.stage(1))
            if not first:
                stage_ms.append(ms)
            first = False
            step_ms.append(timed(st, lambda: plain.step(1)))
        sched = pop.schedule()
        n_stages.append(pop.stage_index)
        evidence.append(pop.log_evidence())
        pooled.append(pop.ensemble.theta()[:, :P])
        lines.append("# seed {0}: {1} stages, log-evidence {2:.4f}; phi {3}".format(
            1000 + seed, pop.stage_index, evidence[-1], " ".join("{0:.4f}".format(v) for v in sched["phi"])))
        lines.append("#   acceptance per stage {0}".format(" ".join("{0:.3f}".format(v) for v in sched["acceptance"])))
        lines.append("#   scale of the last stage {0}; ESS per stage {1}".format(
            " ".join("{0:.4f}".format(v) for v in sched["scale"][-1]), " ".join("{0:.0f}".format(v) for v in sched["ess"])))
    steps_plain = plain.steps_done
    acc_plain = float(plain.acceptance_rate().mean())
    lines += ["# whole stages alternated with plain steps, HIP events, {0} stages (the first one is warm-up and left out); "
              "median (IQR) ms".format(len(stage_ms)),
              "  stage ({0} moves)        {1}".format(args.moves, med_iqr(stage_ms)),
              "  plain PMMH step         {0}".format(med_iqr(step_ms)),
              "  stage - {0} plain steps   {1:.4f}".format(args.moves, float(np.median(stage_ms)) - args.moves * float(np.median(step_ms))),
              "# acceptance: plain PMMH at scale {0} over its first {1} steps {2:.3f}".format(args.scale, steps_plain, acc_plain),
              "# log-evidence over {0} seeds: mean {1:.4f}, sd {2:.4f} (min {3:.4f}, max {4:.4f})".format(
                  args.seeds, float(np.mean(evidence)), float(np.std(evidence, ddof=1)) if args.seeds > 1 else float("nan"),
                  float(np.min(evidence)), float(np.max(evidence)))]

    # the population kernels alone, on the last population
    e = pop.ensemble
    zero = lambda: pop.phi_dev.fill_(0.0)
    kernels = dict(logtarget=(pop.launch_logtarget, None), temper=(pop.launch_temper, zero), gather=(pop.launch_gather, None),
                   scale=(pop.launch_scale, None), accept=(pop.launch_accept, None))
    alone = {}
    for name, (launch, before) in kernels.items():
        v = []
        for _ in range(args.reps + 2):
            if before:
                before()
            e.synchronize()
            v.append(timed(st, launch))
        alone[name] = v[2:]
    rec = pop._record_dev.cpu().numpy()
    lines.append("# the population kernels alone, HIP events, {0} launches each after 2; median (IQR) ms; the temperature kernel "
                 "searched from phi = 0 to delta = {1:.4f} (status {2})".format(args.reps, float(rec[1]),
                                                                              int(rec[8:].view(np.int32)[0])))
    for name, v in alone.items():
        lines.append("  {0:<10} {1}".format(name, med_iqr(v)))
    total = sum(float(np.median(alone[k])) for k in ("logtarget", "temper", "gather", "scale")) + args.moves * float(np.median(alone["accept"]))
    share = total / float(np.median(stage_ms))
    lines.append("  five kernels of a stage (accept x {0}): {1:.4f} ms = {2:.2%} of a stage".format(args.moves, total, share))

    # the burn-in of the independent ensemble towards the tempered populations' mean
    target = np.concatenate(pooled).mean(0)
    lines.append("# tempered populations' pooled mean of (A, LQinv, LRinv): {0}".format(" ".join("{0:.4f}".format(v) for v in target)))
    reached = None
    while plain.steps_done < args.max_steps:
        plain.step(args.check)
        th = plain.theta()[:, :P]
        se = th.std(0, ddof=1) / np.sqrt(chains)
        gap = np.abs(th.mean(0) - target) / se
        lines.append("#   plain step {0:>5}: mean {1}  |gap| / se {2}".format(
            plain.steps_done, " ".join("{0:.4f}".format(v) for v in th.mean(0)), " ".join("{0:.1f}".format(v) for v in gap)))
        if np.all(gap <= 2.0):
            reached = plain.steps_done
            break
    lines.append("# the independent ensemble is within two standard errors on every coordinate after {0} steps".format(
        reached if reached is not None else "more than {0}".format(args.max_steps)))
    print(json.dumps(dict(stages=n_stages, stage_ms=float(np.median(stage_ms)), step_ms=float(np.median(step_ms)),
                          kernels_ms=total, share=share, evidence=evidence, burn_in_steps=reached)), flush=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
