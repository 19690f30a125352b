"""What the score on the sorted filters costs and what sampler='pmala_sorted' buys (needs the GPU; --resources does not).

Shape: the series of bench.py's c2 (SVM, T = 1000), 12288 chains, the whole series in every step, one proposal_scale for every
row, N = 64 and 128 on the sorted filters and N = 1000 on the plain ones:

  launch      ms of the filter launch alone, HIP events, the rows of one N alternated: pfg_cpm_device / pfg_sqmc_device (the
              STAT_NONE instantiations, the launches of correlated / SQMC PMMH) against pfg_cpm_score_device /
              pfg_sqmc_score_device at lambduh = 1 and 0.95 -- what the statistic costs.
  step        whole steps (propose, launch, accept, commit), timed the same way.
  movement    over `--steps` further steps: the acceptance rate and E (theta_j(t + 1) - theta_j(t))^2 of (A, LQinv, LRinv) per
              step and per GPU-second, for 'pmala_sorted' (rho = 0.99 and SQMC; lambduh = 1 and 0.95), correlated and SQMC PMMH at
              the same N, and 'pmala' and 'pmmh' at N = 1000.
  score var   the variance over the chains of every score column at the start parameters (the init pass: every chain at the
              same theta, fresh draws), lambduh = 1 against 0.95: what the shrinkage buys at T = 1000.
  resources   (--resources, no GPU) VGPRs, AGPRs, LDS, scratch and occupancy of every instantiation of the two kernels from the
              compiler's resource-usage remarks, and the workgroups per CU each reaches: the smaller of what the registers allow
              (waves per SIMD x 4 SIMDs / waves per workgroup) and what 160 KB of LDS per CU allow.

There is no pass / fail ratio.

    python tools/pmala_sorted_time.py [--reps 7] [--out profiles/pmala_sorted.txt]
    python tools/pmala_sorted_time.py --resources [--out profiles/pmala_sorted.txt --append]"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"))
import numpy as np  # noqa: E402

RHO = 0.99
LDS_PER_CU = 160 * 1024


def sorted_rows(N):
    """name -> ChainEnsemble keywords of the rows at N particles."""
    rows = {"pmmh-cpm": dict(sampler="pmmh", correlation=RHO), "pmmh-sqmc": dict(sampler="pmmh", sqmc=True)}
    for lam in (1.0, 0.95):
        pf = dict(pf="poyiadjis_N") if lam == 1.0 else dict(pf="nemeth", lambduh=lam)
        rows["sorted-cpm-l{0:g}".format(lam)] = dict(sampler="pmala_sorted", correlation=RHO, **pf)
        rows["sorted-sqmc-l{0:g}".format(lam)] = dict(sampler="pmala_sorted", sqmc=True, **pf)
    return {"{0}-N{1}".format(k, N): dict(v, N=N) for k, v in rows.items()}


def timed(fn, e, st):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    e.synchronize()
    return a.elapsed_time(b)


def measure(rows, w, chains, args, lines, result):
    """One group of rows: build, record the start score's variance, burn, time the launch and the step alternately, then move."""
    import torch
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    st, P = torch.cuda.current_stream(), 3
    ens = {m: ChainEnsemble(w["model"], w["y"], w["p0"], proposal_scale=args.scale, num_chains=chains, prior=w["prior"], seed=2024,
                            **kw) for m, kw in rows.items()}
    for m, e in ens.items():
        if hasattr(e, "grad_cur_dev"):
            g, ll = e.grad_cur_dev[:, :P].cpu().numpy(), e.ll_dev.cpu().numpy()
            result[m] = dict(score_var=g.var(0, ddof=1).tolist(), score_mean=g.mean(0).tolist(), ll_var=float(ll.var(ddof=1)))
    for e in ens.values():
        e.step(args.burn)
        e.synchronize()
    launch, step = {m: [] for m in ens}, {m: [] for m in ens}
    for _ in range(args.reps):
        for m, e in ens.items():
            # (the launch reads theta_prop_dev and the counter and writes out_dev and, under correlation, the buffer the chain
            # does not read: timing it alone leaves the chain's state as it was)
            launch[m].append(timed(e.launch_pf, e, st))
        for m, e in ens.items():
            step[m].append(timed(lambda: e.step(1), e, st))
    for m, e in ens.items():
        med = float(np.median(step[m]))
        n0 = e.accept_dev.cpu().numpy().astype(np.float64)
        prev = e.theta_dev[:, :P].clone()
        sq = torch.zeros(P, dtype=torch.float64, device=prev.device)
        for _ in range(args.steps):
            e.step(1)
            cur = e.theta_dev[:, :P]
            sq += ((cur - prev) ** 2).mean(0)
            prev.copy_(cur)
        e.synchronize()
        assert np.all(np.isfinite(e.theta()))
        esjd = sq.cpu().numpy() / args.steps
        r = result.setdefault(m, {})
        r.update(launch_ms=float(np.median(launch[m])), launch_min=float(np.min(launch[m])), launch_max=float(np.max(launch[m])),
                 step_ms=med, step_min=float(np.min(step[m])), step_max=float(np.max(step[m])),
                 accepted=float(np.mean(e.accept_dev.cpu().numpy() - n0) / args.steps), esjd=esjd.tolist(),
                 esjd_per_gpu_second=(esjd / (med * 1e-3)).tolist(), N=e.N)
    del ens
    torch.cuda.empty_cache()


def gpu_tables(args):
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit("pmala_sorted_time.py measures on the GPU: none is visible (--resources needs none)")
    w = bench.config_workload("c2")
    chains = args.chains or w["chains"]
    T = len(np.reshape(w["y"], -1))
    lines = ["# SVM T = {0}, {1} chains, proposal_scale {2}, correlation {3}; launches and whole steps alternated within a group, HIP "
             "events, {4} rounds after {5} steps".format(T, chains, args.scale, RHO, args.reps, args.burn)]
    result = {}
    groups = [sorted_rows(N) for N in args.N] + [{"pmala-N1000": dict(sampler="pmala", N=1000), "pmmh-N1000": dict(sampler="pmmh", N=1000)}]
    for rows in groups:
        measure(rows, w, chains, args, lines, result)
    fmt = lambda v: " ".join("{0:.3e}".format(x) for x in v)      # noqa: E731
    lines += ["# the filter launch alone and the whole step, ms (median, min .. max); / NONE: the score launch over the STAT_NONE launch "
              "of the same filter and N",
              "# {0:<22} {1:>5} {2:>10} {3:>19} {4:>8} {5:>10} {6:>19}".format("row", "N", "launch", "min .. max", "/ NONE", "step",
                                                                             "min .. max")]
    for group in groups:
        for m in group:
            r = result[m]
            base = "pmmh-{0}-N{1}".format("cpm" if "cpm" in m else "sqmc", r["N"]) if "cpm" in m or "sqmc" in m else None
            ratio = r["launch_ms"] / result[base]["launch_ms"] if base else float("nan")
            lines.append("  {0:<22} {1:>5} {2:>10.3f} {3:>9.3f} ..{4:>8.3f} {5:>8.3f} {6:>10.3f} {7:>9.3f} ..{8:>8.3f}".format(
                m, r["N"], r["launch_ms"], r["launch_min"], r["launch_max"], ratio, r["step_ms"], r["step_min"], r["step_max"]))
    lines += ["# over {0} further steps: acceptance, E (theta_j(t+1) - theta_j(t))^2 of (A, LQinv, LRinv) per step and per "
              "GPU-second".format(args.steps),
              "# {0:<22} {1:>5} {2:>9} {3:>32} {4:>32}".format("row", "N", "accepted", "squared jump / step", "squared jump / GPU-second")]
    for group in groups:
        for m in group:
            r = result[m]
            lines.append("  {0:<22} {1:>5} {2:>9.3f} {3:>32} {4:>32}".format(m, r["N"], r["accepted"], fmt(r["esjd"]),
                                                                            fmt(r["esjd_per_gpu_second"])))
    lines += ["# the init pass (every chain at the start parameters, fresh draws): variance over the chains of the score columns "
              "(LRinv, LQinv, A) and of the log-likelihood estimate",
              "# {0:<22} {1:>5} {2:>32} {3:>32} {4:>10}".format("row", "N", "var score", "mean score", "var ll")]
    for group in groups:
        for m in group:
            r = result[m]
            if "score_var" in r:
                lines.append("  {0:<22} {1:>5} {2:>32} {3:>32} {4:>10.3f}".format(m, r["N"], fmt(r["score_var"]), fmt(r["score_mean"]),
                                                                                r["ll_var"]))
    print(json.dumps(result), flush=True)
    return lines


def resource_table():
    """The compiler's resource-usage remarks of csrc/pfg_cpm.hip and csrc/pfg_sqmc.hip, one line per instantiation."""
    from sgmcmc_ssm_amd import _build
    lines = ["# kernel-resource-usage of cpm_kernel / sqmc_kernel <MODEL (0 SVM, 2 LGSSM), NT, PPT, TRACED, STAT (0 SCORE, 2 NONE)> "
             "(hipcc -Rpass-analysis=kernel-resource-usage, flags of sgmcmc_ssm_amd/_build.py)",
             "# WG/CU: min(waves per SIMD x 4 / waves per workgroup, 160 KB / LDS)",
             "# {0:<44} {1:>5} {2:>5} {3:>8} {4:>7} {5:>9} {6:>6} {7:>6} {8:>6}".format(
                 "kernel", "VGPR", "AGPR", "scratchB", "LDS B", "waves/SIMD", "by reg", "by LDS", "WG/CU")]
    for unit in ("pfg_cpm.hip", "pfg_sqmc.hip"):
        src = os.path.join(_build.CSRC, unit)
        cmd = [_build._hipcc()] + _build.FLAGS + _build._contract(src) + [
            "-I", _build.INCLUDE, "-I", _build.CSRC, "--cuda-device-only", "-c", src, "-o", os.devnull,
            "-Rpass-analysis=kernel-resource-usage"]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if res.returncode != 0:
            raise SystemExit(res.stdout)
        recs, cur = [], None
        for line in res.stdout.splitlines():
            m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
            if not m:
                continue
            key, _, val = m.group(1).partition(": ")
            if key == "Function Name":
                cur = {"mangled": val}
                recs.append(cur)
            elif cur is not None:
                cur[key.strip()] = val.strip()
        for r in recs:
            m = re.search(r"(cpm|sqmc)_kernelILi(\d)ELi(\d+)ELi(\d)ELb([01])ELi(\d)EE", r["mangled"])
            if not m:
                continue
            nt, occ, lds = int(m.group(3)), int(r["Occupancy [waves/SIMD]"]), int(r["LDS Size [bytes/block]"])
            by_reg, by_lds = max(1, occ * 4 // (nt // 64)), LDS_PER_CU // lds
            lines.append("  {0:<44} {1:>5} {2:>5} {3:>8} {4:>7} {5:>9} {6:>6} {7:>6} {8:>6}".format(
                "{0}_kernel<{1}, {2}, {3}, {4}, {5}>".format(m.group(1), m.group(2), nt, m.group(4),
                                                             "true" if m.group(5) == "1" else "false", m.group(6)),
                r["VGPRs"], r["AGPRs"], r["ScratchSize [bytes/lane]"], lds, occ, by_reg, by_lds, min(by_reg, by_lds)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chains", type=int, default=None)
    ap.add_argument("--scale", type=float, default=0.02)
    ap.add_argument("--burn", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--N", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    lines = resource_table() if args.resources else gpu_tables(args)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
