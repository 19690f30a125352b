#!/usr/bin/env python
"""bench.py -- SGLD steps/sec of the particle-filter gradient path on MI355X.

Default workload = BASELINE.json configs[1] (the config the metric is quoted on): SVM synthetic
series, T=1000, N=1000 particles, SGLD on the full sequence (S=-1), pf='poyiadjis_N', bootstrap
kernel, epsilon=0.1, prior variance 100 (nonlinear_ssm_pf_experiment_scripts/svm/
{demo_setup.py:65-79,driver.py:54}).  `--config c1|c3|c4|c5` runs the other BASELINE configs
(parity-test cases with their own profiles; never the headline line).

One bench "step" = one SGLD step (sample_sgld + project_parameters, what evaluator.py:343-347
times) of EVERY chain on the GPU: one particle-filter launch (one workgroup per chain, the whole
T-loop inside) + one update launch.  `value` = chain-steps per second summed over all GPUs (chains
are independent; weak scaling: --chains-per-gpu is fixed as N grows).  Everything is resident in
HBM when the timed region starts.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself
(python -m torch.distributed.run, one per GPU) BEFORE anything in this process touches the GPU,
and exits with their status.

A plain run sets up, warms up, times `--steps` steps and prints the result line.  `--dump-outputs DIR`
then writes what the last timed step handed back (DIR/<name>.npy, float64): the chains' parameters
`theta` [chains, P], their score estimates `grad` [chains, h] and log-likelihood estimates `loglik`
[chains] (g1: `grad` / `loglik` of every window).  Inputs are seeded: the same arguments give the same
inputs on every run.  `--full` adds the legs that need runs of their own: one chain alone, the
replay-arithmetic kernel, the parity checks against the reference fixtures, the CPU baseline and
(g1) the per-timestep kernel times with their roofline.

The JSON line also carries
  roofline      the binding resource of the dominant kernel.  The LDS-resident kernels stream no
                particle state through HBM, so the bound is VALU issue: achieved = (per-class VALU
                instruction counts of the launch, committed rocprofv3 PMC passes) x (issue cycles per
                class, measured on this GPU with tools/calib/valu_calib) / live kernel time; peak =
                1024 SIMDs x the in-kernel shader clock (s_memtime / s_memrealtime stamps of the
                timed launches).  The SURVEY 8(d) HBM model (2*(n+1+h)*8 B per particle-timestep)
                is kept as `hbm_model`, explicitly non-binding.  The large-N kernel (c5) does stream
                its state: there bound = "hbm" and the algorithmic bytes are real traffic.
  cpu_baseline  (--full) the CPU oracle (NumPy restatement of the reference, bit-identical to it)
                timed on this box's host, 1 core, on a bounded sample of the same workload
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd")
for p in (ROOT, PKG_DIR):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

T_SERIES, N_PART = 1000, 1000
HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
N_SIMD = 1024             # 256 CUs x 4 SIMDs
N_CU = 256

RNG_PRECISION = ("device generator: jsf32 per lane keyed by Philox4x32-10(seed; lane, global chain id, step); "
                 "32-bit uniforms searched against a 32-bit fixed-point CDF (LDS-resident kernels) or an fp64 CDF "
                 "(large-N kernel); Box-Muller normals evaluated on the f32 transcendental units (v_log/v_sin/v_cos) "
                 "and widened to f64; all arithmetic on the particle state, weights, CDF sums and statistics is fp64")

CONFIGS = {
    # name: (model, T_series, N, S, B, chains/GPU, description)
    # chains/GPU: enough resident windows to amortise the launch's fixed cost (measured for c2: kernel time =
    # 1.0 ms + 4.83 ms per 1024 chains, i.e. 194 k steps/s at 3072 chains, 207 k at 12288, 212 k asymptotically)
    "c1": ("lgssm", 200, 100, -1, -1, 16384, "LGSSM d=1 synthetic T=200 N=100, SGLD full sequence, optimal kernel (BASELINE configs[0])"),
    "c2": ("svm", 1000, 1000, -1, -1, 12288, "SVM synthetic T=1000 N=1000, SGLD full sequence (S=-1), poyiadjis_N, prior kernel (BASELINE configs[1])"),
    "c3": ("garch", 1000, 1000, 16, 4, 16384, "GARCH synthetic T=1000 N=1000, SGLD buffered PF S=16 B=4, poyiadjis_N, optimal kernel (BASELINE configs[2])"),
    "c4": ("svm", 1000, 4000, -1, -1, 512, "SVM synthetic T=1000 N=4000, SGLD full sequence, poyiadjis_N (BASELINE configs[3], saturating variant)"),
    "c5": ("svm", None, 10000, 16, 4, 2048, "EURUS hourly log returns x1000, 49 gap-split segments, SeqSVM N=10000 S=16 B=4 num_sequences=1 (BASELINE configs[4])"),
    # not a BASELINE config: the reference's OWN giant-N call of the hot-path entry -- the ground truth of its bias experiments,
    # ten pf_gradient_estimate(pf='poyiadjis_N', N=1000000) runs on a buffered 48-step window
    # (gradient_error_fig_scripts/svm_grad_compare.py:58-82: T = 100, L = 16, buffer_size = 16) -- as whole-GPU windows
    "g1": ("svm", 100, 1000000, 16, 16, 10, "SVM synthetic T=100, the 48-step buffered window (L=16, B=16) of svm_grad_compare.py:58-82, poyiadjis_N, N=1000000 particles, 10 repetitions per step (whole-GPU windows)"),
}
STATE_STAT = {"svm": (1, 3), "garch": (2, 4), "lgssm": (1, 4)}


def make_workload(model, T=T_SERIES):
    """(parameters, observations, prior, settings) of one model's synthetic workload."""
    if model == "svm":
        from sgmcmc_ssm_amd.models.svm import SVMParameters, SVMPrior, generate_svm_data
        p = SVMParameters(A=np.eye(1) * 0.95, Q=np.eye(1) * 0.5, R=np.eye(1) * 0.5)
        np.random.seed(12345)
        data = generate_svm_data(T=T, parameters=p)
        prior = SVMPrior.generate_default_prior(var=100.0, n=1, m=1)
        return p, data["observations"], prior, dict(epsilon=0.1, S=-1, B=-1, kernel="prior", n=1, h=3)
    if model == "garch":
        from sgmcmc_ssm_amd.models.garch import GARCHParameters, GARCHPrior, generate_garch_data
        lm, lp, ll = GARCHParameters.convert_alpha_beta_gamma(0.1, 0.8, 0.05)
        p = GARCHParameters(log_mu=lm, logit_phi=lp, logit_lambduh=ll, LRinv=np.eye(1) * 0.3 ** -0.5)
        np.random.seed(222)
        data = generate_garch_data(T=T, parameters=p)
        prior = GARCHPrior.generate_default_prior(var=1.0, n=1, m=1)
        return p, data["observations"], prior, dict(epsilon=0.01, S=16, B=4, kernel="optimal", n=2, h=4)
    if model == "lgssm":
        from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, LGSSMPrior, generate_lgssm_data
        p = LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1), Q=np.eye(1) * 0.7, R=np.eye(1))
        np.random.seed(333)
        data = generate_lgssm_data(T=T, parameters=p)
        prior = LGSSMPrior.generate_default_prior(var=100.0, n=1, m=1)
        return p, data["observations"], prior, dict(epsilon=0.1, S=-1, B=-1, kernel="optimal", n=1, h=4)
    raise ValueError(model)


def config_workload(name):
    """One BASELINE config -> dict(model, p0, y (array or list of segments), prior, S, B, kernel, epsilon, N, ...)."""
    model, T, N, S, B, chains, desc = CONFIGS[name]
    if name == "c5":
        from sgmcmc_ssm_amd.models.svm import SVMParameters, SVMPrior
        path = os.path.join(ROOT, "tests", "golden", "eurus.npz")
        data_kind = "EURUS_processed.npz segments (fixture tests/golden/eurus.npz: data arrays of the reference's demo)"
        if os.path.exists(path):
            g = np.load(path)
            lens = g["segment_lengths"]
            flat = g["segments"]
            th = g["theta0"]
        else:   # same shape, synthetic values
            rs = np.random.RandomState(5)
            lens = rs.randint(48, 127, size=49)
            flat = rs.normal(size=int(lens.sum())) * 0.8
            th = np.array([0.9999, 1.6, 1.5])
            data_kind = "synthetic segments of the EURUS shape (fixture missing)"
        bounds = np.concatenate([[0], np.cumsum(lens)])
        y = [flat[bounds[k]:bounds[k + 1]].reshape(-1, 1) for k in range(len(lens))]
        p = SVMParameters(A=np.eye(1) * th[0], LQinv=np.eye(1) * th[1], LRinv=np.eye(1) * th[2])
        prior = SVMPrior.generate_default_prior(var=100.0, n=1, m=1)
        return dict(name=name, model="svm", p0=p, y=y, prior=prior, S=S, B=B, kernel="prior", epsilon=0.001, N=N,
                    chains=chains, desc=desc, window_T=S + 2 * B, data=data_kind, T_series=int(lens.sum()))
    p, y, prior, cfg = make_workload(model, T)
    return dict(name=name, model=model, p0=p, y=y, prior=prior, S=S, B=B, kernel=cfg["kernel"], epsilon=cfg["epsilon"],
                N=N, chains=chains, desc=desc, window_T=(T if S == -1 else S + 2 * B), data="synthetic", T_series=T)


def run_giant(args, rank, world, dev_index, n_distinct):
    """--config g1: one bench "step" = the reference's ground-truth computation of one trial, ten independent
    pf_gradient_estimate(N = 10^6) repetitions of the buffered 48-step window, as ten resident whole-GPU windows
    (pfg_launch_device_grid: 48 + 2 launches, the particle axis of every window tiled over all CUs).  `value` = windows
    (gradient estimates) per second.  Here the SURVEY 8(d) bytes ARE the traffic: roofline.bound = "hbm"."""
    import torch
    from sgmcmc_ssm_amd import distributed
    from sgmcmc_ssm_amd.grid import ResidentWindows
    model, T_series, N, L, Bf, reps, desc = CONFIGS[args.config]
    p, y_all, prior, cfg = make_workload(model, T_series)
    t0 = (T_series + L) // 2
    y = y_all[t0 - Bf:t0 + L + Bf].reshape(-1)
    T = y.shape[0]
    reps = args.chains_per_gpu or reps
    theta = np.tile(p.theta(), (reps, 1))
    dev = torch.device("cuda", dev_index)
    rw = ResidentWindows(model, y, theta, N, kernel=cfg["kernel"], pf="poyiadjis_N", t1=Bf, tL=Bf + L, prior_mean=0.0,
                         prior_var=10.0, dtype=args.dtype, seed=2024, stream0=rank * reps, device=dev_index)
    for _ in range(args.warmup):
        rw.launch()
    torch.cuda.synchronize(dev)
    distributed.barrier()
    torch.cuda.synchronize(dev)
    t_start = time.perf_counter()
    for _ in range(args.steps):
        rw.launch()
    torch.cuda.synchronize(dev)
    distributed.barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t_start
    g, ll = rw.results()
    if not (np.all(np.isfinite(g)) and np.all(np.isfinite(ll))):
        raise SystemExit("non-finite gradients after the run")
    elapsed, _ = rank_epilogue(torch.from_numpy(g).to(dev), elapsed, device=dev)
    if args.dump_outputs:
        out = gather_rows(np.concatenate([g, ll[:, None]], axis=1), dev)
        if rank == 0:
            dump_outputs(args.dump_outputs, grad=out[:, :-1], loglik=out[:, -1])
    variant = rw.ctx.last_variant()
    if args.full:
        # the dominant kernel's launch duration: HIP events around every timestep launch of a few more repetitions
        kern = []
        for _ in range(min(args.steps, 5)):
            ev = rw.launch_timed()
            torch.cuda.synchronize(dev)
            kern += [a.elapsed_time(b) for a, b in ev]
        kern_ms = float(np.mean(kern))
    if rank != 0:
        return
    line = {"metric": "ground-truth gradient estimates/sec (SVM 48-step buffered window, N=1000000 particles)",
            "value": float(reps) * world * args.steps / elapsed, "unit": "windows/s", "n_gpus": n_distinct, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": desc, "baseline_config": args.config, "windows_per_gpu": reps, "chains_per_gpu": reps, "N": N,
                       "window_T": T, "rng": "device", "kernel_variant": variant, "rng_precision": RNG_PRECISION +
                       "; whole-GPU windows resample with sorted uniforms (exponential spacings)",
                       "parallelism": "independent windows, {0} rank(s) x {1} windows".format(world, reps)},
            "particle_steps_per_s": float(reps) * world * args.steps * N * T / elapsed}
    if args.full:
        n, h = STATE_STAT[model]
        wsize = 8 if args.dtype == "f64" else 4
        alg_bytes = float(reps) * N * 2 * (n + 1 + h) * wsize           # per timestep launch
        alg_gbs = alg_bytes / (kern_ms * 1e-3) / 1e9
        key = "{0}_{1}_{2}".format(args.config, args.dtype, variant)
        trec = (_load_json("hbm_traffic.json") or {}).get(key)
        traffic = trec["bytes_per_launch"] * (float(reps) / trec["chains"]) if trec else None
        line["us_per_pf_timestep"] = kern_ms * 1e3
        line["roofline"] = {"bound": "hbm", "achieved": alg_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg_gbs / HBM_PEAK_GBS,
                            "traffic": traffic, "kernel_ms": kern_ms, "kernel": "pfg_grid_step_dev_kernel (one launch = one timestep of all {0} windows)".format(reps),
                            "whole_window_ms": elapsed / args.steps * 1e3, "launches_per_step": T + 2,
                            "frac_whole_window": float(reps) * N * T * 2 * (n + 1 + h) * wsize / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                            "note": "whole-GPU windows: particle state streams through HBM every timestep (scan + record read, record + scan "
                                    "write = the algorithmic 2 (n + 1 + h) w bytes per particle-step); kernel_ms = HIP events around the "
                                    "timestep launches, frac_whole_window = the same bytes over the wall time of the 50-launch sequence",
                            "stale": profile_is_stale()}
    if args.full and world == 1 and not args.no_single_chain:
        line["parity"] = giant_grad_error_vs_reference(dev_index)
    if args.full and world == 1 and not args.no_cpu_baseline:
        from oracle import pf_oracle as po
        Ts = 24
        t_c = time.perf_counter()
        po.pf_gradient_estimate(model, p.theta(), y[:Ts], N, rng=np.random.RandomState(0), kernel=cfg["kernel"], pf="poyiadjis_N",
                                t1=8, tL=16, prior_mean=0.0, prior_var=10.0)
        el = time.perf_counter() - t_c
        line["cpu_baseline"] = dict(value=1.0 / (el * T / Ts), unit="windows/s", cores=1, kind="port",
                                    sample="one pf_gradient_estimate of the NumPy oracle at N = {0} on the first {1} of the window's "
                                           "{2} timesteps ({3:.1f} s), scaled by {2}/{1}; 1 thread; the reference itself: 38 s per "
                                           "window in the build container".format(N, Ts, T, el))
        line["speedup_vs_cpu_1core"] = line["value"] / line["cpu_baseline"]["value"]
    print(json.dumps(line), flush=True)


def giant_grad_error_vs_reference(dev_index):
    """g1's parity leg: the reference's own N = 10^6 call (tests/golden/giant.npz:g1, written by make_golden.py from the
    reference itself) through the drop-in Helper on the REPLAY path -- np.random.seed(s), NumPy's legacy stream, the
    reference's CDF bit for bit (pfg_grid_cdf.hpp)."""
    path = os.path.join(ROOT, "tests", "golden", "giant.npz")
    if not os.path.exists(path):
        return None
    from sgmcmc_ssm_amd.models.svm import SVMHelper, SVMParameters
    g = np.load(path)
    meta = [m for m in json.loads(str(g["meta"])) if m["key"] == "g1"][0]
    th = g["g1/theta"]
    fm = dict(log_constant=0.0, mean_precision=g["g1/fm_mean_precision"].copy(), precision=g["g1/fm_precision"].reshape(1, 1).copy())
    helper = SVMHelper(n=1, m=1, forward_message=fm)
    p = SVMParameters(A=np.eye(1) * th[0], LQinv=np.eye(1) * th[1], LRinv=np.eye(1) * th[2])
    np.random.seed(meta["seed"])
    t_c = time.perf_counter()
    grad = helper.pf_gradient_estimate(observations=g["g1/y"].reshape(-1, 1), parameters=p, subsequence_start=meta["t1"],
                                       subsequence_end=meta["tL"], weights=g["g1/weights"], pf=meta["pf"], N=meta["N"])
    el = time.perf_counter() - t_c
    nxt = np.random.random_sample()
    got = np.array([float(np.asarray(grad[k]).reshape(-1)[0]) for k in ("A", "LQinv_vec", "LRinv_vec")])
    ref = g["g1/grad"]
    return {"kernel": "REPLAY whole-GPU window (reference operation order, NumPy's cumsum bit for bit, host MT19937 streams)",
            "grad_l2_err_vs_ref": float(np.linalg.norm(got - ref)), "grad_l2_ref_norm": float(np.linalg.norm(ref)),
            "generator_left_where_the_reference_leaves_it": bool(nxt == float(g["g1/next_draw"])),
            "dropin_call_seconds": el,
            "case": "helper.pf_gradient_estimate(pf='poyiadjis_N', N=1000000), 48-step window, np.random.seed({0}): reference "
                    "fixture tests/golden/giant.npz:g1 (the reference: 38 s per call)".format(meta["seed"]),
            "timed_kernel_parity": "tests/test_gpu_grid.py: the device-generator launch records its draws and the CPU oracle "
                                   "replays it (zero ancestor flips, rtol 1e-8)"}


def grad_error_vs_reference():
    """The second half of BASELINE.json's metric: gradient L2 error vs the reference on identical
    seeds.  Runs the HIP path (REPLAY generator, fp64) on the reference's own known-answer case
    committed under tests/golden (SVM T=1000 N=1000, np.random.seed(99): the SURVEY 8c vector,
    produced by the reference itself) and returns the errors.  No oracle involved.  NB this pins the
    REPLAY instantiation; the timed device-generator instantiation is pinned by
    tests/test_gpu_device_replay.py (the oracle replays the launch's own recorded draws)."""
    from sgmcmc_ssm_amd import _capi
    path = os.path.join(ROOT, "tests", "golden", "pf_window.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    meta = [m for m in json.loads(str(g["meta"])) if m["key"] == "w0"][0]
    N, T = meta["N"], meta["T"]
    rs = np.random.RandomState(meta["seed"])      # the reference's consumption order of the legacy stream
    z0 = rs.normal(size=N)
    u, z = np.empty((T, N)), np.empty((T, N))
    for t in range(T):
        u[t] = rs.random_sample(N)
        z[t] = rs.normal(size=N)
    q = dict(model="svm", kernel="prior", smoother="nemeth", stat="score", dtype="f64", rng="replay", N=N, t1=0,
             tL=T, lambduh=1.0, prior_mean=meta["prior_mean"], prior_var=meta["prior_var"], y=g["w0/y"],
             theta=g["w0/theta"], z0=z0, u=u, z=z)
    o = _capi.default_context(torch_device_index()).run_batch([q])[0]
    ref = g["w0/mean_statistic"]
    return {"kernel": "REPLAY instantiation (reference operation order, fp64 CDF, host MT19937 streams)",
            "grad_l2_err_vs_ref": float(np.linalg.norm(o["mean_stat"] - ref)),
            "grad_l2_ref_norm": float(np.linalg.norm(ref)),
            "loglik_abs_err_vs_ref": float(abs(o["loglik"] - float(g["w0/loglikelihood_estimate"]))),
            "case": "SVM T=1000 N=1000, np.random.seed(99), reference fixture tests/golden/pf_window.npz:w0, REPLAY fp64",
            "timed_kernel_parity": "tests/test_gpu_device_replay.py: the timed device-generator instantiation records its "
                                   "draws and the CPU oracle replays the launch (rtol 1e-8, zero ancestor flips)"}


def torch_device_index():
    import torch
    return torch.cuda.current_device()


def cpu_baseline(w, budget_s=12.0):
    """Reference CPU path: SGLD steps/s of ONE chain with the NumPy oracle (bit-identical to the
    reference's arithmetic), single thread.  Bounded: >= 3 steps, about `budget_s` seconds."""
    from oracle import pf_oracle as po
    from sgmcmc_ssm_amd.sgmcmc_sampler import random_subsequence_and_weights
    model, prior = w["model"], w["prior"]
    params = w["p0"].copy()
    segs = w["y"] if isinstance(w["y"], list) else [w["y"]]
    T_total = sum(len(s) for s in segs)
    eps = w["epsilon"]
    rng = np.random.RandomState(0)

    def one_step():
        y = segs[rng.randint(len(segs))] if len(segs) > 1 else segs[0]
        T = y.shape[0]
        if w["S"] == -1 or T - w["S"] <= 0:
            lo, hi, t1, tL, wts = 0, T, 0, T, None
        else:
            np.random.seed(rng.randint(2 ** 31))
            s, e, wts = random_subsequence_and_weights(w["S"], T)
            lo, hi = max(0, s - w["B"]), min(T, e + w["B"])
            t1, tL = s - lo, e - lo
        if model == "garch":
            pm, pv = po.garch_prior_x(params.theta())
        else:
            pm, pv = 0.0, 10.0
        g = po.pf_gradient_estimate(model, params.theta(), y[lo:hi], w["N"], rng=rng, kernel=w["kernel"],
                                    pf="poyiadjis_N", t1=t1, tL=tL, weights=wts, prior_mean=pm,
                                    prior_var=float(np.asarray(pv).reshape(-1)[0]))
        gp = prior.grad_logprior(params)
        scale = T_total / float(T) if len(segs) > 1 else 1.0
        for var in params.var_dict:
            delta = (gp[var] + scale * g[var]) / T_total
            noise = rng.normal(loc=0, scale=np.sqrt(1.0 / T_total), size=params.var_dict[var].shape)
            params.var_dict[var] += eps * delta + np.sqrt(2.0 * eps) * noise
        params.project_parameters()

    one_step()                       # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        one_step()
        n += 1
        el = time.perf_counter() - t0
        if n >= 3 and el >= budget_s:
            break
        if el > 3 * budget_s:
            break
    cores = os.cpu_count() or 1
    return dict(value=n / el, unit="SGLD steps/s", cores=1, kind="port",
                all_cores_bound=n / el * cores,
                sample="{0} full SGLD steps of one chain ({1:.1f} s), NumPy oracle, 1 thread; host has {2} cores; "
                       "all_cores_bound = cores x single-core rate (one independent chain per core)".format(n, el, cores))


# ------------------------------------------------------------------------------------------------
# roofline pieces
# ------------------------------------------------------------------------------------------------
def _load_json(name):
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None
    try:
        return json.load(open(path))
    except Exception:
        return None


def kernel_source_sha():
    """sha256 over the sources the kernels are built from (csrc/*.hpp, csrc/*.hip, include/pfgrad.h, the build
    flags in _build.py): the committed PMC counters (profiles/*.json) carry the hash they were taken at, and a
    roofline computed from counters of OTHER sources is flagged `stale`."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.hpp")) + glob.glob(os.path.join(PKG_DIR, "csrc", "*.hip")))
    files += [os.path.join(ROOT, "include", "pfgrad.h"), os.path.join(PKG_DIR, "sgmcmc_ssm_amd", "_build.py")]
    for p in files:
        h.update(os.path.basename(p).encode())
        h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def profile_is_stale():
    meta = _load_json("profile_meta.json") or {}
    return meta.get("kernel_source_sha") != kernel_source_sha()


def valu_roofline(key, chains, kern_ms, clock_ghz):
    """VALU-issue roofline of an LDS-resident launch: per-class instruction counts (committed PMC passes,
    profiles/valu_issue.json, scaled to `chains`) x issue cycles per class.  `frac` prices every instruction at its
    ARCHITECTED issue cost (MI355X_MICROARCH.md: a SIMD-32 issues a 32-bit wave64 instruction in 2 cycles, fp64 at
    half rate in 4, a transcendental in 8); `frac_vs_measured_streams` at what pure streams of one instruction
    class reach on this GPU with four waves per SIMD (profiles/valu_calibration.json, first start to last end of a
    launch: fp64 4.5, 32-bit 2.5-2.9, transcendental 8.4 cycles)."""
    rec = (_load_json("valu_issue.json") or {}).get(key)
    cal = _load_json("valu_calibration.json")
    if not rec or not cal or not (clock_ghz == clock_ghz):
        return None
    arch = cal["architected_cycles_per_wave_instruction"]
    meas = cal["measured_cycles_per_wave_instruction_at_4_waves_per_simd"]
    scale = float(chains) / rec["chains"]
    cls = rec["classes"]
    f64 = (cls["ADD_F64"] + cls["MUL_F64"] + cls["FMA_F64"]) * scale
    tr64 = cls["TRANS_F64"] * scale
    tr32 = cls["TRANS_F32"] * scale
    total = cls["VALU"] * scale
    other = total - f64 - tr64 - tr32

    def cycles(cost):
        return f64 * cost["f64"] + tr64 * cost["trans_f64"] + tr32 * cost["trans_f32"] + other * cost["b32"]
    peak = N_SIMD * clock_ghz                               # G issue-cycles per second available
    achieved = cycles(arch) / (kern_ms * 1e-3) / 1e9        # G issue-cycles per second delivered, architected costs
    return dict(achieved=achieved, peak=peak, frac=achieved / peak,
                frac_vs_measured_streams=cycles(meas) / (kern_ms * 1e-3) / 1e9 / peak,
                valu_instructions_per_launch=total, fp64_arith_instructions_per_launch=f64,
                issue_cycle_model=arch, measured_stream_costs=meas, counters_from="profiles/valu_issue.json:" + key,
                in_kernel_clock_ghz=clock_ghz)


def lds_roofline(key, chains, kern_ms, clock_ghz):
    """LDS-array utilisation of an LDS-resident launch: SQ_LDS_IDX_ACTIVE (every cycle the LDS array of a CU works,
    bank-conflict cycles included; committed PMC pass, profiles/lds_activity.json, scaled to `chains`) against the
    256 CUs x clock cycles the launch had."""
    rec = (_load_json("lds_activity.json") or {}).get(key)
    if not rec or not (clock_ghz == clock_ghz):
        return None
    scale = float(chains) / rec["chains"]
    active = rec["SQ_LDS_IDX_ACTIVE"] * scale
    conflict = rec["SQ_LDS_BANK_CONFLICT"] * scale
    peak = N_CU * clock_ghz                                  # G LDS-array cycles per second available
    achieved = active / (kern_ms * 1e-3) / 1e9
    return dict(achieved=achieved, peak=peak, frac=achieved / peak, bank_conflict_share=conflict / active,
                frac_conflict_free=(active - conflict) / (kern_ms * 1e-3) / 1e9 / peak,
                lds_array_cycles_per_launch=active, counters_from="profiles/lds_activity.json:" + key)


def replay_arithmetic_leg(w, dev_index, C=None, reps=3):
    """Throughput of the REPLAY-arithmetic kernel (reference operation order, fp64 CDF in the reference's index order,
    -ffp-contract=off) on device-resident pre-generated streams: the cost of parity-pinned arithmetic, on record -- for
    every config: full sequences (c1, c2, c4) and buffered windows (c3, c5: the windows of the ensemble's first step).
    N <= 1024 runs the LDS-resident REPLAY instantiation, larger N pf_mem_kernel ("mem1024")."""
    import torch
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    N = w["N"]
    Tw = w["window_T"]
    if C is None:
        # as many windows as 24 GB of fp64 streams hold (2 x 8 B per particle-step), at most 768 (c2's historical figure)
        C = int(max(32, min(768, (24 << 30) // (16 * Tw * N))))
    ens = ChainEnsemble(w["model"], w["y"], w["p0"], num_chains=C, N=N, pf="poyiadjis_N", kernel=w["kernel"],
                        epsilon=w["epsilon"], prior=w["prior"], subsequence_length=w["S"], buffer_length=w["B"], seed=5,
                        chain_offset=2 * 10 ** 6, device=dev_index)
    dev = ens.device
    d = ens._desc
    Tmax = int(d["T"].max())
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    z0 = torch.randn((C, N), dtype=torch.float64, device=dev, generator=gen)
    u = torch.rand((C, Tmax, N), dtype=torch.float64, device=dev, generator=gen)
    z = torch.randn((C, Tmax, N), dtype=torch.float64, device=dev, generator=gen)
    idx = np.arange(C, dtype=np.uint64)
    d["z0"] = z0.data_ptr() + idx * np.uint64(8 * N)
    d["u"] = u.data_ptr() + idx * np.uint64(8 * Tmax * N)
    d["z"] = z.data_ptr() + idx * np.uint64(8 * Tmax * N)
    sb = ens.ctx.scratch_bytes(ens.model, ens.dtype, "replay", N)     # the REPLAY kernel of this N may keep its state in HBM
    if sb > 0:                                                         # where the ensemble's device-generator kernel does not
        scratch = torch.empty(C * sb, dtype=torch.uint8, device=dev)
        d["scratch"] = scratch.data_ptr() + idx * np.uint64(sb)
    ens.desc_dev.copy_(torch.from_numpy(d.view(np.uint8).reshape(C, -1)))
    st = torch.cuda.current_stream(dev)

    def launch():
        # every window is the Poyiadjis O(N) score: the launch says so (PFG_SMOOTHER_POYIADJIS_N), as pfg_run_batch does for
        # such a batch -- units with a score-only twin run it (bitwise the general kernel's numbers in the REPLAY units)
        ens.ctx.launch_device_smoother(ens.model, ens.kernel, ens.dtype, "replay", "poyiadjis_n", N, C, ens.desc_dev.data_ptr(),
                                       st.cuda_stream)

    launch()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st); launch(); b.record(st)
        torch.cuda.synchronize(dev)
        ms.append(a.elapsed_time(b))
    g, _ = ens.last_gradient_statistics()
    if not np.all(np.isfinite(g)):
        raise SystemExit("non-finite gradients in the replay-arithmetic leg")
    k = float(np.median(ms))
    n, h = STATE_STAT[w["model"]]
    psteps = float(d["T"].astype(np.float64).sum()) * N
    variant = ens.ctx.last_variant()
    out = dict(value=C / (k * 1e-3), unit="SGLD steps/s (PF launch only)", chains=C, kernel_ms=k, kernel_variant=variant,
               particle_steps_per_s=psteps / (k * 1e-3),
               note="REPLAY instantiation on device-resident pre-generated fp64 streams (torch generator; the host "
                    "MT19937 stream of the drop-in path is excluded): the arithmetic the reference fixtures pin")
    if variant.startswith("mem"):
        # state and streams go through memory: 2 (n + 1 + h) 8 B of state + 16 B of replayed draws per particle-step
        alg = psteps * (2 * (n + 1 + h) * 8 + 16)
        out["hbm_model"] = dict(algorithmic_bytes_per_launch=alg, algorithmic_GBps=alg / (k * 1e-3) / 1e9,
                                frac_of_peak=alg / (k * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                note="2 (n + 1 + h) 8 B of particle state + 16 B of replayed u / z per particle-step")
    return out


# ------------------------------------------------------------------------------------------------
# multi-rank plumbing
# ------------------------------------------------------------------------------------------------
def spawn_ranks(n):
    """`--gpus n` without a launcher: start n ranks (one per GPU) as children of this process, which
    has not touched the GPU, and return their exit status."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def rank_epilogue(local_theta, elapsed, device=None):
    """What every rank does after its timed steps: max of the elapsed time over ranks, gather of
    the samples in global chain order.  Returns (elapsed_max, samples [world*C, P])."""
    from sgmcmc_ssm_amd import distributed
    elapsed = distributed.max_over_ranks(elapsed, device=device)
    samples = distributed.gather_samples(local_theta)
    return elapsed, samples


def gather_rows(local, device):
    """[C, X] float64 rows of every rank -> [world*C, X] ndarray in global chain order (a collective: every rank calls it)."""
    import torch
    from sgmcmc_ssm_amd import distributed
    t = torch.as_tensor(np.ascontiguousarray(local, dtype=np.float64), device=device)
    return distributed.gather_samples(t).cpu().numpy()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, **arrays):
    """--dump-outputs: each array as <path>/<name>.npy in float64.  All arrays share their leading (chain / window)
    axis; if together they exceed 64 MB, the same fixed, seeded sample of rows is kept from each."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    rows = len(next(iter(arrays.values())))
    total = sum(a.nbytes for a in arrays.values())
    keep = None
    if total > DUMP_LIMIT_BYTES:
        keep = np.sort(np.random.RandomState(0).choice(rows, size=int(rows * DUMP_LIMIT_BYTES // total), replace=False))
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a if keep is None else a[keep])


def cpu_rehearsal(args):
    """No GPU: the rank logic alone under gloo (spawn, chain ranges, barrier, max-over-ranks,
    gather in global chain order) with ChainEnsemble-shaped [C, P] tensors."""
    import torch
    from sgmcmc_ssm_amd import distributed
    rank, world, _ = distributed.init_from_env(backend="gloo")
    C, P = args.chains_per_gpu or 8, 3
    lo, hi = distributed.chain_range(rank, C)
    theta = torch.arange(lo, hi, dtype=torch.float64).reshape(C, 1) * torch.ones((1, P), dtype=torch.float64)
    distributed.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    elapsed, samples = rank_epilogue(theta, time.perf_counter() - t0)
    ok = bool(torch.equal(samples[:, 0], torch.arange(world * C, dtype=torch.float64)))
    if rank == 0:
        print(json.dumps({"rehearsal": "cpu-gloo", "ranks": world, "n_gpus": 0, "chains_total": world * C,
                          "gathered_in_global_chain_order": ok, "elapsed_max_s": elapsed}), flush=True)
    distributed.barrier()
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: ~6.5 s of timed GPU work on the headline config (54 ms per step), long enough for a 5-s utilisation
    # sampler beside the run to see it; the whole default run still ends within a minute
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--chains-per-gpu", type=int, default=0, help="0 = the config's default")
    ap.add_argument("--model", default=None, choices=["svm", "garch"], help="(compat) svm = c2, garch = c3")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--sampler", default="sgld", choices=["sgld", "sghmc"],
                    help="sghmc: the extension BASELINE configs[4] names (momentum update, friction 0.1); same PF launch")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-single-chain", action="store_true",
                    help="skip the one-chain-alone latency, replay-arithmetic and parity legs (profiling runs: keeps every "
                         "launch of the PF kernel the same size, so rocprofv3's per-kernel average is the launch time)")
    ap.add_argument("--cpu-budget", type=float, default=12.0)
    ap.add_argument("--rehearsal", action="store_true",
                    help="allow more ranks than GPUs (ranks fold onto devices; the line is labelled, n_gpus = distinct devices)")
    ap.add_argument("--cpu-rehearsal", action="store_true", help="no GPU: exercise the multi-rank logic under gloo")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beside the headline figure: one chain alone, replay arithmetic, parity, CPU "
                         "baseline, g1's per-timestep kernel times and roofline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's theta / grad / loglik as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.model is not None:
        args.config = {"svm": "c2", "garch": "c3"}[args.model]

    # ---- launcher: nothing above or below this block has touched the GPU yet ---------------------
    env_world = int(os.environ.get("WORLD_SIZE", "0") or 0)
    if args.gpus > 1 and env_world == 0:
        sys.exit(spawn_ranks(args.gpus))
    if env_world > 0 and env_world != args.gpus:
        raise SystemExit("--gpus {0} but WORLD_SIZE={1}".format(args.gpus, env_world))

    os.environ.setdefault("OMP_NUM_THREADS", "1")
    if args.cpu_rehearsal:
        sys.exit(cpu_rehearsal(args))
    import torch
    from sgmcmc_ssm_amd import distributed
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    ndev = torch.cuda.device_count()
    world_env = max(env_world, 1)
    if world_env > ndev and not args.rehearsal:
        raise SystemExit("--gpus {0} but only {1} GPU(s) visible: ranks would share devices "
                         "(pass --rehearsal to fold them; the line is then labelled)".format(world_env, ndev))
    if world_env > ndev:
        # ranks folded onto fewer devices (--rehearsal): RCCL refuses two ranks on one GPU, the rendezvous runs on gloo
        os.environ.setdefault("PFG_DIST_BACKEND", "gloo")
    rank, world, local_rank = distributed.init_from_env()
    dev_index = local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    n_distinct = min(world, ndev)

    if args.config.startswith("g"):
        run_giant(args, rank, world, dev_index, n_distinct)
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return
    w = config_workload(args.config)
    model = w["model"]
    C = args.chains_per_gpu or w["chains"]
    lo, _ = distributed.chain_range(rank, C)

    def make_ensemble(chains, seed, offset):
        return ChainEnsemble(model, w["y"], w["p0"], num_chains=chains, N=w["N"], pf="poyiadjis_N", kernel=w["kernel"],
                             epsilon=w["epsilon"], prior=w["prior"], subsequence_length=w["S"], buffer_length=w["B"],
                             dtype=args.dtype, seed=seed, chain_offset=offset, device=dev_index,
                             sampler=args.sampler, friction=0.1,
                             # buffered windows of ONE series are drawn on the device (no host work per step);
                             # sequence lists (c5) still sample on the host
                             window_sampling=("device" if w["S"] != -1 and not isinstance(w["y"], list) else "host"))

    ens = make_ensemble(C, 2024, lo)
    ens.enable_stamps()
    for _ in range(args.warmup):
        ens.step(1)
    torch.cuda.synchronize(dev)
    distributed.barrier()
    torch.cuda.synchronize(dev)

    # K timed steps; HIP events (torch.cuda.Event on the launch stream) bracket each PF launch
    stream = torch.cuda.current_stream(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.steps)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        if ens.window_sampling == "device":
            ens.launch_windows(stream)
        elif ens.steps_done > 0 and ens._set_windows():
            ens.desc_dev.copy_(torch.from_numpy(ens._desc.view(np.uint8).reshape(ens.C, -1)), non_blocking=True)
        ev[k][0].record(stream)
        ens.launch_pf(stream)
        ev[k][1].record(stream)
        ens.launch_update(stream)
        ens.steps_done += 1
    torch.cuda.synchronize(dev)
    distributed.barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    # the one collective (RCCL all_gather of the samples) + max over ranks, outside the timing
    elapsed, samples = rank_epilogue(ens.theta_dev[:, :ens.P].contiguous(), elapsed, device=dev)
    torch.cuda.synchronize(dev)
    theta = samples.cpu().numpy()
    if not np.all(np.isfinite(theta)) and not os.environ.get("PFG_BENCH_KNOCKOUT"):
        # (PFG_BENCH_KNOCKOUT: timing / counter runs of knock-out builds that are no valid samplers, tools/lds_split.sh)
        raise SystemExit("non-finite parameters after the run")
    if args.dump_outputs:
        grad, loglik = ens.last_gradient_statistics()
        out = gather_rows(np.concatenate([grad, loglik[:, None]], axis=1), dev)
        if rank == 0:
            dump_outputs(args.dump_outputs, theta=theta, grad=out[:, :-1], loglik=out[:, -1])

    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    variant = ens.ctx.last_variant()                      # the PF kernel the timed launches ran
    clock_ghz, wg_cycles, _ = ens.kernel_clock()          # stamps of the last timed launch

    # latency of ONE chain alone on the GPU (the reference's unit: one chain, one step at a time)
    single = None
    if rank == 0 and args.full and not args.no_single_chain:
        one = make_ensemble(1, 7, 10 ** 6)
        one.step(2)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        one.step(5)
        torch.cuda.synchronize(dev)
        single = 5.0 / (time.perf_counter() - t1)
        del one
    n, h = STATE_STAT[model]
    wsize = 8 if args.dtype == "f64" else 4
    bytes_per_pt = 2 * (n + 1 + h) * wsize
    alg_bytes = float(C) * w["window_T"] * w["N"] * bytes_per_pt        # per launch
    alg_gbs = alg_bytes / (kern_ms * 1e-3) / 1e9
    key = "{0}_{1}_{2}".format(args.config, args.dtype, variant)
    trec = (_load_json("hbm_traffic.json") or {}).get(key)
    traffic = trec["bytes_per_launch"] * (float(C) / trec["chains"]) if trec else None

    if rank == 0:
        total_steps = float(C) * world * args.steps
        streams_state = variant is not None and variant.startswith(("big", "mem"))
        hbm_model = {"algorithmic_bytes_per_launch": alg_bytes, "algorithmic_GBps": alg_gbs, "peak_GBps": HBM_PEAK_GBS,
                     "ratio_to_peak": alg_gbs / HBM_PEAK_GBS, "binding": bool(streams_state),
                     "note": "SURVEY 8(d) model: 2*(n+1+h)*{0} B per particle-timestep as if particle state were streamed "
                             "through HBM every timestep".format(wsize)}
        if streams_state:
            roof = {"bound": "hbm", "achieved": alg_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg_gbs / HBM_PEAK_GBS,
                    "traffic": traffic, "kernel_ms": kern_ms, "in_kernel_clock_ghz": clock_ghz,
                    "note": "large-N kernel: particle records live in a per-window HBM scratch (L2 / Infinity-Cache "
                            "resident while it fits); the algorithmic bytes are real memory-system traffic"}
        else:
            vr = valu_roofline(key, C, kern_ms, clock_ghz)
            lr = lds_roofline(key, C, kern_ms, clock_ghz)
            # `bound` / `frac`: the pipe with the highest USEFUL utilisation -- VALU issue at architected costs against the
            # LDS array's conflict-free cycles (a bank-conflict replay is a busy cycle, not achieved work: VERDICT r3
            # weak 9).  The busier pipe INCLUDING conflict cycles is reported beside it (`busiest_pipe`): that is what a
            # timestep queues on.
            lds_useful = lr["frac_conflict_free"] if lr else None
            lds_binds = bool(lr and vr and lds_useful > vr["frac"])
            top = lr if lds_binds else vr
            roof = {"bound": "lds" if lds_binds else "valu", "achieved": (top["achieved"] if not lds_binds else lr["achieved"] * (1.0 - lr["bank_conflict_share"])) if top else None,
                    "peak": top["peak"] if top else None,
                    "unit": "G conflict-free LDS-array cycles/s" if lds_binds else "G VALU issue-cycles/s",
                    "frac": (lds_useful if lds_binds else vr["frac"]) if top else None,
                    "busiest_pipe": ("lds" if lr["frac"] > vr["frac"] else "valu") if (lr and vr) else None,
                    "busiest_pipe_busy_frac": max(lr["frac"], vr["frac"]) if (lr and vr) else None,
                    "lds_frac_conflict_free": lds_useful,
                    "traffic": traffic, "kernel_ms": kern_ms, "in_kernel_clock_ghz": clock_ghz, "valu": vr, "lds": lr,
                    "hbm_model": hbm_model,
                    "note": "particle state is LDS-resident: HBM bounds nothing here (traffic = measured bytes per launch, "
                            "register spills and descriptors).  Every timestep goes through two pipes, both reported: VALU issue "
                            "(per-class instruction counts x architected issue cycles / (1024 SIMDs x clock)) and the LDS "
                            "array (SQ_LDS_IDX_ACTIVE / (256 CUs x clock); `frac` counts its conflict-free cycles only, "
                            "`busiest_pipe_busy_frac` includes bank-conflict replays).  Counters are committed PMC passes of "
                            "this workload scaled by the chain count, time and clock are live"}
        roof["stale"] = profile_is_stale()
        if roof["stale"]:
            roof["stale_note"] = ("the kernel sources differ from the ones profiles/*.json were measured on (profile_meta.json: "
                                  "kernel_source_sha): instruction / LDS counters and traffic are those of an older kernel")
        line = {
            "metric": ("SGLD steps/sec (T=1000, N=1000 particles)" if args.config == "c2"
                       else "SGLD steps/sec ({0})".format(args.config)),
            "value": total_steps / elapsed,
            "unit": "SGLD steps/s",
            "n_gpus": n_distinct,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": w["data"],
            "config": {
                "workload": w["desc"],
                "baseline_config": args.config,
                "chains_per_gpu": C,
                "chains_total": C * world,
                "rng": "device",
                "sampler": args.sampler + (" (extension: not in the reference, parity-unpinned)" if args.sampler == "sghmc" else ""),
                "rng_precision": RNG_PRECISION,
                "kernel_variant": variant,
                "parallelism": "independent chains, {0} rank(s) x {1} chains, RCCL all_gather of samples".format(world, C),
            },
            "per_chain_steps_per_s": args.steps / elapsed,
            "single_chain_alone_steps_per_s": single,
            "us_per_pf_timestep": kern_ms * 1e3 / w["window_T"],
            "roofline": roof,
        }
        if world != n_distinct:
            line["rehearsal"] = "{0} ranks folded onto {1} GPU(s): NOT a multi-GPU measurement".format(world, n_distinct)
        if args.full and world == 1 and not args.no_single_chain:
            if args.config == "c2":
                line["parity"] = grad_error_vs_reference()
            line["replay_arithmetic"] = replay_arithmetic_leg(w, dev_index)
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(w, budget_s=args.cpu_budget)
            line["speedup_vs_cpu_1core"] = line["value"] / line["cpu_baseline"]["value"]
            if single:
                line["single_chain_speedup_vs_cpu_1core"] = single / line["cpu_baseline"]["value"]
            if line["cpu_baseline"].get("all_cores_bound"):
                # the like-for-like node comparison: every host core running its own chain vs every CU doing so
                line["speedup_vs_cpu_all_cores_bound"] = line["value"] / line["cpu_baseline"]["all_cores_bound"]
        print(json.dumps(line), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
