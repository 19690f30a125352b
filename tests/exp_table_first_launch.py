"""Child process of tests/test_gpu_exp_table.py: the FIRST launch of the SVM 256 x 4 kernel in a process -- the one that
fills the exp table in device memory (csrc/pfg_launch.hpp, ensure_exp_tab_mem) -- and launches behind it.

    python tests/exp_table_first_launch.py ctx|default N

  ctx      the first launch is a pfg_run_batch on a fresh context's own (non-default, non-blocking) stream, twice more on
           that context, then once on a second fresh context; then pfg_launch_device on HIP's default stream;
  default  the first launch is a pfg_launch_device on HIP's default stream, then the same on a side stream, then a
           pfg_run_batch on a fresh context.

Prints one JSON line: {"batch": [hex of mean_stat + loglik per run_batch call], "device": [hex of the out record per
pfg_launch_device call], "variant": [...]}.  Every entry of "batch" must be the same string in both modes and in the
parent, likewise "device"."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

T = 24
THETA_SVM = [0.9, 1.2, 1.1]


def problem(N):
    y = np.random.RandomState(N).normal(size=T)
    return dict(model="svm", kernel="prior", smoother="nemeth", stat="score", dtype="f64", rng="device", N=N, t1=0, tL=T,
                lambduh=1.0, prior_mean=0.0, prior_var=10.0, y=y, theta=THETA_SVM, seed=11 + N, stream=T)


def batch_hex(ctx, q):
    o = ctx.run_batch([dict(q)])[0]
    return np.concatenate([np.asarray(o["mean_stat"], dtype=np.float64).reshape(-1), [o["loglik"]]]).tobytes().hex(), ctx.last_variant()


def device_hex(ctx, q, side):
    """the same window through pfg_launch_device: a descriptor in device memory, on HIP's default stream or a side stream"""
    import torch
    from sgmcmc_ssm_amd import _capi
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(dev)
    yd, thd = t(q["y"]), t(list(q["theta"]) + [0.0] * (_capi.MAX_THETA - len(q["theta"])))
    out = torch.zeros(_capi.OUT_DOUBLES, dtype=torch.float64, device=dev)
    d = np.zeros(1, dtype=_capi.DEV_PROBLEM_DTYPE)
    d["y"], d["theta"], d["out"] = yd.data_ptr(), thd.data_ptr(), out.data_ptr()
    d["prior_mean"], d["prior_var"], d["lambduh"] = q["prior_mean"], q["prior_var"], 1.0
    d["seed"], d["stream"] = q["seed"], q["stream"]
    d["T"], d["t1"], d["tL"], d["N"] = T, 0, T, q["N"]
    d["smoother"], d["stat"] = _capi.SMOOTHER["nemeth"], _capi.STAT["score"]
    desc = torch.from_numpy(d.view(np.uint8).reshape(1, -1)).to(dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev) if side else torch.cuda.current_stream(dev)
    ctx.launch_device("svm", "prior", "f64", "device", q["N"], 1, desc.data_ptr(), s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy().tobytes().hex(), ctx.last_variant()


def main(mode, N):
    os.environ["PFGRAD_VARIANT"] = "wg256x4s"       # (the child's own environment: the importing test sets it by monkeypatch)
    from sgmcmc_ssm_amd import _capi
    q = problem(N)
    batch, device = [], []
    if mode == "ctx":
        a = _capi.Context(0)
        batch += [batch_hex(a, q) for _ in range(3)]
        b = _capi.Context(0)
        batch.append(batch_hex(b, q))
        device.append(device_hex(b, q, side=False))
    else:
        a = _capi.Context(0)
        device.append(device_hex(a, q, side=False))
        device.append(device_hex(a, q, side=True))
        batch.append(batch_hex(_capi.Context(0), q))
    print(json.dumps({"batch": [h for h, _ in batch], "device": [h for h, _ in device],
                      "variant": sorted({v for _, v in batch + device})}))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
