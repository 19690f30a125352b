"""bench.py's plain run and --dump-outputs.  The line carries the headline fields and none of the --full legs.  The dumped
arrays are what a caller of the timed path receives: they equal an independent run of the same chains / windows through
the package API (ChainEnsemble.step, ResidentWindows.launch) for warmup + steps steps, under two different splits of
those steps, so --steps really sets the number of timed steps and two runs with the same arguments compute the same."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHAINS = {"c2": 96, "g1": 2}
FULL_LEGS = {"c2": ("cpu_baseline", "replay_arithmetic", "parity", "speedup_vs_cpu_1core"),
             "g1": ("cpu_baseline", "parity", "speedup_vs_cpu_1core", "roofline", "us_per_pf_timestep")}


def _bench(cfg, out_dir, warmup, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", cfg, "--steps", str(steps),
           "--warmup", str(warmup), "--chains-per-gpu", str(CHAINS[cfg]), "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return lines[0]


def _reference(cfg, total_steps):
    """The same chains (c2) / windows (g1) as bench.py builds them, total_steps steps through the package API."""
    import bench
    if cfg == "g1":
        from sgmcmc_ssm_amd.grid import ResidentWindows
        model, T_series, N, L, Bf, _, _ = bench.CONFIGS[cfg]
        p, y_all, _, wcfg = bench.make_workload(model, T_series)
        t0 = (T_series + L) // 2
        rw = ResidentWindows(model, y_all[t0 - Bf:t0 + L + Bf].reshape(-1), np.tile(p.theta(), (CHAINS[cfg], 1)), N,
                             kernel=wcfg["kernel"], pf="poyiadjis_N", t1=Bf, tL=Bf + L, prior_mean=0.0, prior_var=10.0,
                             dtype="f64", seed=2024, stream0=0, device=0)
        for _ in range(total_steps):
            rw.launch()
        grad, loglik = rw.results()
        return {"grad": grad, "loglik": loglik}
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    w = bench.config_workload(cfg)
    ens = ChainEnsemble(w["model"], w["y"], w["p0"], num_chains=CHAINS[cfg], N=w["N"], pf="poyiadjis_N", kernel=w["kernel"],
                        epsilon=w["epsilon"], prior=w["prior"], subsequence_length=w["S"], buffer_length=w["B"], dtype="f64",
                        seed=2024, chain_offset=0, device=0)
    ens.step(total_steps)
    grad, loglik = ens.last_gradient_statistics()
    return {"theta": ens.theta(), "grad": grad, "loglik": loglik}


@pytest.mark.parametrize("cfg", sorted(CHAINS))
def test_plain_run_dumps_what_the_timed_path_computes(cfg, tmp_path):
    ref = _reference(cfg, 4)
    for warmup, steps in ((1, 3), (2, 2)):
        out = tmp_path / "w{0}s{1}".format(warmup, steps)
        line = _bench(cfg, out, warmup, steps)
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == steps and line["warmup"] == warmup and line["dtype"] == "f64"
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
        assert line["config"]["chains_per_gpu"] == CHAINS[cfg]
        for key in FULL_LEGS[cfg]:
            assert key not in line, key                 # --full legs stay out of a plain run
        assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in ref)
        for name, r in ref.items():
            x = np.load(out / (name + ".npy"))
            assert x.dtype == np.float64 and x.shape == r.shape, (name, x.dtype, x.shape, r.shape)
            assert np.all(np.isfinite(x)), name
            # warmup + steps = 4 steps in both splits: equal to the 4-step reference only if --steps steps were timed
            assert np.array_equal(x, r), (name, warmup, steps, np.max(np.abs(x - r)))
