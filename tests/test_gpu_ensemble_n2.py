"""GPU: ChainEnsemble(pf='poyiadjis_N2') -- the Poyiadjis O(N^2) smoother as chains resident on the device (the SVM /
GARCH / LGSSM experiments' POYIADJIS_N2_100 row: N = 100, S = 40, buffer -1, T = 1000).  The ensemble runs the same
smoother kernel as a batch of device-generator windows, so one step is checked bitwise against ctx.run_batch; graph
replay and rank partitions against eager stepping; the multi-window path against the host reduction of its records."""
import numpy as np
import pytest

from test_host_logic import default_params, GEN
from test_gpu_ensemble_windows import _check_step

pytestmark = pytest.mark.gpu


def _series(model, T, seed=5):
    np.random.seed(seed)
    return GEN[model](T=T, parameters=default_params(model))["observations"]


@pytest.mark.parametrize("model,dtype", [("svm", "f64"), ("garch", "f64"), ("lgssm", "f32")])
def test_one_step_equals_run_batch(model, dtype):
    """Every chain's out record after one step is what ctx.run_batch computes for the same descriptors (device
    generator, the ensemble's seed, stream = global chain id, step 0), bit for bit."""
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    from sgmcmc_ssm_amd.particle_filters import make_problem
    T, C, N = 50, 96, 100
    y = _series(model, T)
    p = default_params(model)
    ens = ChainEnsemble(model, y, p, num_chains=C, N=N, pf="poyiadjis_N2", epsilon=1e-4, dtype=dtype, seed=21, chain_offset=7)
    ens.step(1)
    ens.synchronize()
    assert ens.ctx.last_variant() == "n2_64x2"
    g, ll = ens.last_gradient_statistics()
    d = ens._desc[0]
    assert int(d["smoother"]) == _capi.SMOOTHER["poyiadjis_n2"] and d["lambduh"] == 1.0
    assert ens.scratch_dev is None
    probs = [make_problem(model, ens.kernel, "poyiadjis_N2", y.reshape(-1), p.theta(), N, prior_mean=float(d["prior_mean"]),
                          prior_var=float(d["prior_var"]), flags=int(d["flags"]), dtype=dtype, seed=21, stream=7 + c,
                          rng="device")
             for c in range(C)]
    outs = ens.ctx.run_batch(probs)
    assert ens.ctx.last_variant() == "n2_64x2"
    np.testing.assert_array_equal(g, np.array([o["mean_stat"] for o in outs]))
    np.testing.assert_array_equal(ll, np.array([o["loglik"] for o in outs]))
    assert np.all(np.isfinite(g)) and len({tuple(r) for r in g}) == C


def test_graph_replay_equals_eager():
    """run(n, graph_steps=K) with device window sampling is bitwise the eager steps."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("svm", 200)
    p = default_params("svm")

    def make():
        return ChainEnsemble("svm", y, p, num_chains=128, N=100, pf="poyiadjis_N2", epsilon=1e-4, seed=4,
                             subsequence_length=20, buffer_length=10, window_sampling="device")
    a = make().run(6, thin=2, graph_steps=2)
    b = make().run(6, thin=2)
    assert np.all(np.isfinite(a))
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("windows", ["host", "device"])
def test_partitions_equal_one_ensemble(windows):
    """Two ensembles of C/2 chains at chain_offset 0 and C/2 are the ensemble of C chains, bit for bit.  (C = 256: each
    half keeps more than 64 windows per launch, so all three run n2_64x2.)"""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("garch", 150)
    p = default_params("garch")

    def run(offset, C):
        e = ChainEnsemble("garch", y, p, num_chains=C, N=100, pf="poyiadjis_N2", epsilon=1e-4, seed=13, chain_offset=offset,
                          subsequence_length=20, buffer_length=5, window_sampling=windows)
        e.step(3)
        e.synchronize()
        assert e.ctx.last_variant() == "n2_64x2"
        return e.theta()
    full = run(0, 256)
    np.testing.assert_array_equal(full[:128], run(0, 128))
    np.testing.assert_array_equal(full[128:], run(128, 128))


def test_multi_window_step_equals_host_reduction():
    """minibatch_size = 2: every window record and every chain's reduced record after one step equal ctx.run_batch of the
    device-written windows reduced on the host, bit for bit (tests/test_gpu_ensemble_windows.py's check)."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("svm")
    y = _series("svm", 200).reshape(-1)
    ens = ChainEnsemble("svm", y, p, num_chains=64, N=100, pf="poyiadjis_N2", epsilon=1e-4, seed=17, chain_offset=5,
                        subsequence_length=10, buffer_length=2, minibatch_size=2, window_sampling="device")
    assert ens._multi and ens.W == 2 and ens.scratch_dev is None
    variant, d, _, _ = _check_step(ens, y, p.theta(), "poyiadjis_N2", "f64")
    assert variant == "n2_64x2"
    assert np.all(d["stream"] == (np.repeat(np.arange(64), 2) + 5) * 2 + np.tile(np.arange(2), 64))


def test_multi_window_large_n():
    """N = 2000 on the multi-window path: n2_mem1024 with its state in the descriptors' scratch."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("svm")
    ens = ChainEnsemble("svm", _series("svm", 12).reshape(-1), p, num_chains=2, N=2000, pf="poyiadjis_N2", epsilon=1e-4,
                        seed=3, minibatch_size=1)
    assert ens._multi and ens.scratch_dev is not None
    assert ens.scratch_bytes_per_window == ens.ctx.scratch_bytes_smoother("svm", "f64", "device", "poyiadjis_n2", 2000) > 0
    ens.step(1)
    ens.synchronize()
    assert ens.ctx.last_variant() == "n2_mem1024"
    assert np.all(np.isfinite(ens.theta())) and np.all(np.isfinite(ens.last_gradient_statistics()[0]))


def test_sequence_lists_sghmc_and_sgrld():
    """Host window sampling over a list of sequences with SGHMC; LGSSM with the SGRLD update; run() samples."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("svm", 240).reshape(-1)
    ens = ChainEnsemble("svm", [y[:100], y[100:]], default_params("svm"), num_chains=80, N=64, pf="poyiadjis_N2", epsilon=1e-4,
                        seed=2, subsequence_length=16, buffer_length=4, sampler="sghmc")
    s = ens.run(4, thin=2)
    assert s.shape == (2, 80, 3) and np.all(np.isfinite(s))
    np.testing.assert_array_equal(s[-1], ens.theta())
    lg = ChainEnsemble("lgssm", _series("lgssm", 120), default_params("lgssm"), num_chains=80, N=100, pf="poyiadjis_N2",
                       epsilon=1e-4, seed=6, subsequence_length=16, buffer_length=4, sampler="sgrld", window_sampling="device")
    s = lg.run(4, thin=2)
    assert lg.ctx.last_variant() == "n2_64x2"
    assert s.shape == (2, 80, 4) and np.all(np.isfinite(s))
    np.testing.assert_array_equal(s[-1], lg.theta())
    st = lg.state_dict()
    lg.step(2)
    again = ChainEnsemble("lgssm", _series("lgssm", 120), default_params("lgssm"), num_chains=80, N=100, pf="poyiadjis_N2",
                          epsilon=1e-4, seed=6, subsequence_length=16, buffer_length=4, sampler="sgrld", window_sampling="device")
    again.load_state_dict(st)
    again.step(2)
    np.testing.assert_array_equal(lg.theta(), again.theta())


def test_poyiadjis_n2_100_configuration():
    """The POYIADJIS_N2_100 row at a test's size: 1024 chains, N = 100, S = 40, buffer -1, T = 200, device window
    sampling and graph replay."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    T = 200
    y = _series("svm", T, seed=8)
    ens = ChainEnsemble("svm", y, default_params("svm"), num_chains=1024, N=100, pf="poyiadjis_N2", epsilon=0.1 / T,
                        subsequence_length=40, buffer_length=-1, window_sampling="device", seed=3)
    s = ens.run(4, thin=2, graph_steps=2)
    assert ens.ctx.last_variant() == "n2_64x2"
    assert s.shape == (2, 1024, ens.P) and np.all(np.isfinite(s))
    assert len({tuple(r) for r in s[-1][:512]}) == 512


def test_refusals():
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("svm", 40)
    p = default_params("svm")
    with pytest.raises(NotImplementedError, match="N <= 1024"):
        ChainEnsemble("svm", y, p, num_chains=4, N=2000, pf="poyiadjis_N2")
    with pytest.raises(ValueError, match="multinomial"):
        ChainEnsemble("svm", y, p, num_chains=4, N=100, pf="poyiadjis_N2", resampling="stratified")
    with pytest.raises(ValueError, match="kind='pf'"):
        ChainEnsemble("lgssm", _series("lgssm", 40), default_params("lgssm"), num_chains=4, pf="poyiadjis_N2", kind="marginal")
