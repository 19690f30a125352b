"""GPU: ChainEnsemble(pf='paris') -- PaRIS chains resident on the device (the SVM / GARCH experiments' PARIS_100 row:
N = 100, Ntilde = 2, S = 40, buffer -1, SGLD, T = 1000).  The ensemble runs the same smoother kernel as a batch of
device-generator windows, so one step is checked bitwise against ctx.run_batch; graph replay and rank partitions
against eager stepping."""
import numpy as np
import pytest

from test_host_logic import default_params, GEN

pytestmark = pytest.mark.gpu


def _series(model, T, seed=5):
    np.random.seed(seed)
    return GEN[model](T=T, parameters=default_params(model))["observations"]


@pytest.mark.parametrize("model,dtype,accept_reject", [pytest.param("svm", "f64", True, id="svm-f64"),
                                                       pytest.param("garch", "f64", True, id="garch-f64"),
                                                       pytest.param("lgssm", "f32", True, id="lgssm-f32"),
                                                       pytest.param("svm", "f64", False, id="svm-f64-exact")])
def test_one_step_equals_run_batch(model, dtype, accept_reject):
    """Every chain's out record after one step is what ctx.run_batch computes for the same descriptors (device
    generator, the ensemble's seed, stream = global chain id, step 0), bit for bit.  accept_reject=False: no
    accept-reject round, every backward draw of every child is the device's exact categorical draw
    (max_accept_reject = 0; what that draw returns is checked in tests/test_gpu_paris_device_replay.py)."""
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    from sgmcmc_ssm_amd.particle_filters import make_problem
    T, C, N = 50, 96, 100
    y = _series(model, T)
    p = default_params(model)
    ens = ChainEnsemble(model, y, p, num_chains=C, N=N, pf="paris", epsilon=1e-4, dtype=dtype, seed=21, chain_offset=7,
                        accept_reject=accept_reject)
    ens.step(1)
    ens.synchronize()
    assert ens.ctx.last_variant() == "paris64x2"
    g, ll = ens.last_gradient_statistics()
    d = ens._desc[0]
    assert int(d["smoother"]) == _capi.SMOOTHER["paris"] and d["lambduh"] == 1.0
    assert int(d["Ntilde"]) == 2 and int(d["max_accept_reject"]) == (64 if accept_reject else 0)
    probs = [make_problem(model, ens.kernel, "paris", y.reshape(-1), p.theta(), N, prior_mean=float(d["prior_mean"]),
                          prior_var=float(d["prior_var"]), flags=int(d["flags"]), dtype=dtype, seed=21, stream=7 + c,
                          rng="device", accept_reject=accept_reject)
             for c in range(C)]
    assert probs[0]["max_accept_reject"] == (64 if accept_reject else 0) and int(probs[0].get("flags", 0)) == int(d["flags"])
    outs = ens.ctx.run_batch(probs)
    assert ens.ctx.last_variant() == "paris64x2"
    np.testing.assert_array_equal(g, np.array([o["mean_stat"] for o in outs]))
    np.testing.assert_array_equal(ll, np.array([o["loglik"] for o in outs]))
    assert np.all(np.isfinite(g)) and len({tuple(r) for r in g}) == C


def test_graph_replay_equals_eager():
    """run(n, graph_steps=K) with device window sampling is bitwise the eager steps."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("svm", 200)
    p = default_params("svm")

    def make():
        return ChainEnsemble("svm", y, p, num_chains=128, N=100, pf="paris", epsilon=1e-4, seed=4,
                             subsequence_length=20, buffer_length=10, window_sampling="device")
    a = make().run(6, thin=2, graph_steps=2)
    b = make().run(6, thin=2)
    assert np.all(np.isfinite(a))
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("windows", ["host", "device"])
def test_partitions_equal_one_ensemble(windows):
    """Two ensembles of C/2 chains at chain_offset 0 and C/2 are the ensemble of C chains, bit for bit.  (C = 256: each
    half keeps more than 64 windows per launch, so all three run paris64x2.)"""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("garch", 150)
    p = default_params("garch")

    def run(offset, C):
        e = ChainEnsemble("garch", y, p, num_chains=C, N=100, pf="paris", epsilon=1e-4, seed=13, chain_offset=offset,
                          subsequence_length=20, buffer_length=5, window_sampling=windows)
        e.step(3)
        e.synchronize()
        assert e.ctx.last_variant() == "paris64x2"
        return e.theta()
    full = run(0, 256)
    np.testing.assert_array_equal(full[:128], run(0, 128))
    np.testing.assert_array_equal(full[128:], run(128, 128))


def test_sequence_lists_and_samples():
    """Host window sampling over a list of sequences, SGHMC, run() samples."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("svm", 240).reshape(-1)
    p = default_params("svm")
    ens = ChainEnsemble("svm", [y[:100], y[100:]], p, num_chains=80, N=64, pf="paris", Ntilde=3, epsilon=1e-4, seed=2,
                        subsequence_length=16, buffer_length=4, sampler="sghmc")
    s = ens.run(4, thin=2)
    assert s.shape == (2, 80, 3) and np.all(np.isfinite(s))
    np.testing.assert_array_equal(s[-1], ens.theta())


@pytest.mark.parametrize("model,epsilon", [("svm", 0.1), ("garch", 0.01)])
def test_paris_100_configuration(model, epsilon):
    """The PARIS_100 rows as ensembles: 12288 chains, N = 100, Ntilde = 2, S = 40, buffer -1, T = 1000, device
    window sampling and graph replay; then SGHMC and f32 on the same row."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    T = 1000
    y = _series(model, T, seed=8)
    p = default_params(model)
    kw = dict(N=100, pf="paris", Ntilde=2, epsilon=epsilon / T, subsequence_length=40, buffer_length=-1,
              window_sampling="device", seed=3)
    ens = ChainEnsemble(model, y, p, num_chains=12288, **kw)
    s = ens.run(4, thin=2, graph_steps=2)
    assert ens.ctx.last_variant() == "paris64x2"
    assert s.shape == (2, 12288, ens.P) and np.all(np.isfinite(s))
    assert len({tuple(r) for r in s[-1][:512]}) == 512
    for extra in (dict(sampler="sghmc"), dict(dtype="f32")):
        e = ChainEnsemble(model, y, p, num_chains=1024, **dict(kw, **extra))
        e.step(2)
        assert np.all(np.isfinite(e.theta()))


def test_refusals():
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("svm", 40)
    p = default_params("svm")
    with pytest.raises(NotImplementedError, match="N <= 1024"):
        ChainEnsemble("svm", y, p, num_chains=4, N=2000, pf="paris")
    with pytest.raises(ValueError, match="multinomial"):
        ChainEnsemble("svm", y, p, num_chains=4, N=100, pf="paris", resampling="systematic")
    with pytest.raises(ValueError, match="kind='pf'"):
        ChainEnsemble("lgssm", _series("lgssm", 40), default_params("lgssm"), num_chains=4, pf="paris", kind="marginal")
    e = ChainEnsemble("svm", y, p, num_chains=4, N=100, pf="paris", accept_reject=False)
    assert int(e._desc[0]["max_accept_reject"]) == 0
    e = ChainEnsemble("svm", y, p, num_chains=4, N=100, pf="paris", max_accept_reject=9, Ntilde=5)
    assert int(e._desc[0]["max_accept_reject"]) == 9 and int(e._desc[0]["Ntilde"]) == 5
