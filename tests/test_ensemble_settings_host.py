"""CPU: ChainEnsemble._resolve_settings, the device-free resolution of the constructor's arguments.

The refusals are the argument sets of the GPU refusal tests (test_refusals of test_gpu_ensemble_windows.py and
test_gpu_ensemble_paris.py, test_strict_partition_needs_divisible_length, test_sgrld_refused_off_lgssm,
test_ensemble_refuses_other_models_and_dtypes) with the same exception types and messages: those keep running through the
constructor on the GPU, these run wherever the package imports."""
import numpy as np
import pytest

from sgmcmc_ssm_amd import _capi
from sgmcmc_ssm_amd.ensemble import ChainEnsemble
from test_host_logic import default_params

resolve = ChainEnsemble._resolve_settings
Y60, Y40, Y100 = np.zeros(60), np.zeros(40), np.zeros(100)
SEGS = [np.zeros(20), np.zeros(30), np.zeros(10)]
SVM, LG = default_params("svm"), default_params("lgssm")

REFUSALS = [
    # test_gpu_ensemble_windows.py::test_refusals
    (NotImplementedError, "gibbs", ("lgssm", Y40, LG), dict(num_chains=4, sampler="gibbs", minibatch_size=2)),
    (NotImplementedError, "kind='pf' only",
     ("lgssm", Y40, LG), dict(num_chains=4, kind="marginal", minibatch_size=2, subsequence_length=10)),
    (NotImplementedError, "window_sampling='device'",
     ("svm", Y60, SVM), dict(num_chains=4, N=64, minibatch_size=2, subsequence_length=10, buffer_length=2)),
    (NotImplementedError, "window_sampling='device'", ("svm", SEGS, SVM), dict(num_chains=4, N=64, num_sequences=2)),
    (ValueError, "num_sequences", ("svm", SEGS, SVM), dict(num_chains=4, N=64, num_sequences=0, window_sampling="device")),
    (ValueError, "num_sequences", ("svm", SEGS, SVM), dict(num_chains=4, N=64, num_sequences=4, window_sampling="device")),
    (ValueError, "num_sequences", ("svm", SEGS, SVM), dict(num_chains=4, N=64, num_sequences=-2, window_sampling="device")),
    (ValueError, "num_sequences = 1", ("svm", Y60, SVM), dict(num_chains=4, N=64, num_sequences=2)),
    (NotImplementedError, "16384", ("svm", SEGS, SVM), dict(num_chains=2, N=20000, pf="paris", num_sequences=-1)),
    (NotImplementedError, "16384", ("svm", Y60, SVM), dict(num_chains=2, N=20000, minibatch_size=2)),
    (NotImplementedError, "N <= 1024", ("svm", Y60, SVM), dict(num_chains=4, N=2000, pf="paris")),
    # test_gpu_ensemble_paris.py::test_refusals
    (ValueError, "multinomial", ("svm", Y40, SVM), dict(num_chains=4, N=100, pf="paris", resampling="systematic")),
    (ValueError, "kind='pf'", ("lgssm", Y40, LG), dict(num_chains=4, pf="paris", kind="marginal")),
    # test_gpu_ensemble.py::test_strict_partition_needs_divisible_length
    (ValueError, "does not evenly divide",
     ("svm", Y100, SVM), dict(num_chains=4, N=64, subsequence_length=16, buffer_length=2, partition_style="strict")),
    # test_gpu_lgssm_grid_chains.py::test_sgrld_refused_off_lgssm
    (NotImplementedError, "No Default Preconditioner", ("svm", np.zeros(20), np.full((2, 3), 0.5)), dict(sampler="sgrld")),
    (NotImplementedError, "No Default Preconditioner", ("garch", np.zeros(20), np.full((2, 4), 0.5)), dict(sampler="sgrld")),
    # test_gpu_ffbs.py::test_ensemble_refuses_other_models_and_dtypes
    (NotImplementedError, None, ("svm", np.zeros(50), SVM), dict(num_chains=2, kind="complete", num_samples=10)),
    (NotImplementedError, None, ("lgssm", np.zeros(50), LG), dict(num_chains=2, kind="complete", num_samples=10, dtype="f32")),
    (ValueError, None, ("lgssm", np.zeros(50), LG), dict(num_chains=2, kind="complete")),
    # the other refusals the constructor states before it allocates
    (NotImplementedError, "systematic resampling is built for N <= 1024",
     ("svm", Y40, SVM), dict(num_chains=2, N=2000, resampling="systematic")),
    (NotImplementedError, "Gibbs over lists", ("lgssm", SEGS, LG), dict(num_chains=2, sampler="gibbs")),
    (NotImplementedError, "whole series", ("lgssm", Y40, LG), dict(num_chains=2, sampler="gibbs", subsequence_length=8)),
    (NotImplementedError, "host-side window sampling", ("svm", SEGS, SVM), dict(num_chains=2, window_sampling="device")),
    (ValueError, "window_sampling must be", ("svm", Y40, SVM), dict(num_chains=2, window_sampling="gpu")),
    (ValueError, "does not evenly divide T 20", ("svm", SEGS, SVM),
     dict(num_chains=2, N=64, num_sequences=1, subsequence_length=8, partition_style="strict", window_sampling="device")),
    (ValueError, "num_chains is required", ("svm", Y40, SVM), dict()),
    (ValueError, "Ntilde >= 1", ("svm", Y40, SVM), dict(num_chains=2, N=64, pf="paris", Ntilde=0)),
]


@pytest.mark.parametrize("exc, match, args, kw", REFUSALS)
def test_refusals_need_no_device(exc, match, args, kw):
    with pytest.raises(exc, match=match):
        resolve(*args, **kw)


def test_resolved_values():
    s = resolve("lgssm", Y40, LG, num_chains=3, sampler="gibbs", N=500, pf="nemeth")
    assert (s.kind, s.N, s.stat, s.smoother, s.launch_smoother, s.multi) == ("complete", 1, "gibbs", "kalman_ffbs",
                                                                            "kalman_ffbs", False)
    s = resolve("lgssm", Y40, LG, num_chains=3, kind="complete", num_samples=7, N=500)
    assert (s.N, s.stat, s.smoother, s.lambduh) == (7, "score", "kalman_ffbs", 1.0)
    s = resolve("lgssm", Y40, LG, num_chains=3, kind="marginal")
    assert (s.smoother, s.launch_smoother) == ("kalman", "kalman")
    s = resolve("svm", Y40, SVM, num_chains=3, pf="poyiadjis_N")
    assert (s.smoother, s.launch_smoother, s.lambduh, s.N, s.paris) == ("nemeth", "poyiadjis_n", 1.0, 1000, {})
    s = resolve("svm", Y40, SVM, num_chains=3, pf="nemeth")
    assert (s.smoother, s.launch_smoother, s.lambduh) == ("nemeth", "nemeth", 0.95)
    s = resolve("svm", Y40, SVM, num_chains=3, pf="nemeth", lambduh=1.0)
    assert (s.smoother, s.launch_smoother) == ("nemeth", "poyiadjis_n")
    s = resolve("svm", Y40, SVM, num_chains=3, resampling="systematic")
    assert (s.smoother, s.launch_smoother, s.lambduh) == ("nemeth_systematic", "nemeth_systematic", 1.0)
    s = resolve("svm", Y40, SVM, num_chains=3, N=100, pf="paris", max_accept_reject=9, Ntilde=5)
    assert (s.smoother, s.launch_smoother, s.paris) == ("paris", "paris", dict(Ntilde=5, max_accept_reject=9))
    assert resolve("svm", Y40, SVM, num_chains=3, N=100, pf="paris", accept_reject=False).paris["max_accept_reject"] == 0
    assert resolve("svm", Y40, SVM, num_chains=3, N=100, pf="paris").paris["max_accept_reject"] == 64


def test_resolved_windows():
    s = resolve("svm", Y40, SVM, num_chains=3, subsequence_length=40, buffer_length=-1)          # S >= T: the full series
    assert (s.S, s.B, s.T, s.segments, s.strict, s.multi, s.W) == (-1, 40, 40, None, False, False, 1)
    assert resolve("svm", Y40, SVM, num_chains=3, subsequence_length=50).S == -1
    s = resolve("svm", Y40, SVM, num_chains=3, subsequence_length=8, buffer_length=2, partition_style="strict")
    assert (s.S, s.B, s.strict) == (8, 2, True)
    np.testing.assert_array_equal(s.bounds, [0, 40])
    # a single-window list: S = -1 means whole sequences, S = the longest one; strict asks for no divisibility there
    s = resolve("svm", SEGS, SVM, num_chains=3, buffer_length=4, partition_style="strict")
    assert (s.S, s.B, s.T, s.multi, s.draws) == (30, 4, 60, False, None)
    np.testing.assert_array_equal(s.segments, [0, 20, 50, 60])
    # the multi-window path
    s = resolve("svm", SEGS, SVM, num_chains=2, N=64, num_sequences=-1, subsequence_length=-1, buffer_length=0)
    assert (s.M, s.K, s.W, s.multi, s.draws, s.rescale, s.S) == (1, -1, 3, True, False, False, -1)
    s = resolve("svm", SEGS, SVM, num_chains=2, N=64, num_sequences=2, minibatch_size=3, subsequence_length=16,
                window_sampling="device")
    assert (s.M, s.K, s.W, s.multi, s.draws, s.rescale) == (3, 2, 6, True, True, True)
    s = resolve("svm", Y40, SVM, num_chains=2, N=64, minibatch_size=1)
    assert (s.W, s.multi, s.draws, s.rescale) == (1, True, False, False)
    assert not resolve("lgssm", Y40, LG, num_chains=2, kind="marginal", minibatch_size=1).multi
    s = resolve("svm", Y40, np.full((5, _capi.THETA_DIM["svm"]), 0.5))
    assert s.theta0.shape == (5, 3) and s.proto is None
