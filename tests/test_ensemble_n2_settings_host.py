"""CPU: ChainEnsemble._resolve_settings for pf='poyiadjis_N2', the Poyiadjis O(N^2) smoother as resident chains (the
POYIADJIS_N2_100 row of the reference's experiment tables: N = 100, S = 40, buffer -1).  What it resolves to and the
refusals it states before anything is allocated; runs wherever the package imports."""
import numpy as np
import pytest

from sgmcmc_ssm_amd.ensemble import ChainEnsemble
from test_host_logic import default_params

resolve = ChainEnsemble._resolve_settings
SVM, LG = default_params("svm"), default_params("lgssm")
MULTI = dict(minibatch_size=2, subsequence_length=10, buffer_length=2, window_sampling="device")


def test_resolves_to_the_n2_smoother():
    s = resolve("svm", np.zeros(40), SVM, num_chains=3, N=100, pf="poyiadjis_N2")
    assert (s.smoother, s.launch_smoother, s.lambduh, s.stat, s.multi) == ("poyiadjis_n2", "poyiadjis_n2", 1.0, "score", False)
    assert s.pf == "poyiadjis_N2" and s.kind == "pf" and s.N == 100 and s.paris == {}
    # lambduh is the smoother's, not the caller's
    assert resolve("svm", np.zeros(40), SVM, num_chains=3, N=100, pf="poyiadjis_N2", lambduh=0.5).lambduh == 1.0
    # the single-window path serves N up to 1024
    assert resolve("svm", np.zeros(40), SVM, num_chains=3, N=1024, pf="poyiadjis_N2").N == 1024


def test_multi_window_path_takes_large_n():
    s = resolve("svm", np.zeros(60), SVM, num_chains=3, N=2000, pf="poyiadjis_N2", **MULTI)
    assert s.multi is True and s.N == 2000 and s.W == 2
    assert (s.smoother, s.launch_smoother, s.lambduh, s.stat) == ("poyiadjis_n2", "poyiadjis_n2", 1.0, "score")
    assert resolve("svm", np.zeros(60), SVM, num_chains=3, N=16384, pf="poyiadjis_N2", **MULTI).N == 16384


REFUSALS = [
    (ValueError, "pf='poyiadjis_N2' needs kind='pf'", ("lgssm", np.zeros(40), LG), dict(num_chains=4, pf="poyiadjis_N2", kind="marginal")),
    (ValueError, "pf='poyiadjis_N2' needs kind='pf'",
     ("lgssm", np.zeros(40), LG), dict(num_chains=4, pf="poyiadjis_N2", kind="complete", num_samples=3)),
    (ValueError, "pf='poyiadjis_N2' resamples multinomially",
     ("svm", np.zeros(40), SVM), dict(num_chains=4, N=100, pf="poyiadjis_N2", resampling="stratified")),
    (ValueError, "pf='poyiadjis_N2' resamples multinomially",
     ("svm", np.zeros(40), SVM), dict(num_chains=4, N=100, pf="poyiadjis_N2", resampling="systematic")),
    (NotImplementedError, "n2_mem1024, N <= 16384", ("svm", np.zeros(40), SVM), dict(num_chains=4, N=1025, pf="poyiadjis_N2")),
    (NotImplementedError, "pass minibatch_size / num_sequences for the multi-window path",
     ("svm", np.zeros(40), SVM), dict(num_chains=4, N=2000, pf="poyiadjis_N2")),
    (NotImplementedError, "the multi-window path is built for N <= 16384",
     ("svm", np.zeros(60), SVM), dict(num_chains=2, N=16385, pf="poyiadjis_N2", **MULTI)),
]


@pytest.mark.parametrize("exc,match,args,kw", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals(exc, match, args, kw):
    with pytest.raises(exc, match=match.replace("(", r"\(").replace(")", r"\)").replace("|", r"\|")):
        resolve(*args, **kw)


def test_unknown_pf_names_four_smoothers():
    with pytest.raises(ValueError) as e:
        resolve("svm", np.zeros(40), SVM, num_chains=2, pf="filter")
    assert "'poyiadjis_N' | 'nemeth' | 'paris' | 'poyiadjis_N2'" in str(e.value)
