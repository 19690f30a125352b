"""CPU: the multi-window reduction of ChainEnsemble (pfg_reduce_windows_device, restated in
tests/helpers/window_reduce.py) is, bit for bit, how the drop-in SeqSVMSampler combines the same window records
(_run_grad_problems + _rescale_groups, the reference's sgmcmc_sampler.py:390-425, 1249-1283); and the header declares
the new entry points."""
import os
import sys

import numpy as np
import pytest

from sgmcmc_ssm_amd import sgmcmc_sampler
from sgmcmc_ssm_amd.models.svm import SeqSVMSampler, SVMParameters

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import window_reduce  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seqs(rs):
    lengths = [40, 12, 25, 60, 33, 18, 51]
    return [rs.normal(size=(n, 1)) for n in lengths]


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("K", [-1, 1, 5])
def test_reduction_equals_drop_in_combination(monkeypatch, M, K):
    rs = np.random.RandomState(100 + 7 * M + K)
    seqs = _seqs(rs)
    p = SVMParameters(A=np.eye(1) * 0.9, Q=np.eye(1) * 0.4, R=np.eye(1) * 0.6)
    sampler = SeqSVMSampler(n=1, m=1, observations=seqs, parameters=p.copy())
    seen = {}

    def fake_run_windows(problems, ctx=None, **kw):
        # random window records with a wide spread of magnitudes and signs (rounding shows in the last bits)
        recs = rs.normal(size=(len(problems), 8)) * 10.0 ** rs.uniform(-3, 4, size=(len(problems), 1))
        seen["records"] = recs
        seen["lengths"] = [q["_series_length"] for q in problems]
        return [dict(mean_statistic=r[:3].copy(), loglikelihood_estimate=float(r[4])) for r in recs]

    monkeypatch.setattr(sgmcmc_sampler._pf, "run_windows", fake_run_windows)
    monkeypatch.setattr(sampler, "_speculate_next_stream", lambda flat: None)
    np.random.seed(5)
    grad = sampler._noisy_grad_loglikelihood(num_sequences=K, minibatch_size=M, kind="pf", pf="poyiadjis_N", N=16,
                                             subsequence_length=8, buffer_length=2, rng="device")
    Keff = len(seqs) if K == -1 else K
    recs = seen["records"].copy()
    recs[:, 3] = 0.0                        # SVM: three score columns; the device record's fourth is 0
    got = window_reduce.reduce_chain(recs, seen["lengths"], Keff, M, K != -1, sum(len(s) for s in seqs))
    # score columns [LRinv, LQinv, A] -> the drop-in's dict
    want = np.array([np.reshape(grad[n], -1)[0] for n in ("LRinv_vec", "LQinv_vec", "A")])
    assert got[:3].tobytes() == want.tobytes(), (got[:3], want)
    assert np.all(got[5:] == 0.0)


def test_reduction_matches_reference_loops():
    """The restatement against a literal transcription of the reference loops (sgmcmc_sampler.py:411-418, 1264-1282),
    log-likelihood column included."""
    rs = np.random.RandomState(3)
    for K, M, rescale in [(1, 1, True), (3, 2, True), (4, 3, False), (49, 1, False)]:
        lengths = rs.randint(5, 130, size=K)
        recs = rs.normal(size=(K * M, 8)) * 10.0 ** rs.uniform(-3, 4, size=(K * M, 1))
        T_total = int(lengths.sum()) + 77
        noisy_grad_loglike, S = None, 0.0
        for k in range(K):
            noisy_grad = {j: np.zeros(1) for j in range(5)}
            for s in range(0, M):
                for var in noisy_grad:
                    noisy_grad[var] += recs[k * M + s][var] * 1.0 / M
            S += lengths[k]
            if noisy_grad_loglike is None:
                noisy_grad_loglike = {var: noisy_grad[var] for var in noisy_grad}
            else:
                noisy_grad_loglike = {var: noisy_grad_loglike[var] + noisy_grad[var] for var in noisy_grad}
        if rescale:
            noisy_grad_loglike = {var: noisy_grad_loglike[var] * T_total / S for var in noisy_grad_loglike}
        want = np.array([noisy_grad_loglike[j][0] for j in range(5)])
        got = window_reduce.reduce_chain(recs, np.repeat(lengths, M), K, M, rescale, T_total)
        assert got[:5].tobytes() == want.tobytes()


def test_header_declares_the_window_entry_points():
    src = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    for name in ("pfg_sample_windows_multi_device", "pfg_reduce_windows_device", "pfg_scratch_bytes_smoother"):
        assert "{0}(".format(name) in src, name
    from sgmcmc_ssm_amd import _capi
    assert {"pfg_sample_windows_multi_device", "pfg_reduce_windows_device", "pfg_scratch_bytes_smoother"} <= set(_capi.EXPORTS)
    assert "#define PFG_MAX_DRAWN_SEQUENCES {0}".format(_capi.MAX_DRAWN_SEQUENCES) in src


def test_window_counts_and_refusals_need_no_device():
    """The argument checks of ChainEnsemble's multi-window path run before any device work."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = np.zeros(30)
    seqs = [np.zeros(10), np.zeros(7), np.zeros(12)]
    assert ChainEnsemble._window_counts(y, None, None) == (1, 1, 1)
    assert ChainEnsemble._window_counts(y, 3, None) == (3, 1, 3)
    assert ChainEnsemble._window_counts(seqs, None, -1) == (1, -1, 3)
    assert ChainEnsemble._window_counts(seqs, 2, 2) == (2, 2, 4)
    for obs, M, K in [(y, 1, 2), (y, 0, None), (seqs, 1, 4), (seqs, 1, 0), (seqs, 1, -2)]:
        with pytest.raises(ValueError):
            ChainEnsemble._window_counts(obs, M, K)
