"""CPU: tests/helpers/forced_window.py against the pinned oracle -- the teacher-forced O(N^2) step fed the oracle's own
save_all output must return the oracle's next step, and the ancestor-law statistic must pass on the oracle's own
multinomial ancestors (and fail on shifted ones), before either is used to judge a kernel
(tests/test_gpu_n2_device_replay.py)."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_host_logic import default_params, GEN
from test_gpu_n2_one_wave import _prior_x

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import forced_window  # noqa: E402

CASES = [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal")]


@pytest.mark.parametrize("stat", ["score", "suff", "none"])
@pytest.mark.parametrize("model,kernel", CASES)
def test_forced_steps_return_the_oracles_own_window(model, kernel, stat):
    """po.pf_window(pf='poyiadjis_N2', save_all=True) at N = 60, T = 5, window [1, 4) with weights: from the oracle's
    step t, forced_steps gives the oracle's step t + 1 -- log-weights, statistics, running log-likelihood -- at rtol 1e-12."""
    N, T, t1, tL = 60, 5, 1, 4
    p = default_params(model)
    theta = p.theta()
    np.random.seed(23)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    weights = np.linspace(20.0, 30.0, tL - t1)
    pm, pv = _prior_x(model, theta)
    ref = po.pf_window_rng(model, theta, y, N, rng=np.random.RandomState(4), kernel=kernel, pf="poyiadjis_N2", stat=stat,
                           t1=t1, tL=tL, weights=weights, prior_mean=pm, prior_var=pv, save_all=True)
    lw, st, dll = forced_window.forced_steps(model, kernel, theta, y, ref["all_x_t"], ref["all_log_weights"],
                                             ref["all_statistics"], ref["all_ancestors"], stat=stat, t1=t1, tL=tL,
                                             weights=weights)
    np.testing.assert_allclose(lw, ref["all_log_weights"][1:], rtol=1e-12, atol=0)
    np.testing.assert_allclose(st, ref["all_statistics"][1:], rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.cumsum(dll), ref["all_loglikelihood_estimate"][1:], rtol=1e-12, atol=0)
    if stat == "none":
        assert np.all(st == 0.0)
    else:
        assert np.all(st[:t1] == 0.0) and np.any(st[t1] != 0.0)
        # outside the window the statistics still move from parent to parent
        assert np.any(st[tL] != st[tL - 1])


def test_forced_step_notices_a_wrong_statistic():
    """The recomputed step is a check, not a copy: dropping the importance weight of one window step, or scoring the
    children against the resampled parents' neighbours, moves it by far more than the GPU tests' 1e-8."""
    model, kernel, N, T, t1, tL = "svm", "prior", 60, 5, 1, 4
    p = default_params(model)
    np.random.seed(23)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    weights = np.linspace(20.0, 30.0, tL - t1)
    ref = po.pf_window_rng(model, p.theta(), y, N, rng=np.random.RandomState(4), kernel=kernel, pf="poyiadjis_N2", stat="suff",
                           t1=t1, tL=tL, weights=weights, prior_mean=0.0, prior_var=10.0, save_all=True)
    args = (model, kernel, p.theta(), y, ref["all_x_t"], ref["all_log_weights"], ref["all_statistics"])
    _, st, _ = forced_window.forced_steps(*args, ref["all_ancestors"], stat="suff", t1=t1, tL=tL, weights=None)
    assert np.max(np.abs(st[t1] - ref["all_statistics"][t1 + 1])) > 1.0
    lw, _, _ = forced_window.forced_steps(*args, (ref["all_ancestors"] + 1) % N, stat="suff", t1=t1, tL=tL, weights=weights)
    assert np.allclose(lw, ref["all_log_weights"][1:], rtol=1e-8, atol=1e-8)      # SVM prior: the weight reads the child alone
    q = default_params("lgssm")
    np.random.seed(3)
    y = GEN["lgssm"](T=T, parameters=q)["observations"].reshape(-1)
    ref = po.pf_window_rng("lgssm", q.theta(), y, N, rng=np.random.RandomState(4), kernel="optimal", pf="poyiadjis_N2",
                           prior_mean=0.0, prior_var=10.0, save_all=True)
    lw, _, _ = forced_window.forced_steps("lgssm", "optimal", q.theta(), y, ref["all_x_t"], ref["all_log_weights"],
                                          ref["all_statistics"], (ref["all_ancestors"] + 1) % N)
    assert np.max(np.abs(lw - ref["all_log_weights"][1:])) > 1e-3               # LGSSM optimal: it reads the parent


@pytest.mark.parametrize("model,kernel,N,T", [("svm", "prior", 200, 8), ("garch", "optimal", 700, 5),
                                              ("lgssm", "optimal", 700, 5), ("svm", "prior", 1100, 3)])
def test_ancestor_law_on_the_oracles_multinomial_ancestors(model, kernel, N, T):
    """The oracle's own ancestors (np.random.choice semantics on the legacy stream; the O(N) recursion shares the
    resampling step with the O(N^2) one) at the shapes of the GPU tests: |sum_t Z_t| / sqrt(#steps) < 5.  Shifted by one
    index against the weights the same ancestors fail it wherever the weights vary enough to tell."""
    p = default_params(model)
    np.random.seed(17)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    pm, pv = _prior_x(model, p.theta())
    ref = po.pf_window_rng(model, p.theta(), y, N, rng=np.random.RandomState(N + T), kernel=kernel, pf="poyiadjis_N",
                           prior_mean=pm, prior_var=pv, save_all=True)
    score, steps = forced_window.ancestor_law_score(ref["all_log_weights"], ref["all_ancestors"])
    assert steps == T - 1                       # step 0 resamples equal weights
    assert forced_window.ancestor_law_z(ref["all_log_weights"][0], ref["all_ancestors"][0]) is None
    print("ancestor law", model, N, T, score)
    assert score < 5.0, score
    shifted, _ = forced_window.ancestor_law_score(ref["all_log_weights"], (ref["all_ancestors"] + 1) % N)
    print("  shifted by one", shifted)
    assert shifted > 5.0, shifted
