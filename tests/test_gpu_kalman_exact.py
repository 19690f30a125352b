"""kind='marginal' on the MI355X: the exact Kalman score kernel (PFG_SMOOTHER_KALMAN, csrc/pfg_kalman.hip) against
the reference (tests/golden/kalman.npz, sampler.npz) and the test-side restatement, through pfg_run_batch, the
drop-in samplers and ChainEnsemble(kind='marginal')."""
import os
import sys

import numpy as np
import pytest

from conftest import Golden
import test_kalman_host as host
from test_kalman_host import close, helper_case, params_of, SCORE_TO_VEC

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
from kalman_model import kalman_window  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope="module")
def kg():
    return Golden("kalman.npz")


def _problems(kg):
    from sgmcmc_ssm_amd.models.lgssm import LGSSMHelper
    helper = LGSSMHelper(n=1, m=1)
    cases = [m for m in kg.meta if m["kind"] == "helper"]
    qs = []
    for m in cases:
        y, th, w, fm = helper_case(kg, m)
        qs.append(helper.kalman_problem(y, params_of(th), weights=w, forward_message=fm))
    return cases, qs


def test_kernel_matches_the_reference_helper_in_one_mixed_batch(kg):
    from sgmcmc_ssm_amd import _capi
    ctx = _capi.default_context()
    cases, qs = _problems(kg)
    outs = ctx.run_batch(qs)                        # 108 windows of lengths 1 .. 1000 in one launch
    assert ctx.last_variant() == "kalman"
    for m, q, o in zip(cases, qs, outs):
        lc = kg[m["key"] + "/message"][0]
        close(o["mean_stat"][SCORE_TO_VEC], kg[m["key"] + "/grad"], RTOL)
        close(lc + o["loglik"], kg[m["key"] + "/loglike"], RTOL)
        assert np.all(o["mean_stat"] != 0.0)
    for q, o in zip(qs, outs):                      # each window alone: the same numbers, bitwise
        alone = ctx.run_batch([q])[0]
        np.testing.assert_array_equal(alone["mean_stat"], o["mean_stat"])
        assert alone["loglik"] == o["loglik"]


def test_kernel_reproduces_the_sampler_fixture(golden_sampler):
    from sgmcmc_ssm_amd.models.lgssm import LGSSMHelper, LGSSMParameters
    from sgmcmc_ssm_amd import _capi
    g = golden_sampler
    p = LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1), Q=np.eye(1) * 0.7, R=np.eye(1))
    fm = dict(log_constant=0.0, mean_precision=np.zeros(1),
              precision=np.eye(1) * float(g.get("lgssm", "exact_grad_prior_prec")))
    helper = LGSSMHelper(n=1, m=1, forward_message=fm)
    y = g.get("lgssm", "y")
    grad = helper.gradient_marginal_loglikelihood(observations=y, parameters=p, forward_message=fm)
    assert _capi.default_context().last_variant() == "kalman"
    close(host.vec(grad), g.get("lgssm", "exact_grad"), RTOL)
    ll = helper.marginal_loglikelihood(observations=y, parameters=p, forward_message=fm)
    close(ll, float(g.get("lgssm", "exact_loglike")), RTOL)


def test_drop_in_samplers(kg):
    host.check_sampler_cases(kg, RTOL)
    host.check_trajectories(kg, RTOL)
    host.check_sequences(kg, RTOL)
    host.check_control_variates(kg, RTOL)


def test_long_window_agrees_with_the_restatement():
    from sgmcmc_ssm_amd.models.lgssm import LGSSMHelper, generate_lgssm_data
    from sgmcmc_ssm_amd import _capi
    p = params_of([0.95, 1.0, 1.0 / np.sqrt(0.2), 1.0])
    np.random.seed(4)
    y = generate_lgssm_data(T=10000, parameters=p)["observations"][:, 0]
    w = np.random.uniform(0.5, 2.0, size=10000)
    q = LGSSMHelper(n=1, m=1).kalman_problem(y, p, weights=w)          # S = T: the whole series is the window
    o = _capi.default_context().run_batch([q])[0]
    g, ll = kalman_window(p.theta(), y, 0, 10000, w, q["prior_mean"], q["prior_var"])
    close(o["mean_stat"], g, RTOL)
    close(o["loglik"], ll, RTOL)


def _ensemble(y, C, **kw):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = params_of([0.7, 1.0, 1.5, 1.2])
    th = np.tile(p.theta(), (C, 1)) + np.random.RandomState(3).normal(scale=0.02, size=(C, 4))
    return ChainEnsemble("lgssm", y, th, kind="marginal", epsilon=0.001, seed=77, **kw)


def test_ensemble_host_windows_equal_run_batch():
    import torch
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.models.lgssm import LGSSMHelper, generate_lgssm_data
    np.random.seed(12)
    y = generate_lgssm_data(T=600, parameters=params_of([0.9, 1.0, 3.0, 1.0]))["observations"][:, 0]
    C = 300
    ens = _ensemble(y, C, subsequence_length=40, buffer_length=10, window_sampling="host")
    ens.step(3)
    ens.synchronize()
    # one more launch by hand: the descriptors of step 3, the parameters after three SGLD updates
    theta = ens.theta()
    if ens._set_windows():
        ens.desc_dev.copy_(torch.from_numpy(ens._desc.view(np.uint8).reshape(C, -1)))
    ens.launch_pf()
    ens.synchronize()
    assert ens.ctx.last_variant() == "kalman"
    got = ens.out_dev.cpu().numpy()
    d, base, wbase = ens._desc, ens.y_dev.data_ptr(), ens.weights_dev.data_ptr()
    helper = LGSSMHelper(n=1, m=1)
    qs = []
    for b in range(C):
        left = (int(d["y"][b]) - base) // 8
        start = (int(d["weights"][b]) - wbase) // (8 * 40)
        qs.append(helper.kalman_problem(y[left:left + int(d["T"][b])], params_of(theta[b]), int(d["t1"][b]),
                                        int(d["tL"][b]), ens._weights_table[start]))
        assert start == left + int(d["t1"][b])
    ref = _capi.default_context().run_batch(qs)
    np.testing.assert_array_equal(got[:, :4], np.stack([o["mean_stat"] for o in ref]))
    np.testing.assert_array_equal(got[:, 4], np.array([o["loglik"] for o in ref]))
    np.testing.assert_array_equal(got[:, 5:], 0.0)
    s, ll = ens.last_gradient_statistics()
    np.testing.assert_array_equal(s, got[:, :4])


def test_ensemble_device_windows_graph_replay_is_bitwise_eager():
    from sgmcmc_ssm_amd.models.lgssm import generate_lgssm_data
    np.random.seed(13)
    y = generate_lgssm_data(T=1000, parameters=params_of([0.9, 1.0, 1.0 / np.sqrt(0.1), 1.0]))["observations"][:, 0]
    runs = []
    for K in (16, 0):
        ens = _ensemble(y, 256, subsequence_length=40, buffer_length=-1, window_sampling="device")
        runs.append(ens.run(32, thin=16, graph_steps=K))
        assert ens.ctx.last_variant() == "kalman"
    np.testing.assert_array_equal(runs[0], runs[1])
    assert np.all(np.isfinite(runs[0])) and not np.array_equal(runs[0][0], runs[0][1])
