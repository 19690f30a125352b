"""kind='complete' and Gibbs on the MI355X: the FFBS kernel (PFG_SMOOTHER_KALMAN_FFBS, csrc/pfg_ffbs.hip) against the
reference (tests/golden/ffbs.npz) and the test-side restatement, through pfg_run_batch, the drop-in samplers and
ChainEnsemble(kind='complete'); and the Fisher identity E[complete-data score | y] = the marginal score, against the
exact Kalman kernel (PFG_SMOOTHER_KALMAN), which does not depend on any generator."""
import os
import sys

import numpy as np
import pytest

from conftest import Golden
import test_ffbs_host as host
from test_ffbs_host import close, params_of, path_case, path_cases, SCORE_TO_VEC

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
from ffbs_model import ffbs_window  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-12


@pytest.fixture(scope="module")
def fg():
    return Golden("ffbs.npz")


def _helper():
    from sgmcmc_ssm_amd.models.lgssm import LGSSMHelper
    return LGSSMHelper(n=1, m=1)


def test_kernel_paths_and_gradients_match_the_reference(fg):
    from sgmcmc_ssm_amd import _capi
    ctx = _capi.default_context()
    helper = _helper()
    cases = path_cases(fg)
    qs, qg = [], []
    for m in cases:
        y, th, fm, _, _ = path_case(fg, m)
        S = m["S"] or 1
        np.random.seed(m["seed"])
        z = np.random.standard_normal(m["T"] * S)
        qs.append(helper.ffbs_problem(y, params_of(th), S, forward_message=fm, stat="none", z=z))
        qg.append(helper.ffbs_problem(y, params_of(th), S, forward_message=fm, z=z))
        if m["window"]:
            qg.append(helper.ffbs_problem(y, params_of(th), S, m["t1"], m["tL"], weights=fg[m["key"] + "/weights"],
                                          forward_message=fm, z=z))
    outs = ctx.run_batch(qs, want_trace=True)      # 12 buffers of lengths 1 .. 1000 in one launch
    assert ctx.last_variant() == "kalman_ffbs"
    for m, o in zip(cases, outs):
        ref = fg[m["key"] + "/paths"]
        assert np.max(np.abs(o["paths"] - ref)) <= RTOL * max(1.0, np.max(np.abs(ref))), m["key"]
        np.testing.assert_array_equal(o["paths"], ref)             # the kernel's paths are the reference's, bitwise
        np.testing.assert_array_equal(o["mean_stat"], 0.0)
    grads = iter(ctx.run_batch(qg))
    for m in cases:
        close(next(grads)["mean_stat"][SCORE_TO_VEC], fg[m["key"] + "/grad_all"], RTOL, m["T"])
        if m["window"]:
            close(next(grads)["mean_stat"][SCORE_TO_VEC], fg[m["key"] + "/grad_window"], RTOL, m["tL"] - m["t1"])


def test_mixed_batch_each_window_alone_is_bitwise_the_same():
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.models.lgssm import generate_lgssm_data
    ctx = _capi.default_context()
    helper = _helper()
    rs = np.random.RandomState(21)
    p = params_of([0.9, 1.0, 1.0 / np.sqrt(0.3), 1.2])
    np.random.seed(22)
    y = generate_lgssm_data(T=1000, parameters=p)["observations"][:, 0]
    shapes = [(1, 1), (2, 3), (17, 64), (40, 65), (100, 128), (120, 129), (300, 256), (500, 257), (1000, 100),
              (1000, 1024), (200, 1500)]                           # 1500 > the workgroup: lanes loop
    qs = []
    for i, (T, S) in enumerate(shapes):
        t1 = int(rs.randint(0, T)) if T > 1 else 0
        tL = int(rs.randint(t1, T + 1))
        w = rs.uniform(0.5, 2.0, size=tL - t1) if i % 2 else None
        th = params_of([0.9 - 0.05 * i, 1.0, 1.0 / np.sqrt(0.3 + 0.1 * i), 1.2])
        qs.append(helper.ffbs_problem(y[:T], th, S, t1, tL, weights=w, z=rs.standard_normal(T * S)))
    outs = ctx.run_batch(qs)
    for q, o in zip(qs, outs):
        alone = ctx.run_batch([q])[0]
        np.testing.assert_array_equal(alone["mean_stat"], o["mean_stat"])
        if q["N"] * q["y"].shape[0] <= 300000:                     # the pure-Python restatement
            g, _ = ffbs_window(q)
            close(o["mean_stat"], g, 1e-11, q["tL"] - q["t1"])


def test_drop_in_samplers(fg):
    host.check_sampler_gradients(fg, 1e-10)
    host.check_trajectories(fg, 1e-10, 1e-9)
    from sgmcmc_ssm_amd import _capi
    assert _capi.default_context().last_variant() == "kalman_ffbs"


def _fisher_setup(T=300, t1=100, tL=160):
    from sgmcmc_ssm_amd.models.lgssm import generate_lgssm_data
    p = params_of([0.85, 1.0, 1.0 / np.sqrt(0.4), 1.0 / np.sqrt(0.8)])
    np.random.seed(31)
    y = generate_lgssm_data(T=T, parameters=p)["observations"][:, 0]
    w = np.random.RandomState(32).uniform(0.5, 2.0, size=tL - t1)
    exact = _capi_ctx().run_batch([_helper().kalman_problem(y, p, t1, tL, weights=w)])[0]["mean_stat"]
    return p, y, w, exact


def _capi_ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context()


def _ztest(samples, exact, k=5.0):
    mean = samples.mean(axis=0)
    se = samples.std(axis=0, ddof=1) / np.sqrt(samples.shape[0])
    assert np.all(np.abs(mean - exact) <= k * se), (mean, exact, se)


def test_fisher_identity_device_generator():
    # E[complete-data score over [t1, tL) | y] = the marginal (Kalman) score of the window: 1000 descriptors x 100
    # DEVICE-generator paths with distinct streams
    p, y, w, exact = _fisher_setup()
    helper = _helper()
    qs = [helper.ffbs_problem(y, p, 100, 100, 160, weights=w, rng="device", seed=1234, stream=b) for b in range(1000)]
    outs = _capi_ctx().run_batch(qs)
    _ztest(np.stack([o["mean_stat"] for o in outs]), exact)


def test_fisher_identity_replay():
    p, y, w, exact = _fisher_setup()
    helper = _helper()
    np.random.seed(41)
    qs = [helper.ffbs_problem(y, p, 100, 100, 160, weights=w) for _ in range(100)]
    outs = _capi_ctx().run_batch(qs)
    _ztest(np.stack([o["mean_stat"] for o in outs]), exact)


def _ensemble(y, C, **kw):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = params_of([0.7, 1.0, 1.5, 1.2])
    th = np.tile(p.theta(), (C, 1)) + np.random.RandomState(3).normal(scale=0.02, size=(C, 4))
    return ChainEnsemble("lgssm", y, th, kind="complete", num_samples=100, epsilon=0.001, seed=77, **kw)


def _descriptor_windows(ens, y, S):
    d, base, wbase = ens._desc, ens.y_dev.data_ptr(), ens.weights_dev.data_ptr()
    for b in range(ens.C):
        left = (int(d["y"][b]) - base) // 8
        start = (int(d["weights"][b]) - wbase) // (8 * S)
        assert start == left + int(d["t1"][b])
        yield b, y[left:left + int(d["T"][b])], int(d["t1"][b]), int(d["tL"][b]), ens._weights_table[start]


def test_ensemble_host_windows_equal_run_batch_and_agree_with_the_marginal_score():
    import torch
    from sgmcmc_ssm_amd.models.lgssm import generate_lgssm_data
    np.random.seed(12)
    y = generate_lgssm_data(T=600, parameters=params_of([0.9, 1.0, 3.0, 1.0]))["observations"][:, 0]
    C = 1000
    ens = _ensemble(y, C, subsequence_length=40, buffer_length=10, window_sampling="host")
    ens.step(3)
    ens.synchronize()
    # one more launch by hand: the descriptors of step 3, the parameters after three SGLD updates
    theta = ens.theta()
    if ens._set_windows():
        ens.desc_dev.copy_(torch.from_numpy(ens._desc.view(np.uint8).reshape(C, -1)))
    ens.launch_pf()
    ens.synchronize()
    assert ens.ctx.last_variant() == "kalman_ffbs"
    got = ens.out_dev.cpu().numpy()
    step = int(ens.step_ctr.cpu().numpy()[0])
    helper = _helper()
    qs, qk, inner = [], [], []
    for b, yb, t1, tL, w in _descriptor_windows(ens, y, 40):
        qs.append(helper.ffbs_problem(yb, params_of(theta[b]), 100, t1, tL, weights=w, rng="device", seed=ens.seed,
                                      stream=ens.chain_offset + b, step=step))
        qk.append(helper.kalman_problem(yb, params_of(theta[b]), t1, tL, weights=w))
        inner.append(t1 > 0)
    ref = _capi_ctx().run_batch(qs)
    np.testing.assert_array_equal(got[:, :4], np.stack([o["mean_stat"] for o in ref]))
    np.testing.assert_array_equal(got[:, 4:], 0.0)
    # the chains' FFBS scores minus their windows' exact scores average to zero (Fisher identity)
    exact = np.stack([o["mean_stat"] for o in _capi_ctx().run_batch(qk)])
    inner = np.array(inner)
    assert inner.sum() > 500
    _ztest((got[:, :4] - exact)[inner], np.zeros(4))


def test_ensemble_device_windows_graph_replay_is_bitwise_eager():
    from sgmcmc_ssm_amd.models.lgssm import generate_lgssm_data
    np.random.seed(13)
    y = generate_lgssm_data(T=1000, parameters=params_of([0.9, 1.0, 1.0 / np.sqrt(0.1), 1.0]))["observations"][:, 0]
    runs = []
    for K in (16, 0):
        ens = _ensemble(y, 256, subsequence_length=40, buffer_length=-1, window_sampling="device")
        runs.append(ens.run(32, thin=16, graph_steps=K))
        assert ens.ctx.last_variant() == "kalman_ffbs"
    np.testing.assert_array_equal(runs[0], runs[1])
    assert np.all(np.isfinite(runs[0])) and not np.array_equal(runs[0][0], runs[0][1])


def test_ensemble_refuses_other_models_and_dtypes():
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    from sgmcmc_ssm_amd.models.svm import SVMParameters
    y = np.zeros(50)
    with pytest.raises(NotImplementedError):
        ChainEnsemble("svm", y, SVMParameters(A=np.eye(1) * 0.9, Q=np.eye(1), R=np.eye(1)), num_chains=2,
                      kind="complete", num_samples=10)
    with pytest.raises(NotImplementedError):
        ChainEnsemble("lgssm", y, params_of([0.7, 1.0, 1.5, 1.2]), num_chains=2, kind="complete", num_samples=10,
                      dtype="f32")
    with pytest.raises(ValueError):
        ChainEnsemble("lgssm", y, params_of([0.7, 1.0, 1.5, 1.2]), num_chains=2, kind="complete")
