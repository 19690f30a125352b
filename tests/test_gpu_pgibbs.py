"""GPU: particle Gibbs as a resident ensemble -- pfg_pgibbs_update_device against its mirror and against
pfg_gibbs_update_device, and ChainEnsemble(sampler='pgibbs') on T = 12, N = 8, C = 5 against the host model's step, across
seeds, rank partitions, hipGraph replay and checkpoints."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import csmc_model as cm  # noqa: E402
import keyed_draws as kd  # noqa: E402
import pmmh_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

T, N, C = 12, 8, 5
RTOL, ATOL = 1e-8, 1e-8


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def _dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _hyper(model):
    from sgmcmc_ssm_amd.ensemble import prior_hyper, _model_info
    return prior_hyper(model, _model_info(model)[1].generate_default_prior(var=100.0, n=1, m=1))


def _records(model, n, seed=3):
    """n plausible records: statistics of AR(1) paths of varying length"""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 8))
    for b in range(n):
        Tb = int(rs.randint(5, 60))
        x = cm.sample_prior_paths(cm.THETA[model], Tb, 1, 0.0, 1.0, rs)
        e = rs.standard_normal((1, Tb))
        y = np.exp(x / 2) * e if model == "svm" else x + e
        out[b] = cm.record(model, x, y)[0]
    return out


# ---- 8. the update rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
@pytest.mark.parametrize("off,step", [(0, None), (7, 3), (2 ** 32 + 5, 2 ** 33 + 1)])
def test_pgibbs_update_matches_the_mirror(model, off, step):
    import torch
    n = 300
    stats, hy = _records(model, n), _hyper(model)
    theta, outs = _dev(np.tile([0.5, 1.0, 1.0, 1.0], (n, 1))), _dev(stats)
    ctr = None if step is None else torch.full((1,), step, dtype=torch.int64, device="cuda:0")
    _ctx().pgibbs_update_device(model, n, theta.data_ptr(), outs.data_ptr(), hy, 424242, off, None if ctr is None else ctr.data_ptr())
    torch.cuda.synchronize()
    got = theta.cpu().numpy()
    exp, tie = cm.pgibbs_expected(model, stats, hy, 424242, off, step)
    assert tie.sum() <= 2
    bad = exp.mismatch(got)[~tie]
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:3])
    assert np.all(np.isfinite(got[:, :3]))
    if model == "svm":
        assert np.all(got[:, 3] == 1.0)             # the fourth slot is not SVM's: untouched
    if ctr is not None:
        assert int(ctr.item()) == step + 1          # the counter is bumped afterwards
    if model == "lgssm":                            # ... and bitwise pfg_gibbs_update_device on the same statistics and key
        ref = _dev(np.tile([0.5, 1.0, 1.0, 1.0], (n, 1)))
        c2 = None if step is None else torch.full((1,), step, dtype=torch.int64, device="cuda:0")
        _ctx().gibbs_update_device(model, n, ref.data_ptr(), outs.data_ptr(), hy, 424242, off, None if c2 is None else c2.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(ref.cpu().numpy(), got)


def test_pgibbs_update_refuses_garch():
    theta, outs = _dev(np.zeros((2, 4))), _dev(np.zeros((2, 8)))
    with pytest.raises(NotImplementedError, match="no conjugate Gibbs draw"):
        _ctx().pgibbs_update_device("garch", 2, theta.data_ptr(), outs.data_ptr(), _hyper("garch"), 1)
    with pytest.raises(NotImplementedError):        # ... and pfg_gibbs_update_device keeps refusing SVM
        _ctx().gibbs_update_device("svm", 2, theta.data_ptr(), outs.data_ptr(), _hyper("svm"), 1)


# ---- 9. the ensemble ------------------------------------------------------------------------------------------------------------
def _setup(model):
    np.random.seed(7)
    if model == "svm":
        from sgmcmc_ssm_amd.models.svm import SVMParameters, generate_svm_data
        p = SVMParameters(A=np.eye(1) * 0.9, Q=np.eye(1) * 0.25, R=np.eye(1) * 0.7)
        y = generate_svm_data(T=T, parameters=p)["observations"]
    else:
        from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, generate_lgssm_data
        p = LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1), Q=np.eye(1) * 0.25, R=np.eye(1) * 0.7)
        y = generate_lgssm_data(T=T, parameters=p)["observations"]
    rs = np.random.RandomState(2)
    theta0 = np.tile(p.theta(), (C, 1)) * rs.uniform(0.9, 1.1, size=(C, len(p.theta())))
    if model == "lgssm":
        theta0[:, 1] = 1.0
    return np.asarray(y).reshape(-1), theta0


def _ens(model, y, theta0, seed=5, chain_offset=0):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    return ChainEnsemble(model, y, theta0.copy(), N=N, sampler="pgibbs", seed=seed, chain_offset=chain_offset)


@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_ensemble_step_equals_the_host_models(model):
    """The init pass (an unconditional sweep at counter 0) and one whole step (the conditional sweep at counter 1, then the
    parameter draw) against the restatement, forced on nothing: the host model runs on its own in double."""
    y, theta0 = _setup(model)
    ens = _ens(model, y, theta0, seed=5, chain_offset=3)
    pmean, pvar = float(ens._csmc_desc["prior_mean"][0]), float(ens._csmc_desc["prior_var"][0])
    gids = kd.chain_ids(C, 3)
    path0 = ens.path()
    assert int(ens.step_ctr.item()) == 1 and path0.shape == (C, T) and not ens.n_degenerate().any()
    h0 = cm.sweep(model, theta0, y, None, N, cm.sweep_seed(5), gids, 0, pmean, pvar, has_ref=False)
    np.testing.assert_allclose(path0, h0["path"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(ens.suff_stats(), h0["out"][:, :7], rtol=RTOL, atol=ATOL)
    ens.step(1)
    ens.synchronize()
    h1 = cm.sweep(model, theta0, y, path0, N, cm.sweep_seed(5), gids, 1, pmean, pvar)
    np.testing.assert_allclose(ens.path(), h1["path"], rtol=RTOL, atol=ATOL)
    stats = ens.out_dev.cpu().numpy()
    np.testing.assert_allclose(stats, h1["out"], rtol=RTOL, atol=ATOL)
    assert np.array_equal(ens.last_gradient_statistics()[0], stats[:, :7]) and ens.last_gradient_statistics()[1] is None
    exp, tie = cm.pgibbs_expected(model, stats, ens.hyper, pm.update_seed(5), 3, 1)
    assert not exp.mismatch(ens.theta())[~tie].any() and not tie.all()
    assert int(ens.step_ctr.item()) == 2 and ens.steps_done == 1


@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_ensemble_is_reproducible_and_partition_invariant(model):
    y, theta0 = _setup(model)
    a, b = _ens(model, y, theta0), _ens(model, y, theta0)
    sa, sb = a.run(3), b.run(3)
    assert np.array_equal(sa, sb) and np.array_equal(a.path(), b.path())
    assert not np.array_equal(sa, _ens(model, y, theta0, seed=6).run(3))
    lo, hi = _ens(model, y, theta0[:2]), _ens(model, y, theta0[2:], chain_offset=2)
    assert np.array_equal(np.concatenate([lo.run(3), hi.run(3)], axis=1), sa)
    assert np.array_equal(np.concatenate([lo.path(), hi.path()]), a.path())


@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_graphed_run_equals_eager_run(model):
    y, theta0 = _setup(model)
    eager, graphed = _ens(model, y, theta0), _ens(model, y, theta0)
    se, sg = eager.run(4), graphed.run(4, thin=2, graph_steps=2)
    assert np.array_equal(se[1::2], sg) and np.array_equal(eager.path(), graphed.path())
    assert np.array_equal(eager.n_degenerate(), graphed.n_degenerate()) and graphed.steps_done == 4


@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_checkpoint_round_trip_continues_bitwise(model):
    y, theta0 = _setup(model)
    a = _ens(model, y, theta0)
    a.run(2)
    state = a.state_dict()
    assert state["sampler"] == "pgibbs" and state["T"] == T and state["path"].shape == (C, T)
    b = _ens(model, y, theta0)
    b.load_state_dict(state)
    assert np.array_equal(a.run(2), b.run(2)) and np.array_equal(a.path(), b.path())
    for key, value in (("T", T + 1), ("sampler", "gibbs")):
        with pytest.raises(ValueError, match="checkpoint {0}".format(key)):
            b.load_state_dict(dict(state, **{key: value}))


def test_other_samplers_refuse_a_pgibbs_checkpoint():
    """A 'pgibbs' checkpoint names its sampler; an ensemble of another sampler would drop its path, so it refuses it (and
    still takes its own checkpoints, which name none)."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y, theta0 = _setup("svm")
    state = _ens("svm", y, theta0).state_dict()
    other = ChainEnsemble("svm", y, theta0.copy(), N=N, seed=5)
    with pytest.raises(ValueError, match="checkpoint sampler = pgibbs"):
        other.load_state_dict(state)
    own = other.state_dict()
    assert "sampler" not in own
    other.load_state_dict(own)


def test_accessors_belong_to_pgibbs():
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y, theta0 = _setup("svm")
    ens = ChainEnsemble("svm", y, theta0, N=64, seed=1)
    for name in ("path", "suff_stats", "n_degenerate"):
        with pytest.raises(ValueError, match="belongs to sampler='pgibbs'"):
            getattr(ens, name)()
