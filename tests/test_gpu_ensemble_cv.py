"""GPU: sampler = 'sgd' | 'adagrad' | 'sgld_cv' of ChainEnsemble.

  kernels    pfg_sgd / adagrad / sgld_cv_update_device and pfg_cv_accumulate_device against the host restatement
             (tests/helpers/cv_model.py), B = 130 rows (two blocks of 64 and a tail, edge rows, a key whose high words matter);
             the two SGLD identities of the control-variate step and the accumulation bitwise
  twins      right after construction (theta = centre) a step's two records are bitwise equal, the twins' descriptors are
             their chains' but for theta, out and scratch, and the step is SGLD's on the centre gradient, bitwise
  marginal   with the exact Kalman score the control-variate gradient is the whole-series gradient at the centre, and away
             from it its variance over chains is below the plain window gradient's in every coordinate
  reference  'sgd' and 'adagrad' with the exact gradient reproduce the reference's own trajectories (optim_rules.npz)
  residency  graph replay, checkpoint and resume, the rank partition, re-centring mid-run: all bitwise
"""
import os
import sys

import numpy as np
import pytest

from test_cv_host import GOLDEN, kalman_records
from test_host_logic import GEN, PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cv_model as cv  # noqa: E402
import keyed_draws as kd  # noqa: E402

pytestmark = pytest.mark.gpu

B_ROWS = 130
EPS, TSCALE, SEED = 0.02, 50.0, 0x5EED0000C0DE1234
OFF, STEP = 2 ** 32 - 100, 2 ** 32 + 3          # the chain ids straddle 2^32, the counter is above it
MODELS = ["svm", "garch", "lgssm"]
UPDATE_SEED = 0x5DEECE66D                       # ChainEnsemble._update_key


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _counter(step):
    import torch
    return torch.tensor([step], dtype=torch.int64, device="cuda")


def _sync():
    import torch
    torch.cuda.synchronize()


def _hyper(model):
    from sgmcmc_ssm_amd.ensemble import prior_hyper
    return prior_hyper(model, PRIORS[model].generate_default_prior(var=1.0, n=1, m=1))


def _inputs(model, seed=1):
    """theta [130, MAX_THETA] around the defaults with edge rows in every block -- |A| beyond the clip, negative Cholesky
    factors --, records [130, 8] mostly O(1) with a few +-1e3 and zeros, a second record array and centre gradients."""
    from sgmcmc_ssm_amd import _capi
    rs = np.random.RandomState(seed)
    n, P = B_ROWS, _capi.THETA_DIM[model]
    th = np.zeros((n, _capi.MAX_THETA))
    th[:, :P] = default_params(model).theta() * rs.uniform(0.8, 1.2, size=(n, P))
    th[:, P:] = 7.25                                    # SVM's fourth slot: not the rule's
    if model == "lgssm":
        th[:, 1] = 1.0
    for base in (0, 64, 128):                           # every block, the tail included
        rows = np.arange(base, min(base + 8, n))
        if model != "garch":
            th[rows, 0] = np.resize([0.99995, -0.99991, 1.5, -0.9999, 0.99989, -1.2, 0.9999, 0.999], len(rows))
            th[rows[::2], P - 1] *= -1.0
            th[rows[1::2], P - 2] *= -1.0
        else:
            th[rows, 3] *= -1.0
    g = np.zeros((n, _capi.OUT_DOUBLES))
    g[:, :4] = rs.standard_normal((n, 4))
    big = rs.uniform(size=n) < 0.05
    g[big, :4] = rs.choice([-1e3, 1e3], size=(big.sum(), 4))
    g[rs.uniform(size=n) < 0.05, :4] = 0.0
    g[:, 4:] = rs.standard_normal((n, 4))               # columns the updates must not read
    g2 = g + 0.1 * rs.standard_normal(g.shape)
    return th, g, g2, rs.standard_normal((n, 4))


def _assert_matches(exp, got, what):
    bad = exp.mismatch(got)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("{0}: {1} components off, first row {2} slot {3}: kernel {4!r}, model {5!r}, tol {6:.3g}".format(
            what, int(bad.sum()), i, j, float(got[i, j]), float(exp.theta[i, j]), float(exp.tol[i, j])))


# ---- kernels against the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_sgd_update_matches_the_model(model):
    from sgmcmc_ssm_amd import _capi
    th0, g, _, _ = _inputs(model)
    hy, P = _hyper(model), _capi.THETA_DIM[model]
    theta, outs, ctr = _dev(th0), _dev(g), _counter(STEP)
    _ctx().sgd_update_device(model, B_ROWS, theta.data_ptr(), outs.data_ptr(), hy, EPS, TSCALE, ctr.data_ptr())
    _sync()
    got = theta.cpu().numpy()
    _assert_matches(cv.sgd_expected(model, th0, g, hy, EPS, TSCALE), got, "sgd " + model)
    np.testing.assert_array_equal(got[:, P:], th0[:, P:])
    assert int(ctr.item()) == STEP + 1
    if model != "garch":
        assert (np.abs(th0[:, 0]) > 0.9999).any() and (np.abs(got[:, 0]) <= 0.9999 * (1 + 1e-15)).all()
    assert (th0[:, P - 1] < 0).any() and (got[:, P - 1] > 0).all()


@pytest.mark.parametrize("model", MODELS)
def test_adagrad_two_steps_match_the_model(model):
    """Two steps with the moment carried and the counter bumped, each against the model from the kernel's state before it."""
    from sgmcmc_ssm_amd import _capi
    th0, g, g2, _ = _inputs(model, seed=2)
    hy, P = _hyper(model), _capi.THETA_DIM[model]
    theta, ctr = _dev(th0), _counter(STEP)
    G0 = np.zeros((B_ROWS, _capi.MAX_THETA))
    G0[:, P:] = 3.5                                     # SVM's fourth slot of the moment: untouched
    mom = _dev(G0)
    for k, rec in enumerate((g, g2)):
        before, m_before = theta.cpu().numpy(), mom.cpu().numpy()
        outs = _dev(rec)
        _ctx().adagrad_update_device(model, B_ROWS, theta.data_ptr(), mom.data_ptr(), outs.data_ptr(), hy, EPS, TSCALE,
                                     ctr.data_ptr())
        _sync()
        got, m_got = theta.cpu().numpy(), mom.cpu().numpy()
        exp = cv.adagrad_expected(model, before, rec, hy, EPS, TSCALE, m_before)
        _assert_matches(exp, got, "adagrad {0} step {1}".format(model, k))
        dm = np.abs(m_got[:, :P].astype(np.longdouble) - exp.momentum)
        assert np.all(dm <= exp.mom_tol), ("moment", k, float(np.max(dm / exp.mom_tol)))
        np.testing.assert_array_equal(got[:, P:], th0[:, P:])
        np.testing.assert_array_equal(m_got[:, P:], G0[:, P:])
        assert int(ctr.item()) == STEP + k + 1
    if model == "lgssm":                                # G covers C although the projection pins C
        assert np.all(m_got[:, 1] > 0) and np.all(got[:, 1] == 1.0)


@pytest.mark.parametrize("model", MODELS)
def test_sgld_cv_update_matches_the_model_and_reduces_to_sgld(model):
    from sgmcmc_ssm_amd import _capi
    th0, o, oc, cg = _inputs(model, seed=3)
    hy, P = _hyper(model), _capi.THETA_DIM[model]
    ctx = _ctx()

    def run_cv(outs, outs_centre, centre_grad):
        theta, ctr = _dev(th0), _counter(STEP)
        a, b, c = _dev(outs), _dev(outs_centre), _dev(centre_grad)
        ctx.sgld_cv_update_device(model, B_ROWS, theta.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), hy, EPS, TSCALE,
                                  SEED, OFF, ctr.data_ptr())
        _sync()
        assert int(ctr.item()) == STEP + 1
        return theta.cpu().numpy()

    def run_sgld(outs):
        theta, ctr, a = _dev(th0), _counter(STEP), _dev(outs)
        ctx.sgld_update_device(model, B_ROWS, theta.data_ptr(), a.data_ptr(), hy, EPS, TSCALE, SEED, OFF, ctr.data_ptr())
        _sync()
        return theta.cpu().numpy()

    got = run_cv(o, oc, cg)
    _assert_matches(cv.sgld_cv_expected(model, th0, o, oc, cg, hy, EPS, TSCALE, SEED, OFF, STEP), got, "sgld_cv " + model)
    np.testing.assert_array_equal(got[:, P:], th0[:, P:])
    # the same record on both sides: SGLD on a record holding the centre gradient, bit for bit
    rec = np.zeros_like(o)
    rec[:, :4] = cg
    np.testing.assert_array_equal(run_cv(o, o, cg), run_sgld(rec))
    # no centre: SGLD on the record, bit for bit
    np.testing.assert_array_equal(run_cv(o, np.zeros_like(o), np.zeros_like(cg)), run_sgld(o))
    assert not np.array_equal(got, run_sgld(o))


@pytest.mark.parametrize("R", [1, 3])
def test_cv_accumulate_is_the_stated_order(R):
    rs = np.random.RandomState(10 + R)
    recs = [rs.standard_normal((B_ROWS, 8)) * 10.0 ** rs.randint(-3, 4, size=(B_ROWS, 8)) for _ in range(R)]
    acc0 = np.zeros((B_ROWS, 8))
    acc0[:, 5:] = 9.5
    acc, ctr = _dev(acc0), _counter(STEP)
    for r, rec in enumerate(recs):
        outs = _dev(rec)
        _ctx().cv_accumulate_device(B_ROWS, outs.data_ptr(), acc.data_ptr(), r, R, ctr.data_ptr())
        _sync()
    got = acc.cpu().numpy()
    np.testing.assert_array_equal(got[:, :5], cv.accumulate_expected(recs)[:, :5])
    np.testing.assert_array_equal(got[:, 5:], acc0[:, 5:])
    assert int(ctr.item()) == STEP + R


# ---- twins -------------------------------------------------------------------------------------------------------------------
def _series(model, T, seed=5):
    np.random.seed(seed)
    return np.reshape(GEN[model](T=T, parameters=default_params(model))["observations"], -1)


TWINS = {
    "svm-one-wave-device-windows": dict(model="svm", N=64, T=40, C=130, subsequence_length=8, buffer_length=2,
                                        window_sampling="device"),
    "garch-host-windows": dict(model="garch", N=200, T=40, C=70, subsequence_length=8, buffer_length=2, window_sampling="host"),
    "lgssm-f64-scratch": dict(model="lgssm", N=1100, T=30, C=8, subsequence_length=10, buffer_length=2, window_sampling="device"),
    "svm-multi-window": dict(model="svm", N=64, T=40, C=16, subsequence_length=8, buffer_length=2, minibatch_size=2,
                             window_sampling="device"),
    "lgssm-marginal": dict(model="lgssm", kind="marginal", T=40, C=16, subsequence_length=8, buffer_length=4,
                           window_sampling="device"),
    "svm-adaptive": dict(model="svm", N=64, T=40, C=16, subsequence_length=8, buffer_length=2, ess_threshold=0.5,
                         window_sampling="device"),
}


def _twin_ensemble(case, **more):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    kw = dict(TWINS[case])
    kw.update(more)
    model, T, C = kw.pop("model"), kw.pop("T"), kw.pop("C")
    return ChainEnsemble(model, _series(model, T), default_params(model), num_chains=C, epsilon=0.01, seed=SEED,
                         chain_offset=OFF, sampler="sgld_cv", **kw)


def _descriptors(ens):
    from sgmcmc_ssm_amd import _capi
    return ens.desc_dev.cpu().numpy().reshape(-1).view(_capi.DEV_PROBLEM_DTYPE)


WINDOW_FIELDS = ("y", "weights", "T", "t1", "tL")


@pytest.mark.parametrize("case", sorted(TWINS))
def test_twins_at_the_centre(case):
    from sgmcmc_ssm_amd import _capi
    ens = _twin_ensemble(case)
    C, nd, model = ens.C, ens._nd, ens.model
    th0 = ens.theta_dev.cpu().numpy().copy()
    np.testing.assert_array_equal(ens.theta(), ens.centre())
    ctr0 = int(ens.step_ctr.item())
    ens.step(1)
    ens.synchronize()
    cur, centre = ens.cv_statistics()
    assert np.all(np.isfinite(cur[:, :_capi.STAT_DIM[model]])) and np.all(np.isfinite(cur[:, 4]))
    np.testing.assert_array_equal(cur[:, :5], centre[:, :5])
    # the twins' descriptors: their chains' in every field but theta, out and scratch
    d = _descriptors(ens)
    assert len(d) == 2 * nd
    for f in d.dtype.names:
        if f not in ("theta", "out", "scratch"):
            np.testing.assert_array_equal(d[f][nd:], d[f][:nd], err_msg=f)
    per = nd // C
    rows = ens.theta_centre_dev.data_ptr() + (np.arange(nd, dtype=np.uint64) // np.uint64(per)) * np.uint64(8 * _capi.MAX_THETA)
    np.testing.assert_array_equal(d["theta"][nd:], rows)
    assert len(set(d["out"].tolist())) == 2 * nd
    if case == "lgssm-f64-scratch":                     # every record its own slab
        assert ens.scratch_dev is not None
        slabs = np.sort(d["scratch"])
        assert slabs[0] == ens.scratch_dev.data_ptr() and np.all(np.diff(slabs) == ens.scratch_dev.numel() // (2 * nd))
    assert len(set(d["y"][:nd].tolist())) > 1           # the chains drew different windows
    if case == "svm-multi-window":
        np.testing.assert_array_equal(ens.twin_seq_len_dev.cpu().numpy(), ens.seq_len_dev.cpu().numpy())
        np.testing.assert_array_equal(ens.twin_out_dev.cpu().numpy()[:, :5], ens.win_out_dev.cpu().numpy()[:, :5])
    # the step was SGLD's on the centre gradient, from the same start, bit for bit
    rec = np.zeros((C, _capi.OUT_DOUBLES))
    rec[:, :4] = ens.centre_grad_dev.cpu().numpy()
    theta, outs, ctr = _dev(th0), _dev(rec), _counter(ctr0)
    _ctx().sgld_update_device(model, C, theta.data_ptr(), outs.data_ptr(), ens.hyper, ens.epsilon, float(ens.T),
                              ens.seed ^ UPDATE_SEED, ens.chain_offset, ctr.data_ptr())
    _sync()
    np.testing.assert_array_equal(ens.theta_dev.cpu().numpy(), theta.cpu().numpy())
    assert not np.array_equal(ens.theta_dev.cpu().numpy(), th0)
    # a second step: other windows, the twins' still their chains'
    before = {f: d[f][:nd].copy() for f in WINDOW_FIELDS}
    ens.step(1)
    ens.synchronize()
    d = _descriptors(ens)
    for f in WINDOW_FIELDS:
        np.testing.assert_array_equal(d[f][nd:], d[f][:nd], err_msg=f)
    assert not np.array_equal(d["y"][:nd], before["y"])
    cur, centre = ens.cv_statistics()
    assert not np.array_equal(cur[:, :4], centre[:, :4])           # theta has left the centre


# ---- kind='marginal': exact at the centre, a smaller variance away from it ----------------------------------------------------------
def test_marginal_gradient_at_the_centre_is_the_whole_series_gradient():
    ens = _twin_ensemble("lgssm-marginal")
    y = _series("lgssm", 40)
    ens.launch_windows()
    ens.launch_pf()
    ens.synchronize()
    cur, centre = ens.cv_statistics()
    g = cv.cv_gradient(cur, centre, ens.centre_gradient())[:, :4]
    want = kalman_records(ens.centre(), y)[:, :4]
    assert np.all(np.abs(g - want) <= 1e-9 * np.maximum(1.0, np.abs(want))), np.abs(g - want).max()
    np.testing.assert_array_equal(g, np.tile(g[0], (ens.C, 1)))    # every chain: the same centre, the same gradient
    assert len({tuple(r) for r in cur[:, :4]}) > ens.C // 2         # ... while the plain window gradients differ


def test_marginal_variance_falls_away_from_the_centre():
    """LGSSM, T = 200, S = 8, B = 4, 512 chains at theta = centre + 0.02 in A: per coordinate, the variance over chains of the
    control-variate gradient is below that of the plain scaled window gradient.  On the CPU (kalman_model.kalman_window over
    all 193 window starts of this series) the ratios are 2.1e-4 (LRinv), 5.8e-3 (LQinv), 2.4e-3 (C), 5.8e-3 (A)."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, generate_lgssm_data
    p = LGSSMParameters(A=np.eye(1) * 0.8, C=np.eye(1), Q=np.eye(1) * 0.3, R=np.eye(1) * 0.6)
    np.random.seed(21)
    y = generate_lgssm_data(T=200, parameters=p)["observations"][:, 0]
    C = 512
    start = np.tile(p.theta() + np.array([0.02, 0.0, 0.0, 0.0]), (C, 1))
    ens = ChainEnsemble("lgssm", y, start, kind="marginal", sampler="sgld_cv", centre=p.theta(), epsilon=1e-3, seed=5,
                        subsequence_length=8, buffer_length=4, window_sampling="device")
    np.testing.assert_array_equal(ens.centre(), np.tile(p.theta(), (C, 1)))
    ens.launch_windows()
    ens.launch_pf()
    ens.synchronize()
    cur, centre = ens.cv_statistics()
    g = cv.cv_gradient(cur, centre, ens.centre_gradient())[:, :4]
    v_cv, v_plain = g.var(axis=0), cur[:, :4].var(axis=0)
    print("variance over chains: control variate", v_cv, "plain", v_plain, "ratio", v_cv / v_plain)
    assert np.all(v_cv < v_plain), (v_cv, v_plain)


# ---- the reference's own SGD and ADAGRAD trajectories ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["sgd", "adagrad"])
def test_ensemble_reproduces_the_reference_trajectories(rule):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    z = np.load(GOLDEN)
    want = z[rule + "/trajectory"]                                  # [3, 6, 4], the start included
    ens = ChainEnsemble("lgssm", z["y"], z["theta0"].copy(), kind="marginal", sampler=rule, epsilon=float(z[rule + "/epsilon"]))
    got = ens.run(5)                                                # [5, 3, 4]
    np.testing.assert_allclose(np.transpose(got, (1, 0, 2)), want[:, 1:], rtol=1e-9, atol=0)
    if rule == "adagrad":
        assert np.all(ens.moment() > 0)


# ---- residency ---------------------------------------------------------------------------------------------------------------
def _resident(sampler, C=6, chain_offset=0, **more):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("svm")
    kw = dict(num_chains=C, N=64, epsilon=0.02, seed=17, chain_offset=chain_offset, subsequence_length=8, buffer_length=2,
              window_sampling="device", sampler=sampler)
    if sampler == "sgld_cv":        # a centre away from the start, its gradient averaged over two launches
        kw.update(centre=p.theta() * np.array([0.97, 1.02, 0.99]), centre_repeats=2)
    kw.update(more)
    return ChainEnsemble("svm", _series("svm", 40), p, **kw)


def _state(ens):
    """Everything a chain carries, as arrays."""
    out = [ens.theta_dev.cpu().numpy(), np.array([int(ens.step_ctr.item())])]
    if ens.sampler == "adagrad":
        out.append(ens.moment())
    if ens.sampler == "sgld_cv":
        out += [ens.centre(), ens.centre_grad_dev.cpu().numpy(), np.array([int(ens.centre_ctr_dev.item())])]
    return out


def _assert_same(a, b):
    for x, y in zip(_state(a), _state(b)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("sampler", ["adagrad", "sgld_cv"])
def test_graph_replay_equals_eager_steps(sampler):
    a, b = _resident(sampler), _resident(sampler)
    sa = a.run(8, thin=4, graph_steps=4)
    sb = b.run(8, thin=4)
    np.testing.assert_array_equal(sa, sb)
    _assert_same(a, b)
    assert len({tuple(r) for r in a.theta()}) == a.C and np.all(np.isfinite(a.theta()))


@pytest.mark.parametrize("sampler", ["adagrad", "sgld_cv"])
def test_checkpoint_and_resume(sampler):
    a = _resident(sampler)
    a.step(3)
    state = a.state_dict()
    assert ("moment" in state) == (sampler == "adagrad")
    assert all((k in state) == (sampler == "sgld_cv") for k in ("centre", "centre_gradient", "centre_ctr"))
    a.step(3)
    b = _resident(sampler, **(dict(centre=None, centre_repeats=1) if sampler == "sgld_cv" else {}))
    b.load_state_dict(state)
    b.step(3)
    _assert_same(a, b)
    if sampler == "sgld_cv":        # the counter of the centring launches travelled: re-centring gives the same gradient
        a.set_centre(repeats=2)
        b.set_centre(repeats=2)
        _assert_same(a, b)
        assert int(a.centre_ctr_dev.item()) == 4


def test_existing_checkpoints_keep_their_keys():
    state = _resident("sgld").state_dict()
    assert not {"moment", "centre", "centre_gradient", "centre_ctr"} & set(state)


@pytest.mark.parametrize("sampler", ["adagrad", "sgld_cv"])
def test_chains_do_not_depend_on_the_rank_partition(sampler):
    whole, lo, hi = _resident(sampler, C=6), _resident(sampler, C=3), _resident(sampler, C=3, chain_offset=3)
    for e in (whole, lo, hi):
        e.step(3)
        e.synchronize()
    for x, y, z in zip(_state(whole), _state(lo), _state(hi)):
        if x.ndim == 2:
            np.testing.assert_array_equal(x, np.concatenate([y, z]))
    if sampler == "sgld_cv":
        assert len({tuple(r) for r in whole.centre_gradient()}) == 6      # every chain its own centring draws


def test_recentring_mid_run_then_graph_replay():
    a, b = _resident("sgld_cv"), _resident("sgld_cv")
    a.run(2, thin=2, graph_steps=2)
    b.step(2)
    before = a.centre_gradient()
    a.set_centre()
    b.set_centre()
    np.testing.assert_array_equal(a.centre(), a.theta())
    assert not np.array_equal(a.centre_gradient(), before)
    sa = a.run(4, thin=2, graph_steps=2)            # the graph captured before the re-centring reads the new centre
    sb = b.run(4, thin=2)
    np.testing.assert_array_equal(sa, sb)
    _assert_same(a, b)


def test_a_non_finite_centre_gradient_is_refused():
    """(the Kalman launch: arithmetic only, a NaN observation)"""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    bad = _series("lgssm", 12).copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="sgld_cv: the centre gradient of chain 5 is not finite"):
        ChainEnsemble("lgssm", bad, default_params("lgssm"), num_chains=4, sampler="sgld_cv", kind="marginal", chain_offset=5)
    with pytest.raises(ValueError, match="belongs to sampler='sgld_cv'"):
        _resident("sgd").set_centre()
