"""CPU: sampler = 'sgd' | 'adagrad' | 'sgld_cv' without a device -- the host restatement of the rules (tests/helpers/cv_model.py)
against the reference's own SGD / ADAGRAD trajectories (tests/golden/optim_rules.npz) and against SGLD's restatement,
ChainEnsemble._resolve_settings with every refusal, and the header against the binding."""
import os
import sys

import numpy as np
import pytest

from sgmcmc_ssm_amd import _capi
from sgmcmc_ssm_amd.ensemble import ChainEnsemble, prior_hyper
from test_host_logic import PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cv_model as cv  # noqa: E402
import keyed_draws as kd  # noqa: E402
from kalman_model import kalman_window  # noqa: E402

resolve = ChainEnsemble._resolve_settings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "optim_rules.npz")
Y40 = np.sin(np.arange(40.0))
NEW = ("pfg_sgd_update_device", "pfg_adagrad_update_device", "pfg_sgld_cv_update_device", "pfg_cv_accumulate_device")


def _rows(model, n, seed):
    rs = np.random.RandomState(seed)
    P = _capi.THETA_DIM[model]
    th = np.zeros((n, _capi.MAX_THETA))
    th[:, :P] = default_params(model).theta() * rs.uniform(0.8, 1.2, size=(n, P))
    if model == "lgssm":
        th[:, 1] = 1.0
    return th, rs.standard_normal((n, 8)), rs.standard_normal((n, 8)), rs.standard_normal((n, 4))


# ---- 1. the model: its two reductions to SGLD, the accumulation's order --------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_cv_model_reduces_to_sgld(model):
    hy = prior_hyper(model, PRIORS[model].generate_default_prior(var=1.0, n=1, m=1))
    th, outs, other, cg = _rows(model, 9, 1)
    key = (0.02, 50.0, 0x5EED0000C0DE1234, 2 ** 32 - 4, 7)
    # the same record on both sides: SGLD on the centre gradient
    rec = np.zeros((9, 8))
    rec[:, :4] = cg
    a = cv.sgld_cv_expected(model, th, outs, outs, cg, hy, *key)
    b = kd.sgld_expected(model, th, rec, hy, *key)
    np.testing.assert_array_equal(a.theta, b.theta)
    # no centre: SGLD on the record
    a = cv.sgld_cv_expected(model, th, outs, np.zeros((9, 8)), np.zeros((9, 4)), hy, *key)
    b = kd.sgld_expected(model, th, outs, hy, *key)
    np.testing.assert_array_equal(a.theta, b.theta)
    # and otherwise it is neither
    c = cv.sgld_cv_expected(model, th, outs, other, cg, hy, *key)
    assert not np.array_equal(c.theta, a.theta) and not np.array_equal(c.theta, b.theta)


def test_cv_gradient_operand_order():
    """centre_grad + (outs - outs_centre), not (centre_grad + outs) - outs_centre: the two differ in double."""
    o, oc, cg = np.full((1, 8), 1e16), np.full((1, 8), 1e16 - 2.0), np.full((1, 4), 0.3)
    assert cv.cv_gradient(o, oc, cg)[0, 0] == 0.3 + 2.0
    assert (cg[0, 0] + o[0, 0]) - oc[0, 0] != 0.3 + 2.0


def test_accumulate_expected():
    rs = np.random.RandomState(3)
    recs = [rs.standard_normal((5, 8)) * 10.0 ** rs.randint(-3, 4, size=(5, 8)) for _ in range(3)]
    one = cv.accumulate_expected(recs[:1])
    np.testing.assert_array_equal(one[:, :5], recs[0][:, :5])
    np.testing.assert_array_equal(one[:, 5:], 0.0)
    three = cv.accumulate_expected(recs)
    np.testing.assert_array_equal(three[:, :5], ((recs[0][:, :5] + recs[1][:, :5]) + recs[2][:, :5]) / 3.0)


# ---- 2. the reference's own SGD and ADAGRAD trajectories -----------------------------------------------------------------------
def _golden_hyper(z):
    return {k.split("/")[1]: float(z[k]) for k in z.files if k.startswith("hyper/")}


def kalman_records(theta, y):
    """[C, 8] records of the exact full-series score (tests/helpers/kalman_model.py), score-column order."""
    out = np.zeros((len(theta), 8))
    for c, th in enumerate(theta):
        g, ll = kalman_window(th, y, 0, len(y))
        out[c, :4], out[c, 4] = g, ll
    return out


@pytest.mark.parametrize("rule", ["sgd", "adagrad"])
def test_model_reproduces_the_reference_trajectories(rule):
    z = np.load(GOLDEN)
    y, hy, eps = z["y"], _golden_hyper(z), float(z[rule + "/epsilon"])
    hy.update(scale_mu=0.0, shape_mu=0.0, alpha_phi=0.0, beta_phi=0.0, alpha_lambduh=0.0, beta_lambduh=0.0)
    want = z[rule + "/trajectory"]                          # [3, 6, 4]
    np.testing.assert_array_equal(want[:, 0], z["theta0"])
    th, G = z["theta0"].copy(), np.zeros((3, 4))
    for k in range(1, want.shape[1]):
        recs = kalman_records(th, y)
        if rule == "sgd":
            e = cv.sgd_expected("lgssm", th, recs, hy, eps, float(len(y)))
        else:
            e = cv.adagrad_expected("lgssm", th, recs, hy, eps, float(len(y)), G)
            G = e.momentum.astype(np.float64)
        th = e.theta.astype(np.float64)
        np.testing.assert_allclose(th, want[:, k], rtol=1e-9, atol=0, err_msg="{0} step {1}".format(rule, k))
    assert np.all(np.abs(want[:, -1] - want[:, 0])[:, [0, 2, 3]] > 1e-3)        # the trajectories move


# ---- 3. _resolve_settings ---------------------------------------------------------------------------------------------------
def _p(model):
    return default_params(model)


@pytest.mark.parametrize("sampler", ["sgd", "adagrad"])
@pytest.mark.parametrize("kw", [
    dict(model="svm"), dict(model="garch", dtype="f32", subsequence_length=8, buffer_length=2, window_sampling="device"),
    dict(model="lgssm", kind="marginal"), dict(model="lgssm", kind="complete", num_samples=3),
    dict(model="svm", pf="paris", N=64), dict(model="svm", pf="poyiadjis_N2", N=64),
    dict(model="svm", resampling="stratified", N=3000), dict(model="svm", ess_threshold=0.5, pf="nemeth"),
    dict(model="svm", minibatch_size=2, subsequence_length=8, buffer_length=2, window_sampling="device"),
    dict(model="svm", observations=[Y40, Y40[:17]]),
])
def test_sgd_and_adagrad_resolve_to_what_sgld_does(sampler, kw):
    kw = dict(kw)
    model, obs = kw.pop("model"), kw.pop("observations", Y40)
    kw.setdefault("N", 16)
    a, b = vars(resolve(model, obs, _p(model), num_chains=3, sampler=sampler, **kw)), \
        vars(resolve(model, obs, _p(model), num_chains=3, sampler="sgld", **kw))
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        elif k != "proto":
            assert a[k] == b[k], k


@pytest.mark.parametrize("kw,want", [
    (dict(model="svm", N=64, subsequence_length=8, buffer_length=2, window_sampling="device"),
     ("pf", "nemeth", "poyiadjis_n", False, 1, 8, 1, 64)),
    (dict(model="garch", N=200, subsequence_length=8, buffer_length=2, pf="nemeth", dtype="f32", centre_repeats=8, centre_N=1000),
     ("pf", "nemeth", "nemeth", False, 1, 8, 8, 1000)),
    (dict(model="svm", N=16384, resampling="stratified", centre_N=16384), ("pf", "nemeth_stratified", "nemeth_stratified", False, 1, -1, 1, 16384)),
    (dict(model="svm", N=100, resampling="systematic"), ("pf", "nemeth_systematic", "nemeth_systematic", False, 1, -1, 1, 100)),
    (dict(model="svm", N=64, ess_threshold=0.5, centre_repeats=3), ("pf", "nemeth", "poyiadjis_n", False, 1, -1, 3, 64)),
    (dict(model="svm", N=64, minibatch_size=2, subsequence_length=8, buffer_length=2, window_sampling="device"),
     ("pf", "nemeth", "poyiadjis_n", True, 2, 8, 1, 64)),
    (dict(model="svm", N=64, minibatch_size=1), ("pf", "nemeth", "poyiadjis_n", True, 1, -1, 1, 64)),
    (dict(model="lgssm", kind="marginal", subsequence_length=8, buffer_length=4, centre_repeats=5),
     ("marginal", "kalman", "kalman", False, 1, 8, 1, 1000)),
])
def test_sgld_cv_resolved_values(kw, want):
    kw = dict(kw)
    model = kw.pop("model")
    s = resolve(model, Y40, _p(model), num_chains=3, sampler="sgld_cv", **kw)
    assert (s.kind, s.smoother, s.launch_smoother, s.multi, s.W, s.S, s.centre_repeats, s.centre_N) == want
    # everything else is what SGLD resolves to
    plain = {k: v for k, v in kw.items() if not k.startswith("centre")}
    b = vars(resolve(model, Y40, _p(model), num_chains=3, sampler="sgld", **plain))
    a = {k: v for k, v in vars(s).items() if k not in ("centre_repeats", "centre_N")}
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        elif k != "proto":
            assert a[k] == b[k], k


@pytest.mark.parametrize("kw,exc,match", [
    (dict(observations=[Y40, Y40]), NotImplementedError, "lists of sequences are not built"),
    (dict(pf="paris"), NotImplementedError, "got pf = 'paris'"),
    (dict(pf="poyiadjis_N2"), NotImplementedError, "got pf = 'poyiadjis_N2'"),
    (dict(model="lgssm", kind="complete", num_samples=2), NotImplementedError, "got kind = 'complete'"),
    (dict(N=16385), NotImplementedError, "N <= 16384"),
    (dict(centre_N=16385), NotImplementedError, "1 <= centre_N <= 16384"),
    (dict(centre_N=0), NotImplementedError, "1 <= centre_N <= 16384"),
    (dict(model="lgssm", kind="marginal", centre_N=100), ValueError, "centre_N has no particles to count"),
    (dict(centre_repeats=0), ValueError, "centre_repeats >= 1"),
    (dict(centre_repeats=1.5), ValueError, "centre_repeats >= 1"),
    (dict(sampler="sgld", centre=np.zeros(3)), ValueError, "belong to sampler='sgld_cv'.*got sampler = 'sgld'"),
    (dict(sampler="adagrad", centre_repeats=2), ValueError, "belong to sampler='sgld_cv'.*got sampler = 'adagrad'"),
    (dict(sampler="sgd", centre_N=64), ValueError, "belong to sampler='sgld_cv'.*got sampler = 'sgd'"),
    (dict(sampler="pmmh", proposal_scale=0.1, centre_N=64), ValueError, "belong to sampler='sgld_cv'"),
    (dict(sampler="sgdd"), ValueError, "sampler must be"),
])
def test_refusals(kw, exc, match):
    kw = dict(kw)
    model, obs = kw.pop("model", "svm"), kw.pop("observations", Y40)
    kw.setdefault("sampler", "sgld_cv")
    kw.setdefault("N", 64)
    with pytest.raises(exc, match=match):
        resolve(model, obs, _p(model), num_chains=2, **kw)


def test_sgld_cv_refusals_name_the_sampler():
    with pytest.raises(NotImplementedError, match="sampler='sgld_cv'"):
        resolve("svm", [Y40, Y40], _p("svm"), num_chains=2, sampler="sgld_cv")


@pytest.mark.parametrize("kw", [
    dict(model="svm", sampler="sgld"), dict(model="svm", sampler="sghmc", subsequence_length=4, buffer_length=2),
    dict(model="lgssm", sampler="sgrld", kind="marginal"), dict(model="lgssm", sampler="gibbs"),
    dict(model="svm", sampler="pmmh", proposal_scale=0.2), dict(model="svm", sampler="pmala", proposal_scale=0.2),
    dict(model="svm", sampler="pgibbs", N=8), dict(model="svm", sampler="pmmh", proposal_scale=0.2, correlation=0.9, N=8),
])
def test_existing_settings_resolve_as_before(kw):
    """Without the new keywords -- or with their defaults spelled out -- an existing sampler's namespace is what it was: the
    same fields, none of them new."""
    kw = dict(kw)
    model = kw.pop("model")
    kw.setdefault("N", 16)
    a = vars(resolve(model, Y40, _p(model), num_chains=3, **kw))
    b = vars(resolve(model, Y40, _p(model), num_chains=3, centre=None, centre_repeats=1, centre_N=None, **kw))
    assert set(a) == set(b) == {"proposal_scale", "kind", "pf", "N", "lambduh", "smoother", "launch_smoother", "stat", "paris",
                                "Ntilde", "max_accept_reject", "M", "K", "W", "multi", "S", "B", "strict", "y", "T", "segments",
                                "bounds", "draws", "rescale", "theta0", "proto", "ess_threshold", "correlation"}
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        elif k != "proto":
            assert a[k] == b[k], k


def test_the_new_keywords_come_last():
    import inspect
    sig = inspect.signature(ChainEnsemble.__init__)
    assert list(sig.parameters)[-3:] == ["centre", "centre_repeats", "centre_N"]
    assert list(inspect.signature(resolve).parameters)[-3:] == ["centre", "centre_repeats", "centre_N"]


# ---- 4. the header and the binding ------------------------------------------------------------------------------------------
def test_exports_and_header():
    assert set(NEW) <= set(_capi.EXPORTS)
    src = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    assert all("int {0}(pfg_ctx *ctx".format(n) in src for n in NEW)
    assert "#define PFG_VERSION 126" in src
    for n in NEW:
        assert hasattr(_capi.Context, n[len("pfg_"):])
