"""CPU: sampler='pmmh' of ChainEnsemble without a device -- every refusal and resolved value through
ChainEnsemble._resolve_settings, the host restatement's own sanity (tests/helpers/pmmh_model.py), and which coordinates of
Prior.grad_logprior are the gradient of Prior.logprior in the raw parameterisation.

PMMH targets exp(Prior.logprior(theta)) p(y | theta) in the raw coordinates, SGLD drifts along Prior.grad_logprior.  A
central finite difference of logprior (step 1e-6) against grad_logprior, at the default priors (var 1 and 100):

    svm    A agrees, LRinv agrees, LQinv does NOT (the matrix-normal density of A has the row precision LQinv^2: its
           terms log LQinv - 0.5 LQinv^2 (A - mean_A)^2 / var_col_A are in logprior and not in grad_logprior)
    lgssm  A and C agree, LQinv and LRinv do NOT (the same terms, of A with LQinv and of C with LRinv)
    garch  log_mu and LRinv agree; logit_phi and logit_lambduh agreed as well wherever they were evaluated (to 1e-8), but
           are not asserted here: the reference's expression for them is not pinned as the gradient of its Beta log-density

So PMMH and SGLD target the same prior on (A, LRinv) of SVM, (A, C) of LGSSM and (log_mu, LRinv) of GARCH -- measured:
GARCH's other two as well -- and differ on the Cholesky factor that scales a coefficient's prior."""
import os
import sys

import numpy as np
import pytest

from sgmcmc_ssm_amd import _capi
from sgmcmc_ssm_amd.ensemble import ChainEnsemble
from test_host_logic import PRIORS, default_params, from_theta, vec

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import pmmh_model as pm  # noqa: E402

resolve = ChainEnsemble._resolve_settings
Y40 = np.zeros(40)
SEGS = [np.zeros(10), np.zeros(14), np.zeros(8)]
SVM, LG, GA = default_params("svm"), default_params("lgssm"), default_params("garch")
PM = dict(num_chains=4, N=64, sampler="pmmh", proposal_scale=0.1)
LIST = dict(num_sequences=-1, subsequence_length=-1, buffer_length=0, window_sampling="device")

REFUSALS = [
    (ValueError, "needs proposal_scale", ("svm", Y40, SVM), dict(num_chains=4, N=64, sampler="pmmh")),
    (ValueError, "proposal_scale must be a positive", ("svm", Y40, SVM), dict(PM, proposal_scale=0.0)),
    (ValueError, "proposal_scale must be a positive", ("svm", Y40, SVM), dict(PM, proposal_scale=[0.1, 0.1])),
    (ValueError, "proposal_scale must be a positive", ("svm", Y40, SVM), dict(PM, proposal_scale=[0.1, -0.1, 0.1])),
    (ValueError, "proposal_scale must be a positive", ("svm", Y40, SVM), dict(PM, proposal_scale=float("nan"))),
    # on another sampler
    (ValueError, "proposal_scale is the random walk of sampler='pmmh'", ("svm", Y40, SVM), dict(num_chains=4, N=64, proposal_scale=0.1)),
    (ValueError, "proposal_scale is the random walk of sampler='pmmh'",
     ("lgssm", Y40, LG), dict(num_chains=4, sampler="gibbs", proposal_scale=[0.1] * 4)),
    (ValueError, "pmmh_stat belongs to sampler='pmmh'", ("svm", Y40, SVM), dict(num_chains=4, N=64, pmmh_stat="score")),
    (ValueError, "pmmh_stat must be", ("svm", Y40, SVM), dict(PM, pmmh_stat="suff")),
    # subsampling
    (NotImplementedError, "pmmh needs the whole series", ("svm", Y40, SVM), dict(PM, subsequence_length=10, buffer_length=2)),
    (NotImplementedError, "pmmh needs the whole series", ("svm", Y40, SVM), dict(PM, buffer_length=2)),
    (NotImplementedError, "pmmh needs the whole series", ("svm", SEGS, SVM), dict(PM)),              # one sequence per step
    (NotImplementedError, "pmmh needs the whole series", ("svm", SEGS, SVM), dict(PM, **dict(LIST, num_sequences=2))),
    (NotImplementedError, "pmmh needs the whole series", ("svm", SEGS, SVM), dict(PM, **dict(LIST, subsequence_length=4))),
    (NotImplementedError, "pmmh needs the whole series", ("svm", SEGS, SVM), dict(PM, minibatch_size=2, **LIST)),
    (NotImplementedError, "pmmh needs the whole series", ("svm", Y40, SVM), dict(PM, minibatch_size=2)),
    # kinds and smoothers with no log-likelihood to accept on
    (NotImplementedError, "kind='complete' samples paths", ("lgssm", Y40, LG), dict(PM, kind="complete", num_samples=4)),
    (NotImplementedError, "smoothing of pf = 'paris'", ("svm", Y40, SVM), dict(PM, pf="paris")),
    (NotImplementedError, "smoothing of pf = 'poyiadjis_N2'", ("svm", Y40, SVM), dict(PM, pf="poyiadjis_N2")),
    (NotImplementedError, "N <= 16384", ("svm", Y40, SVM), dict(PM, N=20000)),
    (NotImplementedError, "kind='marginal'", ("svm", Y40, SVM), dict(PM, kind="marginal")),
    (NotImplementedError, "kind='marginal'", ("lgssm", Y40, LG), dict(PM, kind="marginal", dtype="f32")),
    (NotImplementedError, "kind='pf' only", ("lgssm", SEGS, LG), dict(PM, kind="marginal", **LIST)),
]


@pytest.mark.parametrize("exc, match, args, kw", REFUSALS)
def test_pmmh_refusals(exc, match, args, kw):
    with pytest.raises(exc, match=match):
        resolve(*args, **kw)


def test_the_old_refusal_names_pmmh_now():
    with pytest.raises(ValueError, match="'gibbs' or 'pmmh'"):
        resolve("svm", Y40, SVM, num_chains=2, sampler="hmc")


ACCEPTED = [
    # (args, kw) -> stat, smoother, launch smoother, multi
    (("svm", Y40, SVM), dict(PM), ("none", "nemeth", "nemeth", False)),
    (("svm", Y40, SVM), dict(PM, pmmh_stat="score"), ("score", "nemeth", "poyiadjis_n", False)),
    (("svm", Y40, SVM), dict(PM, pf="nemeth"), ("none", "nemeth", "nemeth", False)),
    (("garch", Y40, GA), dict(PM, resampling="stratified"), ("none", "nemeth_stratified", "nemeth_stratified", False)),
    (("garch", Y40, GA), dict(PM, resampling="systematic"), ("none", "nemeth_systematic", "nemeth_systematic", False)),
    (("lgssm", Y40, LG), dict(PM, ess_threshold=0.5), ("none", "nemeth", "nemeth", False)),
    (("lgssm", Y40, LG), dict(PM, dtype="f32"), ("none", "nemeth", "nemeth", False)),
    (("lgssm", Y40, LG), dict(PM, kind="marginal"), ("score", "kalman", "kalman", False)),
    (("lgssm", Y40, LG), dict(PM, subsequence_length=40), ("none", "nemeth", "nemeth", False)),       # S >= T: the whole series
    (("svm", SEGS, SVM), dict(PM, **LIST), ("none", "nemeth", "nemeth", True)),
    (("svm", Y40, SVM), dict(PM, minibatch_size=1), ("none", "nemeth", "nemeth", True)),
]


@pytest.mark.parametrize("args, kw, want", ACCEPTED)
def test_pmmh_resolved_values(args, kw, want):
    s = resolve(*args, **kw)
    assert (s.stat, s.smoother, s.launch_smoother, s.multi) == want
    P = _capi.THETA_DIM[args[0]]
    assert s.proposal_scale.shape == (_capi.MAX_THETA,) and np.all(s.proposal_scale[:P] == 0.1) and np.all(s.proposal_scale[P:] == 0)
    assert s.S == -1
    if s.multi:
        assert s.M == 1 and not s.draws and not s.rescale       # every sequence whole, out[4] summed, nothing rescaled
        assert s.W == (len(args[1]) if isinstance(args[1], list) else 1)


def test_proposal_scale_vector_and_other_samplers_unchanged():
    s = resolve("lgssm", Y40, LG, num_chains=2, sampler="pmmh", proposal_scale=[0.1, 0.2, 0.3, 0.4])
    np.testing.assert_array_equal(s.proposal_scale, [0.1, 0.2, 0.3, 0.4])
    s = resolve("svm", Y40, SVM, num_chains=2, sampler="pmmh", proposal_scale=[0.1, 0.2, 0.3])
    np.testing.assert_array_equal(s.proposal_scale, [0.1, 0.2, 0.3, 0.0])
    s = resolve("svm", Y40, SVM, num_chains=2, N=64)
    assert s.proposal_scale is None and s.stat == "score" and s.launch_smoother == "poyiadjis_n"


def test_exports_and_header():
    names = {"pfg_logprior_device", "pfg_pmmh_propose_device", "pfg_pmmh_accept_device"}
    assert names <= set(_capi.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "pfgrad.h")).read()
    assert all(n in src for n in names)


# ---- the restatement's own sanity ------------------------------------------------------------------------------------
def _start(model, C, seed=3):
    rs = np.random.RandomState(seed)
    th = default_params(model).theta() * rs.uniform(0.9, 1.1, size=(C, _capi.THETA_DIM[model]))
    if model == "lgssm":
        th[:, 1] = 1.0
    return th


@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_forced_invalid_proposals_move_nothing(model):
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    th0 = _start(model, 16)
    calls = []

    def loglik(th, ctr):
        calls.append(th.copy())
        return -np.sum(th ** 2, axis=1)

    th, ll, nacc, trace = pm.run_chains(model, prior, th0, 0.3, loglik, 11, 5, 6, force_invalid=True)
    np.testing.assert_array_equal(th, th0)
    np.testing.assert_array_equal(trace, np.broadcast_to(th0, trace.shape))
    np.testing.assert_array_equal(ll, -np.sum(th0 ** 2, axis=1))
    assert nacc.sum() == 0
    for c in calls:                                  # the launch only ever saw the current, legal parameters
        np.testing.assert_array_equal(c, th0)


@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_log_alpha_is_antisymmetric_and_chains_move(model):
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    a, b = _start(model, 12, seed=4), _start(model, 12, seed=5)
    lla, llb = np.linspace(-30, -20, 12), np.linspace(-25, -28, 12)
    fwd = pm.log_alpha(model, prior, a, b, lla, llb)
    bwd = pm.log_alpha(model, prior, b, a, llb, lla)
    scale = np.abs(lla) + np.abs(llb) + np.abs(pm.logprior(model, prior, a)) + np.abs(pm.logprior(model, prior, b))
    assert np.all(np.abs(fwd + bwd) <= 4 * pm.ULP * scale)
    # and a free run accepts some, rejects some, and keeps ll in step with theta
    th, ll, nacc, trace = pm.run_chains(model, prior, a, 0.05, lambda th, ctr: -np.sum(th ** 2, axis=1), 1, 0, 12)
    assert 0 < nacc.sum() < 12 * 12
    np.testing.assert_array_equal(ll, -np.sum(th ** 2, axis=1))


def test_support_and_normal_slots():
    th = np.array([[0.9999, 1.0, 0.5, 0.5], [0.99991, 1.0, 0.5, 0.5], [-0.9999, 1.0, 1e-300, 0.5], [0.5, 1.0, 0.0, 0.5],
                   [0.5, 1.0, 0.5, -0.1], [np.nan, 1.0, 0.5, 0.5]])
    np.testing.assert_array_equal(pm.in_support("lgssm", th), [True, False, True, False, False, False])
    np.testing.assert_array_equal(pm.in_support("garch", th), [True, True, True, True, False, False])
    pr = pm.propose("lgssm", th[:1], [0.1, 5.0, 0.1, 0.1], 1, 0, 1)
    assert pr.raw[0, 1] == 1.0                               # C stays 1 whatever its scale entry is
    z = pm.proposal_normals(1, 1, 0, 1)
    assert abs(float(pr.raw[0, 2] - (np.longdouble(0.5) + np.longdouble(0.1) * z[0, 2]))) < 1e-18
    # draws are keyed by the global chain id and the counter only
    np.testing.assert_array_equal(pm.proposal_normals(4, 9, 10, 3)[2:], pm.proposal_normals(2, 9, 12, 3))
    np.testing.assert_array_equal(pm.accept_uniform(4, 9, 10, 3)[2:], pm.accept_uniform(2, 9, 12, 3))
    assert not np.array_equal(pm.accept_uniform(2, 9, 12, 3), pm.accept_uniform(2, 9, 12, 4))


# ---- which coordinates of grad_logprior are the gradient of logprior ------------------------------------------------------
H = 1e-6
AGREE = {"svm": (0, 2), "lgssm": (0, 1), "garch": (0, 3)}        # asserted to agree
DIFFER = {"svm": (1,), "lgssm": (2, 3), "garch": ()}             # asserted to differ (see the module docstring)


@pytest.mark.parametrize("var", [1.0, 100.0])
@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_finite_difference_of_logprior_against_grad_logprior(model, var):
    """Tolerance: a logprior value carries the rounding of a handful of terms of size <= max(1, |logprior|) (scipy's
    log-densities and their lgamma constants), bounded here by 32 ulps of that size; the central difference divides the
    difference of two such values by 2 h, so its rounding error is at most 32 eps max(1, |lp|) / h (7e-8 at |lp| = 10),
    and its truncation error h^2 / 6 |f'''| is 1e-12 |f'''|, negligible beside it; theta_j +- h is rounded to an ulp of
    theta_j, which moves the step, and so the quotient, by at most 2 eps |theta_j| / h of the derivative.  Where the two
    disagree they do so by 0.1 or more."""
    prior = PRIORS[model].generate_default_prior(var=var, n=1, m=1)
    for mult in (0.93, 1.07):
        th = default_params(model).theta() * mult
        if model == "lgssm":
            th[1] = 1.0
        g = vec(model, prior.grad_logprior(from_theta(model, th)))
        lp = prior.logprior(from_theta(model, th))
        tol = 32 * np.finfo(float).eps * max(1.0, abs(lp)) / H
        fd = np.zeros(len(th))
        for j in range(len(th)):
            a, b = th.copy(), th.copy()
            a[j] += H
            b[j] -= H
            fd[j] = (prior.logprior(from_theta(model, a)) - prior.logprior(from_theta(model, b))) / (2 * H)
        print(model, var, mult, "grad", g, "fd", fd, "tol", tol)
        for j in AGREE[model]:
            assert abs(fd[j] - g[j]) <= tol + 2 * np.finfo(float).eps * abs(th[j]) / H * abs(g[j]), (model, j, fd[j], g[j])
        for j in DIFFER[model]:
            assert abs(fd[j] - g[j]) > 1e3 * tol, (model, j, fd[j], g[j])
