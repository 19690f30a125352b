"""CPU: sampler='pmala' of ChainEnsemble without a device -- every refusal and resolved value through
ChainEnsemble._resolve_settings, the exports, and the host restatement's own sanity (tests/helpers/pmala_model.py): the
acceptance ratio is antisymmetric, the proposal density is the product of univariate normals it claims to be, a proposal
outside the support moves nothing, and the draws have tags of their own."""
import os
import sys

import numpy as np
import pytest

from sgmcmc_ssm_amd import _capi
from sgmcmc_ssm_amd.ensemble import ChainEnsemble, prior_hyper
from test_host_logic import PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import keyed_draws as kd  # noqa: E402
import pmala_model as pa  # noqa: E402
import pmmh_model as pm  # noqa: E402

resolve = ChainEnsemble._resolve_settings
Y40 = np.zeros(40)
SEGS = [np.zeros(10), np.zeros(14), np.zeros(8)]
SVM, LG, GA = default_params("svm"), default_params("lgssm"), default_params("garch")
PA = dict(num_chains=4, N=64, sampler="pmala", proposal_scale=0.1)
LIST = dict(num_sequences=-1, subsequence_length=-1, buffer_length=0, window_sampling="device")

REFUSALS = [
    (ValueError, "sampler='pmala' needs proposal_scale", ("svm", Y40, SVM), dict(num_chains=4, N=64, sampler="pmala")),
    (ValueError, "proposal_scale must be a positive", ("svm", Y40, SVM), dict(PA, proposal_scale=0.0)),
    (ValueError, "proposal_scale must be a positive", ("svm", Y40, SVM), dict(PA, proposal_scale=[0.1, 0.1])),
    (ValueError, "proposal_scale must be a positive", ("svm", Y40, SVM), dict(PA, proposal_scale=[0.1, -0.1, 0.1])),
    (ValueError, "proposal_scale must be a positive", ("svm", Y40, SVM), dict(PA, proposal_scale=float("inf"))),
    (ValueError, "pmmh_stat belongs to sampler='pmmh'", ("svm", Y40, SVM), dict(PA, pmmh_stat="score")),
    (ValueError, "pmmh_stat belongs to sampler='pmmh'", ("svm", Y40, SVM), dict(PA, pmmh_stat="none")),
    # the other samplers' messages are what they were
    (ValueError, "proposal_scale is the random walk of sampler='pmmh'", ("svm", Y40, SVM), dict(num_chains=4, N=64, proposal_scale=0.1)),
    (ValueError, "pmmh_stat belongs to sampler='pmmh', got sampler = 'sgld'", ("svm", Y40, SVM), dict(num_chains=4, N=64, pmmh_stat="score")),
    (ValueError, "'pmala', 'gibbs' or 'pmmh'", ("svm", Y40, SVM), dict(num_chains=2, sampler="mala")),
    # subsampling
    (NotImplementedError, "pmala needs the whole series", ("svm", Y40, SVM), dict(PA, subsequence_length=10, buffer_length=2)),
    (NotImplementedError, "pmala needs the whole series", ("svm", Y40, SVM), dict(PA, buffer_length=2)),
    (NotImplementedError, "pmala needs the whole series", ("svm", SEGS, SVM), dict(PA)),              # one sequence per step
    (NotImplementedError, "pmala needs the whole series", ("svm", SEGS, SVM), dict(PA, **dict(LIST, num_sequences=2))),
    (NotImplementedError, "pmala needs the whole series", ("svm", SEGS, SVM), dict(PA, **dict(LIST, subsequence_length=4))),
    (NotImplementedError, "pmala needs the whole series", ("svm", SEGS, SVM), dict(PA, minibatch_size=2, **LIST)),
    (NotImplementedError, "pmala needs the whole series", ("svm", Y40, SVM), dict(PA, minibatch_size=2)),
    # kinds and smoothers it is not built for
    (NotImplementedError, "sampler='pmala'.*kind='complete' samples paths", ("lgssm", Y40, LG), dict(PA, kind="complete", num_samples=4)),
    (NotImplementedError, "sampler='pmala'.*score of pf = 'paris'", ("svm", Y40, SVM), dict(PA, pf="paris")),
    (NotImplementedError, "sampler='pmala'.*score of pf = 'poyiadjis_N2'", ("svm", Y40, SVM), dict(PA, pf="poyiadjis_N2")),
    (NotImplementedError, "sampler='pmala' is built for N <= 16384", ("svm", Y40, SVM), dict(PA, N=20000)),
    (NotImplementedError, "kind='marginal'", ("svm", Y40, SVM), dict(PA, kind="marginal")),
    (NotImplementedError, "kind='marginal'", ("lgssm", Y40, LG), dict(PA, kind="marginal", dtype="f32")),
    (NotImplementedError, "kind='pf' only", ("lgssm", SEGS, LG), dict(PA, kind="marginal", **LIST)),
    # the resampling corner keeps its refusals
    (NotImplementedError, "adaptive resampling .* is built for resampling='multinomial'", ("svm", Y40, SVM),
     dict(PA, resampling="stratified", ess_threshold=0.5)),
    (NotImplementedError, "systematic resampling is built for N <= 1024", ("svm", Y40, SVM), dict(PA, resampling="systematic", N=2048)),
]


@pytest.mark.parametrize("exc, match, args, kw", REFUSALS)
def test_pmala_refusals(exc, match, args, kw):
    with pytest.raises(exc, match=match):
        resolve(*args, **kw)


ACCEPTED = [
    # (args, kw) -> stat, smoother, launch smoother, multi: the score launch, as a full-series SGLD step launches it
    (("svm", Y40, SVM), dict(PA), ("score", "nemeth", "poyiadjis_n", False)),
    (("svm", Y40, SVM), dict(PA, pf="nemeth"), ("score", "nemeth", "nemeth", False)),
    (("garch", Y40, GA), dict(PA, resampling="stratified"), ("score", "nemeth_stratified", "nemeth_stratified", False)),
    (("garch", Y40, GA), dict(PA, resampling="systematic"), ("score", "nemeth_systematic", "nemeth_systematic", False)),
    (("lgssm", Y40, LG), dict(PA, ess_threshold=0.5), ("score", "nemeth", "poyiadjis_n", False)),
    (("lgssm", Y40, LG), dict(PA, dtype="f32"), ("score", "nemeth", "poyiadjis_n", False)),
    (("lgssm", Y40, LG), dict(PA, kind="marginal"), ("score", "kalman", "kalman", False)),
    (("lgssm", Y40, LG), dict(PA, subsequence_length=40), ("score", "nemeth", "poyiadjis_n", False)),   # S >= T: the whole series
    (("svm", SEGS, SVM), dict(PA, **LIST), ("score", "nemeth", "poyiadjis_n", True)),
    (("svm", Y40, SVM), dict(PA, minibatch_size=1), ("score", "nemeth", "poyiadjis_n", True)),
]


@pytest.mark.parametrize("args, kw, want", ACCEPTED)
def test_pmala_resolved_values(args, kw, want):
    s = resolve(*args, **kw)
    assert (s.stat, s.smoother, s.launch_smoother, s.multi) == want
    # ... which is what the SGLD ensemble of the same settings resolves to
    sg = resolve(*args, **{k: v for k, v in kw.items() if k not in ("sampler", "proposal_scale")})
    assert (sg.stat, sg.smoother, sg.launch_smoother, sg.multi, sg.lambduh) == want + (s.lambduh,)
    P = _capi.THETA_DIM[args[0]]
    assert s.proposal_scale.shape == (_capi.MAX_THETA,) and np.all(s.proposal_scale[:P] == 0.1) and np.all(s.proposal_scale[P:] == 0)
    assert s.S == -1
    if s.multi:
        assert s.M == 1 and not s.draws and not s.rescale       # every sequence whole, the records summed, nothing rescaled
        assert s.W == (len(args[1]) if isinstance(args[1], list) else 1)


def test_proposal_scale_vector_and_other_samplers_unchanged():
    s = resolve("lgssm", Y40, LG, num_chains=2, sampler="pmala", proposal_scale=[0.1, 0.2, 0.3, 0.4])
    np.testing.assert_array_equal(s.proposal_scale, [0.1, 0.2, 0.3, 0.4])
    s = resolve("svm", Y40, SVM, num_chains=2, sampler="pmala", proposal_scale=[0.1, 0.2, 0.3])
    np.testing.assert_array_equal(s.proposal_scale, [0.1, 0.2, 0.3, 0.0])
    s = resolve("svm", Y40, SVM, num_chains=2, N=64)
    assert s.proposal_scale is None and s.stat == "score" and s.launch_smoother == "poyiadjis_n"
    s = resolve("svm", Y40, SVM, num_chains=2, N=64, sampler="pmmh", proposal_scale=0.1)
    assert (s.stat, s.smoother, s.launch_smoother) == ("none", "nemeth", "nemeth")
    s = resolve("lgssm", Y40, LG, num_chains=2, sampler="gibbs")
    assert s.proposal_scale is None and (s.kind, s.stat) == ("complete", "gibbs")


def test_exports_and_header():
    names = {"pfg_pmala_propose_device", "pfg_pmala_accept_device"}
    assert names <= set(_capi.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "pfgrad.h")).read()
    assert all(n in src for n in names)
    assert hasattr(_capi.Context, "pmala_propose_device") and hasattr(_capi.Context, "pmala_accept_device")


# ---- the restatement's own sanity ------------------------------------------------------------------------------------
MODELS = ["svm", "garch", "lgssm"]


def _start(model, C, seed=3):
    rs = np.random.RandomState(seed)
    th = default_params(model).theta() * rs.uniform(0.9, 1.1, size=(C, _capi.THETA_DIM[model]))
    if model == "lgssm":
        th[:, 1] = 1.0
    return th


def _toy_for(model):
    """A smooth stand-in for the launch: log-likelihood -|theta|^2 and its gradient, in score columns."""
    def f(th, ctr):
        g = np.zeros((th.shape[0], 4))
        for j, col in enumerate(pa.SCORE_COL[model]):
            g[:, col] = -2.0 * th[:, j]
        return -np.sum(th ** 2, axis=1), g
    return f


@pytest.mark.parametrize("model", MODELS)
def test_log_alpha_is_antisymmetric(model):
    """log alpha(a -> b) + log alpha(b -> a) = 0 to rounding for random pairs of (theta, g, ll): the q-ratio carries the
    reverse term with the reverse state's own score.  Tolerance: 8 ulps of the sum of the terms' magnitudes."""
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    hy = prior_hyper(model, prior)
    rs = np.random.RandomState(8)
    a, b = _start(model, 12, seed=4), _start(model, 12, seed=5)
    ga, gb = rs.normal(size=(12, 4)) * 5, rs.normal(size=(12, 4)) * 5
    lla, llb = np.linspace(-30, -20, 12), np.linspace(-25, -28, 12)
    scale = [0.1, 0.2, 0.15, 0.3]
    fwd = pa.log_alpha(model, prior, hy, scale, a, b, lla, llb, ga, gb)
    bwd = pa.log_alpha(model, prior, hy, scale, b, a, llb, lla, gb, ga)
    size = (np.abs(lla) + np.abs(llb) + np.abs(pm.logprior(model, prior, a)) + np.abs(pm.logprior(model, prior, b)) +
            np.abs(pa.log_q(model, a, b, gb, scale, hy)) + np.abs(pa.log_q(model, b, a, ga, scale, hy))).astype(float)
    assert np.all(np.isfinite(fwd.astype(float))) and np.any(np.abs(fwd) > 1.0)
    assert np.all(np.abs(fwd + bwd) <= 8 * pm.ULP * size)
    # the q-ratio is doing work: with both scores exchanged the ratio changes
    other = pa.log_alpha(model, prior, hy, scale, a, b, lla, llb, gb, ga)
    assert np.all(np.abs(other - fwd) > 1e-6)


@pytest.mark.parametrize("model", MODELS)
def test_log_q_is_a_product_of_univariate_normals(model):
    """log_q against a second spelling: the sum over the free coordinates of the N(a_j + (s_j^2 / 2) d_j, s_j) log-density,
    with d spelled from Prior.grad_logprior (the host's own prior gradient, not the mirror's) and the common constant
    -sum_j log(s_j sqrt(2 pi)) added back.  1e-12 relative to the sum of the terms: the two spellings round differently (the
    host's gradient is double) but agree on every term."""
    from test_host_logic import from_theta, vec
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    hy = prior_hyper(model, prior)
    rs = np.random.RandomState(9)
    a, b = _start(model, 10, seed=6), _start(model, 10, seed=7)
    g = rs.normal(size=(10, 4)) * 3
    sc = np.array([0.1, 0.2, 0.15, 0.3])[:pa.P_DIM[model]]
    got = pa.log_q(model, b, a, g, sc, hy).astype(float)
    for c in range(10):
        gl = np.asarray(vec(model, prior.grad_logprior(from_theta(model, a[c]))), dtype=float)     # theta order
        want = terms = 0.0
        for j in pa.FREE[model]:
            d = gl[j] + g[c, pa.SCORE_COL[model][j]]
            mean, sd = a[c, j] + 0.5 * sc[j] ** 2 * d, sc[j]
            lp = -0.5 * ((b[c, j] - mean) / sd) ** 2 - np.log(sd * np.sqrt(2 * np.pi))
            want += lp + np.log(sd * np.sqrt(2 * np.pi))
            terms += abs(lp) + abs(np.log(sd * np.sqrt(2 * np.pi)))
        assert abs(got[c] - want) <= 1e-12 * terms, (model, c, got[c], want)
    if model == "lgssm":        # C takes no density term whatever its entries are
        b2, a2 = b.copy(), a.copy()
        b2[:, 1], a2[:, 1] = 7.0, -3.0
        g2 = g.copy()
        g2[:, 2] = 1e6
        np.testing.assert_array_equal(pa.log_q(model, b2, a2, g2, sc, hy), pa.log_q(model, b, a, g, sc, hy))


@pytest.mark.parametrize("model", MODELS)
def test_forced_invalid_proposals_move_nothing(model):
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    hy = prior_hyper(model, prior)
    th0 = _start(model, 16)
    calls = []
    toy = _toy_for(model)

    def launch(th, ctr):
        calls.append(th.copy())
        return toy(th, ctr)

    th, ll, g, nacc, trace = pa.run_chains(model, prior, hy, th0, 0.3, launch, 11, 5, 6, force_invalid=True)
    np.testing.assert_array_equal(th, th0)
    np.testing.assert_array_equal(trace, np.broadcast_to(th0, trace.shape))
    ll0, g0 = toy(th0, 0)
    np.testing.assert_array_equal(ll, ll0)
    np.testing.assert_array_equal(g, g0)
    assert nacc.sum() == 0
    for c in calls:                                  # the launch only ever saw the current, legal parameters
        np.testing.assert_array_equal(c, th0)


@pytest.mark.parametrize("model", MODELS)
def test_free_chains_move_and_keep_their_estimates(model):
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    hy = prior_hyper(model, prior)
    toy = _toy_for(model)
    th, ll, g, nacc, trace = pa.run_chains(model, prior, hy, _start(model, 12, seed=4), 0.3, toy, 1, 0, 12)
    assert 0 < nacc.sum() < 12 * 12
    ll1, g1 = toy(th, 0)
    np.testing.assert_array_equal(ll, ll1)              # ll and g in step with theta
    np.testing.assert_array_equal(g, g1)
    if model == "lgssm":
        assert np.all(trace[:, :, 1] == 1.0)


def test_a_non_finite_estimate_rejects():
    prior = PRIORS["lgssm"].generate_default_prior(var=1.0, n=1, m=1)
    hy = prior_hyper("lgssm", prior)
    a, b = _start("lgssm", 6, seed=4), _start("lgssm", 6, seed=5)
    g = np.ones((6, 4))
    gp = g.copy()
    gp[0, 0], gp[1, 3], gp[2, 2] = np.nan, np.inf, np.nan           # column 2 is C's: not used
    llp = np.full(6, 1e6)                                           # anything finite would be accepted
    llp[3] = np.nan
    acc, margin = pa.accept("lgssm", prior, hy, 0.1, a, b, np.ones(6), np.zeros(6), llp, g, gp, 1, 0, 1)
    np.testing.assert_array_equal(acc, [False, False, True, False, True, True])
    assert np.all(np.isinf(margin[[0, 1, 3]])) and np.all(np.isfinite(margin[[2, 4, 5]]))
    acc, _ = pa.accept("lgssm", prior, hy, 0.1, a, b, np.zeros(6), np.zeros(6), llp, g, gp, 1, 0, 1)
    assert not acc.any()


def test_tags_slots_and_keys():
    tags = {pa.TAG_Z01, pa.TAG_Z23, pa.TAG_U}
    assert tags == {0x4D4C0001, 0x4D4C0002, 0x4D4C0003}
    assert not tags & {pm.TAG_Z01, pm.TAG_Z23, pm.TAG_U, 0x5A11, 0x5A12}
    assert all((t >> 16) not in (0x61B5,) and (t >> 24) not in (0x53, 0x57) for t in tags)      # Gibbs, window tags
    assert not np.array_equal(pa.proposal_normals(4, 9, 10, 3), pm.proposal_normals(4, 9, 10, 3))
    assert not np.array_equal(pa.accept_uniform(4, 9, 10, 3), pm.accept_uniform(4, 9, 10, 3))
    # PMMH's slot assignment: SVM z0, z1, z2; LGSSM z0, z2, z3 (C takes none); GARCH z0..z3
    assert pa.Z_SLOT == {"svm": (0, 1, 2), "lgssm": (0, None, 2, 3), "garch": (0, 1, 2, 3)}
    z = pa.proposal_normals(1, 1, 0, 1)
    for model in MODELS:
        prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
        hy = prior_hyper(model, prior)
        th, g = _start(model, 1), np.full((1, 4), 0.5)
        sc = [0.1, 5.0, 0.1, 0.1][:pa.P_DIM[model]]
        pr = pa.propose(model, th, g, sc, 1, 0, 1, hy)
        mean, _ = pa.proposal_mean(model, th, g, sc, hy)
        for j, k in enumerate(pa.Z_SLOT[model]):
            if k is None:
                assert pr.raw[0, j] == 1.0                       # C stays 1 whatever its scale entry is
            else:
                assert abs(float(pr.raw[0, j] - (mean[0, j] + np.longdouble(sc[j]) * z[0, k]))) < 1e-17
        # the drift: the prior gradient sgld_update_kernel adds plus the score column of the coordinate
        d, _ = pa.drift(model, th, g, hy)
        gp, _ = kd.prior_gradient(model, th.astype(np.longdouble), kd._hy(hy))
        for j in pa.FREE[model]:
            assert float(abs(d[0, j] - (gp[0, j] + 0.5))) < 1e-15
    # draws are keyed by the global chain id and the counter only
    np.testing.assert_array_equal(pa.proposal_normals(4, 9, 10, 3)[2:], pa.proposal_normals(2, 9, 12, 3))
    np.testing.assert_array_equal(pa.accept_uniform(4, 9, 10, 3)[2:], pa.accept_uniform(2, 9, 12, 3))
    assert not np.array_equal(pa.accept_uniform(2, 9, 12, 3), pa.accept_uniform(2, 9, 12, 4))


def test_with_half_squared_scale_eps_over_T_the_proposal_is_the_sgld_step():
    """s_j^2 / 2 = eps / T for every j: the proposal's mean and standard deviation are those of sgld_update_kernel's step
    before project_parameters (keyed_draws.sgld_expected states that step: drift eps (grad_logprior + g) / T, noise
    sqrt(2 eps / T) z)."""
    eps, T = 0.05, 40.0
    s = np.sqrt(2 * eps / T)
    for model in MODELS:
        prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
        hy = prior_hyper(model, prior)
        th, g = _start(model, 5), np.random.RandomState(2).normal(size=(5, 8))
        mean, _ = pa.proposal_mean(model, th, g[:, :4], s, hy)
        gp, _ = kd.prior_gradient(model, th.astype(np.longdouble), kd._hy(hy))
        want = th + eps * ((gp + g[:, list(kd.SCORE_COL[model])]) / T)
        for j in pa.FREE[model]:
            assert np.all(np.abs((mean[:, j] - want[:, j]).astype(float)) <= 4 * pm.ULP * (np.abs(th[:, j]) + 1.0))
