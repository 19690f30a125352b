"""CPU: sampler='pmala_sorted' without a device -- the NumPy restatement of the score the two sorted filters carry
(tests/helpers/sorted_score_model.py) against the oracle's nemeth / poyiadjis_N recursion, its column order at t = 0 by hand,
ChainEnsemble._resolve_settings (every refusal, the resolved values, exactly one of correlation / sqmc, no new field elsewhere),
the header against the binding, and the host chain step's own sanity."""
import os
import re
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_host_logic import PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cpm_model as cp  # noqa: E402
import keyed_draws as kd  # noqa: E402
import pmala_model as pa  # noqa: E402
import sorted_score_model as ss  # noqa: E402
import sqmc_model as sq  # noqa: E402

from sgmcmc_ssm_amd import _capi  # noqa: E402
from sgmcmc_ssm_amd.ensemble import ChainEnsemble, prior_hyper  # noqa: E402
from sgmcmc_ssm_amd.tempering import TemperedPopulation  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
resolve = ChainEnsemble._resolve_settings
PM, PV = cp.PM, cp.PV
TOL = 1e-9                  # of the terms' magnitude: the tolerance of the project's pins to the oracle


# ---- 1. the estimator against the oracle -------------------------------------------------------------------------------------
def _filter(which, model, th, y, N, T, B, lam, F=np.float64):
    """(res, z0 [B, N], z [B, T, N]) of the helper's filter on its own parents, with the normals the oracle is fed."""
    if which == "cpm":
        U = cp.case_inputs(model, N, T, B)[2]
        res = ss.cpm_score(model, th, y, U, PM, PV, lam=lam, F=F)
        return res, U[:, 0, :N], U[:, 1:, :N]
    res = ss.sqmc_score(model, th, y, N, PM, PV, sq.filter_seed(99), kd.chain_ids(B, 2 ** 32 - 1), 3, lam=lam, F=F)
    return res, res["z"][:, 0], res["z"][:, 1:]


@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("N", [2, 5, 64])
@pytest.mark.parametrize("which", ["cpm", "sqmc"])
@pytest.mark.parametrize("lam", [1.0, 0.95])
@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_score_is_the_oracles_on_the_same_parents(model, lam, which, N, T):
    """The helper's score and log-likelihood equal oracle.pf_oracle.pf_window(kernel='prior', pf='poyiadjis_N' | 'nemeth',
    stat='score') fed the same x_{-1} normals, state normals and parents: the parents mapped from sorted positions to particle
    indices through the returned orders (t = 0: the identity under CPM, the order of x_{-1} under SQMC).  1e-9 of the terms'
    magnitude."""
    if which == "sqmc" and N & (N - 1):
        N = 4               # SQMC takes powers of two: the odd size is CPM's
    B = 3
    th, y, _ = cp.case_theta_y(model, N, T, B)
    res, z0, z = _filter(which, model, th, y, N, T, B, lam)
    parents = ss.particle_parents(res)
    assert not res["degenerate"].any() and np.all(res["mag"] > 0)
    if which == "cpm":
        np.testing.assert_array_equal(parents[:, 0], np.broadcast_to(np.arange(N), (B, N)))
    for b in range(B):
        o = po.pf_window(model, th[b], y, N, z0[b], None, z[b], kernel="prior", pf="poyiadjis_N" if lam == 1.0 else "nemeth",
                         lambduh=lam, stat="score", prior_mean=PM, prior_var=PV, resampler=lambda t, lw: parents[b, t])
        assert np.all(np.abs(o["mean_statistic"] - res["score"][b]) <= TOL * res["mag"][b]), (o["mean_statistic"], res["score"][b])
        assert abs(o["loglikelihood_estimate"] - res["ll"][b]) <= TOL * max(1.0, abs(res["ll"][b]))


def test_the_filter_is_the_existing_helpers():
    """With the score beside it the filter is what cpm_model / sqmc_model restate: the same ll, increments and parents, bitwise."""
    for model in ("svm", "lgssm"):
        th, y, U = cp.case_inputs(model, 20, 7, 4)
        a, b = cp.loglik(model, th, y, U, PM, PV), ss.cpm_score(model, th, y, U, PM, PV, lam=0.95)
        th, y, _ = cp.case_theta_y(model, 16, 7, 4)
        gids = kd.chain_ids(4, 7)
        c, d = sq.loglik(model, th, y, 16, PM, PV, 5, gids, 2), ss.sqmc_score(model, th, y, 16, PM, PV, 5, gids, 2, lam=0.95)
        for want, got in ((a, b), (c, d)):
            for k in ("ll", "inc", "anc", "own"):
                np.testing.assert_array_equal(want[k], got[k], err_msg=k)


@pytest.mark.parametrize("which", ["cpm", "sqmc"])
@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_score_columns_at_t0_by_hand(model, which):
    """lambduh = 1, T = 1: the score is the weighted mean of add(x_{-1} -> x_0, y_0), columns [LRinv, LQinv, A] (SVM) and
    [LRinv, LQinv, C, A] (LGSSM), written out here."""
    N, B = 8, 2
    th, y, _ = cp.case_theta_y(model, N, 1, B)
    res, z0, z = _filter(which, model, th, y, N, 1, B, 1.0)
    for b in range(B):
        A, LQ, LR = th[b, 0], th[b, -2], th[b, -1]
        C = 1.0 if model == "svm" else th[b, 1]
        xm1 = PM + np.sqrt(PV) * z0[b]
        if which == "sqmc":
            xm1 = np.sort(xm1, kind="stable")
        x0 = A * xm1 + z[b, 0] / LQ
        dx = x0 - A * xm1
        g_A, g_LQ = (LQ * LQ + 1e-16) * dx * xm1, 1.0 / LQ - dx * dx * LQ
        if model == "svm":
            lw = -0.5 * y[0] ** 2 * np.exp(-x0) * (LR * LR + 1e-16) - 0.5 * x0
            cols = [1.0 / LR - y[0] ** 2 * np.exp(-x0) * LR, g_LQ, g_A]
        else:
            dy = y[0] - C * x0
            lw = -0.5 * dy * dy * (LR * LR + 1e-16)
            cols = [1.0 / LR - dy * dy * LR, g_LQ, (LR * LR + 1e-16) * dy * x0, g_A]
        w = np.exp(lw - lw.max())
        w /= w.sum()
        want = np.array([np.sum(w * c) for c in cols])
        assert np.all(np.abs(want - res["score"][b]) <= TOL * res["mag"][b]), (want, res["score"][b])


def test_lambduh_one_does_not_read_s_and_shrinkage_moves_the_score():
    th, y, U = cp.case_inputs("lgssm", 32, 7, 3)
    a, b = ss.cpm_score("lgssm", th, y, U, PM, PV, lam=1.0), ss.cpm_score("lgssm", th, y, U, PM, PV, lam=0.95)
    assert np.array_equal(a["ll"], b["ll"]) and np.array_equal(a["anc"], b["anc"]) and not np.allclose(a["score"], b["score"])


# ---- 2. _resolve_settings -----------------------------------------------------------------------------------------------------
Y = np.linspace(-1.0, 1.0, 12)
SVM, LG, GA = default_params("svm"), default_params("lgssm"), default_params("garch")
BASE = dict(num_chains=5, N=8, sampler="pmala_sorted", proposal_scale=0.1)
CPM_WHAT, SQMC_WHAT = "correlation (correlated pseudo-marginal PMMH", "sqmc (PMMH on sequential quasi-Monte Carlo"


@pytest.mark.parametrize("model,params", [("svm", SVM), ("lgssm", LG)])
@pytest.mark.parametrize("opt", [dict(correlation=0.9), dict(sqmc=True)], ids=["cpm", "sqmc"])
def test_resolved_values(model, params, opt):
    s = resolve(model, Y, params, **BASE, **opt)
    assert s.sorted_score == ("sqmc" if "sqmc" in opt else "cpm")
    assert (s.kind, s.pf, s.N, s.W, s.multi, s.S, s.T, s.stat, s.lambduh) == ("pf", "poyiadjis_N", 8, 1, False, -1, 12, "score", 1.0)
    assert s.correlation == opt.get("correlation") and getattr(s, "sqmc", False) == bool(opt.get("sqmc"))
    assert s.proposal_scale.shape == (_capi.MAX_THETA,)
    n = resolve(model, Y, params, pf="nemeth", **BASE, **opt)
    assert (n.pf, n.lambduh) == ("nemeth", 0.95)
    assert resolve(model, Y, params, pf="nemeth", lambduh=0.5, **BASE, **opt).lambduh == 0.5
    assert resolve(model, Y, params, pf="nemeth", lambduh=1.0, **BASE, **opt).lambduh == 1.0
    assert resolve(model, Y, params, kernel="prior", minibatch_size=1, num_sequences=1, **dict(BASE, N=1024), **opt).N == 1024
    assert resolve(model, Y, params, **dict(BASE, N=100), correlation=0.0).correlation == 0.0      # CPM takes any N <= 1024


def test_other_samplers_namespaces_have_no_new_field():
    """A plain 'pmala' / 'pmmh' / 'sgld' call, and 'pmmh' with correlation or sqmc, resolve to namespaces without the new field."""
    for kw in (dict(sampler="pmala", proposal_scale=0.1), dict(sampler="pmmh", proposal_scale=0.1), dict(),
               dict(sampler="pmmh", proposal_scale=0.1, correlation=0.9), dict(sampler="pmmh", proposal_scale=0.1, sqmc=True)):
        s = resolve("lgssm", Y, LG, num_chains=5, N=8, **kw)
        assert not hasattr(s, "sorted_score")
        want = {"proposal_scale", "kind", "pf", "N", "lambduh", "smoother", "launch_smoother", "stat", "paris", "Ntilde",
                "max_accept_reject", "M", "K", "W", "multi", "S", "B", "strict", "y", "T", "segments", "bounds", "draws", "rescale",
                "theta0", "proto", "ess_threshold", "correlation"} | ({"sqmc"} if kw.get("sqmc") else set())
        assert set(vars(s)) == want
    new = resolve("lgssm", Y, LG, correlation=0.9, **BASE)
    assert set(vars(new)) == want - {"sqmc"} | {"sorted_score"}


EXACTLY_ONE = "takes exactly one of correlation=rho .* and sqmc=True"
REFUSALS = [
    # exactly one of the two filters
    (ValueError, EXACTLY_ONE + ".*got neither", "lgssm", {}, dict()),
    (ValueError, EXACTLY_ONE + ".*got both", "lgssm", {}, dict(correlation=0.9, sqmc=True)),
    (ValueError, "pmmh_stat belongs to sampler='pmmh' \\(sampler='pmala_sorted' needs the score launch\\)", "lgssm", {},
     dict(correlation=0.9, pmmh_stat="score")),
    (ValueError, "pmmh_stat belongs to sampler='pmmh'", "lgssm", {}, dict(sqmc=True, pmmh_stat="none")),
    (ValueError, "sampler='pmala_sorted' needs proposal_scale", "lgssm", dict(proposal_scale=None), dict(sqmc=True)),
    (ValueError, r"correlation must lie in \[0, 1\)", "lgssm", {}, dict(correlation=1.0)),
    (ValueError, r"correlation must lie in \[0, 1\)", "lgssm", {}, dict(correlation=-0.1)),
    (ValueError, r"lambduh in \(0, 1\]", "lgssm", {}, dict(correlation=0.9, pf="nemeth", lambduh=0.0)),
    (ValueError, r"lambduh in \(0, 1\]", "lgssm", {}, dict(sqmc=True, pf="nemeth", lambduh=1.5)),
    (ValueError, r"lambduh in \(0, 1\]", "lgssm", {}, dict(sqmc=True, pf="nemeth", lambduh=float("nan"))),
    # the Kalman score is plain pMALA's
    (NotImplementedError, "kind='pf', got kind = 'marginal' \\(sampler='pmala' serves the exact Kalman score\\)", "lgssm", {},
     dict(correlation=0.9, kind="marginal")),
    (NotImplementedError, "kind='pf', got kind = 'complete'", "lgssm", {}, dict(sqmc=True, kind="complete", num_samples=4)),
    # smoothers without a sorted kernel, by name
    (NotImplementedError, "pf = 'poyiadjis_N' \\| 'nemeth', got pf = 'paris'", "lgssm", {}, dict(correlation=0.9, pf="paris")),
    (NotImplementedError, "pf = 'poyiadjis_N' \\| 'nemeth', got pf = 'poyiadjis_N2'", "lgssm", {}, dict(sqmc=True, pf="poyiadjis_N2")),
    (NotImplementedError, "power of two, got N = 100", "lgssm", dict(N=100), dict(sqmc=True)),
    (NotImplementedError, "the sort orders a scalar state", "garch", {}, dict(correlation=0.9)),
    (NotImplementedError, "the sort orders a scalar state", "garch", {}, dict(sqmc=True)),
]
# the family's shared refusals, under either filter, with the family's prefix
for _opt, _what in ((dict(correlation=0.9), CPM_WHAT), (dict(sqmc=True), SQMC_WHAT)):
    REFUSALS += [(NotImplementedError, re.escape(_what) + ".*" + m, "lgssm", kw, _opt) for kw, m in [
        (dict(dtype="f32"), "dtype 'f64'"), (dict(observations=[Y, Y]), "lists of sequences"),
        (dict(subsequence_length=4), "whole series"), (dict(buffer_length=2), "whole series"), (dict(minibatch_size=2), "W = 1 window"),
        (dict(resampling="systematic"), "resampling stays at its default"), (dict(resampling="stratified"), "resampling stays"),
        (dict(ess_threshold=0.5), "adaptive resampling"), (dict(kernel="optimal"), "prior kernel"),
        (dict(N=1), "2 <= N <= 1024"), (dict(N=2048), "2 <= N <= 1024")]]


@pytest.mark.parametrize("exc,match,model,kw,opt", REFUSALS)
def test_refusals(exc, match, model, kw, opt):
    args = dict(BASE, observations=Y, **opt)
    args.update(kw)
    obs = args.pop("observations")
    with pytest.raises(exc, match=match):
        resolve(model, obs, {"lgssm": LG, "svm": SVM, "garch": GA}[model], **args)


def test_the_pinned_refusals_stay_and_tempering_refuses_the_sampler():
    """'pmala' with correlation / sqmc, pmmh_stat='score' under either and pf='nemeth' under 'pmmh' are refused as before; the
    options alone do not switch the new sampler on; TemperedPopulation refuses it by name."""
    pa_kw, pm_kw = dict(num_chains=2, N=8, sampler="pmala", proposal_scale=0.1), dict(num_chains=2, N=8, sampler="pmmh", proposal_scale=0.1)
    with pytest.raises(NotImplementedError, match="pMALA would need a score that is smooth"):
        resolve("lgssm", Y, LG, correlation=0.9, **pa_kw)
    with pytest.raises(NotImplementedError, match="pMALA would need the score on the point set"):
        resolve("lgssm", Y, LG, sqmc=True, **pa_kw)
    for opt in (dict(correlation=0.9), dict(sqmc=True)):
        with pytest.raises(NotImplementedError, match="pmmh_stat stays at its default"):
            resolve("lgssm", Y, LG, pmmh_stat="score", **pm_kw, **opt)
        with pytest.raises(NotImplementedError, match="pf stays at its default"):
            resolve("lgssm", Y, LG, pf="nemeth", **pm_kw, **opt)
    with pytest.raises(ValueError, match="'pmala_sorted', 'pmala', 'gibbs' or 'pmmh'"):
        resolve("lgssm", Y, LG, num_chains=2, sampler="pmala_sort")
    for opt in (dict(correlation=0.9), dict(sqmc=True), dict()):
        with pytest.raises(NotImplementedError, match="sampler='pmala_sorted'.*is not built: sampler stays 'pmmh'"):
            TemperedPopulation.resolve_settings("lgssm", LG, num_chains=8, N=8, sampler="pmala_sorted", **opt)


# ---- 3. header and binding ----------------------------------------------------------------------------------------------------
def test_exports_header_and_binding():
    src = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    assert re.search(r"int pfg_cpm_score_device\(pfg_ctx \*ctx, int model, int dtype, int n_max, int B, const pfg_cpm_problem \*problems, "
                     r"double rho,\s+double lambduh, uint64_t seed, uint64_t chain_offset, const uint64_t \*step_ctr, void \*hip_stream,\s+"
                     r"int traced\);", src)
    assert re.search(r"int pfg_sqmc_score_device\(pfg_ctx \*ctx, int model, int dtype, int n_max, int B, const pfg_sqmc_problem \*problems, "
                     r"double lambduh,\s+uint64_t seed, uint64_t chain_offset, const uint64_t \*step_ctr, void \*hip_stream, int traced\);", src)
    lib = _capi.load_library()
    import ctypes as C
    for name, extra in (("pfg_cpm_score_device", [C.c_double, C.c_double]), ("pfg_sqmc_score_device", [C.c_double])):
        assert name in _capi.EXPORTS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p] + extra + \
            [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int] and fn.restype is C.c_int
    assert hasattr(_capi.Context, "cpm_score_device") and hasattr(_capi.Context, "sqmc_score_device")
    assert lib.pfg_version() == 126 and lib.pfg_struct_size(5) == 88 and lib.pfg_struct_size(6) == 72


# ---- 4. the chain model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_chain_step_at_a_vanishing_scale_accepts_with_log_alpha_zero(model):
    """proposal_scale -> 0 on the same normals (the host model takes rho = 1: U' = U): theta' -> theta, so the estimate, the
    score and with them both proposal densities meet -- log alpha -> 0 and every proposal is accepted.  At scale s the two
    log q differ by O(s |d|) and the estimates by O(s |score|): |log alpha| <= 1e-3 at s = 1e-7."""
    C, N, T, s = 8, 16, 6, 1e-7
    prior = PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)
    hy = prior_hyper(model, prior)
    th, y, U = cp.case_inputs(model, N, T, C)
    th = np.tile(default_params(model).theta(), (C, 1))
    r0 = ss.cpm_score(model, th, y, U, PM, PV, lam=0.95)
    ll, g = np.asarray(r0["ll"], dtype=np.float64), ss._grad4(r0["score"])
    # rho = 1 keeps U: the launch's eps has no weight
    m = ss.chain_step(model, prior, hy, th, ll, g, U, s, 1.0, 0.95, y, N, PM, PV, 11, 0, 0)
    assert m["valid"].all() and not m["amb"].any()
    np.testing.assert_array_equal(m["U_prop"], U)
    la = pa.log_alpha(model, prior, hy, s, th, m["prop"], ll, m["ll_prop"], g, m["grad_prop"]).astype(np.float64)
    assert np.all(np.abs(la) <= 1e-3), la
    assert m["accepted"].all() and np.array_equal(m["theta"], m["prop"]) and np.array_equal(m["grad"], m["grad_prop"])
    # and at a usable scale the step does reject: the decision is not vacuous
    big = [ss.chain_step(model, prior, hy, th, ll, g, U, 0.5, 0.5, 0.95, y, N, PM, PV, 11, 0, k) for k in range(4)]
    acc = np.concatenate([b["accepted"] for b in big])
    assert 0 < acc.sum() < acc.size
    for b in big:
        keep = ~b["accepted"]
        assert np.array_equal(b["theta"][keep], th[keep]) and np.array_equal(b["U"][keep], U[keep]) and np.array_equal(b["grad"][keep], g[keep])
