"""CPU: correlated pseudo-marginal PMMH (sampler='pmmh', correlation=rho) without a device -- the NumPy restatement of the sorted,
correlated filter (tests/helpers/cpm_model.py): its unbiasedness against the Kalman likelihood, what the correlation and the sort
buy in the variance of the accept ratio's noise, the seeds of the device replay, ChainEnsemble._resolve_settings, and the header
against the binding."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cpm_model as cp  # noqa: E402
import kalman_model as km  # noqa: E402
import keyed_draws as kd  # noqa: E402

from sgmcmc_ssm_amd import _capi  # noqa: E402
from sgmcmc_ssm_amd.ensemble import ChainEnsemble  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
resolve = ChainEnsemble._resolve_settings
PM, PV, SEED = cp.PM, cp.PV, cp.SEED


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------
def test_eps_is_keyed_by_row_and_column():
    """The draws of a launch: standard normals, a pure function of (seed, chain id, counter, row, column) -- a chain's array does
    not depend on which other chains are drawn with it, another counter or seed gives another array, and the columns of a wider
    array begin with the narrower one's (column c comes from draw c >> 2 whatever N is)."""
    a = cp.eps(5, 9, 11, [3, 4, 2 ** 32 + 3], 7)
    assert a.shape == (3, 6, 10)
    np.testing.assert_array_equal(a[1], cp.eps(5, 9, 11, [4], 7)[0])
    assert not np.array_equal(a[0], a[2])                                   # the high word of the chain id takes part
    assert not np.array_equal(a[0], cp.eps(5, 9, 11, [3], 8)[0]) and not np.array_equal(a[0], cp.eps(5, 9, 12, [3], 7)[0])
    np.testing.assert_array_equal(cp.eps(5, 14, 11, [3], 7)[0][:, :10], a[0])
    z = cp.eps(40, 255, 5, list(range(8)), 1).astype(float).reshape(-1)
    assert len(np.unique(z)) == z.size
    assert abs(z.mean()) < 4 / np.sqrt(z.size) and abs(z.var() - 1) < 4 * np.sqrt(2.0 / z.size)


def test_proposal_of_u():
    U = np.random.RandomState(1).standard_normal((2, 4, 6))
    up0, e = cp.propose_u(None, 0.0, 3, 5, 9, [0, 1], 2)
    np.testing.assert_array_equal(up0, e.astype(float))
    up, _ = cp.propose_u(U, 0.5, 3, 5, 9, [0, 1], 2)
    np.testing.assert_array_equal(up, 0.5 * U + np.sqrt(0.75) * up0)


@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_filter_structure(model):
    """Parents are sorted positions, non-decreasing in the child's index (systematic resampling on a sorted CDF), the estimate is
    the sum of its increments, and the double evaluation agrees with the long-double one."""
    N, T, B = 37, 9, 6
    th, y, U = cp.case_inputs(model, N, T, B)
    r = cp.loglik(model, th, y, U, PM, PV)
    assert np.all((r["anc"][:, 1:] >= 0) & (r["anc"][:, 1:] < N)) and np.all(r["anc"][:, 0] == -1)
    assert np.all(np.diff(r["anc"][:, 1:], axis=2) >= 0)
    np.testing.assert_allclose(r["inc"].sum(axis=1), r["ll"], rtol=1e-14)
    j = cp.loglik(model, th, y, U, PM, PV, F=np.longdouble, forced=r["anc"])
    np.testing.assert_allclose(r["ll"], j["ll"].astype(float), rtol=0, atol=1e-11)
    assert not r["degenerate"].any()
    # the sort matters: without it another genealogy
    assert not np.array_equal(cp.loglik(model, th, y, U, PM, PV, sort=False)["ll"], r["ll"])


def test_degenerate_chain_is_rejected():
    th, y, U = cp.case_inputs("svm", 8, 4, 3)
    y = y.copy()
    y[2] = 1e300
    r = cp.loglik("svm", th, y, U, PM, PV)
    assert r["degenerate"].all() and np.all(r["ll"] == -np.inf)


# ---- 2. unbiasedness -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, 5])
def test_sorted_systematic_estimate_is_unbiased(N):
    """LGSSM, T = 6: over 120 000 independent U ~ N(0, I), the mean of exp(ll(theta, U) - ll_Kalman(theta)) lies within 4
    standard errors of 1 -- the sorted, systematic filter on one uniform per step is an unbiased likelihood estimate for every
    N, which is all the exactness of the chain needs beside the reversibility of U -> U'."""
    T, n = 6, 120000
    th, y, _ = cp.case_inputs("lgssm", N, T, 1)
    _, exact = km.kalman_window(th[0], y, 0, T, prior_mean=PM, prior_var=PV)
    U = np.random.RandomState(1000 + N).standard_normal((n, T + 1, N + 1))
    ll = cp.loglik("lgssm", np.tile(th, (n, 1)), y, U, PM, PV)["ll"]
    ratio = np.exp(ll - exact)
    mean, se = ratio.mean(), ratio.std(ddof=1) / np.sqrt(n)
    print("N", N, "mean", mean, "se", se, "z", (mean - 1) / se)
    assert abs(mean - 1.0) <= 4.0 * se, (N, mean, se)


# ---- 3. what the correlation and the sort buy ----------------------------------------------------------------------------------
def test_correlation_needs_the_sort():
    """SVM, T = 100, N = 100, 256 chains at one theta: v(rho) = Var(ll(U') - ll(U)) over the chains, U' = rho U + sqrt(1 - rho^2)
    eps with the keyed eps.  v(0.99) < v(0) / 10 with the sort (a prototype measured 0.015 v(0)); without the sort
    v(0.99) > 0.3 v(0) (0.55 there): resampling in index order breaks the continuity the correlation relies on."""
    N, T, C = 100, 100, 256
    th, y, U = cp.case_inputs("svm", N, T, C)
    th = np.tile(cp.THETA["svm"], (C, 1))
    gids = kd.chain_ids(C, 0)

    def v(rho, sort):
        up, _ = cp.propose_u(U, rho, T, N, cp.filter_seed(SEED), gids, 1)
        d = cp.loglik("svm", th, y, up, PM, PV, sort=sort)["ll"] - cp.loglik("svm", th, y, U, PM, PV, sort=sort)["ll"]
        assert np.all(np.isfinite(d))
        return d.var(ddof=1)

    v0, v99, v99_plain = v(0.0, True), v(0.99, True), v(0.99, False)
    print("v(0)", v0, "v(0.99)", v99, "ratio", v99 / v0, "no sort", v99_plain, "ratio", v99_plain / v0)
    assert v99 < v0 / 10.0, (v99, v0)
    assert v99_plain > 0.3 * v0, (v99_plain, v0)


# ---- 4. the seeds of the device replay ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_replay_cases_have_no_search_on_an_edge(model):
    """tests/test_gpu_cpm.py leaves a search out of its comparison when its target lies within 1e-12 of a CDF entry.  For the
    shared cases and seed the model alone leaves out none (so whatever the device test leaves out comes from the device's own
    U' or summation order), every case is live, and the shapes are the ones the kernel's paths call for."""
    Ns, Ts, Bs, rhos = (set(c[k] for c in cp.CASES) for k in range(4))
    assert Ns == {2, 3, 5, 64, 100, 128, 129, 200, 256, 1000, 1024} and Ts == {1, 2, 7, 24}
    assert min(Bs) == 1 and max(Bs) == 70 and rhos == {0.0, 0.5, 0.99}
    for N, T, B, rho in cp.CASES:
        th, y, U = cp.case_inputs(model, N, T, B)
        up, _ = cp.propose_u(U, rho, T, N, cp.filter_seed(SEED), kd.chain_ids(B, 2 ** 32 - 3), 5)
        r = cp.loglik(model, th, y, up, PM, PV)
        assert not r["degenerate"].any() and np.all(np.isfinite(r["ll"]))
        wrong, left_out, total = cp.index_mismatches(r["anc"], r)
        assert (wrong, left_out) == (0, 0) and total == B * (T - 1) * N, (N, T, B, rho, left_out)


# ---- 5. _resolve_settings ------------------------------------------------------------------------------------------------------
Y = np.linspace(-1.0, 1.0, 12)


def _svm():
    from sgmcmc_ssm_amd.models.svm import SVMParameters
    return SVMParameters(A=np.eye(1) * 0.9, Q=np.eye(1) * 0.25, R=np.eye(1) * 0.7)


def _lgssm():
    from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters
    return LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1), Q=np.eye(1) * 0.25, R=np.eye(1) * 0.7)


def _garch():
    from sgmcmc_ssm_amd.models.garch import GARCHParameters
    return GARCHParameters(log_mu=0.0, logit_phi=0.0, logit_lambduh=0.0, LRinv=np.eye(1))


def _fields(ns):
    return {k: v for k, v in vars(ns).items() if k != "correlation"}


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        elif k != "proto":
            assert a[k] == b[k], k


@pytest.mark.parametrize("model,params", [("svm", _svm), ("lgssm", _lgssm)])
def test_resolve_settings_correlated(model, params):
    base = dict(num_chains=5, N=8, sampler="pmmh", proposal_scale=0.1)
    s = resolve(model, Y, params(), correlation=0.99, **base)
    assert s.correlation == 0.99 and isinstance(s.correlation, float)
    assert (s.kind, s.pf, s.N, s.W, s.multi, s.S, s.T, s.stat) == ("pf", "poyiadjis_N", 8, 1, False, -1, 12, "none")
    # everything else is what plain PMMH resolves to
    _equal(_fields(s), _fields(resolve(model, Y, params(), **base)))
    for N, rho in ((2, 0), (1024, 0.0), (100, 0.999999)):
        assert resolve(model, Y, params(), correlation=rho, kernel="prior", pmmh_stat="none", minibatch_size=1, num_sequences=1,
                       **dict(base, N=N)).correlation == float(rho)


@pytest.mark.parametrize("kw", [
    dict(model="svm", sampler="sgld"), dict(model="svm", sampler="pmmh", proposal_scale=0.2),
    dict(model="svm", sampler="pmmh", proposal_scale=0.2, pmmh_stat="score", resampling="stratified", N=3000),
    dict(model="svm", sampler="pmmh", proposal_scale=0.2, ess_threshold=0.5, pf="nemeth"),
    dict(model="garch", sampler="pmmh", proposal_scale=0.2, dtype="f32"), dict(model="lgssm", sampler="pmmh", proposal_scale=0.2, kind="marginal"),
    dict(model="svm", sampler="pmala", proposal_scale=0.2), dict(model="svm", sampler="pgibbs", N=8),
    dict(model="svm", sampler="sgld", subsequence_length=4, buffer_length=2), dict(model="lgssm", sampler="gibbs"),
])
def test_correlation_none_resolves_to_what_it_did(kw):
    """correlation = None (the default) changes nothing: passing it or leaving it out gives the same namespace, whose only new
    field says so."""
    kw = dict(kw)
    model = kw.pop("model")
    params = dict(svm=_svm, lgssm=_lgssm, garch=_garch)[model]()
    kw.setdefault("N", 16)
    a = resolve(model, Y, params, num_chains=3, **kw)
    b = resolve(model, Y, params, num_chains=3, correlation=None, **kw)
    assert a.correlation is None and b.correlation is None
    _equal(_fields(a), _fields(b))
    assert set(_fields(a)) == {"proposal_scale", "kind", "pf", "N", "lambduh", "smoother", "launch_smoother", "stat", "paris", "Ntilde",
                               "max_accept_reject", "M", "K", "W", "multi", "S", "B", "strict", "y", "T", "segments", "bounds", "draws",
                               "rescale", "theta0", "proto", "ess_threshold"}


@pytest.mark.parametrize("kw,exc,match", [
    (dict(sampler="sgld", proposal_scale=None), NotImplementedError, "belongs to sampler='pmmh', got sampler = 'sgld'"),
    (dict(sampler="pmala"), NotImplementedError, "belongs to sampler='pmmh', got sampler = 'pmala'"),
    (dict(sampler="pgibbs", proposal_scale=None), NotImplementedError, "belongs to sampler='pmmh', got sampler = 'pgibbs'"),
    (dict(dtype="f32"), NotImplementedError, "dtype 'f64'"),
    (dict(observations=[Y, Y]), NotImplementedError, "lists of sequences"),
    (dict(subsequence_length=4), NotImplementedError, "whole series"),
    (dict(buffer_length=2), NotImplementedError, "whole series"),
    (dict(minibatch_size=2), NotImplementedError, "W = 1 window"),
    (dict(kind="marginal"), NotImplementedError, "kind='pf'"),
    (dict(kind="complete"), NotImplementedError, "kind='pf'"),
    (dict(pf="nemeth"), NotImplementedError, "pf stays at its default"),
    (dict(pf="paris"), NotImplementedError, "pf stays at its default"),
    (dict(resampling="systematic"), NotImplementedError, "resampling stays at its default"),
    (dict(resampling="stratified"), NotImplementedError, "resampling stays at its default"),
    (dict(ess_threshold=0.5), NotImplementedError, "adaptive resampling"),
    (dict(kernel="optimal"), NotImplementedError, "prior kernel"),
    (dict(pmmh_stat="score"), NotImplementedError, "pmmh_stat stays at its default"),
    (dict(N=1), NotImplementedError, "2 <= N <= 1024"),
    (dict(N=1025), NotImplementedError, "2 <= N <= 1024"),
    (dict(correlation=1.0), ValueError, r"correlation must lie in \[0, 1\)"),
    (dict(correlation=-0.1), ValueError, r"correlation must lie in \[0, 1\)"),
    (dict(correlation=float("nan")), ValueError, r"correlation must lie in \[0, 1\)"),
    (dict(correlation="high"), ValueError, r"correlation must lie in \[0, 1\)"),
])
def test_resolve_settings_correlated_refusals(kw, exc, match):
    args = dict(observations=Y, parameters=_lgssm(), num_chains=2, N=8, sampler="pmmh", proposal_scale=0.1, correlation=0.9)
    args.update(kw)
    obs = args.pop("observations")
    with pytest.raises(exc, match=match):
        resolve("lgssm", obs, **args)


def test_resolve_settings_correlated_refuses_garch():
    with pytest.raises(NotImplementedError, match="the sort orders a scalar state"):
        resolve("garch", Y, _garch(), num_chains=2, N=8, sampler="pmmh", proposal_scale=0.1, correlation=0.9)


# ---- 6. header and binding ----------------------------------------------------------------------------------------------------
def test_header_struct_matches_the_binding():
    src = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    body = re.search(r"typedef struct pfg_cpm_problem \{(.*?)\} pfg_cpm_problem;", src, flags=re.S).group(1)
    names, size = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        ctype, rest = decl.replace("const ", "").split(None, 1)
        fields = [f.strip().lstrip("*").strip() for f in rest.split(",")]
        width = 8 if pointer or ctype == "double" or "64" in ctype else 4
        names += fields
        size += width * len(fields)
    assert tuple(names) == _capi.CPM_PROBLEM_DTYPE.names == ("theta", "y", "u0", "u1", "which", "out", "trace_anc", "trace_ll",
                                                             "prior_mean", "prior_var", "T", "N")
    assert size == _capi.CPM_PROBLEM_DTYPE.itemsize == 88           # no padding: pointers, doubles, then two int32
    lib = _capi.load_library()
    assert lib.pfg_struct_size(5) == 88 and lib.pfg_struct_size(2) == 376 and lib.pfg_version() == 126
    for name in ("pfg_cpm_aux_bytes", "pfg_cpm_device", "pfg_cpm_commit_device"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    for T, N in ((1, 2), (37, 129), (1000, 100), (5, 1024)):
        assert lib.pfg_cpm_aux_bytes(T, N) == _capi.cpm_aux_bytes(T, N) == ((T + 1) * (N + 1) * 8 + 255) // 256 * 256
    assert [lib.pfg_cpm_aux_bytes(T, N) for T, N in ((0, 8), (4, 1), (4, 1025))] == [-1, -1, -1]
    assert 2 * 12288 * _capi.cpm_aux_bytes(1000, 100) == 19881000960         # the 19.9 GB of the headline shape


def test_tags_are_listed_and_disjoint():
    """The filter's tags 0x43500000 | column >> 2 (at most 0x43500100) are stated in pfg_chains.hip's list and share no value
    with the tags listed there."""
    chains = open(os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd", "csrc", "pfg_chains.hip")).read()
    head = chains[:chains.index("#include")]
    assert "0x43500000 | column >> 2" in head and "pfg_cpm.hip" in head
    mine = range(cp.TAG_CPM, cp.TAG_CPM + (1024 >> 2) + 1)
    others = [0x5A11, 0x5A12, 0x504D0001, 0x504D0002, 0x504D0003, 0x4D4C0001, 0x4D4C0002, 0x4D4C0003]
    assert not any(t in mine for t in others)
    for lo, hi in ((0x61B50000, 0x61B5FFFF), (0x53000000, 0x53FFFFFF), (0x57000000, 0x57FFFFFF), (0x43530000, 0x4353FFFF)):
        assert mine[-1] < lo or mine[0] > hi
