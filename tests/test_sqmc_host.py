"""CPU: PMMH on sequential quasi-Monte Carlo (sampler='pmmh', sqmc=True) without a device -- the point set of
csrc/pfg_sqmc.hip (the net property under the digital shift, the rank formula, the comb form of the sorted u), the NumPy
restatement of the filter (tests/helpers/sqmc_model.py): its unbiasedness against the Kalman likelihood and the variance it buys
against the sorted filter on independent normals, ChainEnsemble._resolve_settings, and the header against the binding."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cpm_model as cp  # noqa: E402
import kalman_model as km  # noqa: E402
import keyed_draws as kd  # noqa: E402
import sqmc_model as sq  # noqa: E402

from sgmcmc_ssm_amd import _capi  # noqa: E402
from sgmcmc_ssm_amd.ensemble import ChainEnsemble  # noqa: E402
from sgmcmc_ssm_amd.tempering import TemperedPopulation  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
resolve = ChainEnsemble._resolve_settings
PM, PV, SEED = sq.PM, sq.PV, sq.SEED


def _shifts(n, seed):
    """n shift-word quadruples: random ones and the corners (all zeros, all ones)."""
    rs = np.random.RandomState(seed)
    w = rs.randint(0, 2 ** 32, size=(4, n), dtype=np.uint64)
    w[:, 0], w[:, 1] = 0, 0xFFFFFFFF
    return w


# ---- 1. the point set --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 11))
def test_shifted_points_are_a_net(m):
    """N = 2^m points under 12 digital shifts: every elementary interval 2^-a x 2^-(m-a), a = 0 .. m, holds exactly one point,
    and v lies in (0, 1) on the 2^-52 grid's midpoints."""
    N = 1 << m
    U, V = sq.shifted_points(N, _shifts(12, 100 + m))
    assert U.shape == (12, N) and U.max() < 2 ** 52 and V.max() < 2 ** 52
    for a in range(m + 1):
        cell = (U >> np.uint64(52 - a)) * np.uint64(1 << (m - a)) + (V >> np.uint64(52 - (m - a)) if m > a else np.uint64(0))
        assert np.array_equal(np.sort(cell, axis=1), np.tile(np.arange(N, dtype=np.uint64), (12, 1))), (m, a)
    v = sq.unit(V)
    assert np.all((v > 0) & (v < 1)) and np.array_equal(v * 2.0 ** 52 - 0.5, V.astype(np.float64))


@pytest.mark.parametrize("m", range(1, 11))
def test_rank_formula_and_comb(m):
    """i(k) = bitreverse_m(k ^ (s_a >> (32 - m))) is the argsort of u, and the sorted u are (k + delta) / N exactly."""
    N = 1 << m
    w = _shifts(12, 200 + m)
    U, _ = sq.shifted_points(N, w)
    u = sq.unit(U)
    order = sq.point_of_rank(N, w[0])
    assert np.array_equal(order, np.argsort(u, axis=1, kind="stable"))
    delta = sq.comb_offset(N, w[0], w[2])
    assert np.all((delta > 0) & (delta < 1))
    comb = (np.arange(N, dtype=np.float64)[None, :] + delta[:, None]) / N
    assert np.array_equal(np.take_along_axis(u, order, axis=1), comb)
    # ... in long double as well: nothing was rounded
    combl = (np.arange(N, dtype=np.longdouble)[None, :] + sq.comb_offset(N, w[0], w[2], F=np.longdouble)[:, None]) / np.longdouble(N)
    assert np.array_equal(combl.astype(np.float64), comb) and np.array_equal(combl, comb.astype(np.longdouble))


def test_sobol_direction_numbers():
    """The first points of the two coordinates: van der Corput and the second Sobol' dimension."""
    assert [int(v) >> 28 for v in sq.bitreverse32(np.arange(8))] == [0, 8, 4, 12, 2, 10, 6, 14]
    assert [int(v) >> 28 for v in sq.sobol2(np.arange(8))] == [0, 8, 12, 4, 10, 2, 6, 14]


def test_rows_are_keyed():
    """A chain's shifts are a pure function of (seed, chain id, counter, row); the high word of the id takes part."""
    a = sq.rows(5, 11, [3, 4, 2 ** 32 + 3], 7)
    assert a[0].shape == (3, 6) and len(np.unique(np.stack(a)[:, :2])) == 4 * 2 * 6
    assert not any(np.array_equal(a[q][0], a[q][2]) for q in range(4))
    b = sq.rows(5, 11, [4], 7)
    assert all(np.array_equal(a[q][1], b[q][0]) for q in range(4))
    assert not np.array_equal(a[0][0], sq.rows(5, 11, [3], 8)[0][0]) and not np.array_equal(a[0][0], sq.rows(5, 12, [3], 7)[0][0])
    assert np.array_equal(sq.rows(9, 11, [3], 7)[1][0, :6], a[1][0])          # a longer series begins with the shorter one's rows


# ---- 2. the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_filter_structure(model):
    """Parents are sorted positions, non-decreasing in the child's index, the estimate is the sum of its increments, the double
    evaluation agrees with the long-double one, and a recorded z replays."""
    N, T, B = 32, 9, 6
    th, y, _ = sq.case_theta_y(model, N, T, B)
    gids = kd.chain_ids(B, 2 ** 32 - 3)
    r = sq.loglik(model, th, y, N, PM, PV, SEED, gids, 5)
    assert np.all((r["anc"][:, 1:] >= 0) & (r["anc"][:, 1:] < N)) and np.all(r["anc"][:, 0] == -1)
    assert np.all(np.diff(r["anc"][:, 1:], axis=2) >= 0)
    np.testing.assert_allclose(r["inc"].sum(axis=1), r["ll"], rtol=1e-14)
    j = sq.loglik(model, th, y, N, PM, PV, SEED, gids, 5, F=np.longdouble, forced=r["anc"], z=r["z"])
    np.testing.assert_allclose(r["ll"], j["ll"].astype(float), rtol=0, atol=1e-11)
    assert not r["degenerate"].any() and sq.index_mismatches(r["anc"], j)[0] == 0
    assert not np.array_equal(sq.loglik(model, th, y, N, PM, PV, SEED, gids, 6)["ll"], r["ll"])
    y2 = y.copy()
    y2[2] = 1e300
    d = sq.loglik("svm", th[:, :3], y2, N, PM, PV, SEED, gids, 5)
    assert d["degenerate"].all() and np.all(d["ll"] == -np.inf)


@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_replay_cases_have_no_search_on_an_edge(model):
    """tests/test_gpu_sqmc.py leaves a search out of its comparison when its target lies within 1e-12 of a CDF entry.  For the
    shared cases and seed the model alone leaves out none, and every case is live."""
    assert {c[0] for c in sq.CASES} == {2, 64, 128, 256, 1024} and (64, 12, 5, 256) in sq.CASES
    for N, T, B, _ in sq.CASES:
        th, y, _ = sq.case_theta_y(model, N, T, B)
        r = sq.loglik(model, th, y, N, PM, PV, sq.filter_seed(SEED), kd.chain_ids(B, 2 ** 32 - 3), 5)
        assert not r["degenerate"].any() and np.all(np.isfinite(r["ll"]))
        wrong, left_out, total = sq.index_mismatches(r["anc"], r)
        assert (wrong, left_out) == (0, 0) and total == B * (T - 1) * N, (N, T, B, left_out)


# ---- 3. unbiasedness and variance -----------------------------------------------------------------------------------------------
def test_estimate_is_unbiased():
    """LGSSM, T = 8, N = 16, 4096 chains at one theta: the mean of exp(ll - ll_Kalman) lies within 5 sample standard errors of
    1 -- under the digital shift every point is uniform on its grid, which is all unbiasedness needs."""
    T, N, C = 8, 16, 4096
    th, y, _ = sq.case_theta_y("lgssm", N, T, 1)
    _, exact = km.kalman_window(th[0], y, 0, T, prior_mean=PM, prior_var=PV)
    ll = sq.loglik("lgssm", np.tile(th, (C, 1)), y, N, PM, PV, sq.filter_seed(SEED), kd.chain_ids(C, 0), 1)["ll"]
    ratio = np.exp(ll - exact)
    mean, se = ratio.mean(), ratio.std(ddof=1) / np.sqrt(C)
    print("mean", mean, "se", se, "z", (mean - 1) / se)
    assert abs(mean - 1.0) <= 5.0 * se, (mean, se)


@pytest.mark.parametrize("model", ["svm", "lgssm"])
def test_variance_against_the_sorted_filter_on_independent_normals(model):
    """T = 20, N = 64, 1024 chains at chain_filter_model.THETA: Var(ll_sqmc) < 0.5 Var(ll) of cpm_model.loglik on fresh normals
    (the sorted, systematic filter at rho = 0).  A prototype gave ratios 0.13 (LGSSM) and 0.30 (SVM)."""
    T, N, C = 20, 64, 1024
    _, y, _ = sq.case_theta_y(model, N, T, 1)
    th = np.tile(sq.THETA[model], (C, 1))
    a = sq.loglik(model, th, y, N, PM, PV, sq.filter_seed(SEED), kd.chain_ids(C, 0), 1)["ll"]
    U = np.random.RandomState(77).standard_normal((C, T + 1, N + 1))
    b = cp.loglik(model, th, y, U, PM, PV)["ll"]
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    va, vb = a.var(ddof=1), b.var(ddof=1)
    print(model, "var sqmc", va, "var sorted + iid", vb, "ratio", va / vb)
    assert va < 0.5 * vb, (va, vb)


# ---- 4. _resolve_settings ---------------------------------------------------------------------------------------------------
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


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        elif k != "proto":
            assert a[k] == b[k], k


@pytest.mark.parametrize("model,params", [("svm", _svm), ("lgssm", _lgssm)])
def test_resolve_settings_sqmc(model, params):
    base = dict(num_chains=5, N=8, sampler="pmmh", proposal_scale=0.1)
    s = resolve(model, Y, params(), sqmc=True, **base)
    assert s.sqmc is True and s.correlation is None
    assert (s.kind, s.pf, s.N, s.W, s.multi, s.S, s.T, s.stat) == ("pf", "poyiadjis_N", 8, 1, False, -1, 12, "none")
    # everything else is what plain PMMH resolves to, and sqmc = False IS plain PMMH: the same namespace, no new field
    plain = resolve(model, Y, params(), **base)
    _equal({k: v for k, v in vars(s).items() if k != "sqmc"}, vars(plain))
    _equal(vars(resolve(model, Y, params(), sqmc=False, **base)), vars(plain))
    assert not hasattr(plain, "sqmc")
    for N in (2, 64, 1024):
        assert resolve(model, Y, params(), sqmc=True, kernel="prior", pmmh_stat="none", minibatch_size=1, num_sequences=1,
                       **dict(base, N=N)).N == N


@pytest.mark.parametrize("kw,match", [
    (dict(sampler="sgld", proposal_scale=None), "belongs to sampler='pmmh', got sampler = 'sgld'"),
    (dict(sampler="pmala"), r"belongs to sampler='pmmh', got sampler = 'pmala' \(pMALA would need the score"),
    (dict(sampler="pgibbs", proposal_scale=None), "belongs to sampler='pmmh', got sampler = 'pgibbs'"),
    (dict(correlation=0.9), "correlation stays None"),
    (dict(dtype="f32"), "dtype 'f64'"),
    (dict(observations=[Y, Y]), "lists of sequences"),
    (dict(subsequence_length=4), "whole series"),
    (dict(buffer_length=2), "whole series"),
    (dict(minibatch_size=2), "W = 1 window"),
    (dict(kind="marginal"), "kind='pf', got kind = 'marginal'"),
    (dict(kind="complete"), "kind='pf'"),
    (dict(pf="nemeth"), "pf stays at its default"),
    (dict(resampling="systematic"), "resampling stays at its default"),
    (dict(resampling="stratified"), "resampling stays at its default"),
    (dict(ess_threshold=0.5), "adaptive resampling"),
    (dict(kernel="optimal"), "prior kernel"),
    (dict(pmmh_stat="score"), "pmmh_stat stays at its default"),
    (dict(N=1), "2 <= N <= 1024"),
    (dict(N=2048), "2 <= N <= 1024"),
    (dict(N=100), "power of two, got N = 100"),
    (dict(N=3), "power of two, got N = 3"),
])
def test_resolve_settings_sqmc_refusals(kw, match):
    args = dict(observations=Y, parameters=_lgssm(), num_chains=2, N=8, sampler="pmmh", proposal_scale=0.1, sqmc=True)
    args.update(kw)
    obs = args.pop("observations")
    with pytest.raises(NotImplementedError, match=match) as e:
        resolve("lgssm", obs, **args)
    assert str(e.value).startswith("sqmc (PMMH on sequential quasi-Monte Carlo")


def test_resolve_settings_sqmc_refuses_garch_and_tempering_refuses_sqmc():
    with pytest.raises(NotImplementedError, match="the sort orders a scalar state"):
        resolve("garch", Y, _garch(), num_chains=2, N=8, sampler="pmmh", proposal_scale=0.1, sqmc=True)
    with pytest.raises(NotImplementedError, match="sqmc stays False"):
        TemperedPopulation.resolve_settings("lgssm", _lgssm(), num_chains=8, sqmc=True, N=8)
    TemperedPopulation.resolve_settings("lgssm", _lgssm(), num_chains=8, sqmc=False, N=8)


# ---- 5. header and binding ----------------------------------------------------------------------------------------------------
def test_header_struct_matches_the_binding():
    src = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    body = re.search(r"typedef struct pfg_sqmc_problem \{(.*?)\} pfg_sqmc_problem;", src, flags=re.S).group(1)
    names, size = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        ctype, rest = decl.replace("const ", "").split(None, 1)
        fields = [f.strip().lstrip("*").strip() for f in rest.split(",")]
        names += fields
        size += (8 if pointer or ctype == "double" or "64" in ctype else 4) * len(fields)
    assert tuple(names) == _capi.SQMC_PROBLEM_DTYPE.names == ("theta", "y", "out", "trace_anc", "trace_ll", "trace_z", "prior_mean",
                                                              "prior_var", "T", "N")
    assert size == _capi.SQMC_PROBLEM_DTYPE.itemsize == 72          # no padding: pointers, doubles, then two int32
    lib = _capi.load_library()
    assert lib.pfg_struct_size(6) == 72 and lib.pfg_struct_size(5) == 88 and lib.pfg_struct_size(7) == -1
    assert "pfg_sqmc_device" in _capi.EXPORTS and hasattr(lib, "pfg_sqmc_device")
    assert re.search(r"int pfg_sqmc_device\(pfg_ctx \*ctx, int model, int dtype, int n_max, int B, const pfg_sqmc_problem \*problems, "
                     r"uint64_t seed,\s+uint64_t chain_offset, const uint64_t \*step_ctr, void \*hip_stream, int traced\);", src)


def test_tag_is_listed_and_disjoint():
    """The filter's tag 0x53510000 is stated in pfg_chains.hip's list and shares no value with the tags listed there or with the
    correlated filter's and the sweep's."""
    pkg = os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd", "csrc")
    chains = open(os.path.join(pkg, "pfg_chains.hip")).read()
    head = chains[:chains.index("#include")]
    assert "0x53510000" in head and "pfg_sqmc.hip" in head
    assert "kTagSqmc = 0x53510000u" in open(os.path.join(pkg, "pfg_sqmc.hip")).read()
    t = sq.TAG_SQMC
    assert t not in (0x5A11, 0x5A12, 0x504D0001, 0x504D0002, 0x504D0003, 0x4D4C0001, 0x4D4C0002, 0x4D4C0003, 0x534D0001)
    assert not cp.TAG_CPM <= t <= cp.TAG_CPM + 0x100 and not 0x43530000 <= t <= 0x4353FFFF and not 0x61B50000 <= t <= 0x61B5FFFF
    assert not 0x53000000 <= t < 0x53000000 + 1024 and not 0x57000000 <= t <= 0x57FFFFFF         # the window tags
    assert sq.SQMC_SEED_XOR == 0x53514D43 != cp.CPM_SEED_XOR
