"""Host: the inputs of tests/test_gpu_sorted_filter_edges.py (tests/helpers/sorted_edges.py) do what that file says they do --
checked on the model alone, from the keyed draws, before any launch -- and a rank sort without its tie pass would fail its
section 1 by a thousand times the tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cpm_model as cp  # noqa: E402
import keyed_draws as kd  # noqa: E402
import sorted_edges as se  # noqa: E402
import sqmc_model as sq  # noqa: E402

OFF, STEP = 2 ** 32 - 3, 5          # tests/test_gpu_sorted_score.py's
MODELS = ["svm", "lgssm"]
T, B = se.T_EDGE, se.B_EDGE
GENERIC = (cp.PM, cp.PV)
GIDS = kd.chain_ids(B, OFF)


def _proposed(U, rho):
    return se.host_proposal(U, rho, OFF, STEP)


# ---- the helper's filter is the models' --------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_run_is_the_two_models_filter(model):
    """sorted_edges.run against cpm_model.loglik and sqmc_model.loglik in double: ll, increments, parents and gaps bit for bit,
    free-running and forced, on generic, tied, sharp and clamped inputs."""
    cases = [cp.case_inputs(model, 100, T, B) + (GENERIC,), se.cpm_tie_inputs(model, 64) + (se.TIE_PRIOR["groups"],),
             se.cpm_tie_inputs(model, 3) + (se.TIE_PRIOR["all"],), se.cpm_flat_inputs(model, 200) + (GENERIC,),
             se.clamp_inputs(model, 128, -1, True) + (GENERIC,), se.clamp_inputs(model, 5, 1, True) + (GENERIC,)]
    for th, y, U, prior in cases:
        a, b = cp.loglik(model, th, y, U, prior[0], prior[1]), se.run_cpm(model, th, y, U, prior)
        forced = np.roll(a["anc"], 1, axis=2).clip(0)
        for x, z in ((a, b), (cp.loglik(model, th, y, U, prior[0], prior[1], forced=forced), se.run_cpm(model, th, y, U, prior, forced=forced))):
            for k in ("ll", "inc", "anc", "own", "gap", "degenerate"):
                assert np.array_equal(x[k], z[k], equal_nan=True), k
    seed = sq.filter_seed(sq.SEED)
    for (th, y), N, prior in ((sq.case_theta_y(model, 64, T, B)[:2], 64, GENERIC), (se.sqmc_tie_inputs(model, 128), 128, se.TIE_PRIOR["groups"]),
                              (se.sqmc_tie_inputs(model, 2), 2, se.TIE_PRIOR["all"]), (se.sqmc_flat_inputs(model, 256), 256, GENERIC)):
        a, b = sq.loglik(model, th, y, N, prior[0], prior[1], seed, GIDS, STEP), se.run_sqmc(model, th, y, N, prior, GIDS, STEP)
        for k in ("ll", "inc", "anc", "own", "gap", "degenerate"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- 1. ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("variant", ["all", "groups"])
def test_tie_inputs_tie(model, variant):
    """Every shape of section 1: the moves absorb their normals, no search on an edge, distinct states further than 1e-12
    apart, "all" keeps one state and the identity as parents, "groups" ties from the first resampling on; no chain is
    degenerate.  The count of distinct parents per step is printed."""
    for N in se.CPM_TIE_N["one wave"] + se.CPM_TIE_N["256 x 4"]:
        th, y, U = se.cpm_tie_inputs(model, N)
        d = se.tie_conditions(se.run_cpm(model, th, y, _proposed(U, 0.5), se.TIE_PRIOR[variant]), variant)
        print("cpm", model, variant, N, "distinct parents", int(d.min()), "..", int(d.max()))
        assert np.all(d == N) if variant == "all" else np.all(d >= 1)
    for N in sorted({n for n, _ in se.SQMC_TIE_SHAPES}):
        th, y = se.sqmc_tie_inputs(model, N)
        d = se.tie_conditions(se.run_sqmc(model, th, y, N, se.TIE_PRIOR[variant], GIDS, STEP), variant)
        print("sqmc", model, variant, N, "distinct parents", int(d.min()), "..", int(d.max()))


# ---- 2. the tests can see a broken tie pass ------------------------------------------------------------------------------------
def test_rank_sort_without_tie_pass_sorts_distinct_keys():
    """On distinct keys the emulation IS the sort: what it breaks is the tie pass alone."""
    rs = np.random.RandomState(5)
    x, lw = rs.standard_normal((B, 100)), rs.standard_normal((B, 100))
    for a, b in zip(se.rank_sort_without_tie_pass(x, lw, None), se.stable_sort(x, lw, None)):
        assert np.array_equal(a, b)
    x[:, 7] = x[:, 3]
    sx, slw = se.rank_sort_without_tie_pass(x, lw, (np.full((B, 100), 9.0), np.full((B, 100), 8.0)))
    rank = (x < x[:, 3:4]).sum(axis=1)
    rows = np.arange(B)
    assert np.array_equal(sx[rows, rank], x[:, 7]) and np.array_equal(slw[rows, rank], lw[:, 7])       # the highest index won
    assert np.all(sx[rows, rank + 1] == 9.0) and np.all(slw[rows, rank + 1] == 8.0)                    # the slot nobody wrote


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("N", se.CPM_TIE_N["one wave"])
def test_a_rank_sort_without_its_tie_pass_would_fail_section_1(model, N):
    """The "groups" inputs through a rank sort without its second pass: out[4] moves by more than 1e-6 -- a thousand times
    section 1's tolerance -- and at least one parent differs, in every chain."""
    th, y, U = se.cpm_tie_inputs(model, N)
    Up = _proposed(U, 0.5)
    good = se.run_cpm(model, th, y, Up, se.TIE_PRIOR["groups"])
    bad = se.run_cpm(model, th, y, Up, se.TIE_PRIOR["groups"], sort=se.rank_sort_without_tie_pass)
    dll = np.abs(bad["ll"] - good["ll"])
    moved = (bad["anc"] != good["anc"]).reshape(B, -1).sum(axis=1)
    print(model, N, "|d out[4]|", dll.tolist(), "parents that differ", moved.tolist())
    assert np.all(dll > 1e-6) and np.all(moved >= 1)


# ---- 3. the clamps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("sharp", [False, True], ids=["generic", "sharp"])
@pytest.mark.parametrize("rho", se.CLAMP_RHO)
@pytest.mark.parametrize("N", se.CLAMP_N)
def test_clamp_inputs_clamp(model, sharp, N, rho):
    """U' is finite and the model's uniform is exactly 0 / exactly 1 - 2^-53 at every step; no chain is degenerate; (N - 1) + u
    rounds to N in double; apart from the named child no search is on an edge.  u = 0: no leading weight sits where double
    cannot tell whether its exp is 0, and at N = 5 on the sharp inputs no weight at all has lw - max in (-800, -700) -- at
    N >= 128 some always do (61 of the leading weights of SVM at N = 128), so there the narrower condition stands alone.
    LGSSM, sharp: position 0 and N-1 carry no weight in most (chain, step)s, so the named answers are the unusual ones."""
    for sign in (-1, 1):
        th, y, U = se.clamp_inputs(model, N, sign, sharp)
        Up = _proposed(U, rho)
        assert np.all(np.isfinite(Up))
        u = cp.resampling_uniform(Up[:, 2:, N])
        assert np.all(u == (0.0 if sign < 0 else cp.U_MAX)) and np.all(np.abs(Up[:, 2:, N]) > 38.5)
        res = se.run_cpm(model, th, y, Up, GENERIC)
        assert not res["degenerate"].any()
        named = 0 if sign < 0 else N - 1
        wrong, left_out, n = se.index_mismatches(res["anc"], res, named)
        assert (wrong, left_out) == (0, 0) and n == B * (T - 1) * (N - 1)
        first = se.first_nonzero_weight(res)[:, 1:]
        last_zero = np.stack([res["steps"][t]["d"][:, N - 1] <= se.EXP_ZERO for t in range(1, T)], axis=1)
        print(model, N, "sharp" if sharp else "generic", sign, "first weight > 0 at", first.tolist(), "weight N-1 is 0", int(last_zero.sum()),
              "band", se.band_hits(res), "leading", se.leading_band_hits(res))
        if sign < 0:
            assert se.leading_near_exp_zero(res) == 0
            assert np.array_equal(res["own"][:, 1:, 0], first)           # (in double the model's own search agrees)
            if sharp and N == 5:
                assert se.band_hits(res) == 0
        else:
            assert np.float64(N - 1) + cp.U_MAX == np.float64(N) and np.all(res["own"][:, 1:, N - 1] == N - 1)
        if sharp and model == "lgssm":
            assert (first > 0).any() and last_zero.any()
            assert N < 128 or (2 * int((first > 0).sum()) > first.size and 2 * int(last_zero.sum()) > last_zero.size)


# ---- 4. flat CDFs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_sharp_inputs_flatten_the_cdf(model):
    """LRinv = 300: no chain is degenerate, no search on an edge, and at N >= 128 every chain has a step whose CDF holds a run of
    more than 3 equal entries -- leading zeros or trailing entries equal to the sum.  The weights are unimodal in the state and the CDF
    is in state order, so no such run lies between two parents: the second to PPT-th child of a thread goes past its 3 probes
    into cdf_search(cdf, N, target, j + 1) over tiny weights instead (counted: SVM at N >= 128, and u = 0 on the sharp inputs
    of section 3), and over the trailing run when the clamped last child finds no entry above W (counted: LGSSM,
    u = 1 - 2^-53)."""
    def longest_run(cdf):
        best = run = 1
        for a, b in zip(cdf[:-1], cdf[1:]):
            run = run + 1 if a == b else 1
            best = max(best, run)
        return best

    def conditions(res, N, what):
        assert not res["degenerate"].any()
        assert se.index_mismatches(res["anc"], res)[:2] == (0, 0)
        runs = [max(longest_run(st["cdf"][c]) for st in res["steps"].values()) for c in range(B)]
        past = se.bisect_searches(res, se.ppt_of(N))
        print(what, model, N, "longest run of equal entries per chain", runs, "distinct parents",
              int(se.distinct_parents(res).min()), "..", int(se.distinct_parents(res).max()), "searches past the probes", past)
        assert N < 128 or min(runs) > 3
        return past

    for N in se.FLAT_N["cpm"]:
        th, y, U = se.cpm_flat_inputs(model, N)
        past = conditions(se.run_cpm(model, th, y, _proposed(U, 0.5), GENERIC), N, "cpm")
        assert past >= 1 or model == "lgssm" or N < 128
    for N in se.FLAT_N["sqmc"]:
        th, y = se.sqmc_flat_inputs(model, N)
        past = conditions(se.run_sqmc(model, th, y, N, GENERIC, GIDS, STEP), N, "sqmc")
        assert past >= 1 or model == "lgssm"
    for N, rho in [(n, r) for n in se.CLAMP_N[1:] for r in se.CLAMP_RHO]:
        ppt = se.ppt_of(N)
        th, y, U = se.clamp_inputs(model, N, -1, True)
        low = se.run_cpm(model, th, y, _proposed(U, rho), GENERIC)
        th, y, U = se.clamp_inputs(model, N, 1, True)
        high = se.run_cpm(model, th, y, _proposed(U, rho), GENERIC)
        print("clamped", model, N, rho, "u = 0:", se.bisect_searches(low, ppt), "u = 1 - 2^-53:", se.bisect_searches(high, ppt),
              "of them over a run of equal entries", se.bisect_from_flat_runs(high, ppt))
        if model == "lgssm":
            assert se.bisect_from_flat_runs(high, ppt) >= 1
        else:
            assert se.bisect_searches(low, ppt) >= 1


# ---- 5. a chain that dies late ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 257])
@pytest.mark.parametrize("d", se.LATE_D)
def test_late_death_dies_at_step_d(N, d):
    """In double the chain fed +-1e300 from step d on has finite increments before d and none from d on; its neighbours live."""
    th, y, U = cp.case_inputs("svm", N, 6, B)
    res = cp.loglik("svm", th, se.late_death_y(y, B, 1, d), _proposed(U, 0.5), cp.PM, cp.PV)
    assert res["degenerate"].tolist() == [False, True, False]
    assert np.all(np.isfinite(res["inc"][1, :d])) and np.all(np.isnan(res["inc"][1, d:])) and np.all(np.isfinite(res["inc"][[0, 2]]))
