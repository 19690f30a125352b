"""GPU: the four sorted-filter kernel families (pfg_cpm_device, pfg_cpm_score_device, pfg_sqmc_device, pfg_sqmc_score_device;
csrc/pfg_cpm.hip, csrc/pfg_sqmc.hip, csrc/pfg_chain_filter.hpp) on the inputs generic draws never produce
(tests/helpers/sorted_edges.py), each launch replayed in long double as tests/test_gpu_cpm.py, test_gpu_sqmc.py and
test_gpu_sorted_score.py replay theirs, with their tolerances: 1e-9 on the increments, out[4] and the score, 1e-14 on U', at most
1 search in 10^4 left out as on an edge, exact equality for the children named below.  What a wrong kernel would have to get
wrong to fail, per section:

  1. ties     Equal states (LQinv = 1e30: every child of one parent is bitwise its sibling).  A sort that does not yield a
              permutation under equal keys -- the second pass of the one-wave rank sort (key_less on (state, index) behind its
              extra block_sync and scatter), the index tie-break of the bitonic comparator, its +inf padding beside tied real
              keys -- leaves two particles in one slot and a stale or unwritten (sx, slw, si) in another: the CDF is then
              built from other weights, and the parents, the increments, out[4] and the score move by far more than 1e-9
              (tests/test_sorted_filter_edges_host.py shows > 1e-6 and other parents for a rank sort without its second pass).
              "all": every state equal, so the order must be the index order itself and every parent its child's index.
              Within a tie group the particles are interchangeable in every output: these tests pin "the sort yields a
              permutation under ties", not the order inside a group.
  2. (host)   tests/test_sorted_filter_edges_host.py: the evidence that section 1 sees a broken tie pass.
  3. clamps   u = 0 and u = 1 - 2^-53 exactly.  A search that returns a leading zero-weight position for a target of exactly 0
              (cdf[j] >= target instead of cdf[j] > target), or one that runs past N-1 or stops short of it when no entry
              exceeds the target W, fails the two named children, which are compared exactly and never left out as "on an
              edge".  On the sharp inputs the first answer is not 0 and the second names a particle of zero weight: the
              documented "clamped to N-1" (DESIGN section 7).
  4. flat     LRinv = 300: nearly every weight underflows; the CDF starts with a run of zeros, ends with a run of entries equal
              to the sum, and a step keeps few parents.  A search that mishandles equal entries (stops inside a run, or bounds
              the bisection that follows the 3 probes by the wrong end) picks other parents.  The weights are a unimodal
              function of the state and the CDF is in the order of the states, so a run of equal entries can only lead or
              trail: the probe-then-bisect hand-over is reached over tiny weights (SVM, and u = 0 on the sharp inputs of
              section 3) and over the trailing run by the clamped last child (u = 1 - 2^-53 on them); the host test counts
              both.
  5. late     A chain that dies at the weights of step d = 1, 3, 5 (5: the last step, t == T).  A tail loop that starts at the
              wrong row, or does not run from t = T, leaves rows of U' unwritten (the launch fills them with 0: not the
              proposal) or writes past row T into the padding.
"""
import functools
import os
import sys

import numpy as np
import pytest

from test_gpu_sorted_score import ANC_FILL, LL_FILL, OFF, STEP, TOL, Z_FILL, launch_cpm, launch_sqmc

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import cpm_model as cp  # noqa: E402
import keyed_draws as kd  # noqa: E402
import sorted_edges as se  # noqa: E402
import sorted_score_model as ss  # noqa: E402
import sqmc_model as sq  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
H = ss.H_DIM
LAMS = [1.0, 0.95]
MODELS = ["svm", "lgssm"]
T, B = se.T_EDGE, se.B_EDGE
GENERIC = (cp.PM, cp.PV)


def prior_edit(prior):
    def edit(d):
        d["prior_mean"], d["prior_var"] = prior
    return edit


def check_score(model, got_out, ref, lam):
    """out[0..H-1] against the long-double replay to TOL of the terms' magnitude; a column whose terms are all 0 (the A column
    when every move has dx = 0) is compared absolutely.  Slots H .. 3 and 5 .. 7 are 0."""
    h = H[model]
    want, mag = ref["score"].astype(np.float64), ref["mag"].astype(np.float64)
    err = np.abs(got_out[:, :h] - want) / np.where(mag > 0, mag, 1.0)
    print("score", model, "lambduh", lam, "max |d| / mag", float(err.max()), "mag", float(mag.min()), "..", float(mag.max()))
    assert np.all(np.isfinite(got_out[:, :h])) and np.all(mag >= 0)
    assert np.all(err <= TOL), float(err.max())
    assert np.all(got_out[:, h:4] == 0.0) and np.all(got_out[:, 5:] == 0.0)


def check_indices(anc, ref, N, skip_child=None):
    assert np.all(anc[:, 0] == ANC_FILL) or np.all(anc[:, 0] == -1)
    assert np.all((anc[:, 1:] >= 0) & (anc[:, 1:] < N)) and np.all(np.diff(anc[:, 1:], axis=2) >= 0)
    wrong, left_out, n = se.index_mismatches(anc, ref, skip_child)
    print("indices", n, "left out", left_out, "wrong", wrong)
    assert wrong == 0 and left_out * 10000 <= n, (wrong, left_out, n)
    return left_out


def check_cpm(model, th, y, U, N, rho, prior=GENERIC, skip_child=None, free=False):
    """The standard replay of one correlated-filter case, STAT none and score: the traced launch on the U' it wrote, teacher-forced
    (free: free-running too) in long double; production against traced, bitwise; the score launches bitwise the same filter,
    their score to TOL.  Returns (the traced STAT-none launch, its teacher-forced replay)."""
    edit = prior_edit(prior)
    got = launch_cpm(model, th, y, U, N, rho, None, edit=edit)
    want_u = se.host_proposal(U, rho, OFF, STEP)
    assert np.all(np.isfinite(got["U_prop"]))
    assert np.all(np.abs(got["U_prop"] - want_u) <= 1e-14 * np.maximum(1.0, np.abs(want_u)))
    anc = got["trace_anc"].astype(np.int64)
    ref = se.run_cpm(model, th, y, got["U_prop"], prior, F=LD, forced=anc)
    assert not ref["degenerate"].any()
    left_out = check_indices(anc, ref, N, skip_child)
    np.testing.assert_allclose(got["trace_ll"], ref["inc"].astype(np.float64), rtol=TOL, atol=TOL)
    np.testing.assert_allclose(got["out"][:, 4], ref["ll"].astype(np.float64), rtol=TOL, atol=TOL)
    assert np.all(got["out"][:, [0, 1, 2, 3, 5, 6, 7]] == 0.0)
    if free:
        own = se.run_cpm(model, th, y, got["U_prop"], prior, F=LD)
        assert left_out > 0 or np.array_equal(own["anc"][:, 1:], anc[:, 1:])
        np.testing.assert_allclose(got["out"][:, 4], own["ll"].astype(np.float64), rtol=TOL, atol=TOL)
    prod = launch_cpm(model, th, y, U, N, rho, None, traced=False, edit=edit)
    assert np.array_equal(prod["out"], got["out"]) and np.array_equal(prod["U_prop"], got["U_prop"])
    assert np.all(prod["trace_anc"] == ANC_FILL) and np.all(prod["trace_ll"] == LL_FILL)
    for lam in LAMS:
        sc = launch_cpm(model, th, y, U, N, rho, lam, edit=edit)
        for k in ("U_prop", "U_cur", "trace_anc", "trace_ll"):
            assert np.array_equal(sc[k], got[k]), k
        assert np.array_equal(sc["out"][:, 4], got["out"][:, 4])
        prod = launch_cpm(model, th, y, U, N, rho, lam, traced=False, edit=edit)
        assert np.array_equal(prod["out"], sc["out"]) and np.array_equal(prod["U_prop"], sc["U_prop"])
        sref = ss.cpm_score(model, th, y, sc["U_prop"], prior[0], prior[1], lam=lam, F=LD, forced=anc)
        assert not sref["degenerate"].any()
        np.testing.assert_allclose(sc["out"][:, 4], sref["ll"].astype(np.float64), rtol=TOL, atol=TOL)
        check_score(model, sc["out"], sref, lam)
    return got, ref


def check_sqmc(model, th, y, N, n_max, prior=GENERIC, free=False):
    """As check_cpm for the SQMC filter, on the normals the launch recorded."""
    edit = prior_edit(prior)
    gids, seed = kd.chain_ids(B, OFF), sq.filter_seed(sq.SEED)
    got = launch_sqmc(model, th, y, N, n_max, None, edit=edit)
    anc = got["trace_anc"].astype(np.int64)
    assert np.all(np.isfinite(got["trace_z"]))
    ref = se.run_sqmc(model, th, y, N, prior, gids, STEP, z=got["trace_z"], F=LD, forced=anc)
    assert not ref["degenerate"].any()
    left_out = check_indices(anc, ref, N)
    np.testing.assert_allclose(got["trace_ll"], ref["inc"].astype(np.float64), rtol=TOL, atol=TOL)
    np.testing.assert_allclose(got["out"][:, 4], ref["ll"].astype(np.float64), rtol=TOL, atol=TOL)
    assert np.all(got["out"][:, [0, 1, 2, 3, 5, 6, 7]] == 0.0)
    if free:
        own = se.run_sqmc(model, th, y, N, prior, gids, STEP, z=got["trace_z"], F=LD)
        assert left_out > 0 or np.array_equal(own["anc"][:, 1:], anc[:, 1:])
        np.testing.assert_allclose(got["out"][:, 4], own["ll"].astype(np.float64), rtol=TOL, atol=TOL)
    prod = launch_sqmc(model, th, y, N, n_max, None, traced=False, edit=edit)
    assert np.array_equal(prod["out"], got["out"])
    assert np.all(prod["trace_anc"] == ANC_FILL) and np.all(prod["trace_ll"] == LL_FILL) and np.all(prod["trace_z"] == Z_FILL)
    for lam in LAMS:
        sc = launch_sqmc(model, th, y, N, n_max, lam, edit=edit)
        for k in ("trace_anc", "trace_ll", "trace_z"):
            assert np.array_equal(sc[k], got[k]), k
        assert np.array_equal(sc["out"][:, 4], got["out"][:, 4])
        prod = launch_sqmc(model, th, y, N, n_max, lam, traced=False, edit=edit)
        assert np.array_equal(prod["out"], sc["out"])
        sref = ss.sqmc_score(model, th, y, N, prior[0], prior[1], seed, gids, STEP, lam=lam, F=LD, forced=anc, z=sc["trace_z"])
        assert not sref["degenerate"].any()
        np.testing.assert_allclose(sc["out"][:, 4], sref["ll"].astype(np.float64), rtol=TOL, atol=TOL)
        check_score(model, sc["out"], sref, lam)
    return got, ref


# ---- 1. ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("variant", ["all", "groups"])
@pytest.mark.parametrize("N", se.CPM_TIE_N["one wave"] + se.CPM_TIE_N["256 x 4"])
def test_cpm_ties(model, variant, N):
    """The correlated filter on equal states: one wave with a half-filled last thread (3, 100) and full (64, 128); 256 x 4
    padded to 256 (130, 200) and not at all (1024).  The conditions the case rests on are asserted on the keyed draws before
    the launch and again on the U' it wrote.  "all": the recorded parents are the children's own indices."""
    th, y, U = se.cpm_tie_inputs(model, N)
    prior = se.TIE_PRIOR[variant]
    se.tie_conditions(se.run_cpm(model, th, y, se.host_proposal(U, 0.5, OFF, STEP), prior), variant)
    got, _ = check_cpm(model, th, y, U, N, 0.5, prior, free=True)
    distinct = se.tie_conditions(se.run_cpm(model, th, y, got["U_prop"], prior), variant)
    print("distinct parents per step", int(distinct.min()), "..", int(distinct.max()), "of", N)
    if variant == "all":
        assert np.array_equal(got["trace_anc"][:, 1:], np.broadcast_to(np.arange(N, dtype=np.int32), (B, T - 1, N)))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("variant", ["all", "groups"])
@pytest.mark.parametrize("N,n_max", se.SQMC_TIE_SHAPES)
def test_sqmc_ties(model, variant, N, n_max):
    """The SQMC filter on equal states -- under "all" the sort of x_{-1} ahead of step 0 is a sort of N equal keys too -- in one
    wave (2, 64, 128), in 256 x 4 (256, 1024) and N = 64 in the 256 x 4 shape."""
    th, y = se.sqmc_tie_inputs(model, N)
    prior = se.TIE_PRIOR[variant]
    se.tie_conditions(se.run_sqmc(model, th, y, N, prior, kd.chain_ids(B, OFF), STEP), variant)
    got, _ = check_sqmc(model, th, y, N, n_max, prior, free=True)
    se.tie_conditions(se.run_sqmc(model, th, y, N, prior, kd.chain_ids(B, OFF), STEP, z=got["trace_z"]), variant)
    if variant == "all":
        assert np.array_equal(got["trace_anc"][:, 1:], np.broadcast_to(np.arange(N, dtype=np.int32), (B, T - 1, N)))


# ---- 3. the uniform's two clamps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("sharp", [False, True], ids=["generic", "sharp"])
@pytest.mark.parametrize("sign", [-1, 1], ids=["u=0", "u=1-2^-53"])
@pytest.mark.parametrize("rho", se.CLAMP_RHO)
@pytest.mark.parametrize("N", se.CLAMP_N)
def test_cpm_clamped_uniform(model, sharp, sign, N, rho):
    """The resampling normal of every step at -400 / +400 (rho = 0.99 and 0.5: U' stays beyond -38.5 / 8.3).  Every child but
    the named one is checked as usual; the named one exactly: under u = 0 child 0's parent is the first sorted position whose
    weight is not 0, under u = 1 - 2^-53 child N-1's parent is N-1.  sharp (LRinv = 300): position 0 and N-1 mostly carry no
    weight, so the first is not 0 and the second is a particle of zero weight -- the documented behaviour."""
    th, y, U = se.clamp_inputs(model, N, sign, sharp)
    named = 0 if sign < 0 else N - 1
    got, ref = check_cpm(model, th, y, U, N, rho, skip_child=named)
    u = cp.resampling_uniform(got["U_prop"][:, 2:, N])
    assert np.all(u == (0.0 if sign < 0 else cp.U_MAX))
    rec = got["trace_anc"][:, 1:, named].astype(np.int64)
    if sign < 0:
        assert se.leading_near_exp_zero(ref) == 0 and (se.band_hits(ref) == 0 or not (sharp and N == 5))
        want = se.first_nonzero_weight(ref)[:, 1:]
        print("first position with weight: recorded", rec.tolist(), "model", want.tolist())
        assert np.array_equal(rec, want)
    else:
        zero = np.stack([ref["steps"][t]["d"][:, N - 1].astype(np.float64) <= se.EXP_ZERO for t in range(1, T)], axis=1)
        print("child N-1's parent", rec.tolist(), "of zero weight", zero.tolist())
        assert np.all(rec == N - 1)


# ---- 4. flat CDFs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("N", se.FLAT_N["cpm"])
def test_cpm_flat_cdf(model, N):
    """LRinv = 300 under the correlated filter, one wave (5, 128) and 256 x 4 (200, 1024): the standard replay.  How few parents a
    step keeps, and how many searches went past the 3 probes, is printed (the host test asserts the counts)."""
    th, y, U = se.cpm_flat_inputs(model, N)
    got, _ = check_cpm(model, th, y, U, N, 0.5)
    host = se.run_cpm(model, th, y, got["U_prop"], GENERIC)
    print("distinct parents per step", se.distinct_parents(host).tolist(), "searches past the probes",
          se.bisect_searches(host, se.ppt_of(N)))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("N", se.FLAT_N["sqmc"])
def test_sqmc_flat_cdf(model, N):
    """LRinv = 300 under the SQMC filter (powers of two: 128 in one wave, 256 and 1024 in 256 x 4): the standard replay."""
    th, y = se.sqmc_flat_inputs(model, N)
    got, _ = check_sqmc(model, th, y, N, N)
    host = se.run_sqmc(model, th, y, N, GENERIC, kd.chain_ids(B, OFF), STEP, z=got["trace_z"])
    print("distinct parents per step", se.distinct_parents(host).tolist(), "searches past the probes",
          se.bisect_searches(host, se.ppt_of(N)))


# ---- 5. a chain that dies late ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _late_base(N, lam):
    th, y, U = cp.case_inputs("svm", N, 6, B)
    return th, y, U, launch_cpm("svm", th, np.tile(y, (B, 1)), U, N, 0.5, lam)


@pytest.mark.parametrize("lam", [None, 0.95], ids=["none", "score"])
@pytest.mark.parametrize("d", se.LATE_D)
@pytest.mark.parametrize("N", [5, 257])
def test_cpm_chain_dies_late(N, d, lam):
    """SVM, T = 6, chain 1 of 3 observes +-1e300 from step d on: out[4] is not finite and every other slot 0; the increments
    before step d are the model's and the later ones are not written; EVERY row 0 .. T of U' is the proposal the keyed draws
    give, to 1e-14, and finite; the slab's padding is untouched (launch_cpm asserts it); the neighbours are bitwise what they
    are without the dying chain."""
    th, y, U, base = _late_base(N, lam)
    ys = se.late_death_y(y, B, 1, d)
    got = launch_cpm("svm", th, ys, U, N, 0.5, lam)
    assert not np.abs(got["out"][1, 4]) < np.inf and np.all(got["out"][1, [0, 1, 2, 3, 5, 6, 7]] == 0.0)
    want_u = se.host_proposal(U, 0.5, OFF, STEP)
    assert np.all(np.isfinite(got["U_prop"]))
    np.testing.assert_allclose(got["U_prop"], want_u, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(got["U_cur"], U)
    forced = np.maximum(got["trace_anc"].astype(np.int64), 0)
    ref = cp.loglik("svm", th, ys, got["U_prop"], cp.PM, cp.PV, F=LD, forced=forced)
    # (1e300 squared is finite in long double: the chain dies in double, the device's type)
    dead = cp.loglik("svm", th, ys, got["U_prop"], cp.PM, cp.PV, forced=forced)
    assert dead["degenerate"].tolist() == [False, True, False] and np.all(np.isfinite(dead["inc"][1, :d]))
    assert np.all(np.isnan(dead["inc"][1, d:]))
    np.testing.assert_allclose(got["trace_ll"][1, :d], ref["inc"][1, :d].astype(np.float64), rtol=TOL, atol=TOL)
    assert np.all(got["trace_ll"][1, d:] == LL_FILL)
    assert np.array_equal(got["trace_anc"][1, 1:d + 1], base["trace_anc"][1, 1:d + 1]) and np.all(got["trace_anc"][1, d + 1:] == ANC_FILL)
    for b in (0, 2):
        for k in ("out", "U_prop", "trace_anc", "trace_ll"):
            assert np.array_equal(got[k][b], base[k][b]), (b, k)
    assert np.all(np.isfinite(base["out"]))
