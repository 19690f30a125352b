"""CPU: tests/helpers/predictive_model.py on the oracle alone -- what tests/test_gpu_predictive.py then asks of the kernel.

The helper restates the predictive statistic's fold on a trace.  Here it is pinned to the reference through the oracle
(tests/test_oracle_golden.py ties po.pf_window(stat='predictive') to predictive.npz): fed the oracle's own traced
particles and log-weights, it must return the oracle's statistic.  Then the case list itself is tested: each of the three
deliberate errors of the fold moves at least one case's statistic, and no case has a uniform within 1e-10 of a CDF
entry, so the GPU comparison needs no exemption for flipped ancestors."""
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import predictive_cases as pc  # noqa: E402
import predictive_model as pm  # noqa: E402

WORK_LIMIT = 2 * 10 ** 6        # N T (K + 1) of the cases the helper replays here
TIE_MARGIN = 1e-10
SMALL = tuple(c for c in pc.CASES if np.prod(pc.ROWS[c[1]][:2]) * (pc.ROWS[c[1]][2] + 1) <= WORK_LIMIT)


def _relative(a, want):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.abs(a - want) / np.maximum(np.abs(want), 1.0)))


@pytest.fixture(scope="module")
def replayed():
    """case -> dict(got, want, shift per mutation, tie margin): one oracle run per case, kept as these few numbers."""
    memo = {}

    def get(case):
        if case in memo:
            return memo[case]
        q = pc.replay_problem(case)
        T, small = q["y"].shape[0], case in SMALL
        ref = pc.reference(q, stat="predictive" if small else "none", save_all=True)
        out = dict(margin=pm.tie_margin(ref["all_log_weights"][:T], np.asarray(q["u"]).reshape(T, q["N"])))
        if small:
            pz = q["pred_z"]
            helper = lambda mutate: pm.predictive_from_trace(
                q["model"], q["theta"], q["y"], ref["all_x_t"], ref["all_log_weights"], q["t1"], q["tL"], q["weights"],
                q["num_steps_ahead"], mutate=mutate, pred_normals=None if pz is None else (lambda t, k: pz[t, k]))[0]
            out["want"] = np.asarray(ref["statistics"], dtype=np.float64)
            out["got"] = helper(None)
            out["shift"] = {m: _relative(helper(m), out["want"]) for m in pm.MUTATIONS}
        memo[case] = out
        return out
    return get


@pytest.mark.parametrize("case", SMALL, ids=pc.case_id)
def test_helper_equals_oracle(replayed, case):
    r = replayed(case)
    assert r["got"].shape == r["want"].shape == (pc.ROWS[case[1]][2] + 1,)
    # 1e-12 relative; where the statistic is exactly 0 (K = 0 outside the window: T times log(1)) the oracle's own fp64
    # value is the rounding of log(sum of the normalised weights), a few ulps of 1 per step, and that is the allowance
    T = pc.ROWS[case[1]][1]
    np.testing.assert_allclose(r["got"], r["want"], rtol=1e-12, atol=4 * T * np.finfo(np.float64).eps, err_msg=pc.case_id(case))


def test_each_mutation_is_detectable(replayed, capsys):
    """Reports, past pytest's capture, the case and the size of the shift per mutation, and the smallest tie margin."""
    lines = []
    for mutate in pm.MUTATIONS:
        shifts = {c: replayed(c)["shift"][mutate] for c in SMALL}
        moved = [c for c, s in shifts.items() if not s <= 1e-6]
        finite = {c: s for c, s in shifts.items() if np.isfinite(s)}
        best = max(finite, key=finite.get)
        lines.append("mutation {0}: {1} of {2} cases move by more than 1e-6 relative; the largest finite shift is {3:.3e}, at {4}".format(
            mutate, len(moved), len(shifts), finite[best], pc.case_id(best)))
    margins = {c: replayed(c)["margin"] for c in pc.CASES}
    tightest = min(margins, key=margins.get)
    lines.append("smallest tie margin of the REPLAY cases: {0:.3e}, at {1}".format(margins[tightest], pc.case_id(tightest)))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for mutate in pm.MUTATIONS:
        assert max(s for s in (replayed(c)["shift"][mutate] for c in SMALL) if np.isfinite(s)) > 1e-6, mutate


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_no_near_ties(replayed, case):
    margin = replayed(case)["margin"]
    print("tie margin {0:.3e} at {1}".format(margin, pc.case_id(case)))
    assert margin >= TIE_MARGIN, (pc.case_id(case), margin)


@pytest.mark.parametrize("p", range(len(pc.PAIRS)), ids=lambda p: "-".join(pc.PAIRS[p]))
def test_no_near_ties_in_the_mixed_batch(p):
    for b, q in enumerate(pc.batch_problems(p)):
        T = q["y"].shape[0]
        ref = pc.reference(q, stat="none", save_all=True)
        margin = pm.tie_margin(ref["all_log_weights"][:T], np.asarray(q["u"]).reshape(T, q["N"]))
        print("tie margin {0:.3e} at window {1} of the {2} batch".format(margin, b, "-".join(pc.PAIRS[p])))
        assert margin >= TIE_MARGIN, (pc.PAIRS[p], b, margin)


def test_the_case_list_covers_what_it_claims():
    for p, (model, kernel) in enumerate(pc.PAIRS):
        rows = [pc.ROWS[r] for (pp, r) in pc.CASES if pp == p]
        assert {1, 2, 63, 64, 65, 1000, 1023, 1024, 1025, 2049, 4096, 4097, 5000, 8192, 8193, 16384} <= {r[0] for r in rows}
        assert {0, 1, 5, 15} <= {r[2] for r in rows}
        assert any(r[1] == 3 and r[2] == 5 for r in rows) and any(r[1] == 3 and r[2] == 15 for r in rows)
        assert all(4 <= r[1] <= 12 for r in rows if r[1] > 3) and any(r[1] == 0 for r in rows)
        assert {"full", "partial", "empty"} == {r[3] for r in rows} and sum(r[4] for r in rows) == 1
        assert all(r[1] == 4 for r in rows if r[0] == 16384)
    for T in (3, 4, 5, 12):
        t1, tL = pc.window_of(T, "partial")
        assert 0 < t1 < tL < T
        t1, tL = pc.window_of(T, "empty")
        assert 0 < t1 == tL < T


def test_helper_needs_the_normals_it_uses():
    """Without lead normals the helper answers for LGSSM at any K and for every model at K = 0, and refuses the rest."""
    rs = np.random.RandomState(5)
    N, T = 50, 6
    y = rs.normal(size=T)
    x, lw = rs.normal(size=(T + 1, N, 2)) ** 2, rs.normal(size=(T + 1, N))
    for model in po.MODELS:
        xs, th = x[:, :, :po.STATE_DIM[model]], pc.theta_of(model)
        v, bound = pm.predictive_from_trace(model, th, y, xs, lw, 1, 5, np.linspace(1.0, 2.0, 4), 0)
        assert v.shape == (1,) and np.isfinite(v[0]) and bound > 0.0
        if model == "lgssm":
            assert np.all(np.isfinite(pm.predictive_from_trace(model, th, y, xs, lw, 0, T, None, 3)[0]))
        else:
            with pytest.raises(ValueError, match="needs its normals"):
                pm.predictive_from_trace(model, th, y, xs, lw, 0, T, None, 3)
    with pytest.raises(ValueError):
        pm.predictive_from_trace("lgssm", pc.theta_of("lgssm"), y, x[:, :, :1], lw, 0, T, None, 0, mutate="other")
