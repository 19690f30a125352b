"""The launch planner's size and name queries answer what they answered when the fixture was recorded (no GPU needed).

tests/golden/plan_sizes.npz pins pfg_scratch_bytes_smoother of every smoother id and, for plain windows, pfg_scratch_bytes
and pfg_variant_name, at each side of every size class (tests/golden/make_plan_sizes_golden.py): a ChainEnsemble sizes its
scratch slabs from these, so a planner that answers differently launches kernels on slabs of the wrong size.
"""
import os
import sys

import numpy as np
import pytest

from sgmcmc_ssm_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_plan_sizes_golden as golden  # noqa: E402


@pytest.fixture(scope="module")
def pair():
    saved = {v: os.environ.pop(v, None) for v in ("PFGRAD_VARIANT", "PFGRAD_NO_SCORE1")}    # (the planner reads them)
    try:
        got = golden.record(_capi.load_library())
    finally:
        os.environ.update({v: x for v, x in saved.items() if x is not None})
    with np.load(golden.FIXTURE) as want:
        return got, {k: want[k] for k in want.files}


def test_fixture_covers_the_grid(pair):
    _, want = pair
    assert sorted(want) == ["name", "scratch", "scratch_smoother"]
    assert want["scratch_smoother"].shape == (3, 2, 2, 9, 11) and want["scratch"].shape == want["name"].shape == (3, 2, 2, 11)
    assert golden.SMOOTHERS == tuple(sorted(_capi.SMOOTHER.values()))
    # not a table of refusals: every scheme has sizes on record, and slabs where its large-N twins run
    strat, syst = _capi.SMOOTHER["nemeth_stratified"], _capi.SMOOTHER["nemeth_systematic"]
    n = golden.NS.index
    assert np.all(want["scratch_smoother"][:, :, :, strat, :n(16385)] >= 0) and np.all(want["scratch_smoother"][:, :, :, strat, n(1025):n(16385)] > 0)
    assert np.all(want["scratch_smoother"][:, :, :, strat, n(16385)] == -1)
    assert np.all(want["scratch_smoother"][:, :, 1, syst, :n(1025)] == 0) and np.all(want["scratch_smoother"][:, :, :, syst, n(1025):] == -1)
    assert np.all(want["scratch"] >= 0) and "none" not in set(want["name"].ravel())


@pytest.mark.parametrize("key", ["scratch_smoother", "scratch", "name"])
def test_queries_answer_the_fixture(pair, key):
    got, want = pair
    bad = np.argwhere(got[key] != want[key])
    assert bad.size == 0, [(tuple(i), got[key][tuple(i)], want[key][tuple(i)]) for i in bad[:10]]
