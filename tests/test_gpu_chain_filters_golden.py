"""GPU: the conditional SMC sweep (csrc/pfg_csmc.hip) and the sorted, correlated filter (csrc/pfg_cpm.hip) reproduce
tests/golden/chain_filters.npz bit for bit -- records, paths, degenerate counts, the scratch history, the traces and U' of each
case that tests/golden/make_chain_filters_golden.py states (every launch shape's edge sizes, a key whose high words matter, a
NULL counter, degenerate chains, refused descriptors) -- and the launches that must agree do: the production twin with the
traced one on everything both write, and both models on U'.  The mirror tests (test_gpu_csmc.py, test_gpu_cpm.py) accept 1e-8
against a long-double model; this one notices a change of operand order in a kernel that is meant to keep its numbers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_chain_filters_golden as golden  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    got, same, facts = golden.run_cases()
    return got, same, dict(np.load(golden.PATH)), facts


def _assert_bitwise(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    np.testing.assert_array_equal(got, want, err_msg=name)       # (NaN equals NaN here)
    if want.dtype == np.float64:                                   # ... and so do the bits, signed zeros included
        np.testing.assert_array_equal(got.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)], err_msg=name)


def test_the_fixture_holds_exactly_the_cases_of_its_generator(cases):
    got, same, want, _ = cases
    assert sorted(got) == sorted(want) and set(same) <= set(want)
    kinds = {name.split("/")[0]: set() for name in want}
    for name in want:
        kinds[name.split("/")[0]].add(name.rsplit("/", 1)[1])
    assert kinds == {"csmc": {"out", "path", "n_degenerate", "x", "x_fold", "anc16", "trace_anc", "trace_ref_anc", "trace_k", "trace_w",
                              "trace_w_fold"},
                     "cpm": {"out", "trace_ll", "trace_anc"}, "cpm_u": {"u", "u_fold"}}


def test_the_generator_s_cases_take_the_branches_they_were_built_for(cases):
    got, same, _, facts = cases
    golden.check_coverage(got, same, facts)


@pytest.mark.parametrize("family,model", [("csmc", "svm"), ("csmc", "lgssm"), ("cpm", "svm"), ("cpm", "lgssm"), ("cpm_u", None)])
def test_outputs_equal_the_recorded_ones_bitwise(cases, family, model):
    got, _, want, _ = cases
    names = [n for n in want if n.split("/")[0] == family and (model is None or n.split("/")[1] == model)]
    assert names
    for name in names:
        _assert_bitwise(got[name], want[name], name)


def test_launches_that_must_agree_do(cases):
    """The production twin writes what the traced one writes (out, path, n_degenerate, the history; out and U'), and U' does
    not depend on the model."""
    got, same, _, _ = cases
    assert any(n.startswith("csmc/") for n in same) and any(n.startswith("cpm/") for n in same)
    assert all(len(same[n]) == 3 for n in same if n.startswith("cpm_u/N"))
    for name, others in same.items():
        for a in others:
            _assert_bitwise(a, got[name], name)
