"""GPU: every entry point of csrc/pfg_chains.hip reproduces tests/golden/chain_rules.npz bit for bit -- theta, momentum,
theta_prop, valid, ll_cur, grad_cur, n_accept, logprior and the step counter of each case that
tests/golden/make_chain_rules_golden.py states (B = 130 chains, edge rows, a key whose high words matter).  The mirror
tests (test_gpu_keyed_draws.py) accept a few ulps and the ensemble tests compare a build with itself; this one notices a
change of operand order in a kernel that is meant to keep its numbers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_chain_rules_golden as golden  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return golden.run_cases()[0], dict(np.load(golden.PATH))


def test_the_fixture_holds_exactly_the_cases_of_its_generator(cases):
    got, want = cases
    assert sorted(got) == sorted(want)
    kinds = {name.rsplit("/", 1)[1] for name in want}
    assert kinds == {"theta", "momentum", "theta_prop", "valid", "ll_cur", "grad_cur", "n_accept", "logprior", "ctr"}


@pytest.mark.parametrize("rule", ["sgld", "sgld_null_counter", "sghmc", "sgrld", "gibbs", "pgibbs", "logprior", "pmmh_propose",
                                  "pmmh_accept", "pmmh_init", "pmala_propose", "pmala_accept", "pmala_init"])
def test_outputs_equal_the_recorded_ones_bitwise(cases, rule):
    got, want = cases
    names = [n for n in want if n.split("/")[0] == rule]
    assert names
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)       # (NaN equals NaN here)
        if want[name].dtype == np.float64:                                        # ... and so do the bits, signed zeros included
            np.testing.assert_array_equal(got[name].view(np.uint64)[~np.isnan(want[name])],
                                          want[name].view(np.uint64)[~np.isnan(want[name])], err_msg=name)
