"""GPU: what the device code of a ChainEnsemble / ResidentWindows receives is what tests/golden/ensemble_desc.npz recorded:
the descriptor records after construction and after each of three steps (pointers as (buffer, byte offset)), the resident
window tables, the resolved sizes and flags, and the arguments of every library call of the steps.  Recorded by
tests/golden/make_ensemble_golden.py before the host side was restructured; equality everywhere -- these are integers,
host-computed doubles and Philox-derived integers.

tests/golden/ensemble_samplers.npz does the same for the samplers and chain filters that came later (SAMPLER_CASES), with
the constructor's library calls, the chain-filter records, the checkpoint's keys, its round trip and the checkpoints a
sampler refuses; recorded before the samplers and filters were stated in two tables."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_ensemble_golden as maker  # noqa: E402

pytestmark = pytest.mark.gpu


def _load(path):
    z = np.load(path, allow_pickle=False)
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def golden():
    return _load(maker.FIXTURE)


@pytest.fixture(scope="module")
def sampler_golden():
    return _load(maker.SAMPLER_FIXTURE)


def test_fixture_covers_the_cases(golden):
    _, meta = golden
    assert sorted(meta["cases"]) == sorted(c[0] for c in maker.CASES)
    assert meta["columns"] == maker._columns() and meta["buffers"] == list(maker.BUFFERS)


def test_sampler_fixture_covers_the_cases(sampler_golden):
    from sgmcmc_ssm_amd import _capi
    _, meta = sampler_golden
    assert sorted(meta["cases"]) == sorted(c[0] for c in maker.SAMPLER_CASES)
    assert meta["columns"] == maker._columns() and meta["buffers"] == list(maker.SAMPLER_BUFFERS)
    assert meta["record_columns"] == {attr.lstrip("_"): maker._columns(getattr(_capi, dtype)) for attr, dtype in maker.RECORDS}


def _compare(golden, name, arrays, info):
    z, meta = golden
    want = dict(meta["cases"][name])
    assert sorted(arrays) == sorted(k.split("/", 1)[1] for k in z.files if k.startswith(name + "/"))
    desc = z[name + "/desc"]
    assert arrays["desc"].shape == desc.shape
    for j, column in enumerate(meta["columns"]):
        np.testing.assert_array_equal(arrays["desc"][:, :, j], desc[:, :, j],
                                      err_msg="{0}: {1} [snapshot, descriptor]".format(name, column))
    for key in arrays:
        assert arrays[key].dtype == z[name + "/" + key].dtype, key
        np.testing.assert_array_equal(arrays[key], z[name + "/" + key], err_msg="{0}: {1}".format(name, key))
    calls, want_calls = info.pop("calls"), want.pop("calls")
    assert info == want
    assert len(calls) == len(want_calls)
    for got, ref in zip(calls, want_calls):
        assert got == ref


@pytest.mark.parametrize("case", maker.CASES, ids=[c[0] for c in maker.CASES])
def test_device_sees_the_recorded_inputs(golden, case):
    _compare(golden, case[0], *maker.record_case(case))


@pytest.mark.parametrize("case", maker.SAMPLER_CASES, ids=[c[0] for c in maker.SAMPLER_CASES])
def test_device_sees_the_recorded_sampler_inputs(sampler_golden, case):
    arrays, info = maker.record_sampler_case(case)
    assert info["round_trip"] is True
    _compare(sampler_golden, case[0], arrays, info)
