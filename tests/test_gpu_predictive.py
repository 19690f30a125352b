"""GPU tests: the predictive statistic (stat='predictive'), which lives in pf_mem_kernel alone and has code of its own
in every phase of the timestep -- exact fp64 column maxima over a [K+1][N] scratch, a second barrier, a weighted exp sum
on the CDF phase, a fold that runs one iteration late (nact_prev, the KP - nact_prev unit terms) and a per-model lead
recursion in the sweep.  pfg_run_batch sends every predictive batch there, whatever N is.

A. REPLAY fp64 against po.pf_window on every model and proposal, over tests/helpers/predictive_cases.py: every chunk and
   np2 edge of N, K = 0 .. 15, leads cut off by the end of the series (K >= T included), full / partial weighted / empty
   windows, 40-sigma observations, T = 0.  tests/test_predictive_model_host.py holds every case's uniforms at least 1e-10
   from the CDF entries, so no ancestor can flip and there is no exemption for one.
B. One launch of six windows that differ in N, K, T, window and weights: each against the oracle, and bitwise itself alone.
C. The device generator, replayed from the launch's own trace through tests/helpers/predictive_model.py: the statistic is
   a function of the traced particles and log-weights plus the lead normals, and LGSSM draws none, SVM's lead 0 multiplies
   its normal by sqrt(0), GARCH's lead 0 normal is used only after the last lead.  fp64 at 1e-8; f32 within the helper's
   bound on the f32 arithmetic of the lead terms and the exp (the trace holds the f32 values exactly).
D. SVM / GARCH at K > 0 on the device generator: their lead normals are not recorded, so no replay; the launch is finite
   and reproducible (tests/test_gpu_sampler.py::test_predictive_device_rng_gpu is their statistical check).

Each test prints its error-to-tolerance ratio (`ratio <section> <value> <case>`); the module's last test prints
the largest of each section with capture disabled."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import predictive_cases as pc  # noqa: E402
import predictive_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-9              # the existing predictive comparison (test_gpu_batch_invariance.py)
DEV_RTOL = DEV_ATOL = 1e-8      # test_gpu_device_replay.py's RTOL / ATOL for the table-math units


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


@pytest.fixture(autouse=True)
def _planned(monkeypatch):
    monkeypatch.delenv("PFGRAD_VARIANT", raising=False)


@pytest.fixture(scope="module")
def worst():
    """section -> (largest error-to-tolerance ratio, case) of the tests run so far; the module's last test reports it."""
    return {}


def _note(worst, section, ratio, where):
    print("ratio {0} {1:.3e} {2}".format(section, ratio, where))
    if section not in worst or not ratio <= worst[section][0]:
        worst[section] = (ratio, where)


def _assert_on_oracle(o, q, section, where, worst):
    ref = pc.reference(q, save_all=True)
    want = np.asarray(ref["statistics"], dtype=np.float64)
    got = o["predictive"]
    assert got.shape == want.shape == (q["num_steps_ahead"] + 1,)
    ll = pc.reference_loglik(q, ref)
    ratio = max(float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want)))),
                abs(o["loglik"] - ll) / (1e-9 * max(1.0, abs(ll))))
    _note(worst, section, ratio, where)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=where)
    assert abs(o["loglik"] - ll) <= 1e-9 * max(1.0, abs(ll)), (where, o["loglik"], ll)


# ---------------------------------------------------------------------------------------------------------------------
# A. REPLAY fp64 against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_replay_predictive_on_the_oracle(ctx, worst, case):
    q = pc.replay_problem(case)
    o = ctx.run_batch([q])[0]
    assert ctx.last_variant() == "mem1024"
    if q["y"].shape[0] == 0:
        assert np.array_equal(o["predictive"], np.zeros(q["num_steps_ahead"] + 1)) and o["loglik"] == 0.0
    _assert_on_oracle(o, q, "A", pc.case_id(case), worst)


# ---------------------------------------------------------------------------------------------------------------------
# B. one launch, mixed windows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", range(len(pc.PAIRS)), ids=lambda p: "-".join(pc.PAIRS[p]))
def test_mixed_batch_on_the_oracle_and_alone(ctx, worst, p):
    qs = pc.batch_problems(p)
    outs = ctx.run_batch(qs)
    assert ctx.last_variant() == "mem1024"
    for b, (q, o) in enumerate(zip(qs, outs)):
        where = "{0}-{1} window {2}".format(pc.PAIRS[p][0], pc.PAIRS[p][1], b)
        _assert_on_oracle(o, q, "B", where, worst)
        alone = ctx.run_batch([q])[0]
        assert ctx.last_variant() == "mem1024"
        assert np.array_equal(alone["predictive"].view(np.uint64), o["predictive"].view(np.uint64)), (where, alone["predictive"], o["predictive"])
        assert np.array_equal(alone["mean_stat"].view(np.uint64), o["mean_stat"].view(np.uint64)) and alone["loglik"] == o["loglik"], where


# ---------------------------------------------------------------------------------------------------------------------
# C. the device generator, replayed from the launch's own trace
# ---------------------------------------------------------------------------------------------------------------------
DEVICE = [(model, kernel, K) for model, kernel in pc.PAIRS for K in ((0, 3, 15) if model == "lgssm" else (0,))]
DEVICE_T, DEVICE_T1, DEVICE_TL = 10, 2, 8


def _device_problem(model, kernel, K, N, stream, dtype):
    rs = np.random.RandomState(7000 + N + 31 * K)
    y = rs.normal(size=DEVICE_T) * (0.6 if model == "garch" else 1.5)
    return dict(model=model, kernel=kernel, smoother="filter", stat="predictive", dtype=dtype, rng="device", N=N, t1=DEVICE_T1,
                tL=DEVICE_TL, prior_mean=-0.2, prior_var=1.3, y=y, weights=rs.uniform(0.5, 10.0, size=DEVICE_TL - DEVICE_T1),
                theta=pc.theta_of(model), seed=20261021 + N, stream=stream, num_steps_ahead=K)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("stream", [3, 11])
@pytest.mark.parametrize("N", [100, 1024, 1025, 4097])
@pytest.mark.parametrize("model,kernel,K", DEVICE, ids=lambda v: str(v))
def test_device_predictive_replayed_from_its_trace(ctx, worst, model, kernel, K, N, stream, dtype):
    q = _device_problem(model, kernel, K, N, stream, dtype)
    o = ctx.run_batch([q], want_trace=True)[0]
    assert ctx.last_variant() == "mem1024"
    got = o["predictive"]
    want, bound = pm.predictive_from_trace(model, q["theta"], q["y"], o["all_x_t"], o["all_log_weights"], q["t1"], q["tL"],
                                           q["weights"], K)
    where = "{0}-{1}-K{2}-N{3}-stream{4}-{5}".format(model, kernel, K, N, stream, dtype)
    assert got.shape == want.shape == (K + 1,) and np.all(np.isfinite(got)) and np.isfinite(o["loglik"])
    if dtype == "f64":
        _note(worst, "C-f64", float(np.max(np.abs(got - want) / (DEV_ATOL + DEV_RTOL * np.abs(want)))), where)
        np.testing.assert_allclose(got, want, rtol=DEV_RTOL, atol=DEV_ATOL, err_msg=where)
    else:
        allowed = bound + 1e-8 * np.maximum(1.0, np.abs(want))
        _note(worst, "C-f32", float(np.max(np.abs(got - want) / allowed)), where)
        _note(worst, "C-f32 got-to-bound", float(np.max(np.abs(got - want))) / bound, where)
        assert np.all(np.abs(got - want) <= allowed), (where, got, want, bound)
    # the launch without traces: the same statistic, as test_gpu_device_replay.py holds production to traced launches
    plain = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == "mem1024"
    np.testing.assert_allclose(plain["predictive"], got, rtol=1e-13, atol=1e-13 * max(1.0, float(np.abs(got).max())), err_msg=where)


# ---------------------------------------------------------------------------------------------------------------------
# D. what stays statistical
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model,kernel", [pk for pk in pc.PAIRS if pk[0] != "lgssm"], ids=lambda v: str(v))
def test_device_predictive_with_unrecorded_normals_is_finite_and_reproducible(ctx, model, kernel, dtype):
    q = _device_problem(model, kernel, 3, 1025, 5, dtype)
    a = ctx.run_batch([dict(q)])[0]
    assert ctx.last_variant() == "mem1024"
    b = ctx.run_batch([dict(q)])[0]
    assert a["predictive"].shape == (4,) and np.all(np.isfinite(a["predictive"])) and np.isfinite(a["loglik"])
    assert np.array_equal(a["predictive"].view(np.uint64), b["predictive"].view(np.uint64)) and a["loglik"] == b["loglik"]


def test_report_the_largest_ratios(worst, capsys):
    """Last in the module: the largest error-to-tolerance ratio of each section the run covered, shown in plain -q output."""
    with capsys.disabled():
        print("".join("\npredictive {0}: largest error-to-tolerance ratio {1:.3e} at {2}".format(section, *worst[section])
                      for section in sorted(worst)))
