"""Host checks of SMC^2 over resident PMMH chains (no GPU): the header and the binding, the long-double model of the reweight
kernel (tests/helpers/seq_model.py) against brute force and its own identities, the inputs the GPU test compares parents on,
the argument checks of csrc/pfg_seq_checks.hpp under the sanitizers, and the refusals of SequentialPopulation."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import seq_model as sq  # noqa: E402
import smc_model as sm  # noqa: E402

from test_capi_symbols import declared_functions  # noqa: E402

LD = sq.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_NAMES = ("pfg_seq_reweight_device", "pfg_seq_gather_device", "pfg_seq_adopt_device")
SEED = 0x5EED0000C0DE4321
SHAPES = [2, 63, 64, 65, 1023, 1024, 1025, 4097]


# ---- 1. header and binding ---------------------------------------------------------------------------------------------
def test_header_binding_and_library_export_the_seq_calls():
    from sgmcmc_ssm_amd import _build, _capi
    declared = declared_functions()
    for name in SEQ_NAMES:
        assert name in declared and name in _capi.EXPORTS, name
    if _build.is_stale():
        _build.build_library()
    raw = ctypes.CDLL(_build.LIB_PATH)
    for name in SEQ_NAMES:
        assert hasattr(raw, name), name
    assert _capi.load_library().pfg_version() == 126          # additive: the version stays
    header = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    assert "#define PFG_SEQ_RECORD_DOUBLES {0}\n".format(_capi.SEQ_RECORD_DOUBLES) in header


# ---- 2. the host model ---------------------------------------------------------------------------------------------------
def _brute(logw, incr):
    """The increment and the ESS from the definitions, without any shift (the inputs are small enough for long double)."""
    logw, incr = np.asarray(logw).astype(LD), np.asarray(incr).astype(LD)
    W0, w1 = np.exp(logw), np.exp(logw + incr)
    return np.log(w1.sum() / W0.sum()), w1.sum() ** 2 / (w1 * w1).sum()


def test_model_against_the_definitions():
    """Increment = log(sum W e^incr / sum W) and ESS = (sum W e^incr)^2 / sum (W e^incr)^2 whatever the shifts; the trigger is
    ESS < tau B; a stage that does not resample leaves logw + incr up to a constant, one that does leaves 0 and parents that
    are floor or ceil of B p_i."""
    rng = np.random.default_rng(7)
    for _ in range(200):
        B = int(rng.integers(2, 400))
        logw, incr = rng.normal(scale=2.0, size=B) + rng.normal(scale=30.0), rng.normal(scale=3.0, size=B) - 20.0
        tau, u = float(rng.uniform(0.05, 0.95)), float(rng.uniform())
        r = sq.reweight(logw, incr, tau, u)
        incr_def, ess_def = _brute(logw, incr)
        assert r["status"] == 0
        assert abs(r["increment"] - incr_def) <= 1e-15 * abs(incr_def) + 1e-16
        assert abs(r["ess"] - ess_def) <= 1e-15 * ess_def
        assert r["resampled"] == bool(ess_def < LD(tau) * B) or abs(ess_def - LD(tau) * B) < 1e-12
        p = sq.normalised(logw.astype(LD) + incr.astype(LD))
        if r["resampled"]:
            assert not r["logw"].any()
            counts = np.bincount(r["parent"], minlength=B)
            expect = (p * B).astype(float)
            assert np.all(counts >= np.floor(expect - 1e-9)) and np.all(counts <= np.ceil(expect + 1e-9))
            assert np.all(np.diff(r["parent"]) >= 0)
        else:
            np.testing.assert_array_equal(r["parent"], np.arange(B))
            assert np.max(np.abs(sq.normalised(r["logw"]) - p)) <= 1e-17
            assert r["logw"].max() == 0


def test_model_identities():
    """Equal incr leaves the normalised weights unchanged and gives increment = incr (exactly: the two sums are the same
    number); a one-hot weight gives ESS = 1, an increment of that chain's incr and, resampled, that chain as every parent; an
    incr of -inf is a zero weight, not an error."""
    rng = np.random.default_rng(11)
    for B in SHAPES:
        logw = rng.normal(size=B)
        r = sq.reweight(logw, np.full(B, -41.25), 1e-9, 0.3)
        assert r["status"] == 0 and not r["resampled"] and r["increment"] == LD(-41.25)
        assert np.max(np.abs(sq.normalised(r["logw"]) - sq.normalised(logw))) <= 1e-18
        hot = np.full(B, -np.inf)
        hot[B // 3] = 2.5
        incr = rng.normal(size=B)
        r = sq.reweight(hot, incr, 0.5, 0.3)
        assert r["status"] == 0 and r["ess"] == 1 and abs(r["increment"] - LD(incr[B // 3])) <= 1e-18
        assert r["resampled"] == (B > 2) and (not r["resampled"] or np.all(r["parent"] == B // 3))
        incr[0] = -np.inf
        r = sq.reweight(logw, incr, 1e-9, 0.3)
        assert r["status"] == 0 and r["logw"][0] == -np.inf and sq.normalised(r["logw"])[0] == 0


def test_model_flags():
    z = np.zeros(5)
    assert sq.reweight(z, np.full(5, -np.inf), 0.5, 0.5)["status"] == sq.NO_FINITE
    assert sq.reweight(np.full(5, -np.inf), z, 0.5, 0.5)["status"] == sq.NO_FINITE
    assert sq.reweight(np.r_[-np.inf, 0.0], np.r_[0.0, -np.inf], 0.5, 0.5)["status"] == sq.NO_FINITE
    for bad in (np.nan, np.inf):
        assert sq.reweight(z, np.r_[z[:4], bad], 0.5, 0.5)["status"] == sq.NOT_A_NUMBER
        assert sq.reweight(np.r_[bad, z[:4]], z, 0.5, 0.5)["status"] == sq.NOT_A_NUMBER
    assert sq.reweight(z[:1], z[:1], 0.5, 0.5)["status"] == sq.BAD_B


def test_the_gpu_cases_keep_their_targets_off_the_cdf():
    """Every case tests/test_gpu_seq.py compares parents on: the smallest distance between a child's target and a CDF entry
    exceeds 1e-9 W, so no child has to be left out of the comparison; and the cases cover both sides of the trigger."""
    seen = set()
    for B in SHAPES:
        for k, pattern in enumerate(sq.PATTERNS):
            stage = 3 + k + (1 << 33) * (k % 2)
            logw, incr, tau = sq.case(B, pattern)
            _, _, r = sq.move_off_the_cdf(logw, incr, tau, sm.stage_uniform(SEED, stage))
            assert r["status"] == 0
            seen.add((pattern, r["resampled"]))
            if r["resampled"]:
                assert r["gap"].min() > sq.MIN_GAP, (B, pattern, r["gap"].min())
            if B > 2 and pattern in ("below_target", "above_target"):
                assert r["resampled"] == (pattern == "below_target")
    assert {("equal", False), ("random", True), ("below_target", True), ("above_target", False),
            ("all_but_one_minus_inf", True), ("one_minus_inf", True)} <= seen


# ---- 3. the argument checks, under the sanitizers ------------------------------------------------------------------------------
def test_argument_checks_under_the_sanitizers(tmp_path):
    """csrc/pfg_seq_checks.hpp is what pfg_seq.hip's entry points check their arguments with, free of HIP: a host program of
    its own (tests/seq_host/check_main.cpp), built with -fsanitize=address,undefined, walks the edges of every clause."""
    gxx = shutil.which("g++")
    cxx = gxx or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    # the runtimes linked statically (clang's default), so that the program does not depend on what else the loader brings in
    static = ["-static-libasan", "-static-libubsan"] if gxx else []
    from sgmcmc_ssm_amd import _build
    exe = str(tmp_path / "seq_checks")
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all"] + static + ["-I", _build.CSRC, os.path.join(ROOT, "tests", "seq_host", "check_main.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "seq checks ok" in run.stdout, (run.returncode, run.stdout, run.stderr)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
def _resolve(**kw):
    from sgmcmc_ssm_amd.sequential import SequentialPopulation
    from test_host_logic import default_params
    model = kw.pop("model", "svm")
    kw.setdefault("num_chains", 16)
    kw.setdefault("observations", np.zeros(20))
    return SequentialPopulation.resolve_settings(model, default_params(model), **kw)


REFUSALS = [
    (dict(correlation=0.9), NotImplementedError, "correlation stays None"),
    (dict(sqmc=True), NotImplementedError, "sqmc stays False"),
    (dict(sampler="pmala"), NotImplementedError, "sampler stays 'pmmh'"),
    (dict(sampler="sgld"), NotImplementedError, "sampler stays 'pmmh'"),
    (dict(model="lgssm", kind="marginal"), NotImplementedError, "no particle state to carry"),
    (dict(observations=[np.zeros(5), np.zeros(6)]), NotImplementedError, "lists of sequences"),
    (dict(subsequence_length=8), NotImplementedError, "subsequence_length = buffer_length = -1"),
    (dict(buffer_length=2), NotImplementedError, "subsequence_length = buffer_length = -1"),
    (dict(minibatch_size=2), NotImplementedError, "minibatch_size = num_sequences = 1"),
    (dict(num_sequences=-1), NotImplementedError, "minibatch_size = num_sequences = 1"),
    (dict(pf="nemeth"), NotImplementedError, "pf stays 'poyiadjis_N'"),
    (dict(pf="paris"), NotImplementedError, "pf stays 'poyiadjis_N'"),
    (dict(resampling="stratified"), NotImplementedError, "resampling stays 'multinomial'"),
    (dict(resampling="systematic"), NotImplementedError, "resampling stays 'multinomial'"),
    (dict(ess_threshold=0.5), NotImplementedError, "ess_threshold stays None"),
    (dict(pmmh_stat="score"), NotImplementedError, "pmmh_stat stays None"),
    (dict(dtype="f32"), NotImplementedError, "dtype stays 'f64'"),
    (dict(N=16385), NotImplementedError, "1 <= N <= 16384"),
    (dict(chunk=0), ValueError, "chunk must be >= 1"),
    (dict(num_chains=1), NotImplementedError, "2 <= num_chains <= 2\\^20"),
    (dict(num_chains=(1 << 20) + 1), NotImplementedError, "2 <= num_chains <= 2\\^20"),
    (dict(ess_target=0.0), ValueError, "ess_target"),
    (dict(ess_target=1.0), ValueError, "ess_target"),
    (dict(ess_target=float("nan")), ValueError, "ess_target"),
    (dict(moves=0), ValueError, "moves"),
    (dict(chain_offset=16), NotImplementedError, "one rank of several"),
    (dict(init_sd=0.0), ValueError, "init_sd"),
]


def test_refusals(monkeypatch):
    """Every refusal by name, through resolve_settings, which needs no device: each names SequentialPopulation, not the
    wrapper whose q0 logic it reuses."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for kw, error, match in REFUSALS:
        with pytest.raises(error, match=match) as info:
            _resolve(**dict(kw))
        assert "TemperedPopulation" not in str(info.value), kw
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="SequentialPopulation.*one rank of several"):
        _resolve()


def test_what_is_allowed_and_the_initial_population(monkeypatch):
    """GARCH, kernel='optimal', N = 16384, minibatch_size = num_sequences = 1 and the defaults stated explicitly pass; the
    initial population, q0 and the scale are TemperedPopulation's for the same seed."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    from sgmcmc_ssm_amd.tempering import TemperedPopulation
    from test_host_logic import default_params
    for model in ("svm", "garch", "lgssm"):
        s = _resolve(model=model, N=16384, chunk=7, seed=5, kernel="optimal" if model != "svm" else None, kind="pf",
                     pf="poyiadjis_N", resampling="multinomial", ess_threshold=None, dtype="f64", minibatch_size=1,
                     num_sequences=1, subsequence_length=-1, buffer_length=-1, sampler="pmmh", observations=np.zeros((20, 1)))
        t = TemperedPopulation.resolve_settings(model, default_params(model), num_chains=16, seed=5)
        assert (s.N, s.chunk) == (16384, 7) and s.y.shape == (20,)
        for key in ("theta0", "q0_mean", "q0_sd", "scale0"):
            np.testing.assert_array_equal(getattr(s, key), getattr(t, key), err_msg=key)
        assert (s.ess_target, s.moves, s.scale_factor) == (t.ess_target, t.moves, t.scale_factor)
