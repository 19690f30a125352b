"""The SVM prior 256 x 4 kernel (wg256x4s, bench config c2) may read the table of its eight hot exp per lane-timestep from a
copy in device memory instead of LDS, and reduce their arguments with the magic-number form (PFG_OPT_EXPTABMEM,
PFG_OPT_EXPMAGIC in csrc/pfg_reg_traits.hpp; exp_tab_hot in csrc/pfg_math.hpp).  Whatever the build's switches say, the launch
must still be what the oracle replays from its recorded draws, and the table must be there before its first reader:

  1. replay by the oracle (method and tolerances of tests/test_gpu_device_replay.py::test_device_kernel_replayed_by_oracle:
     zero ancestor flips, rtol 1e-8): a weighted buffered window inside the series, an unweighted whole window, and a window
     that takes the stale-shift retry (the construction of tests/test_gpu_stale_shift.py, y[8] = 2000): the retry uses the
     LDS table and the loop the hot one, so that launch crosses both;
  2. the production twin bitwise equal to the traced twin on the same keys (inside _launch_twins, every case of 1.);
  3. the first launch of a process (it fills the table) equals the third on the same context, a fresh context and the
     launches of a long-running process, bitwise, whether the first reader ran on a context's own non-default stream or on
     HIP's default stream (child processes: tests/exp_table_first_launch.py); one window alone equals the same window
     inside a launch of 300 (more workgroups than the GPU holds at once);
  4. a batch mixing score / suff / none windows plans the general path and equals each window run alone, bitwise.

Shapes: N = 1000 (the full kernel), 257 (slots beyond N in three of the four particle rows), 65 (one wave nearly empty);
T = 24."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_gpu_device_replay import ATOL, RTOL, _series
from test_gpu_raw_score import T1, TL, _oracle_window, _weights, _window_loglik
from test_gpu_stale_shift import NT, PPT, SHAPES, T, VARIANT, _assert_replayed, _launch_twins, _oracle, _outlier_series, _problem, _stable_loglik, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- 1. / 2. replay by the oracle; the twins bitwise -------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPES)
def test_weighted_buffered_window_replayed_by_oracle(ctx, monkeypatch, N):
    q = _problem(N, _series("svm", T, seed=3 * N + T), t1=T1, tL=TL, weights=_weights(TL - T1, N + 5), seed=31337)
    o = _launch_twins(ctx, monkeypatch, q)
    ref = _oracle_window(q, o)
    _assert_replayed(o, ref, _window_loglik(ref["all_log_weights"], T1, TL, q["weights"]))
    np.testing.assert_allclose(o["statistics"], ref["statistics"], rtol=RTOL, atol=1e-7)


@pytest.mark.parametrize("N", SHAPES)
def test_unweighted_whole_window_replayed_by_oracle(ctx, monkeypatch, N):
    q = _problem(N, _series("svm", T, seed=3 * N + T + 1), seed=271828)
    o = _launch_twins(ctx, monkeypatch, q)
    ref = _oracle_window(q, o)
    _assert_replayed(o, ref, _window_loglik(ref["all_log_weights"], 0, T, None))
    np.testing.assert_allclose(o["loglik"], ref["loglikelihood_estimate"], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("N", SHAPES)
def test_retry_window_crosses_both_tables(ctx, monkeypatch, N):
    q = _problem(N, _outlier_series(N, 2000.0), seed=1618)
    o = _launch_twins(ctx, monkeypatch, q)
    ref = _oracle(q, o)
    mx = ref["all_log_weights"].max(axis=1)
    drop, rise = float(mx[8] - mx[9]), float(mx[10] - mx[9])
    print("N", N, "maximum falls by", drop, "and comes back by", rise)
    assert drop > 800.0 and rise > 800.0                        # both directions leave the guard's range: the retry runs
    assert np.all(np.isfinite(ref["all_statistics"]))
    _assert_replayed(o, ref, _stable_loglik(ref["all_log_weights"]))


# ---- 3. the table is there before its first reader and survives ---------------------------------------------------------
def _child(mode, N):
    env = {k: v for k, v in os.environ.items() if k != "PFGRAD_VARIANT"}
    return subprocess.Popen([sys.executable, os.path.join(HERE, "exp_table_first_launch.py"), mode, str(N)],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


def _result(proc):
    out, err = proc.communicate(timeout=300)
    assert proc.returncode == 0, out[-2000:] + err[-4000:]
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def test_first_launch_of_a_process_on_either_stream(ctx, monkeypatch):
    """Two fresh processes: the table's first reader on a context's own stream / on HIP's default stream."""
    import exp_table_first_launch as child
    N = 257
    procs = [_child("ctx", N), _child("default", N)]
    monkeypatch.setenv("PFGRAD_VARIANT", VARIANT)
    q = child.problem(N)
    here_batch, v1 = child.batch_hex(ctx, q)               # this process has launched the kernel many times before
    here_device, v2 = child.device_hex(ctx, q, side=True)
    a, b = _result(procs[0]), _result(procs[1])
    assert a["variant"] == b["variant"] == [VARIANT] and v1 == v2 == VARIANT
    assert len(a["batch"]) == 4 and len(b["device"]) == 2
    assert set(a["batch"]) | set(b["batch"]) == {here_batch}         # first = third = fresh context = other process
    assert set(a["device"]) | set(b["device"]) == {here_device}
    # the out record of pfg_launch_device: three statistic means, a spare slot, the log-likelihood
    rec = np.frombuffer(bytes.fromhex(here_device), dtype=np.float64)
    got = np.frombuffer(bytes.fromhex(here_batch), dtype=np.float64)
    assert np.array_equal(rec[:3], got[:3]) and rec[4] == got[3]


def test_one_window_alone_equals_itself_among_300(ctx, monkeypatch):
    monkeypatch.setenv("PFGRAD_VARIANT", VARIANT)
    monkeypatch.setenv("PFGRAD_NO_SCORE1", "1")
    rs = np.random.RandomState(8)
    Ns = [int(n) for n in rs.choice(SHAPES, size=300)]
    qs = [_problem(N, _series("svm", 6, seed=i), seed=1000 + i, stream=i) for i, N in enumerate(Ns)]
    outs = ctx.run_batch([dict(q) for q in qs], want_final=True)
    assert ctx.last_variant() == VARIANT and not ctx.last_traced()
    for b in (0, 1, 149, 299):
        alone = ctx.run_batch([dict(qs[b])], want_final=True)[0]
        assert ctx.last_variant() == VARIANT
        for k in ("mean_stat", "x_t", "log_weights", "statistics"):
            assert np.array_equal(alone[k], outs[b][k]), (b, k)
        assert alone["loglik"] == outs[b]["loglik"]


# ---- 4. mixed windows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPES)
def test_score_suff_and_none_windows_in_one_launch(ctx, monkeypatch, N):
    monkeypatch.setenv("PFGRAD_VARIANT", VARIANT)
    y = _series("svm", T, seed=N + 11)
    w = _weights(TL - T1, N + 3)
    qs = [_problem(N, y, t1=T1, tL=TL, weights=w, seed=1, stat="score"),
          _problem(N, y, t1=T1, tL=TL, weights=w, seed=2, stat="suff"),
          _problem(N, y, t1=T1, tL=TL, weights=w, seed=3, stat="none")]
    traced = ctx.run_batch([dict(q) for q in qs], want_trace=True, want_draws=True)
    assert ctx.last_variant() == VARIANT and ctx.last_traced()
    production = ctx.run_batch([dict(q) for q in qs], want_final=True)
    assert ctx.last_variant() == VARIANT and not ctx.last_traced()
    for q, got, prod in zip(qs, traced, production):
        alone_t = ctx.run_batch([dict(q)], want_trace=True, want_draws=True)[0]
        alone_p = ctx.run_batch([dict(q)], want_final=True)[0]
        for k in ("mean_stat", "all_x_t", "all_log_weights", "all_ancestors", "all_statistics"):
            assert np.array_equal(alone_t[k], got[k]), (q["stat"], k)
        for k in ("mean_stat", "x_t", "log_weights", "statistics"):
            assert np.array_equal(alone_p[k], prod[k]), (q["stat"], k)
        assert alone_t["loglik"] == got["loglik"] and alone_p["loglik"] == prod["loglik"]
        assert np.array_equal(prod["mean_stat"], got["mean_stat"]), q["stat"]      # production twin = traced twin
        # the weight path does not depend on the statistic: the window is what the oracle replays from its draws
        ref = po.pf_window("svm", q["theta"], q["y"], N, got["rec_z0"], None, got["rec_z"], kernel="prior", pf="poyiadjis_N",
                           stat="score", t1=T1, tL=TL, weights=w, prior_mean=q["prior_mean"], prior_var=q["prior_var"], save_all=True,
                           resampler=lambda t, logw, words=got["rec_u"]: po.device_ancestors(logw, words[t], NT, PPT, "fixed32"))
        assert int(np.sum(got["all_ancestors"] != ref["all_ancestors"])) == 0, q["stat"]
        np.testing.assert_allclose(got["all_x_t"], ref["all_x_t"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got["all_log_weights"], ref["all_log_weights"], rtol=RTOL, atol=ATOL)
        if q["stat"] == "score":
            np.testing.assert_allclose(got["all_statistics"], ref["all_statistics"], rtol=RTOL, atol=1e-7)
