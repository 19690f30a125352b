"""The elementwise-statistics pass (csrc/pfg_elementwise.hip) past the first trip of every loop it contains, against
the trace-driven longdouble reference of tests/helpers/elementwise_model.py (pinned to the oracle on the CPU by
tests/test_elementwise_model_host.py).

Every case runs one replayed window twice on the same streams: once for its trace (particles, log-weights,
ancestors), once with the elementwise pass behind it.  The two runs give identical final particles and log-weights
and ran the same kernel variant, so the pass consumed the very trace the reference is evaluated on.

  O(N)    ews_step_kernel / ews_colsum_kernel / ews_softmax_kernel: Wd = 255 (one column block, one idle lane), 258
          (block 1 has two live lanes; the last [x', x'^2, x x'] triple sits in columns 255 / 256 / 257), 513 (three
          blocks), steps outside the window on both sides; lambda = 0.9 and 1; N = 37..40 (the four N mod 4 tails of the
          column sum's unroll); N = 1100 (the large-N kernel's trace, the softmax's second stride).
  O(N^2)  ews_n2_step_kernel: N = 257 (second j stride, odd tail), 515 (odd, two full strides), 1025 (the trace of
          n2_mem1024), 4096 (all of bw[]), and Wd = 270 (the col += 256 loop).

Tolerance.  Not chosen in advance: a plain float64 NumPy evaluation of the same helper differs from its longdouble
result by at most FLOOR (below; elementwise_model.float64_floors(), max |f64 - ld| / max(1, max |ref|) per case, the
largest over the cases of each family, measured on the CPU on the oracle's filter traces of these very cases).  That
is what any float64 evaluation in another summation order has; the kernels get 16 x that, per family (the O(N^2) pass
goes through exp of large arguments), and never more than the 1e-9 the project uses elsewhere.
    family   float64 floor   tolerance (16 x)   largest kernel error on the MI355X
    O(N)     1.05e-15        1.68e-14           1.19e-15
    O(N^2)   1.28e-15        2.05e-14           1.36e-15"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import elementwise_model as em      # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = {"on": 1.05e-15, "n2": 1.28e-15}        # elementwise_model.float64_floors(), rounded up
FACTOR = 16.0
TOL = {fam: min(FACTOR * f, 1e-9) for fam, f in FLOOR.items()}


@pytest.fixture(scope="module")
def ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def _run_twice(ctx, q):
    """The window for its trace, then with the elementwise pass (the two cannot share a problem)"""
    tr = ctx.run_batch([dict(q)], want_trace=True, want_final=True)[0]
    variant = ctx.last_variant()
    ew = ctx.run_batch([dict(q)], want_elementwise=True, want_final=True)[0]
    assert ctx.last_variant() == variant
    assert np.array_equal(tr["x_t"], ew["x_t"]) and np.array_equal(tr["log_weights"], ew["log_weights"])
    # the final particles are the trace's last step
    assert np.array_equal(tr["all_x_t"][-1], tr["x_t"]) and np.array_equal(tr["all_log_weights"][-1], tr["log_weights"])
    return tr, ew, variant


def _compare(fam, case, ew, stats, mean):
    N, Wd = stats.shape
    assert ew["ew_stats"].shape == (N, Wd) and ew["ew_mean"].shape == (Wd,)
    assert np.all(np.isfinite(ew["ew_stats"])) and np.all(stats[:, 0::3] != 0)       # every block is live in the reference
    e_stats, e_mean = em.normalised_error(ew["ew_stats"], stats), em.normalised_error(ew["ew_mean"], mean)
    print("elementwise {0} {1}: stats {2:.3g} mean {3:.3g} (tolerance {4:.3g})".format(fam, case, e_stats, e_mean, TOL[fam]))
    assert e_stats <= TOL[fam] and e_mean <= TOL[fam], (case, e_stats, e_mean, TOL[fam])


@pytest.mark.parametrize("model,kernel,N,T,t1,tL,lam,salt", em.CASES_ON)
def test_elementwise_on_pass_column_blocks(ctx, model, kernel, N, T, t1, tL, lam, salt):
    inp = em.case_inputs(model, kernel, N, T, t1, tL, salt)
    q = dict(model=model, kernel=kernel, smoother="nemeth", stat="none", dtype="f64", rng="replay", N=N, t1=t1, tL=tL,
             lambduh=lam, prior_mean=0.0, prior_var=1.3, **inp)
    tr, ew, variant = _run_twice(ctx, q)
    if N > 1024:
        assert variant == "mem1024"
    stats, mean = em.ew_reference(model, tr["all_x_t"], tr["all_log_weights"], tr["all_ancestors"], t1, tL, inp["weights"], lam)
    _compare("on", (model, N, T, t1, tL, lam), ew, stats, mean)


@pytest.mark.parametrize("model,kernel,N,T,t1,tL,salt", em.CASES_N2)
def test_elementwise_n2_pass_strides(ctx, model, kernel, N, T, t1, tL, salt):
    inp = em.case_inputs(model, kernel, N, T, t1, tL, salt)
    q = dict(model=model, kernel=kernel, smoother="poyiadjis_n2", stat="none", dtype="f64", rng="replay", N=N, t1=t1, tL=tL,
             lambduh=1.0, prior_mean=0.0, prior_var=1.3, **inp)
    tr, ew, variant = _run_twice(ctx, q)
    assert variant == ("n2_256x1" if N <= 256 else "n2_256x4" if N <= 1024 else "n2_mem1024")
    stats, mean = em.ew_reference_n2(model, inp["theta"], tr["all_x_t"], tr["all_log_weights"], t1, tL, inp["weights"])
    _compare("n2", (model, N, T, t1, tL), ew, stats, mean)
