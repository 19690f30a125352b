"""CPU: the PaRIS additions of oracle/pf_oracle.py and tests/helpers/forced_window.py, judged on the pinned oracle before
they judge a kernel (tests/test_gpu_paris_device_replay.py).

* po.pf_window(pf='paris', paris_parents=...) fed the oracle's own backward parents reproduces the PoolDraws and NpDraws
  runs bit for bit (and accept_reject=False).
* forced_window.forced_paris_steps fed the oracle's save_all output returns the oracle's next step at 1e-12.
* forced_window.backward_law_scores: both scores stay below 5 on the oracle's own parents -- NpDraws with accept-reject
  (the reference's thresholds) and accept_reject=False -- and at least one reaches 5 for each of four wrong samplers at the
  shapes (N, T, Ntilde) of the GPU cases.  5 is the bound of forced_window.ancestor_law_score; all seeds are fixed.

Every (model, N, T, Ntilde) of the GPU file is tested here, read from its case tables.  T = 6 was not enough below
N = 700: at N = 100, T = 6, Ntilde = 2 (1200 draws, SVM) the scores (Z_p / Z_x) were reference -0.7 / 0.1, weights only
-35.7 / -2.4, density only -5.8 / -2.6, J + 1 on one draw in ten -5.5 / 0.7; LGSSM's one-in-ten mutant reached -3.7 only.
At N = 1100, T = 3 two of the three steps have power against the density-only sampler (the log-weights of step 0 are all
0, where it is exact): -2.7 / -3.7 with Ntilde = 3.  GARCH's backward law is close to the filter weights at the default
parameters (the transition density varies little over the parents), so a parent shifted by one index is nearly as likely
as the right one and the one-in-ten mutant needs more draws: it scored -2.0 / -0.2 at optimal 128 / 24 / 2, -5.0 / 0.6 at
prior 200 / 24 / 3 and -4.2 / -1.6 at optimal 700 / 6 / 3 (the other three mutants were beyond 5 there already), hence
T = 96, 48 and 12 for those cases.  Measured at the shapes of the GPU file (Z_p / Z_x; reference: the oracle's
accept_reject=False parents, which the wrong samplers start from):

    model, N, T, Ntilde        reference     weights only   density only    J+1, 1 in 10   next lane
    garch optimal 128 96 3      0.2 /  0.5   -54.4 /  5.6   -22.0 /  -3.3    -7.5 /  0.9    -75.9 /  -2.6
    garch optimal 700 12 3     -1.0 /  0.1   -45.0 /  0.3   -12.0 /  -3.7    -7.3 / -0.5    -59.0 /  -6.8
    garch prior 200 48 3       -0.4 / -1.3   -25.4 /  2.3   -69.3 / -26.2    -9.4 / -3.5    -85.8 / -29.5
    garch prior 700 6 2         0.3 /  0.6   -25.6 / -1.3   -48.8 / -46.3    -7.3 / -3.7    -61.6 / -44.8
    lgssm optimal 100 24 3     -0.9 /  0.0   -35.6 / -6.8   -18.1 /  -0.6    -6.5 / -1.3    -53.3 /  -6.5
    lgssm optimal 200 24 2     -0.6 / -0.1   -39.7 / -5.1   -19.7 /  -1.5    -6.1 / -1.4    -58.1 /  -5.3
    lgssm optimal 700 6 2      -0.0 /  0.9   -63.7 / -7.4   -21.6 /  -3.7    -8.5 / -1.4    -79.6 / -22.6
    lgssm prior 128 24 3        1.1 / -0.2   -37.9 /  1.0   -26.7 /  -7.5    -6.9 / -1.4    -70.1 /  -7.4
    svm prior 100 24 3         -0.9 / -0.5   -60.0 / -3.1    -7.3 /  -1.7    -7.6 /  0.6    -75.4 /   0.3
    svm prior 200 24 2         -0.9 /  0.8   -61.9 /  4.6   -10.2 /  -3.8    -9.0 /  1.4    -80.9 /  -7.0
    svm prior 700 6 3           1.6 / -0.0   -55.5 / 12.2   -10.6 / -10.5    -7.1 / -4.4    -78.0 / -60.2
    svm prior 1100 6 2         -0.8 /  0.3   -42.0 / -7.4    -6.0 /  -8.9    -5.7 / -5.2    -55.7 / -51.4
    svm prior 1100 6 3         -0.6 / -2.0   -74.3 / -5.7   -13.4 / -13.7   -10.2 / -4.6   -104.3 / -58.8

"next lane" is what the device fallback returns if it reads its result from lane Lsel + 1: that lane's own resolve, which
stops at its first entry, parent Lsel + 1 of chunk 0."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from test_host_logic import default_params, GEN
from test_gpu_n2_one_wave import _prior_x

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import forced_window  # noqa: E402
import test_gpu_paris_device_replay as gpu_file  # noqa: E402  (its case tables; nothing in it runs without a GPU)

# (model, kernel, N, T, Ntilde) of every case of tests/test_gpu_paris_device_replay.py, and the statistic it runs there
GPU_CASES = sorted({(c[1], c[2], c[3], c[4], c[5], c[7]) for c in gpu_file.REG_CASES} |
                   {("svm", "prior", 1100, 6, nt, stat) for nt, _, stat in gpu_file.MEM_CASES} |
                   {(c[1], c[2], c[3], c[4], c[5], "score") for c in gpu_file.F32_CASES})
SHAPES = sorted({c[:5] for c in GPU_CASES})
assert len(SHAPES) == 13 and min(N * T * Nt for _, _, N, T, Nt in SHAPES) == 7200


def _window(N, T):
    """[2, T - 1); the large-N unit's cases start at 1"""
    return (2, T - 1) if N <= 1024 else (1, T - 1)


@functools.lru_cache(maxsize=None)
def _oracle_window(model, kernel, N, T, Ntilde, accept_reject, stat="score"):
    """One PaRIS window of the oracle on the legacy stream (NpDraws, the reference's default thresholds), save_all."""
    p = default_params(model)
    theta = p.theta()
    np.random.seed(17)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    pm, pv = _prior_x(model, theta)
    t1, tL = _window(N, T)
    kw = dict(kernel=kernel, stat=stat, t1=t1, tL=tL, weights=np.linspace(20.0, 30.0, tL - t1), prior_mean=pm, prior_var=pv,
              Ntilde=Ntilde)
    ref = po.pf_window_paris_rng(model, theta, y, N, rng=np.random.RandomState(1000 + N + T), save_all=True,
                                 accept_reject=accept_reject, **kw)
    return theta, y, kw, ref


def _same(a, b):
    for k in ("all_x_t", "all_log_weights", "all_statistics", "all_loglikelihood_estimate", "all_ancestors", "all_paris_J",
              "mean_statistic", "statistics"):
        assert np.array_equal(a[k], b[k]), k
    assert a["loglikelihood_estimate"] == b["loglikelihood_estimate"]


@pytest.mark.parametrize("model,kernel", [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal")])
@pytest.mark.parametrize("stat", ["score", "suff"])
def test_oracle_fed_its_own_parents_repeats_itself_bitwise(model, kernel, stat):
    """paris_parents replaces the backward draw and nothing else: the NpDraws run (accept-reject, and accept_reject=False)
    and the PoolDraws run, each fed the filter streams it consumed and its own J with no paris_draws at all, come back
    bit for bit."""
    N, T, Ntilde = 60, 5, 3
    theta, y, kw, _ = _oracle_window(model, kernel, N, T, Ntilde, True, stat)
    for ar in (True, False):
        # NpDraws: the filter's draws interleave with the backward ones on one generator; keep what the run took
        rs = np.random.RandomState(7)
        z0, U, Z = rs.normal(size=N), po._LazyStreams(rs, N, "u"), po._LazyStreams(rs, N, "z")
        ref = po.pf_window(model, theta, y, N, z0, U, Z, pf="paris", save_all=True, paris_draws=po.NpDraws(rs),
                           accept_reject=ar, **kw)
        assert ref["all_paris_J"].shape == (T, N, Ntilde) and ref["all_paris_J"].min() >= 0 and ref["all_paris_J"].max() < N
        u, z = np.array([U.cache[t] for t in range(T)]), np.array([Z.cache[t] for t in range(T)])
        again = po.pf_window(model, theta, y, N, z0, u, z, pf="paris", save_all=True,
                             paris_parents=lambda t: ref["all_paris_J"][t], **kw)
        _same(again, ref)
    # PoolDraws: the streams are plain arrays
    rs = np.random.RandomState(3)
    R = 3
    z0, u, z = po.draw_streams(rs, N, T)
    pools = [rs.random_sample((T, Ntilde, R, N)), rs.random_sample((T, Ntilde, R, N)), rs.random_sample((T, Ntilde, N))]
    ref = po.pf_window(model, theta, y, N, z0, u, z, pf="paris", save_all=True, max_accept_reject=R, manual_sample_threshold=0,
                       paris_draws=po.PoolDraws(*pools), **kw)
    again = po.pf_window(model, theta, y, N, z0, u, z, pf="paris", save_all=True, paris_parents=lambda t: ref["all_paris_J"][t],
                         **kw)
    _same(again, ref)
    # other parents give another window; no draws and no parents is refused
    other = po.pf_window(model, theta, y, N, z0, u, z, pf="paris", save_all=True,
                         paris_parents=lambda t: (ref["all_paris_J"][t] + 1) % N, **kw)
    assert np.array_equal(other["all_x_t"], ref["all_x_t"]) and not np.array_equal(other["all_statistics"], ref["all_statistics"])
    with pytest.raises(ValueError, match="paris_draws"):
        po.pf_window(model, theta, y, N, z0, u, z, pf="paris", **kw)


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "{0}-{1}-N{2}-T{3}-Nt{4}-{5}".format(*c))
def test_forced_paris_steps_return_the_oracles_own_window(case):
    """(a) From the oracle's step t and its backward parents, forced_paris_steps gives the oracle's step t + 1 --
    log-weights, statistics, running log-likelihood -- at 1e-12, at every GPU shape with the statistic it runs there."""
    shape, stat = case[:5], case[5]
    model, kernel, N, T, Ntilde = shape
    theta, y, kw, ref = _oracle_window(model, kernel, N, T, Ntilde, False, stat)
    t1, tL = kw["t1"], kw["tL"]
    lw, st, dll = forced_window.forced_paris_steps(model, kernel, theta, y, ref["all_x_t"], ref["all_log_weights"],
                                                   ref["all_statistics"], ref["all_ancestors"], ref["all_paris_J"], stat=stat,
                                                   t1=t1, tL=tL, weights=kw["weights"])
    np.testing.assert_allclose(lw, ref["all_log_weights"][1:], rtol=1e-12, atol=0)
    np.testing.assert_allclose(st, ref["all_statistics"][1:], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.cumsum(dll), ref["all_loglikelihood_estimate"][1:], rtol=1e-12, atol=0)
    assert np.all(st[:t1] == 0.0) and np.any(st[t1] != 0.0)
    # a check, not a copy: parents shifted by one index move the statistics far beyond the GPU tests' 1e-7
    _, bad, _ = forced_window.forced_paris_steps(model, kernel, theta, y, ref["all_x_t"], ref["all_log_weights"],
                                                 ref["all_statistics"], ref["all_ancestors"], (ref["all_paris_J"] + 1) % N,
                                                 stat=stat, t1=t1, tL=tL, weights=kw["weights"])
    # (from the second window step on: GARCH's sufficient statistic reads the child alone, so the first one cannot tell)
    assert np.max(np.abs(bad[t1 + 1] - ref["all_statistics"][t1 + 2])) > 1e-3


@pytest.mark.parametrize("accept_reject", [True, False], ids=["accept_reject", "exact"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{0}-{1}-N{2}-T{3}-Nt{4}".format(*s))
def test_backward_law_on_the_oracles_own_parents(shape, accept_reject):
    """(b) Both scores below 5 on the oracle's own J, every term counted (no backward law of these windows is constant)."""
    model, kernel, N, T, Ntilde = shape
    theta, y, kw, ref = _oracle_window(model, kernel, N, T, Ntilde, accept_reject)
    zp, zx, terms = forced_window.backward_law_scores(model, po.derived(model, theta), ref["all_x_t"], ref["all_log_weights"],
                                                      ref["all_paris_J"])
    print("backward law", shape, "accept-reject" if accept_reject else "exact", zp, zx, terms)
    assert terms == T * N * Ntilde
    assert abs(zp) < 5.0 and abs(zx) < 5.0, (zp, zx)


def wrong_samplers(model, d, ref, rs):
    """Four wrong backward samplers on the oracle's trace -> {name: J [T, N, Ntilde]}."""
    x, lw, J = ref["all_x_t"], ref["all_log_weights"], ref["all_paris_J"]
    T, N, Ntilde = J.shape
    by_weight, by_density = np.empty_like(J), np.empty_like(J)
    for t in range(T):
        # the filter weights alone: as if every accept-reject candidate were accepted
        by_weight[t] = po.multinomial_ancestors(po.log_normalize(lw[t]), rs.random_sample(N * Ntilde)).reshape(N, Ntilde)
        # the transition density alone: the parents' log-weights dropped
        q = forced_window.backward_law(model, d, x[t], np.zeros(N), x[t + 1])
        for i in range(N):
            by_density[t, i] = po.multinomial_ancestors(q[i], rs.random_sample(Ntilde))
    tenth = J.reshape(-1).copy()
    tenth[::10] = (tenth[::10] + 1) % N
    # the lane-major enumeration of the device fallback holds parent k in lane k % 64, and the owning lane Lsel resolves
    # the chunk within its own entries.  Reading the result from lane Lsel + 1 (clamped to 63) returns what THAT lane
    # resolved: its local target is negative, so it stops at its first entry -- parent Lsel + 1 of chunk 0, clamped to N - 1
    next_lane = np.minimum(np.minimum(J % 64 + 1, 63), N - 1)
    return {"weights only": by_weight, "density only": by_density, "J + 1 on one draw in ten": tenth.reshape(J.shape),
            "next lane": next_lane}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{0}-{1}-N{2}-T{3}-Nt{4}".format(*s))
def test_backward_law_rejects_wrong_samplers(shape):
    """(c) Each wrong sampler drives at least one score to 5 or beyond at every (model, N, T, Ntilde) of the GPU file, GARCH
    included (the smallest: N = 100, T = 24, Ntilde = 3, 7200 draws); measured scores in the module docstring."""
    model, kernel, N, T, Ntilde = shape
    theta, y, kw, ref = _oracle_window(model, kernel, N, T, Ntilde, False)
    d = po.derived(model, theta)
    for name, J in wrong_samplers(model, d, ref, np.random.RandomState(5)).items():
        assert J.min() >= 0 and J.max() < N
        zp, zx, terms = forced_window.backward_law_scores(model, d, ref["all_x_t"], ref["all_log_weights"], J)
        print("backward law", shape, name, zp, zx)
        assert terms == T * N * Ntilde
        assert max(abs(zp), abs(zx)) >= 5.0, (name, zp, zx)
