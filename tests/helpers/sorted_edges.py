"""Inputs that drive the two sorted filters (csrc/pfg_cpm.hip, csrc/pfg_sqmc.hip) into the branches generic draws never reach,
and the host conditions that say they got there (NumPy, test-only).  Used by tests/test_gpu_sorted_filter_edges.py and
tests/test_sorted_filter_edges_host.py.

  ties     LQinv = 1e30: x = fl(xp A) whatever the normal, so every child of one parent is bitwise its sibling.  prior (1, 1e-60):
           every particle equal from x_{-1} on ("all"); prior (1, 0.25): distinct x_{-1}, tie groups from the first resampling on
           ("groups").
  clamps   the resampling normal of every step at -400 / +400: u = 0 and u = 1 - 2^-53 exactly.
  sharp    LRinv = 300: nearly every weight underflows to 0, the CDF has long flat runs and few parents survive a step.
  late     y = +-1e300 from step d on: the chain dies at the weights of step d.

`run` restates the filter of cpm_model.loglik / sqmc_model.loglik (the same expressions in the same order: the host test pins it
to both, bit for bit in double) and keeps what they do not return: per resampling step the sorted states, lw - max and the CDF.
It takes the sort as an argument, so the same recursion runs on a sort that is wrong on purpose (rank_sort_without_tie_pass).
"""
import numpy as np

import cpm_model as cp
import keyed_draws as kd
import sqmc_model as sq
from chain_filter_model import EDGE_REL, consts, logw, search

T_EDGE, B_EDGE = 7, 3
LQ_COL = {"svm": 1, "lgssm": 2}
LR_COL = {"svm": 2, "lgssm": 3}
TIE_LQINV = 1e30
TIE_PRIOR = {"all": (1.0, 1e-60), "groups": (1.0, 0.25)}
SHARP_LRINV = 300.0
GROUP_REL = 1e-12                   # distinct tie groups lie further apart than this, relative: long double orders them as double does
EXP_ZERO = -745.1332191019412       # exp(d) rounds to 0 in double below log(2^-1075)
BAND = (-800.0, -700.0)             # lw - max in here: an exp may give a denormal on one side and 0 on the other

TIE_SEED = {3: cp.SEED + 3}          # N = 3: a seed under which every chain of both models has a step with equal states
CLAMP_SEED = {5: cp.SEED + 5}        # N = 5: a seed under which no weight of the sharp u = 0 cases has lw - max in BAND
CPM_TIE_N = {"one wave": [3, 64, 100, 128], "256 x 4": [130, 200, 1024]}
SQMC_TIE_SHAPES = [(2, 2), (64, 64), (128, 128), (256, 256), (1024, 1024), (64, 256)]      # (N, n_max)
CLAMP_N = [5, 128, 200, 1024]
CLAMP_RHO = [0.99, 0.5]             # 400 rho stays far beyond 38.5 and 8.3
FLAT_N = {"cpm": [5, 128, 200, 1024], "sqmc": [128, 256, 1024]}        # (SQMC takes powers of two: no 5)
LATE_D = [1, 3, 5]


# ---- the sorts ---------------------------------------------------------------------------------------------------------------
def stable_sort(x, lw, prev):
    """Ascending by (state, index): sx, slw [C, N]."""
    order = np.argsort(x, axis=1, kind="stable")
    return np.take_along_axis(x, order, axis=1), np.take_along_axis(lw, order, axis=1)


def rank_sort_without_tie_pass(x, lw, prev):
    """The one-wave rank sort of pfg::sort_by_state WITHOUT its second pass: particle i goes to slot count(x_j < x_i); equal
    states collide on a slot and the highest index wins; a slot nobody writes keeps the (sx, slw) of the step before (`prev`;
    None ahead of the first sort: a state of 0 with weight 0)."""
    C, N = x.shape
    pos = (x[:, None, :] < x[:, :, None]).sum(axis=-1)
    sx, slw = (np.zeros_like(x), np.full_like(lw, -np.inf)) if prev is None else (prev[0].copy(), prev[1].copy())
    rows = np.arange(C)
    for i in range(N):
        sx[rows, pos[:, i]] = x[:, i]
        slw[rows, pos[:, i]] = lw[:, i]
    return sx, slw


# ---- the filter --------------------------------------------------------------------------------------------------------------
def run(model, theta, y, xm1, z, targets, sort0, F=np.float64, forced=None, sort=stable_sort):
    """xm1 [C, N] by index; z [C, T, N] the state normals of step t by child; targets(t) [C, N] as fractions of the weight sum;
    sort0: sort x_{-1} ahead of step 0 (SQMC).  Returns dict: ll, inc, anc, own, gap, degenerate as cpm_model.loglik, and
    steps[t] for t = 1 .. T-1: dict(x, d = lw - max, cdf, W) in sorted order, moved [C, T, N] the states after the move of step t
    and from_ [C, T, N] the states they moved from."""
    th = np.asarray(theta, dtype=np.float64)
    C, N = xm1.shape
    y = np.asarray(y, dtype=np.float64)
    T = y.shape[-1]
    y = np.broadcast_to(y, (C, T)).astype(F)
    c = consts(model, th, F)
    logN = np.log(F(N))
    prev = None
    lw0 = np.zeros((C, N), dtype=F)
    if sort0:
        xm1, _ = sort(xm1, lw0, prev)
    x = c["iLQ"] * z[:, 0].astype(F) + xm1 * c["A"]
    lw = logw(model, c, x, y[:, 0:1], F)
    ll = np.zeros(C, dtype=F)
    inc = np.full((C, T), np.nan, dtype=F)
    anc = np.full((C, T, N), -1, dtype=np.int64)
    own = np.full((C, T, N), -1, dtype=np.int64)
    gap = np.full((C, T, N), np.inf)
    moved, from_ = np.zeros((C, T, N), dtype=F), np.zeros((C, T, N), dtype=F)
    moved[:, 0], from_[:, 0] = x, xm1
    alive = np.ones(C, dtype=bool)
    steps = {}
    for t in range(1, T + 1):
        if t < T:
            x, lw = sort(x, lw, prev)
            prev = (x, lw)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            m = np.max(np.where(np.isnan(lw) | np.isnan(x), np.inf, lw), axis=1, keepdims=True)
            cdf = np.cumsum(np.exp(lw - m), axis=1)
            W = cdf[:, -1]
            good = (W > 0) & np.isfinite(W)
            alive &= good
            step_inc = (m[:, 0] + np.log(np.where(good, W, 1))) - logN
        inc[:, t - 1] = np.where(alive, step_inc, np.nan)
        ll = ll + np.where(alive, step_inc, 0)
        if t == T:
            break
        steps[t] = dict(x=x, d=lw - m, cdf=cdf, W=W)
        cdf = np.where(good[:, None], cdf, np.arange(1, N + 1, dtype=F)[None, :])
        W = np.where(good, W, N)
        j, g = search(cdf, targets(t).astype(F) * W[:, None])
        own[:, t], gap[:, t] = j, g
        anc[:, t] = j if forced is None else np.asarray(forced)[:, t]
        xp = np.take_along_axis(x, anc[:, t], axis=1)
        x = c["iLQ"] * z[:, t].astype(F) + xp * c["A"]
        lw = logw(model, c, x, y[:, t:t + 1], F)
        moved[:, t], from_[:, t] = x, xp
    ll = np.where(alive, ll, -np.inf)
    return dict(ll=ll, inc=inc, anc=anc, own=own, gap=gap, degenerate=~alive, steps=steps, moved=moved, from_=from_, A=c["A"])


def run_cpm(model, theta, y, U, prior, **kw):
    """`run` on the normals U [C, T+1, N+1] of the correlated filter."""
    U = np.asarray(U, dtype=np.float64)
    N = U.shape[2] - 1
    F = kw.get("F", np.float64)
    xm1 = F(prior[0]) + np.sqrt(F(prior[1])) * U[:, 0, :N].astype(F)
    r = np.arange(N, dtype=F)[None, :]
    return run(model, theta, y, xm1, U[:, 1:, :N], lambda t: (r + cp.resampling_uniform(U[:, t + 1, N]).astype(F)[:, None]) / F(N),
               False, **kw)


def run_sqmc(model, theta, y, N, prior, gids, step, z=None, **kw):
    """`run` on the normals of the SQMC filter at (seed, gids, step) (or the recorded z [C, T+1, N]) and its comb."""
    T = np.asarray(y).shape[-1]
    zz, _, delta = sq.normals(N, T, sq.filter_seed(sq.SEED), gids, step)
    if z is not None:
        zz = np.asarray(z, dtype=np.float64)
    F = kw.get("F", np.float64)
    xm1 = F(prior[0]) + np.sqrt(F(prior[1])) * zz[:, 0].astype(F)
    k = np.arange(N, dtype=F)[None, :]
    return run(model, theta, y, xm1, zz[:, 1:], lambda t: (k + delta[:, t + 1].astype(F)[:, None]) / F(N), True, **kw)


def index_mismatches(rec_anc, res, skip_child=None):
    """cpm_model.index_mismatches with the children `skip_child` (an index) of every step taken out of the count altogether:
    (wrong, left out, total)."""
    ok = ~res["degenerate"]
    rec = np.asarray(rec_anc, dtype=np.int64)[ok][:, 1:]
    own, gap = res["own"][ok][:, 1:], res["gap"][ok][:, 1:]
    keep = np.ones(rec.shape, dtype=bool)
    if skip_child is not None:
        keep[:, :, skip_child] = False
    edge = (gap <= EDGE_REL) & keep
    wrong = (rec != own) & ~edge & keep
    return int(wrong.sum()), int(edge.sum()), int(keep.sum())


# ---- 1. ties -----------------------------------------------------------------------------------------------------------------
def tie_theta(model, th):
    th = np.array(th, dtype=np.float64)
    th[:, LQ_COL[model]] = TIE_LQINV
    return th


def cpm_tie_inputs(model, N):
    """theta (LQinv = 1e30), y, the current U of a tie case; rho is 0.5."""
    th, y, U = cp.case_inputs(model, N, T_EDGE, B_EDGE, TIE_SEED.get(N, cp.SEED))
    return tie_theta(model, th), y, U


def sqmc_tie_inputs(model, N):
    th, y, _ = sq.case_theta_y(model, N, T_EDGE, B_EDGE)
    return tie_theta(model, th), y


def tie_conditions(res, variant):
    """What a tie case rests on, from a run of the model in double: every move absorbed its normal (x = fl(xp A) bitwise), so
    the children of one parent are equal; no search on an edge; distinct states of a step lie more than GROUP_REL apart,
    relative; "all": one state per step and every parent its child's index; "groups": every step from the first resampling
    on has equal states.  Returns the number of distinct parents per (chain, step)."""
    assert not res["degenerate"].any()
    assert np.array_equal(res["moved"], res["from_"] * res["A"][:, :, None])
    assert np.all(res["gap"][:, 1:] > EDGE_REL)
    C, T, N = res["anc"].shape
    distinct = np.array([[len(np.unique(res["anc"][c, t])) for t in range(1, T)] for c in range(C)])
    for t, st in res["steps"].items():
        for c in range(C):
            v = np.unique(st["x"][c])
            if len(v) > 1:
                assert np.min(np.diff(v) / np.maximum(np.abs(v[1:]), np.abs(v[:-1]))) > GROUP_REL
            if variant == "all":
                assert len(v) == 1 and np.array_equal(res["anc"][c, t], np.arange(N))
            elif t >= 2 and N >= 64:
                assert len(v) < N
    if variant == "groups" and N >= 3:          # (N = 3 can pick three distinct parents at a step; not at every one)
        assert all(any(len(np.unique(st["x"][c])) < N for st in res["steps"].values()) for c in range(C))
    return distinct


# ---- 3. the clamps ------------------------------------------------------------------------------------------------------------
def clamp_inputs(model, N, sign, sharp=False, seed=None):
    """case_inputs with the resampling normal of every step at sign * 400 (sharp: LRinv = 300 as well)."""
    th, y, U = cp.case_inputs(model, N, T_EDGE, B_EDGE, CLAMP_SEED.get(N, cp.SEED) if seed is None else seed)
    U[:, 2:, N] = sign * 400.0
    if sharp:
        th[:, LR_COL[model]] = SHARP_LRINV
    return th, y, U


def first_nonzero_weight(res):
    """[C, T] the first sorted position of step t (rows 1 .. T-1) whose weight exp(lw - max) is not 0 in double."""
    C, T, N = res["anc"].shape
    out = np.full((C, T), -1, dtype=np.int64)
    for t, st in res["steps"].items():
        out[:, t] = np.argmax(st["d"].astype(np.float64) > EXP_ZERO, axis=1)
    return out


def leading_band_hits(res):
    """How many weights up to and including the first one with lw - max >= BAND[1] lie in BAND: the ones that could decide
    where a target of exactly 0 lands."""
    n = 0
    for st in res["steps"].values():
        d = st["d"].astype(np.float64)
        lead = np.cumsum(d >= BAND[1], axis=1) - (d >= BAND[1]) == 0
        n += int(((d > BAND[0]) & (d < BAND[1]) & lead).sum())
    return n


def leading_near_exp_zero(res, width=1e-6):
    """How many weights up to and including the first non-zero one have lw - max within `width` of EXP_ZERO: double rounds
    lw - max to 1e-13 there, so outside it the device's exp and the model's agree on which weight is 0."""
    n = 0
    for st in res["steps"].values():
        d = st["d"].astype(np.float64)
        lead = np.cumsum(d > EXP_ZERO, axis=1) - (d > EXP_ZERO) == 0
        n += int((np.abs(d - EXP_ZERO) <= width)[lead].sum())
    return n


def band_hits(res):
    """How many weights of the resampling steps have lw - max in BAND."""
    return sum(int(((st["d"] > BAND[0]) & (st["d"] < BAND[1])).sum()) for st in res["steps"].values())


# ---- 4. flat CDFs --------------------------------------------------------------------------------------------------------------
def sharp_theta(model, th):
    th = np.array(th, dtype=np.float64)
    th[:, LR_COL[model]] = SHARP_LRINV
    return th


def cpm_flat_inputs(model, N):
    th, y, U = cp.case_inputs(model, N, T_EDGE, B_EDGE)
    return sharp_theta(model, th), y, U


def sqmc_flat_inputs(model, N):
    th, y, _ = sq.case_theta_y(model, N, T_EDGE, B_EDGE)
    return sharp_theta(model, th), y


def ppt_of(n_max):
    """The particles per thread of the launch shape: 64 x 2 up to 128, 256 x 4 above."""
    return 2 if n_max <= 128 else 4


def bisect_searches(res, ppt):
    """How many searches of a run in double the kernel's second to PPT-th child of a thread answers past its 3 probes, in
    cdf_search(cdf, N, target, j + 1): the child's answer lies more than 3 entries above its left neighbour's."""
    N = res["own"].shape[2]
    inner = (np.arange(1, N) % ppt) != 0
    return sum(int((np.diff(res["own"][:, t], axis=1)[:, inner] > 3).sum()) for t in res["steps"])


def bisect_from_flat_runs(res, ppt):
    """How many searches of a run in double the kernel's second to PPT-th child of a thread answers past its 3 probes, in
    cdf_search(cdf, N, target, j + 1), BECAUSE the CDF is flat: the child's answer lies more than 3 entries above its left
    neighbour's and every entry from that one up to its own (exclusive) is the same number -- a run of more than 3 equal
    entries."""
    C, T, N = res["own"].shape
    n = 0
    for t, st in res["steps"].items():
        own = res["own"][:, t]
        for r in range(1, N):
            if r % ppt == 0:
                continue
            for c in np.nonzero(own[:, r] - own[:, r - 1] > 3)[0]:
                run_ = st["cdf"][c, own[c, r - 1]:own[c, r]]
                n += int(np.all(run_ == run_[0]))
    return n


def distinct_parents(res):
    C, T, N = res["own"].shape
    return np.array([[len(np.unique(res["own"][c, t])) for t in range(1, T)] for c in range(C)])


# ---- 5. a chain that dies late ---------------------------------------------------------------------------------------------------
def late_death_y(y, B, chain, d):
    """y [B, T]: chain `chain` observes +-1e300 from step d on."""
    ys = np.tile(np.asarray(y, dtype=np.float64), (B, 1))
    T = ys.shape[1]
    ys[chain, d:] = 1e300 * (-1.0) ** np.arange(d, T)
    return ys


def host_proposal(U, rho, off, step):
    """U' of a launch of tests/test_gpu_sorted_score.py's launch_cpm, from the keyed draws."""
    B, T, N = U.shape[0], U.shape[1] - 1, U.shape[2] - 1
    return cp.propose_u(U, rho, T, N, cp.filter_seed(cp.SEED), kd.chain_ids(B, off), step)[0]
