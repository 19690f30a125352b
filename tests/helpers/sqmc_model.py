"""Host restatement of the sequential quasi-Monte Carlo filter for SVM and LGSSM (NumPy, test-only): the filter of
csrc/pfg_sqmc.hip and a whole PMMH step on top of pmmh_model.py, written from the equations.

  model    x_{-1} ~ N(prior_mean, prior_var);  x_t = A x_{t-1} + z / LQinv;  SVM: y_t ~ N(0, R exp(x_t));  LGSSM: y_t ~ N(C x_t, R)
  points   index i in [0, N), N = 2^m: a_i = bitreverse32(i) (van der Corput), b_i = XOR over the set bits k of i of V_k,
           V_0 = 0x80000000, V_{k+1} = V_k ^ (V_k >> 1) (the second Sobol' dimension)
  shift    row r = 0 .. T (row 0: x_{-1}, row t+1: step t): one Philox4x32-10 draw under (seed_lo, seed_hi), counter {gid_lo,
           step_lo, r ^ (step_hi ^ gid_hi), 0x53510000} gives (s_a, s_b, l_a, l_b);  U52 = ((a_i ^ s_a) << 20) | (l_a >> 12),
           u = (U52 + 0.5) 2^-52;  V52, v likewise from b_i, s_b, l_b.  z = Phi^-1(v).
  rank     the rank of point i in u-order is (a_i ^ s_a) >> (32 - m); sorted position k takes point
           i(k) = bitreverse_m(k ^ (s_a >> (32 - m))) and u_(k) = (k + delta) / N
  filter   row 0: x_{-1}^i = prior_mean + sqrt(prior_var) z_i (particle = point index).  t = 0: the particles in ascending order
           of (x_{-1}, index), the child at position k moves from the parent at position k with z of row 1's point i(k).  t >= 1:
           ascending order of (state, index); the CDF of exp(lw - max lw) in that order; child k searches with u_(k) W, the
           smallest j with cdf[j] > target, at most N-1; it gathers the sorted state at j and moves with z of row t+1's point i(k).
  ll       sum_t log((1 / N) sum_i w_t^i), the Gaussian constants included; -inf for a chain whose weight sum is zero or
           not finite at some step.

Every chain of a call is filtered at once (arrays [C, ...]) in the floating type `F` (np.float64: the device's; np.longdouble:
the judge).  `forced` replays recorded parents (sorted coordinates): the states then follow the recording while `own` keeps what
this model's search would have chosen and `gap` how far, relative to the weight sum, its target lay from the nearest CDF edge.
`z` replays recorded normals [C, T+1, N] (row 0 by particle, the later rows by child) instead of Phi^-1 of the points.
"""
import numpy as np
from scipy.special import ndtri

import keyed_draws as kd
import pmmh_model as pm
from chain_filter_model import EDGE_REL, LD, PM, PV, SEED, THETA, Key, case_theta_y, consts, logw, search  # noqa: F401

TAG_SQMC = 0x53510000
SQMC_SEED_XOR = 0x53514D43          # ChainEnsemble keys the filter's shifts with seed ^ this (ensemble_settings.py, FILTERS["sqmc"].salt)
U32 = np.uint64(0xFFFFFFFF)


def filter_seed(seed):
    return (int(seed) ^ SQMC_SEED_XOR) & 0xFFFFFFFFFFFFFFFF


def log2_exact(N):
    m = int(N).bit_length() - 1
    if N < 2 or N > 1024 or (1 << m) != N:
        raise ValueError("N must be a power of two in 2 .. 1024, got {0}".format(N))
    return m


def bitreverse32(i):
    i = np.asarray(i, dtype=np.uint64)
    r = np.zeros_like(i)
    for k in range(32):
        r |= ((i >> np.uint64(k)) & np.uint64(1)) << np.uint64(31 - k)
    return r


def sobol2(i):
    """b_i as a 32-bit integer fraction."""
    i = np.asarray(i, dtype=np.uint64)
    b, v = np.zeros_like(i), np.uint64(0x80000000)
    for k in range(32):
        b ^= np.where((i >> np.uint64(k)) & np.uint64(1), v, np.uint64(0))
        v = v ^ (v >> np.uint64(1))
    return b


def shifted_points(N, words):
    """(U52, V52) [..., N] uint64 of the N points under the shift words = (s_a, s_b, l_a, l_b), arrays [...] of 32-bit values."""
    i = np.arange(N, dtype=np.uint64)
    sa, sb, la, lb = (np.asarray(w, dtype=np.uint64)[..., None] for w in words)
    U = ((bitreverse32(i) ^ sa) << np.uint64(20)) | (la >> np.uint64(12))
    V = ((sobol2(i) ^ sb) << np.uint64(20)) | (lb >> np.uint64(12))
    return U, V


def unit(U52, F=np.float64):
    """(U52 + 0.5) 2^-52: exact in double."""
    return (np.asarray(U52).astype(F) + F(0.5)) * F(2.0 ** -52)


def point_of_rank(N, sa):
    """i(k) [..., N]: the point whose u has rank k under the shift word s_a [...]."""
    m = log2_exact(N)
    k = np.arange(N, dtype=np.uint64)
    top = np.asarray(sa, dtype=np.uint64)[..., None] >> np.uint64(32 - m)
    return (bitreverse32(k ^ top) >> np.uint64(32 - m)).astype(np.int64)


def comb_offset(N, sa, la, F=np.float64):
    """delta [...] of u_(k) = (k + delta) / N: exact in double."""
    m = log2_exact(N)
    low = np.asarray(sa, dtype=np.uint64) & np.uint64((1 << (32 - m)) - 1)
    rem = (low << np.uint64(20)) | (np.asarray(la, dtype=np.uint64) >> np.uint64(12))
    return (rem.astype(F) + F(0.5)) * F(2.0 ** (m - 52))


def rows(T, seed, gids, step):
    """The shift words of rows 0 .. T of the chains with global ids `gids` at counter `step`: [4][C, T+1] uint64."""
    key = Key(gids, seed, step)
    w = [key.draw(r, TAG_SQMC) for r in range(T + 1)]           # each [4][C, 1]
    return [np.concatenate([w[r][q] for r in range(T + 1)], axis=1).astype(np.uint64) for q in range(4)]


def normals(N, T, seed, gids, step):
    """z [C, T+1, N] float64 as the filter uses them -- row 0 by particle (= point index), row t+1 by child (sorted position k
    takes point i(k)) -- with v [C, T+1, N] in the same layout and delta [C, T+1] (row 0's is not used)."""
    sa, sb, la, lb = rows(T, seed, gids, step)
    _, V = shifted_points(N, (sa, sb, la, lb))                   # [C, T+1, N] by point index
    order = point_of_rank(N, sa)                                 # [C, T+1, N]
    order[:, 0] = np.arange(N)
    v = unit(np.take_along_axis(V, order, axis=2))
    return ndtri(v), v, comb_offset(N, sa, la)


def loglik(model, theta, y, N, prior_mean, prior_var, seed, gids, step, F=np.float64, forced=None, z=None):
    """The filter of C chains.  theta [C, P], y [T] or [C, T].  forced: recorded parents [C, T, N] (row 0 ignored); z: recorded
    normals [C, T+1, N].  Returns dict: ll [C], inc [C, T], anc / own / gap [C, T, N] (row 0: -1 / inf), degenerate [C], z."""
    th = np.asarray(theta, dtype=np.float64)
    C = th.shape[0]
    y = np.asarray(y, dtype=np.float64)
    T = y.shape[-1]
    y = np.broadcast_to(y, (C, T)).astype(F)
    zz, _, delta = normals(N, T, seed, gids, step)
    if z is not None:
        zz = np.asarray(z, dtype=np.float64)
    c = consts(model, th, F)
    logN = np.log(F(N))
    xm1 = F(prior_mean) + np.sqrt(F(prior_var)) * zz[:, 0].astype(F)
    xm1 = np.take_along_axis(xm1, np.argsort(xm1, axis=1, kind="stable"), axis=1)
    x = c["iLQ"] * zz[:, 1].astype(F) + xm1 * c["A"]
    lw = logw(model, c, x, y[:, 0:1], F)
    ll = np.zeros(C, dtype=F)
    inc = np.full((C, T), np.nan, dtype=F)
    anc = np.full((C, T, N), -1, dtype=np.int64)
    own = np.full((C, T, N), -1, dtype=np.int64)
    gap = np.full((C, T, N), np.inf)
    alive = np.ones(C, dtype=bool)
    k = np.arange(N, dtype=F)[None, :]
    for t in range(1, T + 1):
        if t < T:
            order = np.argsort(x, axis=1, kind="stable")        # ties in index order: the key (state, index)
            x, lw = np.take_along_axis(x, order, axis=1), np.take_along_axis(lw, order, axis=1)
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
        cdf = np.where(good[:, None], cdf, np.arange(1, N + 1, dtype=F)[None, :])
        W = np.where(good, W, N)
        u = (k + delta[:, t + 1].astype(F)[:, None]) / F(N)
        j, g = search(cdf, u * W[:, None])
        own[:, t], gap[:, t] = j, g
        anc[:, t] = j if forced is None else np.asarray(forced)[:, t]
        xp = np.take_along_axis(x, anc[:, t], axis=1)
        x = c["iLQ"] * zz[:, t + 1].astype(F) + xp * c["A"]
        lw = logw(model, c, x, y[:, t:t + 1], F)
    ll = np.where(alive, ll, -np.inf)
    return dict(ll=ll, inc=inc, anc=anc, own=own, gap=gap, degenerate=~alive, z=zz)


def index_mismatches(rec_anc, res):
    """Recorded parents [C, T, N] against what `res` (a filter forced on them) would have searched: (wrong, left out, total).
    A search whose target lies within EDGE_REL of a CDF entry is left out; every other index must be the model's."""
    ok = ~res["degenerate"]
    rec = np.asarray(rec_anc, dtype=np.int64)[ok][:, 1:]
    own, gap = res["own"][ok][:, 1:], res["gap"][ok][:, 1:]
    edge = gap <= EDGE_REL
    wrong = (rec != own) & ~edge
    return int(wrong.sum()), int(edge.sum()), int(rec.size)


def chain_init(model, theta, y, N, prior_mean, prior_var, seed, chain_offset):
    """The init pass: the filter at counter 0.  Returns ll [C]."""
    C = np.asarray(theta).shape[0]
    return np.asarray(loglik(model, theta, y, N, prior_mean, prior_var, filter_seed(seed), kd.chain_ids(C, chain_offset), 0)["ll"],
                      dtype=np.float64)


def chain_step(model, prior, theta, ll, scale, y, N, prior_mean, prior_var, seed, chain_offset, step):
    """One step (from 0) of C SQMC PMMH chains: pmmh_model's proposal and decision around this file's filter.  theta [C, P],
    ll [C]: the chains' states.  Returns dict: theta, ll (the new states), accepted, margin, prop, valid, ll_prop."""
    theta = np.asarray(theta, dtype=np.float64)
    C = theta.shape[0]
    ctr = pm.step_counter(step)
    useed = pm.update_seed(seed)
    pr = pm.propose(model, theta, scale, useed, chain_offset, ctr)
    prop = np.where(pr.valid[:, None], pr.raw, theta.astype(LD)).astype(np.float64)
    llp = np.asarray(loglik(model, prop, y, N, prior_mean, prior_var, filter_seed(seed), kd.chain_ids(C, chain_offset), ctr)["ll"],
                     dtype=np.float64)
    acc, margin = pm.accept(model, prior, theta, prop, pr.valid, ll, llp, useed, chain_offset, ctr)
    th, l2 = theta.copy(), np.asarray(ll, dtype=np.float64).copy()
    th[acc], l2[acc] = prop[acc], llp[acc]
    return dict(theta=th, ll=l2, accepted=acc, margin=margin, prop=prop, valid=pr.valid, ll_prop=llp)


# ---- the cases the CPU and the device tests share ---------------------------------------------------------------------------
# (N, T, B, n_max) of the device replay (tests/test_gpu_sqmc.py): the ends 2 and 1024, both sides of the one-wave switch
# (128 | 256), T = 1 (no resampling at all), and N = 64 in the 256 x 4 shape
CASES = [(2, 1, 3, 2), (64, 12, 5, 64), (128, 12, 4, 128), (256, 6, 3, 256), (1024, 3, 2, 1024), (64, 12, 5, 256)]
