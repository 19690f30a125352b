"""Host restatement of correlated pseudo-marginal PMMH for SVM and LGSSM (NumPy, test-only): the sorted, correlated filter of
csrc/pfg_cpm.hip and a whole chain step on top of pmmh_model.py, written from the equations.

  model    x_{-1} ~ N(prior_mean, prior_var);  x_t = A x_{t-1} + z / LQinv;  SVM: y_t ~ N(0, R exp(x_t));  LGSSM: y_t ~ N(C x_t, R)
  U        [T+1][N+1] standard normals per chain.  Row 0, columns 0 .. N-1: the normals of x_{-1}; row t+1, columns 0 .. N-1: the
           state normals of step t; row t+1, column N: the resampling normal of step t (t >= 1).
  propose  U' = rho U + sqrt(1 - rho^2) eps (rho = 0: eps), eps entry (row, col) from Philox4x32-10 under (seed_lo, seed_hi),
           counter {gid_lo, step_lo, row ^ (step_hi ^ gid_hi), 0x43500000 | col >> 2}: normal_pair(r0, r1) -> columns 4q, 4q + 1,
           normal_pair(r2, r3) -> columns 4q + 2, 4q + 3.
  filter   t = 0: x_{-1}^i = prior_mean + sqrt(prior_var) U[0][i], x_0^i from U[1][i], lw = log g(y_0 | x_0).  t >= 1: the particles in
           ascending order of (state, index); the CDF of exp(lw - max lw) in that order; child r searches with ((r + u) / N) W,
           u = min(Phi(U[t+1][N]), 1 - 2^-53), the smallest j with cdf[j] > target, at most N-1; it gathers the state at sorted
           position j and moves with U[t+1][r].  sort = False keeps the particles in index order (plain systematic resampling).
  ll       sum_t log((1 / N) sum_i w_t^i), the Gaussian constants included; -inf for a chain whose weight sum is zero or
           not finite at some step.

Every chain of a call is filtered at once (arrays [C, ...]) in the floating type `F` (np.float64: the device's; np.longdouble:
the judge).  `forced` replays recorded parents (sorted coordinates): the states then follow the recording while `own` keeps what
this model's search would have chosen and `gap` how far, relative to the weight sum, its target lay from the nearest CDF edge.
"""
import math

import numpy as np

import keyed_draws as kd
import pmmh_model as pm
from chain_filter_model import EDGE_REL, LD, PM, PV, SEED, THETA, Key, case_theta_y, consts, logw, search  # noqa: F401

TAG_CPM = 0x43500000
CPM_SEED_XOR = 0x43504D4D           # ChainEnsemble keys the filter's eps with seed ^ this (ensemble_settings.py, FILTERS["cpm"].salt)
U_MAX = 1.0 - 2.0 ** -53

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def filter_seed(seed):
    return (int(seed) ^ CPM_SEED_XOR) & 0xFFFFFFFFFFFFFFFF


def eps(T, N, seed, gids, step):
    """[C, T+1, N+1] long double: every eps of the launch at counter `step` of the chains with global ids `gids`."""
    key = Key(gids, seed, step)
    q = np.arange((N >> 2) + 1, dtype=np.uint64)
    out = np.zeros((len(gids), T + 1, 4 * len(q)), dtype=LD)
    for row in range(T + 1):
        r = key.draw(row, np.uint64(TAG_CPM) | q)
        a, b = kd.normal_pair(r[0], r[1])
        c, d = kd.normal_pair(r[2], r[3])
        out[:, row] = np.stack([a, b, c, d], axis=-1).reshape(len(gids), -1)
    return out[:, :, :N + 1]


def propose_u(U, rho, T, N, seed, gids, step):
    """U' [C, T+1, N+1] float64 as the kernel forms it: rho * U + sqrt(1 - rho * rho) * eps on the f64 eps; rho = 0 reads no U.
    Also returns eps in long double."""
    e = eps(T, N, seed, gids, step)
    e64 = e.astype(np.float64)
    if rho == 0:
        return e64, e
    rho = np.float64(rho)
    return rho * np.asarray(U, dtype=np.float64) + np.sqrt(np.float64(1.0) - rho * rho) * e64, e


def resampling_uniform(z):
    """u = min(Phi(z), 1 - 2^-53), Phi(z) = erfc(-z / sqrt 2) / 2, in double."""
    return np.minimum(0.5 * _erfc(-np.asarray(z, dtype=np.float64) / np.float64(1.4142135623730951)), U_MAX)


def loglik(model, theta, y, U, prior_mean, prior_var, sort=True, F=np.float64, forced=None):
    """The filter of C chains on U [C, T+1, N+1].  theta [C, P], y [T].  forced: recorded parents [C, T, N] (row 0 ignored).
    Returns dict: ll [C], inc [C, T], anc / own / gap [C, T, N] (row 0: -1 / inf), degenerate [C]."""
    th = np.asarray(theta, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    C, T, N = th.shape[0], U.shape[1] - 1, U.shape[2] - 1
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), (C, T)).astype(F)
    c = consts(model, th, F)
    logN = np.log(F(N))
    xm1 = F(prior_mean) + np.sqrt(F(prior_var)) * U[:, 0, :N].astype(F)
    x = c["iLQ"] * U[:, 1, :N].astype(F) + xm1 * c["A"]
    lw = logw(model, c, x, y[:, 0:1], F)
    ll = np.zeros(C, dtype=F)
    inc = np.full((C, T), np.nan, dtype=F)
    anc = np.full((C, T, N), -1, dtype=np.int64)
    own = np.full((C, T, N), -1, dtype=np.int64)
    gap = np.full((C, T, N), np.inf)
    alive = np.ones(C, dtype=bool)
    r = np.arange(N, dtype=F)[None, :]
    for t in range(1, T + 1):
        if sort and t < T:
            order = np.argsort(x, axis=1, kind="stable")        # ties in index order: the key (state, index)
            x, lw = np.take_along_axis(x, order, axis=1), np.take_along_axis(lw, order, axis=1)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            m = np.max(np.where(np.isnan(lw), -np.inf, lw), axis=1, keepdims=True)
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
        u = resampling_uniform(U[:, t + 1, N]).astype(F)[:, None]
        j, g = search(cdf, ((r + u) / F(N)) * W[:, None])
        own[:, t], gap[:, t] = j, g
        anc[:, t] = j if forced is None else np.asarray(forced)[:, t]
        xp = np.take_along_axis(x, anc[:, t], axis=1)
        x = c["iLQ"] * U[:, t + 1, :N].astype(F) + xp * c["A"]
        lw = logw(model, c, x, y[:, t:t + 1], F)
    ll = np.where(alive, ll, -np.inf)
    return dict(ll=ll, inc=inc, anc=anc, own=own, gap=gap, degenerate=~alive)


def index_mismatches(rec_anc, res):
    """Recorded parents [C, T, N] against what `res` (a filter forced on them) would have searched: (wrong, left out, total).
    A search whose target lies within EDGE_REL of a CDF entry is left out; every other index must be the model's."""
    ok = ~res["degenerate"]
    rec = np.asarray(rec_anc, dtype=np.int64)[ok][:, 1:]
    own, gap = res["own"][ok][:, 1:], res["gap"][ok][:, 1:]
    edge = gap <= EDGE_REL
    wrong = (rec != own) & ~edge
    return int(wrong.sum()), int(edge.sum()), int(rec.size)


def chain_step(model, prior, theta, ll, U, scale, rho, y, prior_mean, prior_var, seed, chain_offset, step, sort=True):
    """One step (from 0) of C correlated PMMH chains: pmmh_model's proposal and decision around this file's filter.  theta [C, P],
    ll [C], U [C, T+1, N+1]: the chains' states.  Returns dict: theta, ll, U (the new states), accepted, margin, prop, valid,
    ll_prop, U_prop."""
    theta = np.asarray(theta, dtype=np.float64)
    C, T, N = theta.shape[0], U.shape[1] - 1, U.shape[2] - 1
    ctr = pm.step_counter(step)
    useed = pm.update_seed(seed)
    pr = pm.propose(model, theta, scale, useed, chain_offset, ctr)
    prop = np.where(pr.valid[:, None], pr.raw, theta.astype(LD)).astype(np.float64)
    Up, _ = propose_u(U, rho, T, N, filter_seed(seed), kd.chain_ids(C, chain_offset), ctr)
    llp = np.asarray(loglik(model, prop, y, Up, prior_mean, prior_var, sort=sort)["ll"], dtype=np.float64)
    acc, margin = pm.accept(model, prior, theta, prop, pr.valid, ll, llp, useed, chain_offset, ctr)
    th, l2, U2 = theta.copy(), np.asarray(ll, dtype=np.float64).copy(), np.asarray(U, dtype=np.float64).copy()
    th[acc], l2[acc], U2[acc] = prop[acc], llp[acc], Up[acc]
    return dict(theta=th, ll=l2, U=U2, accepted=acc, margin=margin, prop=prop, valid=pr.valid, ll_prop=llp, U_prop=Up)


def chain_init(model, theta, y, T, N, prior_mean, prior_var, seed, chain_offset):
    """The init pass: rho = 0 at counter 0.  Returns (ll [C], U [C, T+1, N+1])."""
    C = np.asarray(theta).shape[0]
    U, _ = propose_u(None, 0.0, T, N, filter_seed(seed), kd.chain_ids(C, chain_offset), 0)
    return np.asarray(loglik(model, theta, y, U, prior_mean, prior_var)["ll"], dtype=np.float64), U


# ---- the cases the CPU and the device tests share ---------------------------------------------------------------------------
# (N, T, B, rho) of the device replay (tests/test_gpu_cpm.py): N on both sides of the one-wave switch (128 | 129), powers of
# two and not (the padding), the ends 2 and 1024; T = 1 (no resampling at all), 2, 7, 24; B from 1 to 70; rho 0 (reads no U),
# 0.5 and 0.99
CASES = [(2, 1, 1, 0.0), (2, 24, 3, 0.5), (3, 7, 70, 0.99), (5, 2, 70, 0.5), (64, 7, 3, 0.0), (100, 24, 5, 0.99),
         (128, 24, 70, 0.5), (129, 2, 3, 0.99), (200, 7, 2, 0.5), (256, 24, 3, 0.0), (1000, 7, 70, 0.99), (1024, 24, 1, 0.5),
         (1024, 1, 3, 0.0)]


def case_inputs(model, N, T, B, seed=SEED):
    """theta [B, P], y [T], the current U [B, T+1, N+1] of a case: deterministic, moderate."""
    th, y, rs = case_theta_y(model, N, T, B, seed)
    U = rs.standard_normal((B, T + 1, N + 1))
    return th, y, U
