"""Host restatement of the score the two sorted filters carry (NumPy, test-only): cpm_model.loglik (csrc/pfg_cpm.hip) and
sqmc_model.loglik (csrc/pfg_sqmc.hip) with Poyiadjis' O(N) additive statistic and the fixed-lag shrinkage of Nemeth, Sherlock and
Fearnhead (2016), and a whole step of sampler='pmala_sorted' on top of pmala_model.py -- written from the equations.

  filter   cpm_model's / sqmc_model's, draw for draw: the same x_{-1}, sort (ascending (state, index)), CDF, search and move.
  add      the complete-data score increment of the move xp -> x under observation y, H columns in score-column order
             SVM    [LRinv, LQinv, A]:     1 / LRinv - (y^2 exp(-x)) LRinv;  1 / LQinv - dx^2 LQinv;  (Qinv dx) xp
             LGSSM  [LRinv, LQinv, C, A]:  1 / LRinv - dy^2 LRinv;  1 / LQinv - dx^2 LQinv;  (Rinv dy) x;  (Qinv dx) xp
           dx = x - A xp, dy = y - C x, Qinv = LQinv^2 + 1e-16, Rinv = LRinv^2 + 1e-16
  alpha    t = 0: alpha_i = add(x_{-1}^i -> x_0^i, y_0) (SQMC: the parent at sorted position i).
           t >= 1: alpha_r = lam alpha_parent(r) + (1 - lam) S_{t-1} + add(x_parent -> x_r, y_t),  S_{t-1} = sum_i w_i alpha_i / sum_i w_i
           under the weights the CDF of step t is built from.  lam == 1 does not read S.
  score    S_{T-1}, the weighted mean of the last step's alpha.
  mag      the same recursion on the absolute values of every term (|1 / LQinv| + |dx^2 LQinv|, ...): the sum of the absolute values
           of the terms of every score column, the magnitude a tolerance on `score` is relative to.
  orders   orders[t] [C, N], t = 0 .. T-1: the sort ahead of step t as sorted position -> index before the sort (the index of a
           child of step t-1; t = 0: the index of x_{-1}).  The identity where there is no sort (CPM: t = 0).  A parent recorded
           in sorted coordinates, anc[t][r] = j, is the particle orders[t][j].

Every chain of a call is filtered at once (arrays [C, ...]) in the floating type `F` (np.float64 or np.longdouble).  `forced`
replays recorded parents (sorted coordinates) as in cpm_model / sqmc_model.
"""
import numpy as np

import cpm_model as cm
import keyed_draws as kd
import pmala_model as pl
import pmmh_model as pm
import sqmc_model as sq
from chain_filter_model import LD, consts, logw, search

H_DIM = {"svm": 3, "lgssm": 4}


def add_terms(model, th, c, xp, x, y, F):
    """(add, |terms|) [C, N, H] of the moves xp -> x [C, N] under y [C, 1]."""
    th = np.asarray(th, dtype=F)
    LQ, LR = (th[:, 1:2], th[:, 2:3]) if model == "svm" else (th[:, 2:3], th[:, 3:4])
    one = F(1)
    iLQ, iLR = one / LQ, one / LR
    dx = x - c["A"] * xp
    a_A = (c["Qinv"] * dx) * xp
    q = (dx * dx) * LQ
    a_LQ = iLQ - q
    m_LQ = np.abs(iLQ) + np.abs(q)
    with np.errstate(over="ignore", invalid="ignore"):
        if model == "svm":
            r = ((y * y) * np.exp(-x)) * LR
            cols = [iLR - r, a_LQ, a_A]
            mags = [np.abs(iLR) + np.abs(r), m_LQ, np.abs(a_A)]
        else:
            dy = y - c["C"] * x
            r = (dy * dy) * LR
            a_C = (c["Rinv"] * dy) * x
            cols = [iLR - r, a_LQ, a_C, a_A]
            mags = [np.abs(iLR) + np.abs(r), m_LQ, np.abs(a_C), np.abs(a_A)]
    shape = x.shape
    return (np.stack([np.broadcast_to(v, shape) for v in cols], axis=-1).astype(F),
            np.stack([np.broadcast_to(v, shape) for v in mags], axis=-1).astype(F))


def _take(a, idx):
    """a [C, N] or [C, N, H] gathered along axis 1 by idx [C, N]."""
    return np.take_along_axis(a, idx if a.ndim == 2 else idx[:, :, None], axis=1)


def _filter(model, theta, y, xm1, sort0, z, targets, lam, F, forced):
    """The shared recursion.  xm1 [C, N] by index; sort0: sort x_{-1} ahead of step 0 (SQMC); z [C, T, N] the state normals of
    step t by child; targets(t) -> [C, N] the search targets of step t as fractions of the weight sum."""
    th = np.asarray(theta, dtype=np.float64)
    C, N = xm1.shape
    y = np.asarray(y, dtype=np.float64)
    T = y.shape[-1]
    y = np.broadcast_to(y, (C, T)).astype(F)
    H = H_DIM[model]
    c = consts(model, th, F)
    lam = F(lam)
    logN = np.log(F(N))
    ident = np.broadcast_to(np.arange(N), (C, N))
    orders = [ident.copy() for _ in range(T)]
    if sort0:
        orders[0] = np.argsort(xm1, axis=1, kind="stable")
        xm1 = _take(xm1, orders[0])
    x = c["iLQ"] * z[:, 0].astype(F) + xm1 * c["A"]
    lw = logw(model, c, x, y[:, 0:1], F)
    alpha, amag = add_terms(model, th, c, xm1, x, y[:, 0:1], F)
    ll = np.zeros(C, dtype=F)
    inc = np.full((C, T), np.nan, dtype=F)
    anc = np.full((C, T, N), -1, dtype=np.int64)
    own = np.full((C, T, N), -1, dtype=np.int64)
    gap = np.full((C, T, N), np.inf)
    alive = np.ones(C, dtype=bool)
    S, Smag = np.zeros((C, H), dtype=F), np.zeros((C, H), dtype=F)
    for t in range(1, T + 1):
        if t < T:
            order = np.argsort(x, axis=1, kind="stable")        # ties in index order: the key (state, index)
            orders[t] = order
            x, lw, alpha, amag = _take(x, order), _take(lw, order), _take(alpha, order), _take(amag, order)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            m = np.max(np.where(np.isnan(lw) | np.isnan(x), np.inf, lw), axis=1, keepdims=True)
            w = np.exp(lw - m)
            cdf = np.cumsum(w, axis=1)
            W = cdf[:, -1]
            good = (W > 0) & np.isfinite(W)
            alive &= good
            step_inc = (m[:, 0] + np.log(np.where(good, W, 1))) - logN
            Wd = np.where(good, W, 1)[:, None]
            S = np.sum(w[:, :, None] * alpha, axis=1) / Wd
            Smag = np.sum(w[:, :, None] * amag, axis=1) / Wd
        inc[:, t - 1] = np.where(alive, step_inc, np.nan)
        ll = ll + np.where(alive, step_inc, 0)
        if t == T:
            break
        cdf = np.where(good[:, None], cdf, np.arange(1, N + 1, dtype=F)[None, :])
        W = np.where(good, W, N)
        j, g = search(cdf, targets(t).astype(F) * W[:, None])
        own[:, t], gap[:, t] = j, g
        anc[:, t] = j if forced is None else np.asarray(forced)[:, t]
        xp = _take(x, anc[:, t])
        x = c["iLQ"] * z[:, t].astype(F) + xp * c["A"]
        lw = logw(model, c, x, y[:, t:t + 1], F)
        add, addmag = add_terms(model, th, c, xp, x, y[:, t:t + 1], F)
        pa, pmag = _take(alpha, anc[:, t]), _take(amag, anc[:, t])
        if lam == 1:        # the plain recursion: S is not read
            alpha, amag = pa + add, pmag + addmag
        else:
            alpha = (lam * pa + (F(1) - lam) * S[:, None, :]) + add
            amag = (lam * pmag + (F(1) - lam) * Smag[:, None, :]) + addmag
    ll = np.where(alive, ll, -np.inf)
    score = np.where(alive[:, None], S, 0)
    return dict(ll=ll, inc=inc, anc=anc, own=own, gap=gap, degenerate=~alive, score=score, mag=Smag, orders=np.stack(orders, axis=1))


def cpm_score(model, theta, y, U, prior_mean, prior_var, lam=1.0, F=np.float64, forced=None):
    """cpm_model.loglik with the score: the filter of C chains on U [C, T+1, N+1].  Returns dict: cpm_model.loglik's entries and
    score, mag [C, H], orders [C, T, N]."""
    U = np.asarray(U, dtype=np.float64)
    C, T, N = U.shape[0], U.shape[1] - 1, U.shape[2] - 1
    xm1 = F(prior_mean) + np.sqrt(F(prior_var)) * U[:, 0, :N].astype(F)
    r = np.arange(N, dtype=F)[None, :]

    def targets(t):
        u = cm.resampling_uniform(U[:, t + 1, N]).astype(F)[:, None]
        return (r + u) / F(N)
    return _filter(model, theta, np.asarray(y, dtype=np.float64).reshape(-1)[:T], xm1, False, U[:, 1:, :N], targets, lam, F, forced)


def sqmc_score(model, theta, y, N, prior_mean, prior_var, seed, gids, step, lam=1.0, F=np.float64, forced=None, z=None):
    """sqmc_model.loglik with the score.  z: recorded normals [C, T+1, N] (row 0 by particle, the later rows by child).  Returns
    dict: sqmc_model.loglik's entries and score, mag [C, H], orders [C, T, N]."""
    y = np.asarray(y, dtype=np.float64)
    T = y.shape[-1]
    zz, _, delta = sq.normals(N, T, seed, gids, step)
    if z is not None:
        zz = np.asarray(z, dtype=np.float64)
    xm1 = F(prior_mean) + np.sqrt(F(prior_var)) * zz[:, 0].astype(F)
    k = np.arange(N, dtype=F)[None, :]
    res = _filter(model, theta, y, xm1, True, zz[:, 1:], lambda t: (k + delta[:, t + 1].astype(F)[:, None]) / F(N), lam, F, forced)
    res["z"] = zz
    return res


def particle_parents(res):
    """[C, T, N] the parents of `res` as particle indices: row t >= 1 through orders[t]; row 0 is orders[0] itself (the identity
    under CPM, the order of x_{-1} under SQMC)."""
    out = res["orders"].copy()
    out[:, 1:] = np.take_along_axis(res["orders"][:, 1:], res["anc"][:, 1:], axis=2)
    return out


# ---- a whole step of sampler='pmala_sorted' -----------------------------------------------------------------------------------
def _grad4(score):
    g = np.zeros((score.shape[0], 4))
    g[:, :score.shape[1]] = np.asarray(score, dtype=np.float64)
    return g


def estimate(model, theta, y, N, prior_mean, prior_var, seed, chain_offset, ctr, lam, U=None, rho=None):
    """(ll [C], g [C, 4], U' or None, mag [C, 4]) of the launch at counter `ctr`: the correlated filter on U' = rho U +
    sqrt(1 - rho^2) eps when rho is given (rho = 0 reads no U), the SQMC filter otherwise.  The filter seed is CPM's or SQMC's own."""
    theta = np.asarray(theta, dtype=np.float64)
    C = theta.shape[0]
    gids = kd.chain_ids(C, chain_offset)
    T = np.asarray(y).shape[-1]
    if rho is not None:
        Up, _ = cm.propose_u(U, rho, T, N, cm.filter_seed(seed), gids, ctr)
        res = cpm_score(model, theta, y, Up, prior_mean, prior_var, lam=lam)
    else:
        Up = None
        res = sqmc_score(model, theta, y, N, prior_mean, prior_var, sq.filter_seed(seed), gids, ctr, lam=lam)
    return np.asarray(res["ll"], dtype=np.float64), _grad4(res["score"]), Up, _grad4(res["mag"])


def chain_init(model, theta, y, N, prior_mean, prior_var, seed, chain_offset, lam, correlated):
    """The init pass: counter 0 (the correlated filter: rho = 0).  Returns (ll [C], g [C, 4], U or None, mag [C, 4])."""
    return estimate(model, theta, y, N, prior_mean, prior_var, seed, chain_offset, 0, lam, rho=0.0 if correlated else None)


def chain_step(model, prior, hy, theta, ll, grad, U, scale, rho, lam, y, N, prior_mean, prior_var, seed, chain_offset, step):
    """One step (from 0) of C chains of sampler='pmala_sorted': pmala_model's proposal and decision around this file's filters.
    theta [C, P], ll [C], grad [C, 4], U [C, T+1, N+1] (rho given) or None (SQMC): the chains' states.  Returns dict: theta, ll,
    grad, U (the new states), accepted, margin, prop, valid, amb, ll_prop, grad_prop, mag_prop (the magnitude of the
    score's terms), U_prop."""
    theta = np.asarray(theta, dtype=np.float64)
    ctr = pm.step_counter(step)
    useed = pm.update_seed(seed)
    pr = pl.propose(model, theta, grad, scale, useed, chain_offset, ctr, hy)
    prop = np.where(pr.valid[:, None], pr.raw, theta.astype(LD)).astype(np.float64)
    llp, gp, Up, magp = estimate(model, prop, y, N, prior_mean, prior_var, seed, chain_offset, ctr, lam, U=U, rho=rho)
    acc, margin = pl.accept(model, prior, hy, scale, theta, prop, pr.valid, ll, llp, grad, gp, useed, chain_offset, ctr)
    th, l2, g2 = theta.copy(), np.asarray(ll, dtype=np.float64).copy(), np.asarray(grad, dtype=np.float64).copy()
    th[acc], l2[acc], g2[acc] = prop[acc], llp[acc], gp[acc]
    U2 = None
    if rho is not None:
        U2 = np.asarray(U, dtype=np.float64).copy()
        U2[acc] = Up[acc]
    return dict(theta=th, ll=l2, grad=g2, U=U2, accepted=acc, margin=margin, prop=prop, valid=pr.valid, amb=pr.amb, ll_prop=llp,
                grad_prop=gp, mag_prop=magp, U_prop=Up)
