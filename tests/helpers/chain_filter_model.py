"""What the host restatements of the two filters that run one workgroup per chain share (NumPy, test-only): csmc_model.py (the
conditional SMC sweep of csrc/pfg_csmc.hip) and cpm_model.py (the sorted, correlated filter of csrc/pfg_cpm.hip).

  model    x_{-1} ~ N(prior_mean, prior_var);  x_t = A x_{t-1} + z / LQinv;  SVM: y_t ~ N(0, R exp(x_t));  LGSSM: y_t ~ N(C x_t, R);
           Qinv = LQinv^2 + 1e-16, Rinv = LRinv^2 + 1e-16, R = 1 / Rinv
  key      Philox4x32-10 under (seed_lo, seed_hi), counter {gid_lo, step_lo, index ^ (step_hi ^ gid_hi), tag}: the chain key of
           keyed_draws.ChainKeys with a time step (sweep) or a row of U (filter) XORed into the third word
  search   the smallest j with cdf[j] > target, at most N-1
"""
import numpy as np

import keyed_draws as kd

LD = np.longdouble
LOG_2PI = LD("1.8378770664093454835606594728112353")
EDGE_REL = 1e-12                    # a search whose target lies this close, relative to the weight sum, to a CDF entry is on an edge


class Key(object):
    """The keys of the chains with global ids `gids` at counter `step`: draw(index, tags) -> Philox words [4][C, len(tags)]."""

    def __init__(self, gids, seed, step):
        self.keys = kd.ChainKeys(gids, seed, step)

    def draw(self, index, tags):
        k = self.keys
        tags = np.atleast_1d(np.asarray(tags, dtype=np.uint64))[None, :]
        return kd.philox4x32_10((k.gid[:, None], k.c1[:, None], np.uint64(int(index)) ^ k.c2[:, None], tags), k.k)


def consts(model, th, F):
    th = np.asarray(th, dtype=F)
    if model == "svm":
        A, Cc, LQ, LR = th[:, 0], np.ones(len(th), dtype=F), th[:, 1], th[:, 2]
    else:
        A, Cc, LQ, LR = th[:, 0], th[:, 1], th[:, 2], th[:, 3]
    one = F(1)
    return dict(A=A[:, None], C=Cc[:, None], iLQ=(one / LQ)[:, None], Qinv=(LQ * LQ + F(1e-16))[:, None],
                Rinv=(LR * LR + F(1e-16))[:, None], logLR=np.log(LR)[:, None], c0=F(-0.5) * F(LOG_2PI))


def logw(model, c, x, y, F):
    """log g(y | x): svm/kernels.py:56-62, lgssm/kernels.py:58-62 in the kernel's order of operations."""
    half = F(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        if model == "svm":
            return ((c["c0"] + ((-half * (y * y)) * np.exp(-x)) * c["Rinv"]) + c["logLR"]) + (-half * x)
        d = y - c["C"] * x
        return (c["c0"] + (-half * (d * d)) * c["Rinv"]) + c["logLR"]


def search(cdf, target):
    """smallest j with cdf[j] > target, at most N-1, per row; and the relative distance of target to the nearest edge.
    cdf [C, N]; target [C] or [C, M]."""
    N = cdf.shape[-1]
    one = target.ndim == 1
    tg = target[:, None] if one else target
    if N <= 32:
        j = (cdf[:, None, :] <= tg[:, :, None]).sum(axis=-1)
    else:
        j = np.stack([np.searchsorted(cdf[c], tg[c], side="right") for c in range(cdf.shape[0])])
    below = np.take_along_axis(cdf, np.clip(j - 1, 0, N - 1), axis=1)
    above = np.take_along_axis(cdf, np.clip(j, 0, N - 1), axis=1)
    gap = np.minimum(np.abs(tg - below), np.abs(above - tg)) / cdf[:, -1:]
    j = np.minimum(j, N - 1)
    return (j[:, 0], gap[:, 0]) if one else (j, gap)


# ---- the cases the CPU and the device tests share ---------------------------------------------------------------------------
THETA = {"svm": [0.9, 2.0, 1.2], "lgssm": [0.9, 1.0, 2.0, 1.2]}
PM, PV = 0.0, 10.0
SEED = 20261019


def case_theta_y(model, N, T, B, seed=SEED):
    """theta [B, P] and y [T] of a case -- deterministic, moderate -- and the generator they came from, for what the case
    draws beyond them."""
    rs = np.random.RandomState(seed % (2 ** 31) + 7 * N + 131 * T + B)
    th = np.tile(THETA[model], (B, 1)) * rs.uniform(0.95, 1.05, size=(B, len(THETA[model])))
    if model == "lgssm":
        th[:, 1] = 1.0
    x = rs.standard_normal() * np.sqrt(PV)
    xs = np.zeros(T)
    for t in range(T):
        x = THETA[model][0] * x + rs.standard_normal() / (THETA[model][2] if model == "lgssm" else THETA[model][1])
        xs[t] = x
    y = np.exp(xs / 2) * rs.standard_normal(T) / THETA[model][-1] if model == "svm" else xs + rs.standard_normal(T) / THETA[model][-1]
    return th, y, rs
