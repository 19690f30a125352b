"""Host restatement of density-tempered SMC over resident PMMH chains (sgmcmc_ssm_amd/tempering.py; csrc/pfg_smc.hip and the
smc kernels of csrc/pfg_chains.hip), NumPy long double, test-only.  Built on pmmh_model.py (propose, in_support, the accept
uniform) and keyed_draws.py (Philox, uniform53).

  logprior_value   the device's log-prior: Prior.logprior of the raw row less its terms in the hyper-parameters alone
  log_q0, log_target   h = (ll + logprior_value) - log q0
  temper           the temperature search, the evidence increment, the CDF and the systematic parents of one stage
  scale            c * sd per moving slot, two passes
  accept           the tempered accept step
  Population       the whole law driven by a `loglik` callable (pmmh_model.run_chains's convention)
  kalman_loglik    a vectorised NumPy Kalman log-likelihood of LGSSM rows (kalman_model.py's forward recursion)
"""
import math

import numpy as np

import pmmh_model as pm
from keyed_draws import LD, philox4x32_10, split_seed, uniform53

TAG_SMC, SEED_SMC = 0x534D0001, 0x534D4353
MOVING = {"svm": (0, 1, 2), "lgssm": (0, 2, 3), "garch": (0, 1, 2, 3)}
BISECTIONS = 60
NO_FINITE, NOT_A_NUMBER, ZERO_STEP, BAD_PHI = 1, 2, 4, 8
RNG_SALT = 0x534D43


def stage_uniform(seed, stage):
    """The resampling uniform of stage `stage`: counter {stage_lo, stage_hi, 0, 0x534D0001} under seed ^ 0x534D4353."""
    s = int(stage)
    r = philox4x32_10((s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF, 0, TAG_SMC),
                      split_seed((int(seed) ^ SEED_SMC) & 0xFFFFFFFFFFFFFFFF))
    return uniform53(r[0], r[1]).reshape(-1)[0]


def hyper_of(model, prior):
    first = lambda v: float(np.asarray(v).reshape(-1)[0])
    return {k: first(v) for k, v in prior.hyperparams.items()}


def _chol_logprior(L, df, scale):
    P = L * L + LD(1e-16)
    return (LD(0.5) * (LD(df) - LD(2.0))) * np.log(P) - (LD(0.5) * P) / LD(scale)


def _coef_logprior(L, x, mean, var_col):
    r = L * (x - LD(mean))
    return LD(-0.5) * ((r * r) / LD(var_col)) + np.log(L)


def logprior_value(model, hy, theta):
    """[C] long double: logprior_value of csrc/pfg_chains.hip, expression for expression."""
    th = np.asarray(theta, dtype=float).astype(LD)
    if model == "svm":
        return (_chol_logprior(th[:, 1], hy["df_Qinv"], hy["scale_Qinv"]) + _chol_logprior(th[:, 2], hy["df_Rinv"], hy["scale_Rinv"])
                + _coef_logprior(th[:, 1], th[:, 0], hy["mean_A"], hy["var_col_A"]))
    if model == "lgssm":
        return (_chol_logprior(th[:, 2], hy["df_Qinv"], hy["scale_Qinv"]) + _chol_logprior(th[:, 3], hy["df_Rinv"], hy["scale_Rinv"])
                + _coef_logprior(th[:, 2], th[:, 0], hy["mean_A"], hy["var_col_A"])
                + _coef_logprior(th[:, 3], th[:, 1], hy["mean_C"], hy["var_col_C"]))
    mu = np.exp(th[:, 0])
    xp = (LD(1.0) + LD(1.0) / (LD(1.0) + np.exp(-th[:, 1]))) / LD(2.0)
    xl = (LD(1.0) + LD(1.0) / (LD(1.0) + np.exp(-th[:, 2]))) / LD(2.0)
    lp = -(LD(hy["shape_mu"]) + LD(1.0)) * th[:, 0] - LD(hy["scale_mu"]) / mu
    lp = lp + ((LD(hy["alpha_phi"]) - 1) * np.log(xp) + (LD(hy["beta_phi"]) - 1) * np.log1p(-xp))
    lp = lp + ((LD(hy["alpha_lambduh"]) - 1) * np.log(xl) + (LD(hy["beta_lambduh"]) - 1) * np.log1p(-xl))
    return lp + _chol_logprior(th[:, 3], hy["df_Rinv"], hy["scale_Rinv"])


def log_q0(model, theta, mean, sd):
    th = np.asarray(theta, dtype=float).astype(LD)
    q = np.zeros(th.shape[0], dtype=LD)
    for j in MOVING[model]:
        m, s = LD(float(mean[j])), LD(float(sd[j]))
        r = th[:, j] - m
        q = q + (-((r * r) / (LD(2.0) * (s * s))) - np.log(s * np.sqrt(LD(2.0) * LD(math.pi))))
    return q


def log_target(model, hy, theta, ll, mean, sd):
    with np.errstate(invalid="ignore"):
        return (np.asarray(ll, dtype=float).astype(LD) + logprior_value(model, hy, theta)) - log_q0(model, theta, mean, sd)


def log_q0_mass(model, mean, sd):
    Phi = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
    P = pm.P_DIM[model]
    out = sum(math.log(Phi(mean[j] / sd[j])) for j in ((3,) if model == "garch" else (P - 2, P - 1)))
    if model != "garch":
        out += math.log(Phi((pm.A_MAX - mean[0]) / sd[0]) - Phi((-pm.A_MAX - mean[0]) / sd[0]))
    return out


def weights(h, hmax, d):
    h = np.asarray(h, dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isneginf(h), LD(0.0), np.exp(LD(d) * (h - hmax)))


def ess(h, hmax, d):
    w = weights(h, hmax, d)
    s1 = w.sum()
    return (s1 * s1) / (w * w).sum()


def systematic_parents(cdf, u):
    """(parent [C], gap [C]): child r takes the smallest j with cdf[j] > ((r + u) / C) W, W = cdf[-1], clamped to C - 1; gap
    is the distance of the child's target to the nearest CDF entry, relative to W."""
    C = cdf.shape[0]
    W = cdf[-1]
    target = ((np.arange(C).astype(LD) + LD(u)) / LD(C)) * W
    j = np.minimum(np.searchsorted(cdf, target, side="right"), C - 1)
    near = np.minimum(np.abs(cdf[j] - target), np.abs(cdf[np.maximum(j - 1, 0)] - target))
    return j.astype(np.int64), (near / W).astype(float)


def temper(h, phi, tau, u):
    """One stage's population arithmetic on h [C] (any float type; evaluated in long double) -> dict(status; and for status 0:
    phi_new, delta, increment, ess, hmax, W, cdf, parent, gap, last)."""
    h = np.asarray(h, dtype=float).astype(LD)
    C = h.shape[0]
    status = 0
    if not (0.0 <= phi < 1.0):
        status |= BAD_PHI
    if np.any(np.isnan(h) | np.isposinf(h)):
        status |= NOT_A_NUMBER
    elif not np.any(np.isfinite(h)):
        status |= NO_FINITE
    if status:
        return dict(status=status)
    hmax = h[np.isfinite(h)].max()
    want, rest = LD(tau) * LD(C), LD(1.0) - LD(phi)
    last = ess(h, hmax, rest) >= want
    delta = rest
    if not last:
        lo, hi = LD(0.0), rest
        for _ in range(BISECTIONS):
            mid = LD(0.5) * (lo + hi)
            if ess(h, hmax, mid) >= want:
                lo = mid
            else:
                hi = mid
        delta = lo
    if delta == 0:
        return dict(status=ZERO_STEP)
    w = weights(h, hmax, delta)
    cdf = np.cumsum(w)
    W = cdf[-1]
    parent, gap = systematic_parents(cdf, u)
    return dict(status=0, phi_new=LD(1.0) if last else LD(phi) + delta, delta=delta, increment=delta * hmax + np.log(W / LD(C)),
                ess=(W * W) / (w * w).sum(), hmax=hmax, W=W, cdf=cdf, parent=parent, gap=gap, last=bool(last))


def scale(theta, model, c, previous):
    """[P] the proposal scale of the (resampled) population theta [C, >= P]: c * sd per moving slot (two passes, divisor C); a
    slot whose sd is 0 or not finite, and every slot that does not move, keeps `previous`."""
    th = np.asarray(theta, dtype=float).astype(LD)
    out = np.array(previous, dtype=float).astype(LD)
    for j in MOVING[model]:
        mean = th[:, j].sum() / LD(th.shape[0])
        d = th[:, j] - mean
        sd = np.sqrt((d * d).sum() / LD(th.shape[0]))
        if np.isfinite(sd) and sd > 0:
            out[j] = LD(c) * sd
    return out


def accept(model, hy, theta, theta_prop, valid, ll_cur, ll_prop, mean, sd, phi, seed, chain_offset, ctr):
    """smc_accept_kernel's decisions -> (accepted [C] bool, margin [C] = |log u - log alpha| (inf where the comparison does
    not decide), log_alpha [C] long double)."""
    theta, theta_prop = np.asarray(theta, dtype=float), np.asarray(theta_prop, dtype=float)
    C = theta.shape[0]
    llp, llc = np.asarray(ll_prop, dtype=float), np.asarray(ll_cur, dtype=float)
    live = np.asarray(valid).astype(bool) & np.isfinite(llp)
    with np.errstate(invalid="ignore"):
        d_post = (llp.astype(LD) + logprior_value(model, hy, theta_prop)) - (llc.astype(LD) + logprior_value(model, hy, theta))
        d_q0 = log_q0(model, theta_prop, mean, sd) - log_q0(model, theta, mean, sd)
        la = LD(phi) * d_post + (LD(1.0) - LD(phi)) * d_q0
        logu = np.log(pm.accept_uniform(C, seed, chain_offset, ctr))
        acc = live & (logu < la)
        margin = np.where(live & ~np.isnan(la), np.abs(logu - la), np.inf)
    return acc, margin.astype(float), la


def initial_population(model, C, seed, mean, sd):
    """tempering.py's draw: q0 by rejection to the support under np.random.default_rng([seed, 0x534D43])."""
    P, slots = pm.P_DIM[model], list(MOVING[model])
    rng = np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, RNG_SALT])
    mean, sd = np.asarray(mean, dtype=float), np.asarray(sd, dtype=float)
    th = np.zeros((C, P))
    if model == "lgssm":
        th[:, 1] = 1.0
    todo = np.arange(C)
    while todo.size:
        th[np.ix_(todo, slots)] = mean[slots] + sd[slots] * rng.standard_normal((todo.size, len(slots)))
        todo = todo[~pm.in_support(model, th[todo])]
    return th


class Population(object):
    """The law of TemperedPopulation on the host: C chains, loglik(theta [C, P] double, ctr) -> [C] estimates (the init pass
    calls it with ctr 0).  Records every stage's temper() result, parents and decisions."""

    def __init__(self, model, hy, loglik, C, seed, mean, sd, tau=0.5, moves=2, c=None, theta0=None, scale0=None, chain_offset=0):
        self.model, self.hy, self.loglik, self.C, self.seed = model, hy, loglik, C, int(seed)
        self.mean, self.sd, self.tau, self.moves = np.asarray(mean, float), np.asarray(sd, float), tau, moves
        self.c = 2.38 / math.sqrt(len(MOVING[model])) if c is None else c
        P = pm.P_DIM[model]
        self.theta = initial_population(model, C, seed, mean, sd) if theta0 is None else np.array(theta0, dtype=float)[:, :P]
        self.ll = np.asarray(loglik(self.theta.copy(), 0), dtype=float).copy()
        self.scale = np.ones(P) if scale0 is None else np.array(scale0, dtype=float)[:P]
        self.phi, self.stage_index, self.ctr, self.log_z, self.offset = 0.0, 0, 1, LD(0.0), chain_offset
        self.records = []

    def stage(self):
        m = self.model
        h = log_target(m, self.hy, self.theta, self.ll, self.mean, self.sd)
        t = temper(h, self.phi, self.tau, stage_uniform(self.seed, self.stage_index))
        if t["status"]:
            raise RuntimeError("status {0}".format(t["status"]))
        self.theta, self.ll = self.theta[t["parent"]], self.ll[t["parent"]]
        self.scale = scale(self.theta, m, self.c, self.scale).astype(float)
        self.phi = float(t["phi_new"])
        useed = pm.update_seed(self.seed)
        t["accepted"], t["margin"], t["scale"] = [], [], self.scale.copy()
        for _ in range(self.moves):
            pr = pm.propose(m, self.theta, self.scale, useed, self.offset, self.ctr)
            prop = np.where(pr.valid[:, None], pr.raw, self.theta.astype(LD)).astype(float)
            llp = np.asarray(self.loglik(prop.copy(), self.ctr), dtype=float)
            acc, margin, _ = accept(m, self.hy, self.theta, prop, pr.valid, self.ll, llp, self.mean, self.sd, self.phi, useed,
                                    self.offset, self.ctr)
            self.theta = np.where(acc[:, None], prop, self.theta)
            self.ll = np.where(acc, llp, self.ll)
            t["accepted"].append(acc)
            t["margin"].append(margin)
            self.ctr += 1
        self.log_z += t["increment"]
        self.stage_index += 1
        self.records.append(t)
        return t

    def run(self, max_stages=1000):
        while self.phi < 1.0 and self.stage_index < max_stages:
            self.stage()
        return self

    def log_evidence(self):
        return float(self.log_z) + log_q0_mass(self.model, self.mean, self.sd)


def kalman_loglik(theta, y, prior_mean=0.0, prior_var=10.0):
    """[C] the exact LGSSM log-likelihood of the rows theta [C, 4] = (A, C, LQinv, LRinv): kalman_model.py's forward
    recursion (information form), vectorised over the rows, double."""
    th = np.asarray(theta, dtype=float)
    A, Cc, Qinv, Rinv = th[:, 0], th[:, 1], th[:, 2] ** 2, th[:, 3] ** 2
    P = np.full(th.shape[0], 1.0 / prior_var)
    m = prior_mean * P
    ll = np.zeros(th.shape[0])
    for yt in np.asarray(y, dtype=float).reshape(-1):
        J = A * Qinv / (A * A * Qinv + P)
        pmn, pP = J * m, Qinv - A * Qinv * J
        y_prec = Rinv - Cc * Rinv * (Cc * Rinv / (Cc * Cc * Rinv + pP))
        r = yt - Cc * (pmn / pP)
        ll = ll + (-0.5 * r * r * y_prec + 0.5 * np.log(np.abs(y_prec)) - 0.5 * math.log(2.0 * math.pi))
        m, P = pmn + Cc * Rinv * yt, pP + Cc * Cc * Rinv
    return ll
