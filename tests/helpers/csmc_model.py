"""Host restatement of particle Gibbs for SVM and LGSSM (NumPy, test-only): the conditional SMC sweep with ancestor sampling
of csrc/pfg_csmc.hip and the parameter draw of pgibbs_update_kernel (csrc/pfg_chains.hip), written from the equations.

  model    chain_filter_model.py states it, with the key and the search
  sweep    t = 0: particles 0 .. N-2 draw x_{-1} and x_0, particle N-1 is x*_0.  t >= 1: a free particle draws its parent from
           the weights of step t-1 (cumsum; the smallest j with cdf[j] > u W, at most N-1), moves and is weighted with
           log g(y_t | x_t); particle N-1 is x*_t and draws its parent from w_i f(x*_t | x_{t-1}^i).  Then k ~ W_{T-1} and the
           lineage of k is the new path.  has_ref = False: every particle is free.  A chain whose weight sum or
           ancestor-weight sum is zero or not finite keeps its path (has_ref = False: a NaN record).
  record   out[0..7] of the new path: [sum_{t>=1} x_{t-1}^2, sum_{t>=1} x_t x_{t-1}, sum_{t>=1} x_t^2, E3, E4, E5, T, 0] with
           LGSSM (E3, E4, E5) = (sum x_t^2, sum y_t x_t, sum y_t^2), SVM (sum y_t^2 exp(-x_t), 0, 0)
  draws    Philox4x32-10 under (seed_lo, seed_hi), counter {gid_lo, step_lo, t ^ (step_hi ^ gid_hi), tag}:
           0x43530000 | i  free particle i: t = 0 normal_pair(r0, r1) -> the normals of x_{-1}, x_0; t >= 1 uniform53(r0, r1) -> its
                           resampling uniform, normal_pair(r2, r3)[0] -> its state normal
           0x43531000      uniform53(r0, r1): the ancestor-sampling uniform of step t;   0x43532000  (t = T) the final index's

Every chain of a call is swept at once (arrays [C, ...]), in the floating type `F` (np.float64: the device's; np.longdouble:
the judge).  `forced` replays recorded indices: the states then follow the recording while `own_*` keeps what this model's
search would have chosen and `gap_*` how far, relative to the weight sum, its target lay from the nearest CDF edge.
"""
import numpy as np

import keyed_draws as kd
from chain_filter_model import EDGE_REL, LD, PM, PV, SEED, THETA, Key, case_theta_y, consts, logw, search  # noqa: F401

TAG_PARTICLE, TAG_ANCESTOR, TAG_FINAL = 0x43530000, 0x43531000, 0x43532000
CSMC_SEED_XOR = 0x43534D43          # ChainEnsemble keys the sweep with seed ^ this (ensemble_settings.py, FILTERS["csmc"].salt)
EDGE_SHARE = 0.01                   # a recorded index may be the neighbour on a CDF edge (EDGE_REL): at most this share of a case


def sweep_seed(seed):
    return (int(seed) ^ CSMC_SEED_XOR) & 0xFFFFFFFFFFFFFFFF


def record(model, path, y, F=np.float64):
    """out[0..7] of paths [C, T] (y [C, T]), summed from the end as the kernel sums them."""
    x = np.asarray(path, dtype=F)
    y = np.asarray(y, dtype=F)
    C, T = x.shape
    s = np.zeros((C, 8), dtype=F)

    def emission(t):
        if model == "svm":
            with np.errstate(over="ignore", invalid="ignore"):
                s[:, 3] += (y[:, t] * y[:, t]) * np.exp(-x[:, t])
        else:
            s[:, 3] += x[:, t] * x[:, t]
            s[:, 4] += y[:, t] * x[:, t]
            s[:, 5] += y[:, t] * y[:, t]
    emission(T - 1)
    for t in range(T - 2, -1, -1):
        s[:, 0] += x[:, t] * x[:, t]
        s[:, 1] += x[:, t + 1] * x[:, t]
        s[:, 2] += x[:, t + 1] * x[:, t + 1]
        emission(t)
    s[:, 6] = T
    return s


def sweep(model, theta, y, path, N, seed, gids, step, prior_mean, prior_var, has_ref=True, F=np.float64, forced=None):
    """One sweep of C chains.  theta [C, P], y [T] or [C, T], path [C, T] (has_ref = False: not read), gids [C] global chain
    ids, `seed` the sweep's own (sweep_seed of the ensemble's).  forced: dict(anc [C, T, N], k [C]) of recorded indices.
    Returns a dict: x [C, T, N], anc [C, T, N] (row 0: -1), w [C, T, N] normalised, ref_anc [C, T], k [C], path [C, T], out
    [C, 8], degenerate [C], own_anc / gap_anc [C, T, N], own_k / gap_k [C]."""
    th = np.asarray(theta, dtype=np.float64)
    C = th.shape[0]
    y = np.asarray(y, dtype=np.float64)
    T = y.shape[-1]
    y = np.broadcast_to(y, (C, T)).astype(F)
    ref = None if not has_ref else np.asarray(path, dtype=np.float64).astype(F)
    c = consts(model, th, F)
    key = Key(gids, seed, step)
    n_free = N - 1 if has_ref else N
    free = np.arange(n_free)
    x = np.zeros((C, T, N), dtype=F)
    lw = np.zeros((C, N), dtype=F)
    w = np.zeros((C, T, N), dtype=F)
    anc = np.full((C, T, N), -1, dtype=np.int64)
    own = np.full((C, T, N), -1, dtype=np.int64)
    gap = np.full((C, T, N), np.inf)
    ref_anc = np.full((C, T), -1, dtype=np.int64)
    alive = np.ones(C, dtype=bool)

    r = key.draw(0, TAG_PARTICLE | free)
    za, zb = kd.normal_pair(r[0], r[1])
    xm1 = F(prior_mean) + np.sqrt(F(prior_var)) * za.astype(F)
    x[:, 0, :n_free] = c["iLQ"] * zb.astype(F) + xm1 * c["A"]
    if has_ref:
        x[:, 0, N - 1] = ref[:, 0]
    lw[:] = logw(model, c, x[:, 0], y[:, 0:1], F)

    def weights(lw_, extra=None):
        l = lw_ if extra is None else lw_ + extra
        with np.errstate(over="ignore", invalid="ignore"):
            m = np.max(np.where(np.isnan(l), -np.inf, l), axis=1, keepdims=True)
            wv = np.exp(l - m)
            cdf = np.cumsum(wv, axis=1)
        tot = cdf[:, -1]
        good = (tot > 0) & np.isfinite(tot)
        return wv, cdf, tot, good

    for t in range(1, T + 1):
        wv, cdf, W, good = weights(lw)
        if has_ref and t < T:
            d = ref[:, t:t + 1] - c["A"] * x[:, t - 1]
            ld = (-F(0.5) * (d * d)) * c["Qinv"]
            _, cdf2, V, good2 = weights(lw, ld)
            good = good & good2
        alive &= good
        safe = np.where(good, W, 1)[:, None]
        w[:, t - 1] = np.where(good[:, None], wv / safe, np.nan)
        cdf = np.where(good[:, None], cdf, np.arange(1, N + 1, dtype=F)[None, :])
        W = np.where(good, W, N)
        if t == T:
            r = key.draw(T, TAG_FINAL)
            own_k, gap_k = search(cdf, kd.uniform53(r[0], r[1])[:, 0].astype(F) * W)
            break
        r = key.draw(t, TAG_PARTICLE | free)
        u = kd.uniform53(r[0], r[1]).astype(F)
        j, g = search(cdf, u * W[:, None])
        own[:, t, :n_free], gap[:, t, :n_free] = j, g
        if has_ref:
            cdf2 = np.where(good[:, None], cdf2, np.arange(1, N + 1, dtype=F)[None, :])
            V = np.where(good, V, N)
            ra = key.draw(t, TAG_ANCESTOR)
            ja, ga = search(cdf2, kd.uniform53(ra[0], ra[1])[:, 0].astype(F) * V)
            own[:, t, N - 1], gap[:, t, N - 1] = ja, ga
        anc[:, t] = own[:, t] if forced is None else np.asarray(forced["anc"])[:, t]
        z, _ = kd.normal_pair(r[2], r[3])
        xp = np.take_along_axis(x[:, t - 1], anc[:, t, :n_free], axis=1)
        x[:, t, :n_free] = c["iLQ"] * z.astype(F) + xp * c["A"]
        if has_ref:
            x[:, t, N - 1] = ref[:, t]
            ref_anc[:, t] = anc[:, t, N - 1]
        lw = logw(model, c, x[:, t], y[:, t:t + 1], F)

    k = own_k if forced is None else np.asarray(forced["k"], dtype=np.int64)
    new = np.zeros((C, T), dtype=F)
    kk = k.copy()
    rows = np.arange(C)
    for t in range(T - 1, -1, -1):
        new[:, t] = x[rows, t, kk]
        if t > 0:
            kk = np.where(alive, anc[rows, t, kk], 0)
    if has_ref:
        new = np.where(alive[:, None], new, ref)
    out = record(model, new, y, F)
    if not has_ref:
        out[~alive] = np.nan
    return dict(x=x, anc=anc, w=w, ref_anc=ref_anc, k=k, path=new, out=out, degenerate=~alive, own_anc=own, gap_anc=gap,
                own_k=own_k, gap_k=gap_k)


def index_mismatches(rec_anc, rec_k, res):
    """Recorded indices (anc [C, T, N] with row 0 ignored, k [C]) against what `res` (a sweep forced on them) would have
    searched: (number outside the rule, number that used the edge tolerance, number of indices).  The rule: the same index,
    or its neighbour when the target lies within EDGE_REL of a CDF edge."""
    ok_rows = ~res["degenerate"]
    rec_anc = np.asarray(rec_anc, dtype=np.int64)[ok_rows][:, 1:]
    own, gap = res["own_anc"][ok_rows][:, 1:], res["gap_anc"][ok_rows][:, 1:]
    rk, ok, gk = np.asarray(rec_k, dtype=np.int64)[ok_rows], res["own_k"][ok_rows], res["gap_k"][ok_rows]
    diff = np.concatenate([(rec_anc - own).reshape(-1), rk - ok])
    gaps = np.concatenate([gap.reshape(-1), gk])
    edge = (np.abs(diff) == 1) & (gaps <= EDGE_REL)
    wrong = (diff != 0) & ~edge
    return int(wrong.sum()), int(edge.sum()), int(diff.size)


# ---- the parameter draw: pgibbs_update_kernel (pfg_chains.hip) -----------------------------------------------------------------
def svm_posterior(stats, hy):
    """The SVM conditional's parameters from a record [C, 8]: (df_Q, scale_Q, mean_A, Spp, df_R, scale_R) with
    Qinv ~ scale_Q chi2(df_Q), A | Q ~ N(mean_A, 1 / ((Qinv + 1e-9) Spp)), Rinv ~ scale_R chi2(df_R)."""
    hy = kd._hy(hy)
    s = np.asarray(stats, dtype=np.float64)
    T = s[:, 6].astype(LD)
    dfq, scq, Spp, Scp, kq = kd.conjugate(hy["df_Qinv"], hy["scale_Qinv"], hy["mean_A"], hy["var_col_A"], s[:, 0], s[:, 1], s[:, 2],
                                        T - 1)
    dfr = LD(hy["df_Rinv"]) + T
    scr = LD(1) / (LD(1) / LD(hy["scale_Rinv"]) + s[:, 3].astype(LD))
    return dfq, scq, Scp / Spp, Spp, dfr, scr, kq


def pgibbs_expected(model, stats, hy, seed, chain_offset, step):
    """pgibbs_update_kernel of C chains: (Expected, tie [C]).  LGSSM: gibbs_update_kernel's mirror.  SVM: theta (A, LQinv, LRinv)."""
    if model == "lgssm":
        exp, tie, _, _ = kd.gibbs_expected(stats, hy, seed, chain_offset, step)
        return exp, tie
    s = np.asarray(stats, dtype=np.float64)
    C = s.shape[0]
    keys = kd.ChainKeys(kd.chain_ids(C, chain_offset), seed, step)
    dfq, scq, mean, Spp, dfr, scr, kq = svm_posterior(s, hy)
    gq, tq, aq = kd.gamma_draw(keys, 0, LD(0.5) * dfq)
    gr, tr, ar = kd.gamma_draw(keys, 1, LD(0.5) * dfr)
    aq, ar = aq + kq, ar + 1
    Qinv, Rinv = scq * (2 * gq), scr * (2 * gr)
    ra = keys.draw(2, 0)
    zA, _ = kd.normal_pair(ra[0], ra[1])
    noise = np.sqrt((LD(1) / (Qinv + LD(1e-9))) * (LD(1) / Spp)) * zA
    A = mean + noise
    LQ, LR = np.sqrt(Qinv), np.sqrt(Rinv)
    tol = np.column_stack([np.abs(mean) + np.abs(noise) * aq, np.abs(LQ) * aq, np.abs(LR) * ar]) * (kd.TOL_ULPS * kd.ULP)
    th = np.column_stack([A, LQ, LR])
    new, other, amb = th.copy(), th.copy(), np.zeros(th.shape, bool)
    new[:, 0], other[:, 0], amb[:, 0] = kd._clip_A(A, tol[:, 0])
    return kd.Expected(new, tol, other, amb), tq | tr


# ---- exact smoothing moments of the scalar LGSSM (the invariance tests' reference) ------------------------------------------
def lgssm_smoother(theta, y, prior_mean, prior_var):
    """The joint smoothing law of x_0 .. x_{T-1} given y: mean [T] and covariance [T, T], from the joint Gaussian of the model
    (x_{-1} ~ N(prior_mean, prior_var) integrated out) -- linear algebra, no recursion to get wrong."""
    A, Cc, LQ, LR = (float(v) for v in theta[:4])
    Q, R = 1.0 / (LQ * LQ), 1.0 / (LR * LR)
    y = np.asarray(y, dtype=np.float64)
    T = len(y)
    # precision of (x_0 .. x_{T-1}): x_0 ~ N(A prior_mean, A^2 prior_var + Q), then the AR(1) transitions
    J = np.zeros((T, T))
    h = np.zeros(T)
    v0 = A * A * prior_var + Q
    J[0, 0] += 1.0 / v0
    h[0] += A * prior_mean / v0
    for t in range(1, T):
        J[t, t] += 1.0 / Q
        J[t - 1, t - 1] += A * A / Q
        J[t, t - 1] -= A / Q
        J[t - 1, t] -= A / Q
    J[np.arange(T), np.arange(T)] += Cc * Cc / R
    h += Cc * y / R
    cov = np.linalg.inv(J)
    return cov @ h, cov


def moment_bounds(mean, cov, n, sigmas=5.0):
    """For n independent draws of N(mean, cov): the exact values of E x_t [T] and E x_t x_{t-1} [T-1] and `sigmas` standard errors
    of their sample averages, from the second moments and Isserlis' formula for the fourth:
      Var(x_t) = S_tt;  Var(x_t x_s) = S_tt S_ss + S_ts^2 + m_t^2 S_ss + m_s^2 S_tt + 2 m_t m_s S_ts."""
    m, S = np.asarray(mean), np.asarray(cov)
    d = np.diag(S)
    e1, se1 = m, np.sqrt(d / n)
    mt, ms, Stt, Sss, Sts = m[1:], m[:-1], d[1:], d[:-1], np.diag(S, -1)
    e2 = mt * ms + Sts
    var2 = Stt * Sss + Sts ** 2 + mt ** 2 * Sss + ms ** 2 * Stt + 2 * mt * ms * Sts
    return e1, sigmas * se1, e2, sigmas * np.sqrt(var2 / n)


def sample_smoother(mean, cov, n, rs):
    return mean[None, :] + rs.standard_normal((n, len(mean))) @ np.linalg.cholesky(cov).T


def sample_prior_paths(theta, T, n, prior_mean, prior_var, rs):
    """n paths x_0 .. x_{T-1} of the model's own prior: over-dispersed starts for the invariance tests."""
    A, LQ = float(theta[0]), float(theta[2] if len(theta) > 3 else theta[1])
    x = prior_mean + np.sqrt(prior_var) * rs.standard_normal(n)
    out = np.zeros((n, T))
    for t in range(T):
        x = A * x + rs.standard_normal(n) / LQ
        out[:, t] = x
    return out


# ---- the cases the CPU and the device tests share ---------------------------------------------------------------------------
# the (N, T, B) cases of the device replay (tests/test_gpu_csmc.py): a partial wave, both sides of the one-wave switch, a ragged
# last slot and the maximum; T = 1 (no resampling at all), 2, 3 and 37, where the parents stay in LDS up to N = 128 (T N <=
# 8192) and are read back from the scratch above it
CASES = [(2, 1, 1), (2, 37, 3), (5, 2, 70), (64, 3, 3), (65, 37, 1), (128, 37, 70), (129, 2, 3), (257, 37, 3), (1000, 3, 70),
         (1024, 37, 1), (1024, 1, 3)]


def case_inputs(model, N, T, B, seed=SEED):
    """theta [B, P], y [T], reference paths [B, T] of a case: deterministic, moderate."""
    th, y, rs = case_theta_y(model, N, T, B, seed)
    return th, y, sample_prior_paths(THETA[model], T, B, PM, PV, rs)
