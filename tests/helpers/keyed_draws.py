"""Host mirror of the counter-keyed Philox4x32-10 draws outside the particle filters (NumPy, test-only).

Every draw of the resident chain updates, the window samplers and the device-generator FFBS is a pure function of
(seed, chain id, step counter, tag), so the host regenerates each one exactly and evaluates the formula the kernel
documents in np.longdouble.  Each function names the kernel or device helper it mirrors (files relative to
stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd/csrc).

  philox4x32_10         pfg_math.hpp philox4x32_10 (Random123 Philox4x32-10)
  sgld / sghmc / sgrld  pfg_chains.hip sgld_update_kernel, chain_normals: ctr {gid_lo, step_lo, step_hi ^ gid_hi, 0x5A11 | 0x5A12},
                        key (seed_lo, seed_hi); normals A, C, Q, R (SVM A, Q, R; GARCH log_mu, logit_phi, logit_lambduh, LR)
  gibbs                 pfg_chains.hip ChainKey: tag 0x61B50000 | var << 8 | attempt, the boost draw var | 0x80
  windows, one          pfg_windows.hip sample_windows_kernel: ctr {chain_lo, chain_hi, ctr_lo, ctr_hi}, key (seed_lo ^ 0x57494E44, seed_hi)
  windows, multi        pfg_windows.hip sample_windows_multi_kernel: ctr {gid_lo, gid_hi ^ ctr_hi, ctr_lo, 0x53000000 | j or 0x57000000 | w}
  lane generator        pfg_math.hpp: lane_rng_init then jsf32, 8 warm-up rounds
"""
import numpy as np

import lgssm_chain_rules as rules

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not wider than double here: the mirror needs 64-bit mantissas"

U32 = np.uint32
MASK32 = 0xFFFFFFFF
PI = LD("3.14159265358979323846264338327950288")
ULP = 2.0 ** -52
TOL_ULPS = 16.0


# ---- Philox4x32-10: pfg_math.hpp philox4x32_10 ---------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (or scalars), key: 2; returns 4 uint32 arrays, broadcast together."""
    x, y, z, w = (np.asarray(c, dtype=np.uint64) & MASK32 for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & MASK32 for k in key)
    x, y, z, w, k0, k1 = np.broadcast_arrays(x, y, z, w, k0, k1)
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    m, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * x, M1 * z
        x, y, z, w = (p1 >> s32) ^ y ^ k0, p1 & m, (p0 >> s32) ^ w ^ k1, p0 & m
        k0, k1 = (k0 + W0) & m, (k1 + W1) & m
    return tuple(v.astype(U32) for v in (x, y, z, w))


def _lo(v):
    return np.asarray([int(t) & MASK32 for t in np.atleast_1d(v)], dtype=np.uint64)


def _hi(v):
    return np.asarray([(int(t) >> 32) & MASK32 for t in np.atleast_1d(v)], dtype=np.uint64)


def split_seed(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & MASK32, seed >> 32


def chain_ids(C, chain_offset):
    return [int(chain_offset) + b for b in range(C)]


# ---- transforms -----------------------------------------------------------------------------------------------------
def normal_pair(a, b):
    """Math<double, false>::normal_pair (pfg_math.hpp): u1 = (a + 0.5) 2^-32, angle b 2^-31 half-turns;
    evaluated in long double."""
    u1 = (np.asarray(a, dtype=LD) + LD(0.5)) / LD(4294967296.0)
    r = np.sqrt(LD(-2.0) * np.log(u1))
    ang = PI * (np.asarray(b, dtype=LD) / LD(2147483648.0))
    return r * np.cos(ang), r * np.sin(ang)


def normal_pair_f32(a, b):
    """Math<double, true>::normal_pair_f32 (pfg_math.hpp) with its inputs quantised as the kernel does --
    (float)a + 0.5f and (b >> 8) / 2^24 in float32 -- and the transcendentals exact (long double): the kernel's
    v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32 units differ from this by their own error only."""
    a = np.asarray(a, dtype=U32)
    b = np.asarray(b, dtype=U32)
    u1 = (a.astype(np.float32) + np.float32(0.5)) * np.float32(2.3283064365386963e-10)
    u2 = (b >> U32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    r = np.sqrt(LD(-2.0) * np.log(u1.astype(LD)))
    ang = LD(2.0) * PI * u2.astype(LD)
    return r * np.cos(ang), r * np.sin(ang)


def uniform53(a, b):
    """uniform53 (pfg_chains.hip): ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53, in (0, 1); exact."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)).astype(LD) * LD(67108864.0) + (b >> np.uint64(6)).astype(LD) + LD(0.5)) / LD(2.0 ** 53)


def umul64hi(bits, rng):
    """__umul64hi(bits, range): the high 64 bits of the 128-bit product, with Python ints."""
    bits = np.atleast_1d(bits)
    rng = np.broadcast_to(np.asarray(rng), bits.shape)
    return np.array([(int(x) * int(r)) >> 64 for x, r in zip(bits.tolist(), rng.tolist())], dtype=np.int64)


def bits64(r):
    """((uint64_t)r.x << 32) | r.y of a Philox output."""
    return [(int(x) << 32) | int(y) for x, y in zip(np.atleast_1d(r[0]).tolist(), np.atleast_1d(r[1]).tolist())]


# ---- the four normals of a resident chain update: sgld_update_kernel, chain_normals (pfg_chains.hip) --------------------------
def chain_normals(C, seed, chain_offset, step):
    """[C, 4] long-double normals in draw order (A, C, Q, R; SVM A, Q, R; GARCH its four variables)."""
    gid = chain_ids(C, chain_offset)
    s = int(step or 0)
    c1 = s & MASK32
    c2 = (_hi([s]) ^ _hi(gid))
    k0, k1 = split_seed(seed)
    r0 = philox4x32_10((_lo(gid), c1, c2, 0x5A11), (k0, k1))
    r1 = philox4x32_10((_lo(gid), c1, c2, 0x5A12), (k0, k1))
    z0, z1 = normal_pair(r0[0], r0[1])
    z2, z3 = normal_pair(r1[0], r1[1])
    return np.column_stack([z0, z1, z2, z3])


# ---- SGLD / SGHMC: sgld_update_kernel (pfg_chains.hip) ---------------------------------------------------------------------------
SLOTS = {"svm": ("A", "LQ", "LR"), "lgssm": ("A", "C", "LQ", "LR"), "garch": ("log_mu", "logit_phi", "logit_lambduh", "LR")}
# score column of each theta slot (pfgrad.h: SVM [LR, LQ, A], LGSSM [LR, LQ, C, A], GARCH [LR, log_mu, phi, lambduh])
SCORE_COL = {"svm": (2, 1, 0), "lgssm": (3, 2, 1, 0), "garch": (1, 2, 3, 0)}


def _hy(hy):
    """pfg_prior_hyper (ctypes) or dict -> dict of floats."""
    if isinstance(hy, dict):
        return dict(hy)
    return {n: float(getattr(hy, n)) for n, _ in hy._fields_}


def prior_gradient(model, theta, hy):
    """grad log-prior at theta [C, P] (long double), theta order, and the sum of the absolute values of its terms
    (the scale of its rounding).  SVM / LGSSM: lgssm_chain_rules.grad_logprior (SVM has no C); GARCH: garch_var.py:152-165
    as sgld_update_kernel states it."""
    th = np.asarray(theta, dtype=LD)
    if model in ("svm", "lgssm"):
        full = th if model == "lgssm" else np.column_stack([th[:, 0], np.ones(len(th), dtype=LD), th[:, 1], th[:, 2]])
        g = rules.grad_logprior(full, hy)
        A, C, LQ, LR = (full[:, j] for j in range(4))
        Qinv, Rinv = LQ * LQ + 1e-16, LR * LR + 1e-16
        mag = np.column_stack([np.abs(Qinv * (A - hy["mean_A"])) / hy["var_col_A"] + np.abs(Qinv * hy["mean_A"]) / hy["var_col_A"],
                               np.abs(Rinv * (C - hy["mean_C"])) / hy["var_col_C"],
                               np.abs((hy["df_Qinv"] - 2.0) / LQ) + np.abs(LQ / hy["scale_Qinv"]),
                               np.abs((hy["df_Rinv"] - 2.0) / LR) + np.abs(LR / hy["scale_Rinv"])])
        keep = [0, 1, 2, 3] if model == "lgssm" else [0, 2, 3]
        return g[:, keep], mag[:, keep]
    lmu, lphi, llam, LR = (th[:, j] for j in range(4))
    mu, phi, lam = np.exp(lmu), 1 / (1 + np.exp(-lphi)), 1 / (1 + np.exp(-llam))
    a_p, b_p = (hy["alpha_phi"] - 1.0) / (1 + phi), (hy["beta_phi"] - 1.0) / (1 - phi)
    a_l, b_l = (hy["alpha_lambduh"] - 1.0) / (1 + lam), (hy["beta_lambduh"] - 1.0) / (1 - lam)
    g = np.column_stack([-hy["shape_mu"] - 1.0 + hy["scale_mu"] / mu,
                         (a_p - b_p) * phi * (1 - phi), (a_l - b_l) * lam * (1 - lam),
                         (hy["df_Rinv"] - 2.0) / LR - LR / hy["scale_Rinv"]])
    mag = np.column_stack([abs(hy["shape_mu"]) + 1.0 + np.abs(hy["scale_mu"] / mu),
                           (np.abs(a_p) + np.abs(b_p)) * phi, (np.abs(a_l) + np.abs(b_l)) * lam,
                           np.abs((hy["df_Rinv"] - 2.0) / LR) + np.abs(LR / hy["scale_Rinv"])])
    return g, mag


def _reflect(L, tol):
    """reflect_chol (pfg_chains.hip) with the other branch where L lies within tol of 0."""
    taken = np.where(L < 0, np.sqrt(L * L + LD(1e-16)), L)
    other = np.where(L < 0, L, np.sqrt(L * L + LD(1e-16)))
    return taken, other, np.abs(L) <= tol


def _clip_A(A, tol):
    """|A| > 0.9999 -> A * (0.9999 / |A|) (clip_ar, pfg_chains.hip), with the other branch where |A|
    lies within tol of 0.9999."""
    aa = np.abs(A)
    clipped = A * (LD(0.9999) / aa)
    taken = np.where(aa > LD(0.9999), clipped, A)
    other = np.where(aa > LD(0.9999), A, clipped)
    return taken, other, np.abs(aa - LD(0.9999)) <= tol


class Expected(object):
    """What a kernel must have written: theta [C, P] (and momentum), per-component tolerances, and for components
    near a projection's threshold the other branch's value (`other`, where `amb` is True)."""

    def __init__(self, theta, tol, other=None, amb=None, momentum=None, mom_tol=None):
        self.theta, self.tol = theta, tol
        self.other = theta.copy() if other is None else other
        self.amb = np.zeros(theta.shape, bool) if amb is None else amb
        self.momentum, self.mom_tol = momentum, mom_tol

    def mismatch(self, got, cols=None):
        """[C, P] bool: components outside their tolerance on both accepted branches."""
        got = np.asarray(got, dtype=LD)[:, :self.theta.shape[1]]
        bad = np.abs(got - self.theta) > self.tol
        bad &= ~(self.amb & (np.abs(got - self.other) <= self.tol))
        bad |= np.isnan(got) != np.isnan(self.theta.astype(float))
        if cols is not None:
            bad = bad[:, cols]
        return bad


def sgld_expected(model, theta, ghat, hy, eps, T, seed, chain_offset, step, momentum=None, alpha=1.0):
    """One sgld_update_kernel step (momentum None: SGLD; else SGHMC with friction alpha) of C chains: theta [C, P] and
    ghat [C, 8] as the kernel reads them (double), evaluated in long double."""
    hy = _hy(hy)
    th = np.asarray(theta, dtype=float)[:, :len(SLOTS[model])].astype(LD)
    C, P = th.shape
    g = np.asarray(ghat, dtype=float)[:, list(SCORE_COL[model])].astype(LD)
    gp, gmag = prior_gradient(model, th, hy)
    z = chain_normals(C, seed, chain_offset, step)
    if model == "svm":
        z = z[:, :3]
    eps_l, T_l, a_l = LD(eps), LD(T), LD(alpha)
    nsd = np.sqrt(LD(1) / T_l) * np.sqrt(LD(2) * eps_l) * (np.sqrt(a_l) if momentum is not None else LD(1))
    drift = eps_l * ((gp + g) / T_l)
    noise = nsd * z
    mag = np.abs(th) + eps_l * (gmag + np.abs(g)) / T_l + np.abs(noise)
    d = drift + noise
    mom = None
    if momentum is not None:
        m0 = np.asarray(momentum, dtype=float)[:, :P].astype(LD)
        mom = (LD(1) - a_l) * m0 + d
        mag = mag + np.abs((LD(1) - a_l) * m0)
        d = mom
    tol = TOL_ULPS * ULP * mag
    pre = th + d
    new, other, amb = pre.copy(), pre.copy(), np.zeros(pre.shape, bool)
    if model in ("svm", "lgssm"):
        new[:, 0], other[:, 0], amb[:, 0] = _clip_A(pre[:, 0], tol[:, 0])
        if model == "lgssm":
            new[:, 1] = other[:, 1] = 1.0
        for j in (P - 2, P - 1):
            new[:, j], other[:, j], amb[:, j] = _reflect(pre[:, j], tol[:, j])
    else:
        new[:, 3], other[:, 3], amb[:, 3] = _reflect(pre[:, 3], tol[:, 3])
    mom_tol = None if mom is None else TOL_ULPS * ULP * mag
    return Expected(new, tol, other, amb, mom, mom_tol)


def sgrld_expected(theta, ghat, hy, eps, T, seed, chain_offset, step):
    """One sgrld_update_kernel step (pfg_chains.hip) of C LGSSM chains, in long double, by the rules of
    lgssm_chain_rules: theta' = project(theta + sgrld_drift + sqrt(2 eps) sqrt(1 / T) noise_factor z)."""
    hy = _hy(hy)
    th = np.asarray(theta, dtype=float)[:, :4].astype(LD)
    gh = np.asarray(ghat, dtype=float)[:, :4].astype(LD)
    C = th.shape[0]
    eps_l, T_l = LD(eps), LD(T)
    z = chain_normals(C, seed, chain_offset, step)
    drift = rules.sgrld_drift(th, gh, hy, eps_l, T_l)
    noise = np.sqrt(LD(2) * eps_l) * np.sqrt(LD(1) / T_l) * rules.sgrld_noise_factor(th) * z
    _, gmag = prior_gradient("lgssm", th, hy)
    gabs = gmag + np.abs(gh[:, [rules.SCORE_COL[v] for v in rules.THETA]])
    dmag = eps_l * (rules.sgrld_precondition(th, gabs, LD(1) / T_l) + np.abs(rules.sgrld_correction(th, LD(1) / T_l)))
    mag = np.abs(th) + np.abs(dmag) + np.abs(noise)
    tol = TOL_ULPS * ULP * mag
    pre = th + drift + noise
    new, other, amb = pre.copy(), pre.copy(), np.zeros(pre.shape, bool)
    new[:, 0], other[:, 0], amb[:, 0] = _clip_A(pre[:, 0], tol[:, 0])
    new[:, 1] = other[:, 1] = 1.0
    for j in (2, 3):
        new[:, j], other[:, j], amb[:, j] = _reflect(pre[:, j], tol[:, j])
    return Expected(new, tol, other, amb)


# ---- Gibbs: gibbs_update_kernel (pfg_chains.hip) ----------------------------------------------------------------------------------
K_MAX_ROUNDS = 64
TIE_REL = 1e-12


class ChainKeys(object):
    """ChainKey of C chains (pfg_chains.hip, as gibbs_update_kernel keys it): draw(var, attempt) = Philox of
    {gid_lo, step_lo, step_hi ^ gid_hi, 0x61B50000 | var << 8 | attempt} under (seed_lo, seed_hi)."""

    def __init__(self, gids, seed, step):
        s = int(step or 0)
        self.gid = _lo(gids)
        self.c1 = np.full(len(self.gid), s & MASK32, dtype=np.uint64)
        self.c2 = _hi([s]) ^ _hi(gids)
        self.k = split_seed(seed)

    def subset(self, idx):
        o = ChainKeys.__new__(ChainKeys)
        o.gid, o.c1, o.c2, o.k = self.gid[idx], self.c1[idx], self.c2[idx], self.k
        return o

    def draw(self, var, attempt):
        return philox4x32_10((self.gid, self.c1, self.c2, 0x61B50000 | (int(var) << 8) | int(attempt)), self.k)


def gamma_draw(keys, var, shape):
    """gamma_draw (pfg_chains.hip) of each chain: Marsaglia-Tsang on shape (shape + 1 below 1, then times
    U^(1 / shape)), at most 64 keyed rounds, in long double.  Returns (x, tie, amp): `tie` marks a chain whose
    acceptance test differed by less than TIE_REL between its two sides in some round (double may decide it the other
    way), `amp` the relative-error amplification of the boost, 1 + |log(U) / shape|."""
    shape = np.broadcast_to(np.asarray(shape, dtype=LD), keys.gid.shape).copy()
    n = len(shape)
    x = np.full(n, np.nan, dtype=LD)
    tie = np.zeros(n, bool)
    amp = np.ones(n, dtype=LD)
    ok = (shape > 0) & np.isfinite(shape)
    boost = ok & (shape < 1)
    a = np.where(boost, shape + 1, shape)
    d = a - LD(1) / LD(3)
    c = LD(1) / np.sqrt(LD(9) * np.where(ok, d, 1))
    live = ok.copy()
    for k in range(K_MAX_ROUNDS):
        if not live.any():
            break
        r = keys.draw(var, k)
        z, _ = normal_pair(r[0], r[1])
        t = 1 + c * z
        pos = live & (t > 0)
        v = t * t * t
        u = uniform53(r[2], r[3])
        lhs = np.log(u)
        rhs = LD(0.5) * z * z + d - d * v + d * np.log(np.where(pos, v, 1))
        close = pos & (np.abs(lhs - rhs) <= TIE_REL * np.maximum(np.abs(lhs), np.abs(rhs)))
        tie |= close
        acc = pos & (lhs < rhs)
        x[acc] = (d * v)[acc]
        live &= ~acc
    done = ok & ~np.isnan(x)
    bst = done & boost
    if bst.any():
        s = keys.subset(np.nonzero(bst)[0]).draw(int(var) | 0x80, 0)
        e = np.log(uniform53(s[0], s[1])) / shape[bst]
        x[bst] = x[bst] * np.exp(e)
        amp[bst] = 1 + np.abs(e)
    return x, tie, amp


def conjugate(df0, scale0, mean, var_col, spp, scp, scc, count):
    """(df, scale, Spp, Scp, kappa) of one Wishart block: conjugate (pfg_chains.hip) in long double.  kappa is the
    condition of the scale's denominator 1 / scale0 + Scc - Scp^2 / Spp, the sum of its terms' magnitudes over its
    value: the double evaluation's relative error is kappa ulps, large when the path explains the series closely."""
    spp, scp, scc, count = (np.asarray(v, dtype=LD) for v in (spp, scp, scc, count))
    mean_prec = LD(mean) / LD(var_col)
    Spp = LD(1) / LD(var_col) + spp
    Scp = mean_prec + scp
    Scc = LD(mean) * mean_prec + scc
    den = LD(1) / LD(scale0) + (Scc - Scp * Scp / Spp)
    kappa = (np.abs(LD(1) / LD(scale0)) + np.abs(Scc) + Scp * Scp / np.abs(Spp)) / np.abs(den)
    return LD(df0) + count, LD(1) / den, Spp, Scp, kappa


def gibbs_expected(stats, hy, seed, chain_offset, step):
    """gibbs_update_kernel (pfg_chains.hip) of C chains with statistics stats [C, 8]: long double draws of
    Qinv, Rinv and A | Q by the keyed attempts the kernel makes.  Returns (Expected, tie [C], shape_Q, shape_R)."""
    hy = _hy(hy)
    s = np.asarray(stats, dtype=float)
    C = s.shape[0]
    keys = ChainKeys(chain_ids(C, chain_offset), seed, step)
    T = s[:, 6].astype(LD)
    dfq, scq, Spp, Scp, kq = conjugate(hy["df_Qinv"], hy["scale_Qinv"], hy["mean_A"], hy["var_col_A"], s[:, 0], s[:, 1],
                                   s[:, 2], T - 1)
    dfr, scr, _, _, kr = conjugate(hy["df_Rinv"], hy["scale_Rinv"], hy["mean_C"], hy["var_col_C"], s[:, 3], s[:, 4], s[:, 5], T)
    shq, shr = LD(0.5) * dfq, LD(0.5) * dfr
    gq, tq, aq = gamma_draw(keys, 0, shq)
    gr, tr, ar = gamma_draw(keys, 1, shr)
    aq, ar = aq + kq, ar + kr          # relative-error scale of Qinv, Rinv: the boost's and the scale's
    Qinv, Rinv = scq * (2 * gq), scr * (2 * gr)
    ra = keys.draw(2, 0)
    zA, _ = normal_pair(ra[0], ra[1])
    mean = Scp / Spp
    noise = np.sqrt((LD(1) / (Qinv + LD(1e-9))) * (LD(1) / Spp)) * zA
    A = mean + noise
    LQ, LR = np.sqrt(Qinv), np.sqrt(Rinv)
    tol = np.column_stack([np.abs(mean) + np.abs(noise) * aq, np.zeros(C, dtype=LD), np.abs(LQ) * aq,
                           np.abs(LR) * ar]) * (TOL_ULPS * ULP)
    th = np.column_stack([A, np.ones(C, dtype=LD), LQ, LR])
    new, other, amb = th.copy(), th.copy(), np.zeros(th.shape, bool)
    new[:, 0], other[:, 0], amb[:, 0] = _clip_A(A, tol[:, 0])
    # LQ, LR are square roots of positive draws: reflect_chol never changes them
    return Expected(new, tol, other, amb), tq | tr, shq, shr


# ---- window samplers ---------------------------------------------------------------------------------------------
def windows_one(C, T, S, buffer, strict, seed, chain_offset, step):
    """sample_windows_kernel (pfg_windows.hip): per chain (y offset, T, t1, tL, weights offset in doubles), int64."""
    gid = chain_ids(C, chain_offset)
    s = int(step or 0)
    k0, k1 = split_seed(seed)
    r = philox4x32_10((_lo(gid), _hi(gid), s & MASK32, s >> 32), (k0 ^ 0x57494E44, k1))
    rng = T // S if strict else T - S + 1
    idx = umul64hi(bits64(r), rng)
    start = idx * S if strict else idx
    left = np.maximum(start - buffer, 0)
    right = np.minimum(start + S + buffer, T)
    return dict(yoff=left, T=right - left, t1=start - left, tL=start + S - left, woff=start * S)


def windows_multi(C, bounds, K, M, S, buffer, strict, seed, chain_offset, step, weight_offsets=None):
    """sample_windows_multi_kernel (pfg_windows.hip): [C * W] window records, chain-major (y offset in the
    concatenated series, T, t1, tL, weights offset or -1, sequence length) and the chosen sequences [C, K]."""
    bounds = [int(v) for v in bounds]
    n_seq = len(bounds) - 1
    Keff = n_seq if K == -1 else K
    W = Keff * M
    s = int(step or 0)
    k0, k1 = split_seed(seed)
    gid = chain_ids(C, chain_offset)
    c1 = _hi([s]) ^ _hi(gid)

    def draw(tags):
        r = philox4x32_10((_lo(gid)[:, None], c1[:, None], s & MASK32, np.asarray(tags, dtype=np.uint64)[None, :]),
                          (k0, k1))
        return [[(int(x) << 32) | int(y) for x, y in zip(rx, ry)] for rx, ry in zip(r[0].tolist(), r[1].tolist())]

    chosen = np.tile(np.arange(n_seq), (C, 1)) if K == -1 else np.zeros((C, K), np.int64)
    if K != -1:
        seq_bits = draw([0x53000000 | j for j in range(K)])
        for c in range(C):
            chosen[c] = choose_sequences(seq_bits[c], n_seq)
    win_bits = draw([0x57000000 | w for w in range(W)])
    out = {k: np.zeros(C * W, np.int64) for k in ("yoff", "T", "t1", "tL", "woff", "seq_len")}
    for c in range(C):
        for w in range(W):
            seq = int(chosen[c, w // M])
            lo, Tk = bounds[seq], bounds[seq + 1] - bounds[seq]
            whole = S < 1 or Tk - S <= 0
            start, ln = 0, Tk
            if not whole:
                rng = Tk // S if strict else Tk - S + 1
                idx = (win_bits[c][w] * rng) >> 64
                start, ln = (idx * S if strict else idx), S
            left, right = max(start - buffer, 0), min(start + ln + buffer, Tk)
            i = c * W + w
            out["yoff"][i], out["T"][i], out["t1"][i], out["tL"][i] = lo + left, right - left, start - left, start + ln - left
            woff = 0 if weight_offsets is None else int(weight_offsets[seq])
            out["woff"][i] = -1 if whole else woff + start * S
            out["seq_len"][i] = Tk
    return out, chosen


def choose_sequences(bits, n_seq):
    """The walk of sample_windows_multi_kernel (pfg_windows.hip): draw j is the r-th (r uniform on n_seq - j)
    sequence not chosen yet.  bits: the K 64-bit draws of the "S" tags."""
    chosen, srt = [], []
    for j, b in enumerate(bits):
        r = (int(b) * (n_seq - j)) >> 64
        i = 0
        while i < j and srt[i] <= r:
            r += 1
            i += 1
        srt.insert(i, r)
        chosen.append(r)
    return chosen


# ---- the lane generator of the device-generator units: lane_rng_init, pfg_math.hpp ----------------------------------------
class LaneRng(object):
    """jsf32 lanes keyed by lane_rng_init(seed, stream, step, lane), vectorised over lanes."""

    def __init__(self, seed, stream, step, lanes):
        lanes = np.asarray(lanes, dtype=np.uint64)
        seed, stream, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(step)
        r = philox4x32_10((lanes, step & MASK32, stream & MASK32, ((stream >> 32) ^ (step >> 32)) & MASK32),
                          (seed & MASK32, seed >> 32))
        self.s = [r[0].copy(), r[1].copy(), r[2].copy(), r[3] | U32(1)]
        for _ in range(8):
            self.next()

    def next(self):
        s0, s1, s2, s3 = self.s
        with np.errstate(over="ignore"):
            e = s0 - ((s1 << U32(27)) | (s1 >> U32(5)))
            n0 = s1 ^ ((s2 << U32(17)) | (s2 >> U32(15)))
            n1 = s2 + s3
            n2 = s3 + e
            n3 = e + n0
        self.s = [n0, n1, n2, n3]
        return n3.copy()


def ffbs_normals(seed, stream, step, N, T):
    """The T normals of each of N FFBS paths (pfg_ffbs.hip): lane s draws Box-Muller pairs on the f32 units, the
    first variate for one time, the second for the next, from t = T - 1 down.  Returns z [T * N] in the reference's
    order (z[k N + s]: path s at time T - 1 - k), long double."""
    g = LaneRng(seed, stream, step, np.arange(N))
    z = np.zeros((T, N), dtype=LD)
    for k in range(0, T, 2):
        a = g.next()
        b = g.next()
        z0, z1 = normal_pair_f32(a, b)
        z[k] = z0
        if k + 1 < T:
            z[k + 1] = z1
    return z.reshape(-1)
