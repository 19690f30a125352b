// Every update rule of resident chains, kernels then entry points (pfg_*_update_device): one lane per chain, f64.
//   sgld   every model: theta += eps (grad_logprior + ghat) / T + N(0, 2 eps / T), then project_parameters; sghmc: the
//          same kernel with a momentum buffer and friction alpha.
//   sgrld  SGMCMCSampler.sample_sgrld with LGSSMPreconditioner (sgmcmc_sampler.py:631-641, base_parameters.py:588-661,
//          models/lgssm.py:51-54), then project_parameters.  With theta = (A, C, LQinv, LRinv), Qinv = LQinv^2 + 1e-16,
//          Q = 1 / Qinv, g_v = grad_logprior_v(theta) + ghat_v and every preconditioner term at the pre-step theta:
//            A     += eps (Q g_A / T)                          + sqrt(2 eps) (z_A / LQinv) sqrt(1 / T)
//            C     += eps (R g_C / T)                          + sqrt(2 eps) (z_C / LRinv) sqrt(1 / T)   (not taken: C = 1 after)
//            LQinv += eps ((0.5 Qinv g_LQinv) / T + LQinv / T) + sqrt(2 eps) (sqrt(0.5) LQinv z_Q) sqrt(1 / T)
//            LRinv += eps ((0.5 Rinv g_LRinv) / T + LRinv / T) + sqrt(2 eps) (sqrt(0.5) LRinv z_R) sqrt(1 / T)
//          (the LQinv / T, LRinv / T terms: correction_term, (n + 1) / 2 L with n = 1).  The four normals of chain b are
//          those of sgld_update_kernel (spelled out in both: a shared helper changed that kernel's instructions):
//          Philox4x32-10 keyed by (seed, chain_offset + b, *step_ctr), drawn A, C, Q, R.
//   gibbs  LGSSMPrior.sample_posterior (base_parameters.py:354-377, 437-450) from the statistics an FFBS window with
//          PFG_STAT_GIBBS left in out[0..7] (pfg_ffbs.hip), block by block: Qinv, Rinv (1 x 1 Wishart = scale chi2(df)),
//          A given Q, then project_parameters.  The C draw is skipped: the projection pins C to 1 whatever it drew.
//          chi2(df) = 2 Gamma(df / 2), Gamma by Marsaglia-Tsang (shape >= 1) or Gamma(a + 1) U^(1/a) (shape < 1); every
//          attempt is keyed by (seed, chain, *step_ctr, variable, attempt), so a draw is a pure function of its key.
//          A variable still rejected after kMaxRounds attempts is NaN.
//   pmmh   particle marginal Metropolis-Hastings (Andrieu, Doucet and Holenstein 2010), two kernels around a particle
//          filter (or Kalman) launch that leaves its log-likelihood estimate in out[4]:
//            propose  theta' = theta + scale (.) z in the raw parameterisation (SVM A, LQinv, LRinv; LGSSM A, C, LQinv, LRinv
//                     with C' = 1 whatever scale_C is; GARCH log_mu, logit_phi, logit_lambduh, LRinv).  Support: what
//                     project_parameters leaves unchanged, |A| <= 0.9999 and every Cholesky factor > 0 (and finite
//                     numbers).  Outside it valid = 0 and theta' = theta, so the launch that follows never sees an
//                     illegal parameter vector.
//            accept   log alpha = (out[4] + logprior(theta')) - (ll_cur + logprior(theta)); accepted iff valid, out[4] is
//                     finite and log(u) < log alpha (a NaN log alpha rejects).  ll_cur is NEVER refreshed for a chain that
//                     rejects: the estimate a chain was accepted with is part of its state, and that is what makes the
//                     chain exact for every N.
//          logprior is Prior.logprior (base_parameters.py) of the raw theta row without Jacobian terms and without the
//          terms that depend on the hyper-parameters only (they cancel in log alpha).
//          Draws: Philox4x32-10, counter {gid_lo, step_lo, step_hi ^ gid_hi, tag} under key (seed_lo, seed_hi), gid =
//          chain_offset + b, step = *step_ctr -- the layout of the 0x5A11 / 0x5A12 normals above with tags of their own:
//            0x504D0001  normal_pair(r.x, r.y) -> z0, z1      0x504D0002  normal_pair(r.x, r.y) -> z2, z3
//            0x504D0003  uniform53(r.x, r.y)   -> u, the accept uniform in (0, 1)
//          (SVM: z0, z1, z2 for A, LQinv, LRinv; LGSSM: z0, z2, z3 for A, LQinv, LRinv; GARCH: z0..z3 in theta order).
//          Disjoint from 0x5A11 / 0x5A12, the Gibbs tags 0x61B5vvaa and the window tags 0x53...... / 0x57.......
//   pmala  particle Metropolis-adjusted Langevin (Nemeth, Sherlock and Fearnhead 2016), two kernels around the SCORE
//          launch, which leaves the score estimate in out[0..3] and the log-likelihood estimate in out[4].  In PMMH's
//          coordinates and support, with s_j = scale[j] and the drift of coordinate j
//            d_j(theta, g) = grad_logprior_j(theta) + g_j       (the prior gradient and the score columns of
//                                                                sgld_update_kernel: SVM [LR, LQ, A], LGSSM [LR, LQ, C, A],
//                                                                GARCH [LR, log_mu, logit_phi, logit_lambduh])
//            propose  theta'_j = (theta_j + (0.5 (s_j s_j)) d_j(theta, grad_cur)) + s_j z_j; LGSSM's C stays 1 (no normal,
//                     no density term).  Outside the support valid = 0 and theta' = theta, as for pmmh.
//            accept   log q(b | a, g) = -sum_j (b_j - (a_j + (0.5 (s_j s_j)) d_j(a, g)))^2 / (2 (s_j s_j)) over the free
//                     coordinates, and
//                       log alpha = (((out[4] + logprior(theta')) - (ll_cur + logprior(theta)))
//                                    + log q(theta | theta', out[0..3])) - log q(theta' | theta, grad_cur);
//                     accepted iff valid, out[4] and every score component the drift uses are finite, and
//                     log(u) < log alpha (a NaN rejects).  On accept theta = theta', ll_cur = out[4], grad_cur =
//                     out[0..3] verbatim (score-column order); a chain that rejects keeps theta, ll_cur AND grad_cur:
//                     neither estimate is ever refreshed, which is what makes the chain exact for every N (the pair
//                     (ll, g) is the auxiliary variable of the pseudo-marginal argument; the drift may be any function
//                     of (theta, g) as long as q is evaluated with the same one in both directions).
//          With (s_j s_j) / 2 = eps / T for every j the proposal is the law of sgld_update_kernel's step before
//          project_parameters.  Draws: the counter layout of pmmh under tags of their own,
//            0x4D4C0001  normal_pair(r.x, r.y) -> z0, z1      0x4D4C0002  normal_pair(r.x, r.y) -> z2, z3
//            0x4D4C0003  uniform53(r.x, r.y)   -> u
//          with pmmh's slot assignment (SVM z0, z1, z2; LGSSM z0, z2, z3; GARCH z0..z3).  Disjoint from every tag above.
//   pgibbs particle Gibbs (Andrieu, Doucet and Holenstein 2010): the parameter draw from the statistics the conditional SMC
//          sweep of pfg_csmc.hip left in out[0..7], keyed by ChainKey exactly as gibbs is (same tags: a chain runs one of
//          the two).  LGSSM: gibbs, expression for expression, in a kernel of its own (gibbs_update_kernel stays as it is).
//          SVM: (Qinv, A) from out[0..2] with conjugate(df_Qinv, scale_Qinv, mean_A, var_col_A, ..., T - 1) and A | Q as
//          gibbs; Rinv = scale chi2(df), df = df_Rinv + T, scale = 1 / (1 / scale_Rinv + out[3]), out[3] = sum_t y_t^2
//          exp(-x_t) -- the emission law is y_t ~ N(0, R exp(x_t)) (svm/kernels.py:56-62, svm_logw) --, then SVM's
//          project_parameters.  The transition sums run over t >= 1: the theta-dependence of x_0's law is left out of the
//          conditional, as in the reference's LGSSM Gibbs.
//          The sweep's own draws: tags 0x43530000 | particle, 0x43531000, 0x43532000 with the time step in the counter's
//          third word (pfg_csmc.hip).  Disjoint from every tag above.
// Built with -ffp-contract=off; IEEE division and ::sqrt / ::log throughout.
#include "pfg_host.hpp"
#include "pfg_math.hpp"

using namespace pfg_host;

namespace {

constexpr int kMaxRounds = 64;

// ---- what the rules share: the prior gradients, the projection ----
// grad_logprior of a Cholesky factor L of a 1 x 1 Wishart precision (covariance.py:272-284, n = 1) ...
__device__ __forceinline__ double chol_prior_grad(double L, double df, double scale) { return (df - 2.0) / L - L / scale; }
// ... and of the AR / emission coefficient x paired with the precision prec (matrices.py:597-607)
__device__ __forceinline__ double coef_prior_grad(double prec, double x, double mean, double var_col) { return -1.0 * (prec * (x - mean)) / var_col; }

// project_parameters: |A| <= 0.9999 (_utils.py:165-170), a Cholesky factor reflected (covariance.py:68-80)
__device__ __forceinline__ double clip_ar(double A) {
    const double aa = fabs(A);
    if (aa > 0.9999) A *= 0.9999 / aa;
    return A;
}
__device__ __forceinline__ double reflect_chol(double L) { return L < 0.0 ? sqrt(L * L + 1e-16) : L; }

// project_parameters of LGSSM: the two above and C = 1 (lgssm/parameters.py:39-42)
__device__ __forceinline__ void lgssm_project_store(double *th, double A, double LQ, double LR) {
    th[0] = clip_ar(A); th[1] = 1.0; th[2] = reflect_chol(LQ); th[3] = reflect_chol(LR);
}

// momentum == nullptr: SGLD.  Otherwise SGHMC with friction alpha: the increment d of each
// variable becomes v <- (1 - alpha) v + drift + sqrt(alpha) * noise (noise ~ N(0, 2 eps / T)).
__global__ void sgld_update_kernel(int model, int B, double *__restrict__ theta,
                                   const double *__restrict__ outs, pfg_prior_hyper hy, double eps,
                                   double Tscale, uint64_t seed, uint64_t chain_offset,
                                   const uint64_t *step_ctr, double *__restrict__ momentum, double alpha) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    const double *g = outs + (size_t)b * PFG_OUT_DOUBLES;
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const uint32_t c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32);
    pfg::u32x4 r0 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x5A11u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    pfg::u32x4 r1 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x5A12u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double nsd = sqrt(1.0 / Tscale) * sqrt(2.0 * eps) * (momentum ? sqrt(alpha) : 1.0);
    double *mv = momentum ? momentum + (size_t)b * PFG_MAX_THETA : nullptr;
    // one variable's increment: SGLD drift + noise, or the SGHMC momentum recursion
    auto incr = [&](int slot, double drift, double noise) {
        const double d = drift + noise;
        if (!mv) return d;
        const double v = (1.0 - alpha) * mv[slot] + d;
        mv[slot] = v;
        return v;
    };
    double nz[4];
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(r0.x, r0.y, nz[0], nz[1]);
    mth.normal_pair(r1.x, r1.y, nz[2], nz[3]);
    if (model == PFG_MODEL_SVM || model == PFG_MODEL_LGSSM) {
        const bool lg = model == PFG_MODEL_LGSSM;
        double A = th[0], C = lg ? th[1] : 1.0, LQ = th[lg ? 2 : 1], LR = th[lg ? 3 : 2];
        double Qinv = LQ * LQ + 1e-16, Rinv = LR * LR + 1e-16;
        // score columns: SVM [LR, LQ, A]; LGSSM [LR, LQ, C, A]
        double gLR = g[0], gLQ = g[1], gC = lg ? g[2] : 0.0, gA = g[lg ? 3 : 2];
        double pLQ = chol_prior_grad(LQ, hy.df_Qinv, hy.scale_Qinv);
        double pLR = chol_prior_grad(LR, hy.df_Rinv, hy.scale_Rinv);
        double pA = coef_prior_grad(Qinv, A, hy.mean_A, hy.var_col_A);
        double pC = coef_prior_grad(Rinv, C, hy.mean_C, hy.var_col_C);
        int j = 0;
        A += incr(0, eps * ((pA + gA) / Tscale), nsd * nz[j]); ++j;
        if (lg) { C += incr(1, eps * ((pC + gC) / Tscale), nsd * nz[j]); ++j; }
        LQ += incr(lg ? 2 : 1, eps * ((pLQ + gLQ) / Tscale), nsd * nz[j]); ++j;
        LR += incr(lg ? 3 : 2, eps * ((pLR + gLR) / Tscale), nsd * nz[j]); ++j;
        // project_parameters: _utils.py:165-170, covariance.py:68-80, lgssm/parameters.py:39-42
        A = clip_ar(A);
        if (lg) C = 1.0;
        LQ = reflect_chol(LQ); LR = reflect_chol(LR);
        th[0] = A;
        if (lg) { th[1] = C; th[2] = LQ; th[3] = LR; } else { th[1] = LQ; th[2] = LR; }
    } else {
        double lmu = th[0], lphi = th[1], llam = th[2], LR = th[3];
        double mu = exp(lmu), phi = 1.0 / (1.0 + exp(-lphi)), lam = 1.0 / (1.0 + exp(-llam));
        // garch_var.py:152-165
        double p0 = -hy.shape_mu - 1.0 + hy.scale_mu / mu;
        double p1 = ((hy.alpha_phi - 1.0) / (1.0 + phi) - (hy.beta_phi - 1.0) / (1.0 - phi)) * phi * (1.0 - phi);
        double p2 = ((hy.alpha_lambduh - 1.0) / (1.0 + lam) - (hy.beta_lambduh - 1.0) / (1.0 - lam)) * lam * (1.0 - lam);
        double pLR = chol_prior_grad(LR, hy.df_Rinv, hy.scale_Rinv);
        // score columns [LR, log_mu, logit_phi, logit_lambduh]
        lmu += incr(0, eps * ((p0 + g[1]) / Tscale), nsd * nz[0]);
        lphi += incr(1, eps * ((p1 + g[2]) / Tscale), nsd * nz[1]);
        llam += incr(2, eps * ((p2 + g[3]) / Tscale), nsd * nz[2]);
        LR += incr(3, eps * ((pLR + g[0]) / Tscale), nsd * nz[3]);
        th[0] = lmu; th[1] = lphi; th[2] = llam; th[3] = reflect_chol(LR);
    }
}

__global__ void bump_counter_kernel(uint64_t *ctr) { *ctr += 1; }

__global__ void sgrld_update_kernel(int B, double *__restrict__ theta, const double *__restrict__ outs, pfg_prior_hyper hy,
                                    double eps, double Tscale, uint64_t seed, uint64_t chain_offset,
                                    const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    const double *g = outs + (size_t)b * PFG_OUT_DOUBLES;
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const uint32_t c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32);
    const pfg::u32x4 r0 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x5A11u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const pfg::u32x4 r1 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x5A12u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    double zA, zC, zQ, zR;
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(r0.x, r0.y, zA, zC);
    mth.normal_pair(r1.x, r1.y, zQ, zR);
    (void)zC;       // C's step is not taken: the projection pins C to 1 whatever it would be
    const double A = th[0], LQ = th[2], LR = th[3];
    const double Qinv = LQ * LQ + 1e-16, Rinv = LR * LR + 1e-16;
    const double Q = 1.0 / Qinv;
    // score columns [LRinv, LQinv, C, A]
    const double pLQ = chol_prior_grad(LQ, hy.df_Qinv, hy.scale_Qinv);
    const double pLR = chol_prior_grad(LR, hy.df_Rinv, hy.scale_Rinv);
    const double pA = coef_prior_grad(Qinv, A, hy.mean_A, hy.var_col_A);
    const double gA = pA + g[3], gLQ = pLQ + g[1], gLR = pLR + g[0];
    const double scale = 1.0 / Tscale, nsd = sqrt(2.0 * eps), rs = sqrt(scale), half = sqrt(0.5);
    const double nA = (zA / LQ) * rs;
    const double nQ = ((half * LQ) * zQ) * rs, nR = ((half * LR) * zR) * rs;
    const double A1 = A + (eps * ((Q * gA) * scale + 0.0) + nsd * nA);
    const double LQ1 = LQ + (eps * (((0.5 * Qinv) * gLQ) * scale + LQ * scale) + nsd * nQ);
    const double LR1 = LR + (eps * (((0.5 * Rinv) * gLR) * scale + LR * scale) + nsd * nR);
    lgssm_project_store(th, A1, LQ1, LR1);
}

// The keyed draws of one chain and step: attempt k of variable v is Philox4x32-10 of (chain, step, tag(v, k)).
struct ChainKey {
    uint32_t gid, c1, c2, k0, k1;
    __device__ __forceinline__ pfg::u32x4 draw(uint32_t var, uint32_t attempt) const {
        return pfg::philox4x32_10({gid, c1, c2, 0x61B50000u | (var << 8) | attempt}, k0, k1);
    }
};

__device__ __forceinline__ double uniform53(uint32_t a, uint32_t b) {      // (0, 1)
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

// Gamma(shape, 1): Marsaglia & Tsang (2000) on (shape + 1 when shape < 1, then times U^(1 / shape)); NaN when every
// round is rejected or shape is not a positive number
__device__ double gamma_draw(const ChainKey &key, uint32_t var, double shape) {
    if (!(shape > 0.0) || !(shape < INFINITY)) return NAN;
    const bool boost = shape < 1.0;
    const double a = boost ? shape + 1.0 : shape;
    const double d = a - 1.0 / 3.0, c = 1.0 / ::sqrt(9.0 * d);
    const pfg::Math<double, false> mth = {};
    for (uint32_t k = 0; k < (uint32_t)kMaxRounds; ++k) {
        const pfg::u32x4 r = key.draw(var, k);
        double z, unused;
        mth.normal_pair(r.x, r.y, z, unused);
        const double t = 1.0 + c * z;
        if (t <= 0.0) continue;
        const double v = t * t * t;
        const double u = uniform53(r.z, r.w);
        if (::log(u) < 0.5 * z * z + d - d * v + d * ::log(v)) {
            double x = d * v;
            if (boost) {
                const pfg::u32x4 s = key.draw(var | 0x80u, 0);
                x *= ::exp(::log(uniform53(s.x, s.y)) / shape);
            }
            return x;
        }
    }
    return NAN;
}

// Qinv | x, y of one Wishart block (covariance.py:207-240, 1 x 1): its posterior df and scale, from the paired matrix's
// prior (mean, var_col) and the statistics (S_prevprev, S_curprev, S_curcur)
struct Conj { double df, scale, Spp, Scp; };
__device__ __forceinline__ Conj conjugate(double df0, double scale0, double mean, double var_col, double spp, double scp,
                                          double scc, double count) {
    const double mean_prec = mean * (1.0 / var_col), prec = 1.0 / var_col;
    Conj o;
    o.Spp = prec + spp;
    o.Scp = mean_prec + scp;
    const double Scc = mean * mean_prec + scc;
    const double schur = Scc - (o.Scp * o.Scp) / o.Spp;
    o.df = df0 + count;
    o.scale = 1.0 / (1.0 / scale0 + schur);
    return o;
}

__global__ void gibbs_update_kernel(int B, double *__restrict__ theta, const double *__restrict__ outs, pfg_prior_hyper hy,
                                    uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    const double *s = outs + (size_t)b * PFG_OUT_DOUBLES;
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const ChainKey key{(uint32_t)gid, (uint32_t)step, (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32), (uint32_t)seed,
                       (uint32_t)(seed >> 32)};
    const double T = s[6];
    // transitions (t >= 1): T - 1 of them; emissions: T
    const Conj q = conjugate(hy.df_Qinv, hy.scale_Qinv, hy.mean_A, hy.var_col_A, s[0], s[1], s[2], T - 1.0);
    const Conj r = conjugate(hy.df_Rinv, hy.scale_Rinv, hy.mean_C, hy.var_col_C, s[3], s[4], s[5], T);
    const double Qinv = q.scale * (2.0 * gamma_draw(key, 0, 0.5 * q.df));
    const double Rinv = r.scale * (2.0 * gamma_draw(key, 1, 0.5 * r.df));
    const double LQ = ::sqrt(Qinv), LR = ::sqrt(Rinv);
    // A | Q ~ N(Scp / Spp, 1 / ((LQinv^2 + 1e-9) Spp)) (matrices.py:556-580)
    const pfg::u32x4 ra = key.draw(2, 0);
    double zA, unused;
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(ra.x, ra.y, zA, unused);
    const double P = LQ * LQ + 1e-9;
    const double A = q.Scp / q.Spp + ::sqrt((1.0 / P) * (1.0 / q.Spp)) * zA;
    lgssm_project_store(th, A, LQ, LR);
}

// ---- PMMH: the log-prior value, propose, accept ----
// log-density of a Cholesky factor L of a 1 x 1 Wishart precision at P = L^2 + 1e-16 (scipy.stats.wishart.logpdf,
// base_parameters.py WishartPrecisionPrior.logprior), less its terms in (df, scale) alone ...
__device__ __forceinline__ double chol_logprior(double L, double df, double scale) {
    const double P = L * L + 1e-16;
    return (0.5 * (df - 2.0)) * ::log(P) - (0.5 * P) / scale;
}
// ... and of the coefficient x paired with the factor L (MatrixNormalPrior.logprior, 1 x 1), less its constants
__device__ __forceinline__ double coef_logprior(double L, double x, double mean, double var_col) {
    const double r = L * (x - mean);
    return -0.5 * ((r * r) / var_col) + ::log(L);
}
// Prior.logprior of one raw theta row, up to a constant of the hyper-parameters.  GARCH (GARCHVarsPrior.logprior):
// mu ~ InvGamma, (1 + phi) / 2 and (1 + lambduh) / 2 ~ Beta with phi = expit(logit_phi), as the host evaluates them
__device__ double logprior_value(int model, const double *th, const pfg_prior_hyper &hy) {
    if (model == PFG_MODEL_SVM)
        return chol_logprior(th[1], hy.df_Qinv, hy.scale_Qinv) + chol_logprior(th[2], hy.df_Rinv, hy.scale_Rinv) +
               coef_logprior(th[1], th[0], hy.mean_A, hy.var_col_A);
    if (model == PFG_MODEL_LGSSM)
        return chol_logprior(th[2], hy.df_Qinv, hy.scale_Qinv) + chol_logprior(th[3], hy.df_Rinv, hy.scale_Rinv) +
               coef_logprior(th[2], th[0], hy.mean_A, hy.var_col_A) + coef_logprior(th[3], th[1], hy.mean_C, hy.var_col_C);
    const double mu = ::exp(th[0]);
    const double xp = (1.0 + 1.0 / (1.0 + ::exp(-th[1]))) / 2.0, xl = (1.0 + 1.0 / (1.0 + ::exp(-th[2]))) / 2.0;
    double lp = -(hy.shape_mu + 1.0) * th[0] - hy.scale_mu / mu;
    lp = lp + ((hy.alpha_phi - 1.0) * ::log(xp) + (hy.beta_phi - 1.0) * ::log1p(-xp));
    lp = lp + ((hy.alpha_lambduh - 1.0) * ::log(xl) + (hy.beta_lambduh - 1.0) * ::log1p(-xl));
    return lp + chol_logprior(th[3], hy.df_Rinv, hy.scale_Rinv);
}

__global__ void logprior_kernel(int model, int B, const double *__restrict__ theta, pfg_prior_hyper hy,
                                double *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[b] = logprior_value(model, theta + (size_t)b * PFG_MAX_THETA, hy);
}

__global__ void pmmh_propose_kernel(int model, int B, const double *__restrict__ theta, double *__restrict__ theta_prop,
                                    int32_t *__restrict__ valid, const double *__restrict__ scale, uint64_t seed,
                                    uint64_t chain_offset, const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *th = theta + (size_t)b * PFG_MAX_THETA;
    double *tp = theta_prop + (size_t)b * PFG_MAX_THETA;
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const uint32_t c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32);
    const pfg::u32x4 r0 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x504D0001u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const pfg::u32x4 r1 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x504D0002u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    double z[4];
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(r0.x, r0.y, z[0], z[1]);
    mth.normal_pair(r1.x, r1.y, z[2], z[3]);
    double p[PFG_MAX_THETA];
    bool ok;
    if (model == PFG_MODEL_SVM) {
        p[0] = th[0] + scale[0] * z[0]; p[1] = th[1] + scale[1] * z[1]; p[2] = th[2] + scale[2] * z[2]; p[3] = th[3];
        ok = fabs(p[0]) <= 0.9999 && p[1] > 0.0 && p[1] < INFINITY && p[2] > 0.0 && p[2] < INFINITY;
    } else if (model == PFG_MODEL_LGSSM) {
        p[0] = th[0] + scale[0] * z[0]; p[1] = 1.0; p[2] = th[2] + scale[2] * z[2]; p[3] = th[3] + scale[3] * z[3];
        ok = fabs(p[0]) <= 0.9999 && p[2] > 0.0 && p[2] < INFINITY && p[3] > 0.0 && p[3] < INFINITY;
    } else {
        for (int j = 0; j < 4; ++j) p[j] = th[j] + scale[j] * z[j];
        ok = fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY && p[3] > 0.0 && p[3] < INFINITY;
    }
    valid[b] = ok ? 1 : 0;
    for (int j = 0; j < PFG_MAX_THETA; ++j) tp[j] = ok ? p[j] : th[j];
}

// init != 0: ll_cur = out[4], nothing else.  Otherwise the accept / reject step; a chain that rejects keeps theta AND
// ll_cur, the estimate it was accepted with (never a fresh one: see the header)
__global__ void pmmh_accept_kernel(int model, int B, double *__restrict__ theta, const double *__restrict__ theta_prop,
                                   const int32_t *__restrict__ valid, const double *__restrict__ outs,
                                   double *__restrict__ ll_cur, uint64_t *__restrict__ n_accept, pfg_prior_hyper hy, int init,
                                   uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double ll_prop = outs[(size_t)b * PFG_OUT_DOUBLES + 4];
    if (init) { ll_cur[b] = ll_prop; return; }
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    const double *tp = theta_prop + (size_t)b * PFG_MAX_THETA;
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const uint32_t c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32);
    const pfg::u32x4 r = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x504D0003u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u = uniform53(r.x, r.y);
    const double log_alpha = (ll_prop + logprior_value(model, tp, hy)) - (ll_cur[b] + logprior_value(model, th, hy));
    const bool finite = fabs(ll_prop) < INFINITY;        // false for a NaN as well
    if (valid[b] != 0 && finite && ::log(u) < log_alpha) {
        for (int j = 0; j < PFG_MAX_THETA; ++j) th[j] = tp[j];
        ll_cur[b] = ll_prop;
        n_accept[b] += 1;
    }
}

// ---- pMALA: the drift, the proposal's log-density, propose, accept ----
// d_j(theta, g) = grad_logprior_j(theta) + g_j in theta order, the prior gradient and the score columns as sgld_update_kernel
// states them (spelled out here: that kernel stays as it is); 0 for the slot that does not move (LGSSM's C, SVM's fourth)
__device__ void pmala_drift(int model, const double *th, const double *g, const pfg_prior_hyper &hy, double *d) {
    if (model == PFG_MODEL_SVM || model == PFG_MODEL_LGSSM) {
        const bool lg = model == PFG_MODEL_LGSSM;
        const double A = th[0], LQ = th[lg ? 2 : 1], LR = th[lg ? 3 : 2];
        const double Qinv = LQ * LQ + 1e-16;
        // score columns: SVM [LR, LQ, A]; LGSSM [LR, LQ, C, A]
        d[0] = coef_prior_grad(Qinv, A, hy.mean_A, hy.var_col_A) + g[lg ? 3 : 2];
        d[lg ? 1 : 3] = 0.0;
        d[lg ? 2 : 1] = chol_prior_grad(LQ, hy.df_Qinv, hy.scale_Qinv) + g[1];
        d[lg ? 3 : 2] = chol_prior_grad(LR, hy.df_Rinv, hy.scale_Rinv) + g[0];
    } else {
        const double mu = exp(th[0]), phi = 1.0 / (1.0 + exp(-th[1])), lam = 1.0 / (1.0 + exp(-th[2]));
        // garch_var.py:152-165; score columns [LR, log_mu, logit_phi, logit_lambduh]
        d[0] = (-hy.shape_mu - 1.0 + hy.scale_mu / mu) + g[1];
        d[1] = ((hy.alpha_phi - 1.0) / (1.0 + phi) - (hy.beta_phi - 1.0) / (1.0 - phi)) * phi * (1.0 - phi) + g[2];
        d[2] = ((hy.alpha_lambduh - 1.0) / (1.0 + lam) - (hy.beta_lambduh - 1.0) / (1.0 - lam)) * lam * (1.0 - lam) + g[3];
        d[3] = chol_prior_grad(th[3], hy.df_Rinv, hy.scale_Rinv) + g[0];
    }
}
// the coordinates a proposal moves: SVM 0..2, LGSSM 0, 2, 3, GARCH 0..3
__device__ __forceinline__ bool pmala_free(int model, int j) { return model == PFG_MODEL_SVM ? j < 3 : (model == PFG_MODEL_LGSSM ? j != 1 : true); }
// the mean of the proposal from a with drift d: a_j + (s_j^2 / 2) d_j
__device__ __forceinline__ double pmala_mean(double a, double s, double d) { return a + (0.5 * (s * s)) * d; }
// log q(b | a, g), d = d(a, g), less the constant of the scales
__device__ double pmala_log_q(int model, const double *b, const double *a, const double *d, const double *s) {
    double q = 0.0;
    for (int j = 0; j < PFG_MAX_THETA; ++j) {
        if (!pmala_free(model, j)) continue;
        const double r = b[j] - pmala_mean(a[j], s[j], d[j]);
        q = q + (r * r) / (2.0 * (s[j] * s[j]));
    }
    return -q;
}

__global__ void pmala_propose_kernel(int model, int B, const double *__restrict__ theta, const double *__restrict__ grad_cur,
                                     double *__restrict__ theta_prop, int32_t *__restrict__ valid,
                                     const double *__restrict__ scale, pfg_prior_hyper hy, uint64_t seed, uint64_t chain_offset,
                                     const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *th = theta + (size_t)b * PFG_MAX_THETA;
    double *tp = theta_prop + (size_t)b * PFG_MAX_THETA;
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const uint32_t c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32);
    const pfg::u32x4 r0 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x4D4C0001u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const pfg::u32x4 r1 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x4D4C0002u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    double z[4];
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(r0.x, r0.y, z[0], z[1]);
    mth.normal_pair(r1.x, r1.y, z[2], z[3]);
    double a[PFG_MAX_THETA], d[PFG_MAX_THETA], p[PFG_MAX_THETA];
    for (int j = 0; j < PFG_MAX_THETA; ++j) a[j] = th[j];
    pmala_drift(model, a, grad_cur + (size_t)b * PFG_MAX_THETA, hy, d);
    bool ok;
    if (model == PFG_MODEL_SVM) {
        for (int j = 0; j < 3; ++j) p[j] = pmala_mean(a[j], scale[j], d[j]) + scale[j] * z[j];
        p[3] = a[3];
        ok = fabs(p[0]) <= 0.9999 && p[1] > 0.0 && p[1] < INFINITY && p[2] > 0.0 && p[2] < INFINITY;
    } else if (model == PFG_MODEL_LGSSM) {
        p[0] = pmala_mean(a[0], scale[0], d[0]) + scale[0] * z[0];
        p[1] = 1.0;
        p[2] = pmala_mean(a[2], scale[2], d[2]) + scale[2] * z[2];
        p[3] = pmala_mean(a[3], scale[3], d[3]) + scale[3] * z[3];
        ok = fabs(p[0]) <= 0.9999 && p[2] > 0.0 && p[2] < INFINITY && p[3] > 0.0 && p[3] < INFINITY;
    } else {
        for (int j = 0; j < 4; ++j) p[j] = pmala_mean(a[j], scale[j], d[j]) + scale[j] * z[j];
        ok = fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY && p[3] > 0.0 && p[3] < INFINITY;
    }
    valid[b] = ok ? 1 : 0;
    for (int j = 0; j < PFG_MAX_THETA; ++j) tp[j] = ok ? p[j] : a[j];
}

// init != 0: ll_cur = out[4] and grad_cur = out[0..3], nothing else.  Otherwise the accept / reject step; a chain that
// rejects keeps theta, ll_cur AND grad_cur, the estimates it was accepted with (never fresh ones: see the header)
__global__ void pmala_accept_kernel(int model, int B, double *__restrict__ theta, const double *__restrict__ theta_prop,
                                    const int32_t *__restrict__ valid, const double *__restrict__ outs,
                                    double *__restrict__ ll_cur, double *__restrict__ grad_cur, uint64_t *__restrict__ n_accept,
                                    pfg_prior_hyper hy, const double *__restrict__ scale, int init, uint64_t seed,
                                    uint64_t chain_offset, const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *o = outs + (size_t)b * PFG_OUT_DOUBLES;
    double *gc = grad_cur + (size_t)b * PFG_MAX_THETA;
    const double ll_prop = o[4];
    double gp[PFG_MAX_THETA];
    for (int j = 0; j < PFG_MAX_THETA; ++j) gp[j] = o[j];
    if (init) {
        ll_cur[b] = ll_prop;
        for (int j = 0; j < PFG_MAX_THETA; ++j) gc[j] = gp[j];
        return;
    }
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    double a[PFG_MAX_THETA], p[PFG_MAX_THETA], g[PFG_MAX_THETA], s[PFG_MAX_THETA], da[PFG_MAX_THETA], dp[PFG_MAX_THETA];
    for (int j = 0; j < PFG_MAX_THETA; ++j) {
        a[j] = th[j]; p[j] = theta_prop[(size_t)b * PFG_MAX_THETA + j]; g[j] = gc[j]; s[j] = scale[j];
    }
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const uint32_t c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32);
    const pfg::u32x4 r = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x4D4C0003u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u = uniform53(r.x, r.y);
    pmala_drift(model, a, g, hy, da);
    pmala_drift(model, p, gp, hy, dp);
    const double q_fwd = pmala_log_q(model, p, a, da, s), q_rev = pmala_log_q(model, a, p, dp, s);
    const double log_alpha = (((ll_prop + logprior_value(model, p, hy)) - (ll_cur[b] + logprior_value(model, a, hy))) + q_rev) - q_fwd;
    // the score components the drift uses (LGSSM: not C's column 2; SVM: columns 0..2); false for a NaN as well
    bool finite = fabs(ll_prop) < INFINITY;
    for (int j = 0; j < PFG_MAX_THETA; ++j)
        if (model == PFG_MODEL_SVM ? j < 3 : (model == PFG_MODEL_LGSSM ? j != 2 : true)) finite = finite && fabs(gp[j]) < INFINITY;
    if (valid[b] != 0 && finite && ::log(u) < log_alpha) {
        for (int j = 0; j < PFG_MAX_THETA; ++j) { th[j] = p[j]; gc[j] = gp[j]; }
        ll_cur[b] = ll_prop;
        n_accept[b] += 1;
    }
}

// ---- particle Gibbs: the parameter draw from the statistics of a conditional SMC path (pfg_csmc.hip) ----
// LGSSM: gibbs_update_kernel's arithmetic, spelled out again (that kernel stays as it is).  SVM: see the header
__global__ void pgibbs_update_kernel(int model, int B, double *__restrict__ theta, const double *__restrict__ outs,
                                     pfg_prior_hyper hy, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    const double *s = outs + (size_t)b * PFG_OUT_DOUBLES;
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const ChainKey key{(uint32_t)gid, (uint32_t)step, (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32), (uint32_t)seed,
                       (uint32_t)(seed >> 32)};
    const double T = s[6];
    // transitions (t >= 1): T - 1 of them; emissions: T
    const Conj q = conjugate(hy.df_Qinv, hy.scale_Qinv, hy.mean_A, hy.var_col_A, s[0], s[1], s[2], T - 1.0);
    double r_df, r_scale;
    if (model == PFG_MODEL_LGSSM) {
        const Conj r = conjugate(hy.df_Rinv, hy.scale_Rinv, hy.mean_C, hy.var_col_C, s[3], s[4], s[5], T);
        r_df = r.df; r_scale = r.scale;
    } else {
        r_df = hy.df_Rinv + T;
        r_scale = 1.0 / (1.0 / hy.scale_Rinv + s[3]);
    }
    const double Qinv = q.scale * (2.0 * gamma_draw(key, 0, 0.5 * q.df));
    const double Rinv = r_scale * (2.0 * gamma_draw(key, 1, 0.5 * r_df));
    const double LQ = ::sqrt(Qinv), LR = ::sqrt(Rinv);
    // A | Q ~ N(Scp / Spp, 1 / ((LQinv^2 + 1e-9) Spp)) (matrices.py:556-580)
    const pfg::u32x4 ra = key.draw(2, 0);
    double zA, unused;
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(ra.x, ra.y, zA, unused);
    const double P = LQ * LQ + 1e-9;
    const double A = q.Scp / q.Spp + ::sqrt((1.0 / P) * (1.0 / q.Spp)) * zA;
    if (model == PFG_MODEL_LGSSM) {
        lgssm_project_store(th, A, LQ, LR);
    } else {
        th[0] = clip_ar(A); th[1] = reflect_chol(LQ); th[2] = reflect_chol(LR);
    }
}

// ---- the entry points: one prologue, one epilogue ----
// What every rule checks of its arguments (`what` names the entry point).  lgssm_only: how SGRLD and Gibbs refuse other
// models' chains (the reference's one preconditioner and conjugate prior).  Gibbs has no step size: the defaults pass.
int check_update(pfg_ctx *ctx, const char *what, int model, const double *theta, const double *outs,
                 const pfg_prior_hyper *hyper, const char *lgssm_only = nullptr, double epsilon = 1.0, double Tscale = 1.0) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!theta || !outs || !hyper) return fail(ctx, PFG_ERR_INVALID, std::string(what) + ": NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (lgssm_only && model != PFG_MODEL_LGSSM)          // sgmcmc_sampler.py:643-646
        return fail(ctx, PFG_ERR_UNSUPPORTED, std::string(what) + lgssm_only + (model == PFG_MODEL_SVM ? "SVMSampler" : "GARCHSampler"));
    if (!(epsilon > 0.0) || !(Tscale > 0.0)) return fail(ctx, PFG_ERR_INVALID, "epsilon and Tscale must be > 0");
    return PFG_OK;
}

// `kernel` over the B chains, then the step counter's bump
template <typename Kernel, typename... Args>
int run_update(pfg_ctx *ctx, int B, uint64_t *step_ctr, void *hip_stream, Kernel kernel, Args... args) {
    if (B <= 0) return PFG_OK;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(kernel, dim3((B + 127) / 128), dim3(128), 0, st, args...);
    if (step_ctr) hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, st, step_ctr);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

}  // namespace

int pfg_sgld_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                           const pfg_prior_hyper *hyper, double epsilon, double Tscale, uint64_t seed,
                           uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    return pfg_sghmc_update_device(ctx, model, B, theta, nullptr, outs, hyper, epsilon, 1.0, Tscale, seed, chain_offset, step_ctr, hip_stream);
}

int pfg_sghmc_update_device(pfg_ctx *ctx, int model, int B, double *theta, double *momentum, const double *outs,
                            const pfg_prior_hyper *hyper, double epsilon, double alpha, double Tscale,
                            uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!(alpha > 0.0 && alpha <= 1.0)) return fail(ctx, PFG_ERR_INVALID, "SGHMC friction alpha must be in (0, 1]");
    if (const int rc = check_update(ctx, "pfg_sgld_update_device", model, theta, outs, hyper, nullptr, epsilon, Tscale)) return rc;
    return run_update(ctx, B, step_ctr, hip_stream, sgld_update_kernel, model, B, theta, outs, *hyper, epsilon, Tscale, seed,
                      chain_offset, (const uint64_t *)step_ctr, momentum, alpha);
}

int pfg_sgrld_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                            const pfg_prior_hyper *hyper, double epsilon, double Tscale,
                            uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_update(ctx, __func__, model, theta, outs, hyper, ": No Default Preconditioner for ", epsilon, Tscale)) return rc;
    return run_update(ctx, B, step_ctr, hip_stream, sgrld_update_kernel, B, theta, outs, *hyper, epsilon, Tscale, seed,
                      chain_offset, (const uint64_t *)step_ctr);
}

int pfg_gibbs_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                            const pfg_prior_hyper *hyper, uint64_t seed, uint64_t chain_offset,
                            uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_update(ctx, __func__, model, theta, outs, hyper, ": no conjugate Gibbs draw for ")) return rc;
    return run_update(ctx, B, step_ctr, hip_stream, gibbs_update_kernel, B, theta, outs, *hyper, seed, chain_offset,
                      (const uint64_t *)step_ctr);
}

int pfg_logprior_device(pfg_ctx *ctx, int model, int B, const double *theta, const pfg_prior_hyper *hyper, double *logprior,
                        void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!theta || !hyper || !logprior) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (B < 0) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": B must be >= 0");
    return run_update(ctx, B, nullptr, hip_stream, logprior_kernel, model, B, theta, *hyper, logprior);
}

int pfg_pmmh_propose_device(pfg_ctx *ctx, int model, int B, const double *theta, double *theta_prop, int32_t *valid,
                            const double *scale, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr,
                            void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!theta || !theta_prop || !valid || !scale) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (B < 0) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": B must be >= 0");
    // (no bump: the accept step that closes the PMMH step advances the counter)
    return run_update(ctx, B, nullptr, hip_stream, pmmh_propose_kernel, model, B, theta, theta_prop, valid, scale, seed,
                      chain_offset, step_ctr);
}

int pfg_pmmh_accept_device(pfg_ctx *ctx, int model, int B, double *theta, const double *theta_prop, const int32_t *valid,
                           const double *outs, double *ll_cur, uint64_t *n_accept, const pfg_prior_hyper *hyper, int init,
                           uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!theta || !theta_prop || !valid || !outs || !ll_cur || !n_accept || !hyper)
        return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (B < 0) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": B must be >= 0");
    return run_update(ctx, B, init ? nullptr : step_ctr, hip_stream, pmmh_accept_kernel, model, B, theta, theta_prop, valid,
                      outs, ll_cur, n_accept, *hyper, init, seed, chain_offset, (const uint64_t *)step_ctr);
}

int pfg_pmala_propose_device(pfg_ctx *ctx, int model, int B, const double *theta, const double *grad_cur, double *theta_prop,
                             int32_t *valid, const double *scale, const pfg_prior_hyper *hyper, uint64_t seed,
                             uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!theta || !grad_cur || !theta_prop || !valid || !scale || !hyper)
        return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (B < 0) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": B must be >= 0");
    // (no bump: the accept step that closes the pMALA step advances the counter)
    return run_update(ctx, B, nullptr, hip_stream, pmala_propose_kernel, model, B, theta, grad_cur, theta_prop, valid, scale,
                      *hyper, seed, chain_offset, step_ctr);
}

int pfg_pmala_accept_device(pfg_ctx *ctx, int model, int B, double *theta, const double *theta_prop, const int32_t *valid,
                            const double *outs, double *ll_cur, double *grad_cur, uint64_t *n_accept,
                            const pfg_prior_hyper *hyper, const double *scale, int init, uint64_t seed, uint64_t chain_offset,
                            uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!theta || !theta_prop || !valid || !outs || !ll_cur || !grad_cur || !n_accept || !hyper || !scale)
        return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (B < 0) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": B must be >= 0");
    return run_update(ctx, B, init ? nullptr : step_ctr, hip_stream, pmala_accept_kernel, model, B, theta, theta_prop, valid,
                      outs, ll_cur, grad_cur, n_accept, *hyper, scale, init, seed, chain_offset, (const uint64_t *)step_ctr);
}

int pfg_pgibbs_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                             const pfg_prior_hyper *hyper, uint64_t seed, uint64_t chain_offset,
                             uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_update(ctx, __func__, model, theta, outs, hyper)) return rc;
    if (model == PFG_MODEL_GARCH)
        return fail(ctx, PFG_ERR_UNSUPPORTED, std::string(__func__) + ": no conjugate Gibbs draw for GARCHSampler");
    return run_update(ctx, B, step_ctr, hip_stream, pgibbs_update_kernel, model, B, theta, outs, *hyper, seed, chain_offset,
                      (const uint64_t *)step_ctr);
}
