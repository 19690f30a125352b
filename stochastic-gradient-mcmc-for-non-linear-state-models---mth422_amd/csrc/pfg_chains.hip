// Every update rule of resident chains, kernels then entry points (pfg_*_update_device): one lane per chain, f64.
// What the rules share is stated once, ahead of the kernels:
//   key      make_key and uniform53 (pfg_chain_filter.hpp, shared with the filters that run one workgroup per chain): the
//            draws of chain b at one step are Philox4x32-10 of the counter {gid_lo, step_lo, step_hi ^ gid_hi, tag} under
//            key (seed_lo, seed_hi), gid = chain_offset + b, step = *step_ctr (0 for a NULL counter), so a draw is a pure
//            function of its key.  normals4 turns two tags into four normals, normal_pair(r.x, r.y) of each.
//              0x5A11, 0x5A12            sgld / sghmc / sgrld: z0, z1 and z2, z3, one per theta slot
//              0x61B5vvaa                gibbs / pgibbs: attempt aa of variable vv (0 Qinv, 1 Rinv, 2 A; vv | 0x80 the boost)
//              0x504D0001, 0x504D0002    pmmh:  z0, z1 and z2, z3         0x504D0003  uniform53(r.x, r.y) -> u in (0, 1)
//              0x4D4C0001, 0x4D4C0002    pmala: z0, z1 and z2, z3         0x4D4C0003  uniform53(r.x, r.y) -> u
//            z_j belongs to theta slot j (SVM A, LQinv, LRinv: z0, z1, z2; LGSSM A, C, LQinv, LRinv: C's z1 is not used by
//            sgrld, pmmh and pmala; GARCH log_mu, logit_phi, logit_lambduh, LRinv: z0..z3).  All disjoint from one another,
//            from the window tags 0x53...... / 0x57......, from the sweep's 0x4353.... (pfg_csmc.hip) and from the correlated
//            filter's 0x43500000 | column >> 2, at most 0x43500100 (pfg_cpm.hip).
//              0x53510000                sqmc: the digital shift of a row of the point set (pfg_sqmc.hip), with the row XORed
//                                        into the counter's third word
//              0x534D0001                smc: the resampling uniform of a tempering stage (pfg_smc.hip), keyed by the stage and
//                                        not by a chain: counter {stage_lo, stage_hi, 0, tag}.  The window tag 0x53000000 | j
//                                        stops at j < PFG_MAX_DRAWN_SEQUENCES = 1024, far below 0x4D0001.
//   drift    d_j(theta, g) = grad_logprior_j(theta) + g_j in theta order, g the score columns of a launch (SVM [LR, LQ,
//            A], LGSSM [LR, LQ, C, A], GARCH [LR, log_mu, logit_phi, logit_lambduh]).  sgld, sgrld and pmala use it.
//   project  project_parameters: |A| <= 0.9999, a negative Cholesky factor reflected, LGSSM's C = 1.
//   support  what project leaves unchanged (and finite numbers): where pmmh and pmala may propose.  moves(model, j) names
//            the slots a proposal moves (theta order), score_used(model, j) the score columns its drift reads.
//   accept   metropolis: u, the decision valid && finite && log(u) < log alpha (a NaN rejects), the commit.
//   conjugate, gamma_draw: the Wishart block and its chi2 draw of gibbs and pgibbs.
// The rules:
//   sgld   every model: theta += eps (d(theta, ghat) / T) + N(0, 2 eps / T), then project; sghmc: the same kernel with a
//          momentum buffer and friction alpha.  LGSSM's C takes its increment before project pins it to 1: under sghmc it
//          is part of the momentum.
//   sgd    SGMCMCSampler.step_sgd (sgmcmc_sampler.py:467-484): theta += eps (d(theta, ghat) / T), then project.  No draws.
//   adagrad  SGMCMCSampler.step_adagrad (sgmcmc_sampler.py:504-527) with a moment buffer G [B][4], one kernel with sgd:
//          g = d(theta, ghat) / T, G += g g, theta += eps (g / sqrt(G + 1e-9)) (the reference's NOISE_NUGGET), then project.
//          G covers every variable, LGSSM's C included although project pins C; SVM's fourth slot is untouched.  No draws.
//   sgld_cv  SGLD with control variates (Baker, Fearnhead, Fox and Nemeth 2019): sgld's step -- its operations, its normals, its
//          key -- on g_k = centre_grad_k + (out_k - out_centre_k), k the four score columns: `out` the record of the chain's
//          window at theta, `out_centre` the record of the SAME window on the SAME draws at the centre, centre_grad the
//          whole-data score at the centre (raw, unscaled, without the prior: d adds the prior's gradient at theta).  With
//          out == out_centre it is sgld on centre_grad, with centre_grad = out_centre = 0 sgld on out, both bit for bit.
//          cv_accumulate: the mean over R launches behind centre_grad -- repeat r adds columns 0..4 of a record to the
//          accumulator (r = 0 stores), the last one divides once by R: a fixed order without atomics.
//   sgrld  SGMCMCSampler.sample_sgrld with LGSSMPreconditioner (sgmcmc_sampler.py:631-641, base_parameters.py:588-661,
//          models/lgssm.py:51-54), then project.  With theta = (A, C, LQinv, LRinv), Qinv = LQinv^2 + 1e-16,
//          Q = 1 / Qinv, g_v = d_v(theta, ghat) and every preconditioner term at the pre-step theta:
//            A     += eps (Q g_A / T)                          + sqrt(2 eps) (z_A / LQinv) sqrt(1 / T)
//            C     += eps (R g_C / T)                          + sqrt(2 eps) (z_C / LRinv) sqrt(1 / T)   (not taken: C = 1 after)
//            LQinv += eps ((0.5 Qinv g_LQinv) / T + LQinv / T) + sqrt(2 eps) (sqrt(0.5) LQinv z_Q) sqrt(1 / T)
//            LRinv += eps ((0.5 Rinv g_LRinv) / T + LRinv / T) + sqrt(2 eps) (sqrt(0.5) LRinv z_R) sqrt(1 / T)
//          (the LQinv / T, LRinv / T terms: correction_term, (n + 1) / 2 L with n = 1), on sgld's four normals.
//   gibbs  LGSSMPrior.sample_posterior (base_parameters.py:354-377, 437-450) from the statistics an FFBS window with
//          PFG_STAT_GIBBS left in out[0..7] (pfg_ffbs.hip), block by block: Qinv, Rinv (1 x 1 Wishart = scale chi2(df)),
//          A given Q, then project.  The C draw is skipped: the projection pins C to 1 whatever it drew.
//          chi2(df) = 2 Gamma(df / 2), Gamma by Marsaglia-Tsang (shape >= 1) or Gamma(a + 1) U^(1/a) (shape < 1).
//          A variable still rejected after kMaxRounds attempts is NaN.
//   pgibbs particle Gibbs (Andrieu, Doucet and Holenstein 2010): the same draw from the statistics the conditional SMC
//          sweep of pfg_csmc.hip left in out[0..7] -- one kernel serves both; a chain runs one of the two.  LGSSM: gibbs.
//          SVM: (Qinv, A) from out[0..2] with conjugate(df_Qinv, scale_Qinv, mean_A, var_col_A, ..., T - 1) and A | Q as
//          gibbs; Rinv = scale chi2(df), df = df_Rinv + T, scale = 1 / (1 / scale_Rinv + out[3]), out[3] = sum_t y_t^2
//          exp(-x_t) -- the emission law is y_t ~ N(0, R exp(x_t)) (svm/kernels.py:56-62, svm_logw) --, then project.
//          The transition sums run over t >= 1: the theta-dependence of x_0's law is left out of the conditional, as in
//          the reference's LGSSM Gibbs.
//   pmmh   particle marginal Metropolis-Hastings (Andrieu, Doucet and Holenstein 2010), two kernels around a particle
//          filter (or Kalman) launch that leaves its log-likelihood estimate in out[4]:
//            propose  theta'_j = theta_j + s_j z_j on the slots that move, s = scale, in the raw parameterisation; LGSSM's
//                     C' = 1 whatever s_C is.  Outside the support valid = 0 and theta' = theta, so the launch that
//                     follows never sees an illegal parameter vector.
//            accept   log alpha = (out[4] + logprior(theta')) - (ll_cur + logprior(theta)); finite: out[4] is.  ll_cur is
//                     NEVER refreshed for a chain that rejects: the estimate a chain was accepted with is part of its
//                     state, and that is what makes the chain exact for every N.
//          logprior is Prior.logprior (base_parameters.py) of the raw theta row without Jacobian terms and without the
//          terms that depend on the hyper-parameters only (they cancel in log alpha).
//   pmala  particle Metropolis-adjusted Langevin (Nemeth, Sherlock and Fearnhead 2016), two kernels around the SCORE
//          launch, which leaves the score estimate in out[0..3] and the log-likelihood estimate in out[4].  In pmmh's
//          coordinates and support:
//            propose  theta'_j = (theta_j + (0.5 (s_j s_j)) d_j(theta, grad_cur)) + s_j z_j; LGSSM's C stays 1 (no normal,
//                     no density term).  Outside the support valid = 0 and theta' = theta, as for pmmh.
//            accept   log q(b | a, g) = -sum_j (b_j - (a_j + (0.5 (s_j s_j)) d_j(a, g)))^2 / (2 (s_j s_j)) over the slots
//                     that move, and
//                       log alpha = (((out[4] + logprior(theta')) - (ll_cur + logprior(theta)))
//                                    + log q(theta | theta', out[0..3])) - log q(theta' | theta, grad_cur);
//                     finite: out[4] and every score column the drift uses are.  On accept theta = theta', ll_cur =
//                     out[4], grad_cur = out[0..3] verbatim (score-column order); a chain that rejects keeps theta, ll_cur
//                     AND grad_cur: neither estimate is ever refreshed, which is what makes the chain exact for every N
//                     (the pair (ll, g) is the auxiliary variable of the pseudo-marginal argument; the drift may be any
//                     function of (theta, g) as long as q is evaluated with the same one in both directions).
//          With (s_j s_j) / 2 = eps / T for every j the proposal is the law of sgld's step before project.
//   smc    the two chain-wise kernels of density-tempered SMC over PMMH chains (the population kernels: pfg_smc.hip).  With
//          q0 the product over the slots that move of N(m_j, s_j^2), log q0(theta) = sum_j -(theta_j - m_j)^2 / (2 s_j^2) -
//          log(s_j sqrt(2 pi)):
//            logtarget  h = (ll_cur + logprior(theta)) - log q0(theta), what a stage's weights exp(delta h) are made of
//            accept     pmmh's accept step on the target q0^(1 - phi) (exp(logprior) p-hat)^phi, phi read from device memory:
//                         log alpha = phi ((out[4] + logprior(theta')) - (ll_cur + logprior(theta)))
//                                     + (1 - phi) (log q0(theta') - log q0(theta))
//                       on pmmh's own uniform tag, with pmmh's commit.  At phi = 1 this is pmmh's log alpha exactly (1 x + 0 y =
//                       x for a finite y), so the decision is pmmh_accept_kernel's bit for bit.
// Built with -ffp-contract=off; IEEE division and ::sqrt / ::log throughout.
#include <initializer_list>

#include "pfg_chain_filter.hpp"

using namespace pfg_host;

namespace {

constexpr int kMaxRounds = 64;
constexpr uint32_t kTagNormals0 = 0x5A11u, kTagNormals1 = 0x5A12u;         // sgld, sghmc, sgrld
constexpr uint32_t kTagGibbs = 0x61B50000u;                                // | variable << 8 | attempt
constexpr uint32_t kTagPmmh = 0x504D0000u, kTagPmala = 0x4D4C0000u;        // | kNormals0, kNormals1, kUniform
constexpr uint32_t kNormals0 = 1u, kNormals1 = 2u, kUniform = 3u;

// ---- the key ----
using pfg::ChainKey;
using pfg::make_key;
using pfg::uniform53;
__device__ __forceinline__ pfg::u32x4 gibbs_draw(const ChainKey &key, uint32_t var, uint32_t attempt) {
    return key.draw_tag(kTagGibbs | (var << 8) | attempt);
}
__device__ __forceinline__ void normals4(const ChainKey &key, uint32_t tag0, uint32_t tag1, double *z) {
    const pfg::u32x4 r0 = key.draw_tag(tag0), r1 = key.draw_tag(tag1);
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(r0.x, r0.y, z[0], z[1]);
    mth.normal_pair(r1.x, r1.y, z[2], z[3]);
}

// ---- the drift ----
// grad_logprior of a Cholesky factor L of a 1 x 1 Wishart precision (covariance.py:272-284, n = 1) ...
__device__ __forceinline__ double chol_prior_grad(double L, double df, double scale) { return (df - 2.0) / L - L / scale; }
// ... and of the AR / emission coefficient x paired with the precision prec (matrices.py:597-607)
__device__ __forceinline__ double coef_prior_grad(double prec, double x, double mean, double var_col) { return -1.0 * (prec * (x - mean)) / var_col; }

// d = grad_logprior(th) + g in theta order (SVM's fourth slot: 0)
__device__ __forceinline__ void drift(int model, const double *th, const double *g, const pfg_prior_hyper &hy, double *d) {
    if (model == PFG_MODEL_GARCH) {
        const double mu = exp(th[0]), phi = 1.0 / (1.0 + exp(-th[1])), lam = 1.0 / (1.0 + exp(-th[2]));
        // garch_var.py:152-165; score columns [LR, log_mu, logit_phi, logit_lambduh]
        d[0] = (-hy.shape_mu - 1.0 + hy.scale_mu / mu) + g[1];
        d[1] = ((hy.alpha_phi - 1.0) / (1.0 + phi) - (hy.beta_phi - 1.0) / (1.0 - phi)) * phi * (1.0 - phi) + g[2];
        d[2] = ((hy.alpha_lambduh - 1.0) / (1.0 + lam) - (hy.beta_lambduh - 1.0) / (1.0 - lam)) * lam * (1.0 - lam) + g[3];
        d[3] = chol_prior_grad(th[3], hy.df_Rinv, hy.scale_Rinv) + g[0];
        return;
    }
    // score columns: SVM [LR, LQ, A]; LGSSM [LR, LQ, C, A]
    const bool lg = model == PFG_MODEL_LGSSM;
    const double A = th[0], LQ = lg ? th[2] : th[1], LR = lg ? th[3] : th[2];
    const double Qinv = LQ * LQ + 1e-16, Rinv = LR * LR + 1e-16;
    const double dA = coef_prior_grad(Qinv, A, hy.mean_A, hy.var_col_A) + (lg ? g[3] : g[2]);
    const double dLQ = chol_prior_grad(LQ, hy.df_Qinv, hy.scale_Qinv) + g[1];
    const double dLR = chol_prior_grad(LR, hy.df_Rinv, hy.scale_Rinv) + g[0];
    if (lg) {
        d[0] = dA; d[1] = coef_prior_grad(Rinv, th[1], hy.mean_C, hy.var_col_C) + g[2]; d[2] = dLQ; d[3] = dLR;
    } else {
        d[0] = dA; d[1] = dLQ; d[2] = dLR; d[3] = 0.0;
    }
}

// ---- the projection and the support ----
// project_parameters: |A| <= 0.9999 (_utils.py:165-170), a Cholesky factor reflected (covariance.py:68-80), LGSSM's C = 1
// (lgssm/parameters.py:39-42).  Stores the projection of p in th; SVM's fourth slot is not its own and stays.
__device__ __forceinline__ double clip_ar(double A) {
    const double aa = fabs(A);
    if (aa > 0.9999) A *= 0.9999 / aa;
    return A;
}
__device__ __forceinline__ double reflect_chol(double L) { return L < 0.0 ? sqrt(L * L + 1e-16) : L; }
__device__ __forceinline__ void project_store(int model, double *th, const double *p) {
    if (model == PFG_MODEL_GARCH) {
        th[0] = p[0]; th[1] = p[1]; th[2] = p[2]; th[3] = reflect_chol(p[3]);
    } else if (model == PFG_MODEL_LGSSM) {
        th[0] = clip_ar(p[0]); th[1] = 1.0; th[2] = reflect_chol(p[2]); th[3] = reflect_chol(p[3]);
    } else {
        th[0] = clip_ar(p[0]); th[1] = reflect_chol(p[1]); th[2] = reflect_chol(p[2]);
    }
}
// the slots of theta a proposal moves: SVM 0..2, LGSSM not C (slot 1), GARCH 0..3 ...
__device__ __forceinline__ bool moves(int model, int j) { return model == PFG_MODEL_SVM ? j < 3 : (model == PFG_MODEL_LGSSM ? j != 1 : true); }
// ... and the score columns its drift reads: SVM 0..2, LGSSM not C's (column 2), GARCH 0..3
__device__ __forceinline__ bool score_used(int model, int j) { return model == PFG_MODEL_SVM ? j < 3 : (model == PFG_MODEL_LGSSM ? j != 2 : true); }
__device__ __forceinline__ bool in_support(int model, const double *p) {
    auto chol = [](double L) { return L > 0.0 && L < INFINITY; };
    if (model == PFG_MODEL_GARCH) return fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY && chol(p[3]);
    const bool lg = model == PFG_MODEL_LGSSM;
    return fabs(p[0]) <= 0.9999 && chol(lg ? p[2] : p[1]) && chol(lg ? p[3] : p[2]);
}
// The end of a propose kernel: p's moved slots are the caller's; valid and theta' = p in the support, theta outside it
__device__ __forceinline__ void store_proposal(int model, const double *th, double *p, double *tp, int32_t *valid) {
    for (int j = 0; j < PFG_MAX_THETA; ++j)
        if (!moves(model, j)) p[j] = model == PFG_MODEL_LGSSM ? 1.0 : th[j];
    const bool ok = in_support(model, p);
    *valid = ok ? 1 : 0;
    for (int j = 0; j < PFG_MAX_THETA; ++j) tp[j] = ok ? p[j] : th[j];
}

// ---- the Metropolis step ----
// u of (key, tag); accepted iff ok (valid and finite estimates) and log(u) < log_alpha, false for a NaN.  An accepting chain
// takes theta', the proposal's estimate and a count; the caller commits what else it carries.
__device__ __forceinline__ bool metropolis(const ChainKey &key, uint32_t tag, bool ok, double log_alpha, double *th,
                                           const double *tp, double *ll_cur, double ll_prop, uint64_t *n_accept) {
    const pfg::u32x4 r = key.draw_tag(tag);
    const double u = uniform53(r.x, r.y);
    if (!(ok && ::log(u) < log_alpha)) return false;
    for (int j = 0; j < PFG_MAX_THETA; ++j) th[j] = tp[j];
    *ll_cur = ll_prop;
    *n_accept += 1;
    return true;
}

// ---- SGLD / SGHMC, SGRLD ----
// momentum == nullptr: SGLD.  Otherwise SGHMC with friction alpha: the increment of each
// variable becomes v <- (1 - alpha) v + drift + sqrt(alpha) * noise (noise ~ N(0, 2 eps / T)).
__global__ void sgld_update_kernel(int model, int B, double *__restrict__ theta,
                                   const double *__restrict__ outs, pfg_prior_hyper hy, double eps,
                                   double Tscale, uint64_t seed, uint64_t chain_offset,
                                   const uint64_t *step_ctr, double *__restrict__ momentum, double alpha) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    double z[4], d[PFG_MAX_THETA];
    normals4(make_key(seed, chain_offset, b, step_ctr), kTagNormals0, kTagNormals1, z);
    drift(model, th, outs + (size_t)b * PFG_OUT_DOUBLES, hy, d);
    const double nsd = sqrt(1.0 / Tscale) * sqrt(2.0 * eps) * (momentum ? sqrt(alpha) : 1.0);
    double *mv = momentum ? momentum + (size_t)b * PFG_MAX_THETA : nullptr;
    // slot j after its increment: SGLD drift + noise, or the SGHMC momentum recursion
    auto step = [&](int j) {
        double v = eps * (d[j] / Tscale) + nsd * z[j];
        if (mv) {
            v = (1.0 - alpha) * mv[j] + v;
            mv[j] = v;
        }
        return th[j] + v;
    };
    const double p[PFG_MAX_THETA] = {step(0), step(1), step(2), model == PFG_MODEL_SVM ? 0.0 : step(3)};      // SVM has three
    project_store(model, th, p);
}

// SGLD with control variates: g_k = centre_grad_k + (out_k - out_centre_k), in that operand order, then sgld_update_kernel's
// step without a momentum, operation for operation (the tests hold the two to each other bitwise).  It is written out in
// both: a shared helper changed sgld_update_kernel's instructions.
__global__ void sgld_cv_update_kernel(int model, int B, double *__restrict__ theta, const double *__restrict__ outs,
                                      const double *__restrict__ outs_centre, const double *__restrict__ centre_grad,
                                      pfg_prior_hyper hy, double eps, double Tscale, uint64_t seed, uint64_t chain_offset,
                                      const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    const double *o = outs + (size_t)b * PFG_OUT_DOUBLES, *oc = outs_centre + (size_t)b * PFG_OUT_DOUBLES;
    const double *cg = centre_grad + (size_t)b * PFG_MAX_THETA;
    double z[4], d[PFG_MAX_THETA], g[PFG_MAX_THETA];
    for (int k = 0; k < PFG_MAX_THETA; ++k) g[k] = cg[k] + (o[k] - oc[k]);
    normals4(make_key(seed, chain_offset, b, step_ctr), kTagNormals0, kTagNormals1, z);
    drift(model, th, g, hy, d);
    const double nsd = sqrt(1.0 / Tscale) * sqrt(2.0 * eps) * 1.0;
    auto step = [&](int j) { return th[j] + (eps * (d[j] / Tscale) + nsd * z[j]); };
    const double p[PFG_MAX_THETA] = {step(0), step(1), step(2), model == PFG_MODEL_SVM ? 0.0 : step(3)};      // SVM has three
    project_store(model, th, p);
}

// repeat r of R of the centring pass: acc[0..4] = (r == 0 ? out : acc + out), the last repeat divided by R
__global__ void cv_accumulate_kernel(int B, const double *__restrict__ outs, double *__restrict__ acc, int r, int R) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *o = outs + (size_t)b * PFG_OUT_DOUBLES;
    double *a = acc + (size_t)b * PFG_OUT_DOUBLES;
    for (int j = 0; j < 5; ++j) {
        double v = r == 0 ? o[j] : a[j] + o[j];
        if (r == R - 1) v = v / (double)R;
        a[j] = v;
    }
}

// ---- SGD, ADAGRAD ----
// moment == nullptr: SGD.  Otherwise ADAGRAD: G <- G + g g per slot, the increment g / sqrt(G + 1e-9).  No draws.
__global__ void optim_update_kernel(int model, int B, double *__restrict__ theta, const double *__restrict__ outs,
                                    pfg_prior_hyper hy, double eps, double Tscale, double *__restrict__ moment) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    double d[PFG_MAX_THETA];
    drift(model, th, outs + (size_t)b * PFG_OUT_DOUBLES, hy, d);
    double *G = moment ? moment + (size_t)b * PFG_MAX_THETA : nullptr;
    auto step = [&](int j) {
        double g = d[j] / Tscale;
        if (G) {
            const double Gj = G[j] + g * g;
            G[j] = Gj;
            g = g / sqrt(Gj + 1e-9);
        }
        return th[j] + eps * g;
    };
    const double p[PFG_MAX_THETA] = {step(0), step(1), step(2), model == PFG_MODEL_SVM ? 0.0 : step(3)};      // SVM has three
    project_store(model, th, p);
}

__global__ void bump_counter_kernel(uint64_t *ctr) { *ctr += 1; }

__global__ void sgrld_update_kernel(int B, double *__restrict__ theta, const double *__restrict__ outs, pfg_prior_hyper hy,
                                    double eps, double Tscale, uint64_t seed, uint64_t chain_offset,
                                    const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    double z[4], g[PFG_MAX_THETA];         // z[1], g[1]: C's step is not taken, the projection pins C to 1 whatever it would be
    normals4(make_key(seed, chain_offset, b, step_ctr), kTagNormals0, kTagNormals1, z);
    drift(PFG_MODEL_LGSSM, th, outs + (size_t)b * PFG_OUT_DOUBLES, hy, g);
    const double A = th[0], LQ = th[2], LR = th[3];
    const double Qinv = LQ * LQ + 1e-16, Rinv = LR * LR + 1e-16;
    const double Q = 1.0 / Qinv;
    const double scale = 1.0 / Tscale, nsd = sqrt(2.0 * eps), rs = sqrt(scale), half = sqrt(0.5);
    const double nA = (z[0] / LQ) * rs;
    const double nQ = ((half * LQ) * z[2]) * rs, nR = ((half * LR) * z[3]) * rs;
    const double p[PFG_MAX_THETA] = {A + (eps * ((Q * g[0]) * scale + 0.0) + nsd * nA), 1.0,
                                     LQ + (eps * (((0.5 * Qinv) * g[2]) * scale + LQ * scale) + nsd * nQ),
                                     LR + (eps * (((0.5 * Rinv) * g[3]) * scale + LR * scale) + nsd * nR)};
    project_store(PFG_MODEL_LGSSM, th, p);
}

// ---- Gibbs and particle Gibbs: the conjugate draw ----
// Gamma(shape, 1): Marsaglia & Tsang (2000) on (shape + 1 when shape < 1, then times U^(1 / shape)); NaN when every
// round is rejected or shape is not a positive number
__device__ double gamma_draw(const ChainKey &key, uint32_t var, double shape) {
    if (!(shape > 0.0) || !(shape < INFINITY)) return NAN;
    const bool boost = shape < 1.0;
    const double a = boost ? shape + 1.0 : shape;
    const double d = a - 1.0 / 3.0, c = 1.0 / ::sqrt(9.0 * d);
    const pfg::Math<double, false> mth = {};
    for (uint32_t k = 0; k < (uint32_t)kMaxRounds; ++k) {
        const pfg::u32x4 r = gibbs_draw(key, var, k);
        double z, unused;
        mth.normal_pair(r.x, r.y, z, unused);
        const double t = 1.0 + c * z;
        if (t <= 0.0) continue;
        const double v = t * t * t;
        const double u = uniform53(r.z, r.w);
        if (::log(u) < 0.5 * z * z + d - d * v + d * ::log(v)) {
            double x = d * v;
            if (boost) {
                const pfg::u32x4 s = gibbs_draw(key, var | 0x80u, 0);
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

// The parameter draw from the statistics of an FFBS path (gibbs: LGSSM) or of a conditional SMC path (pgibbs: LGSSM, SVM)
__global__ void pgibbs_update_kernel(int model, int B, double *__restrict__ theta, const double *__restrict__ outs,
                                     pfg_prior_hyper hy, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *s = outs + (size_t)b * PFG_OUT_DOUBLES;
    const ChainKey key = make_key(seed, chain_offset, b, step_ctr);
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
    const pfg::u32x4 ra = gibbs_draw(key, 2, 0);
    double zA, unused;
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(ra.x, ra.y, zA, unused);
    const double P = LQ * LQ + 1e-9;
    const double A = q.Scp / q.Spp + ::sqrt((1.0 / P) * (1.0 / q.Spp)) * zA;
    const double p[PFG_MAX_THETA] = {A, model == PFG_MODEL_LGSSM ? 1.0 : LQ, model == PFG_MODEL_LGSSM ? LQ : LR, LR};
    project_store(model, theta + (size_t)b * PFG_MAX_THETA, p);
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
    double z[4], p[PFG_MAX_THETA];
    normals4(make_key(seed, chain_offset, b, step_ctr), kTagPmmh | kNormals0, kTagPmmh | kNormals1, z);
    for (int j = 0; j < PFG_MAX_THETA; ++j)
        if (moves(model, j)) p[j] = th[j] + scale[j] * z[j];
    store_proposal(model, th, p, theta_prop + (size_t)b * PFG_MAX_THETA, valid + b);
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
    const double log_alpha = (ll_prop + logprior_value(model, tp, hy)) - (ll_cur[b] + logprior_value(model, th, hy));
    const bool finite = fabs(ll_prop) < INFINITY;        // false for a NaN as well
    metropolis(make_key(seed, chain_offset, b, step_ctr), kTagPmmh | kUniform, valid[b] != 0 && finite, log_alpha, th, tp,
               ll_cur + b, ll_prop, n_accept + b);
}

// ---- tempered SMC over PMMH chains: log q0, the log-target ratio, the tempered accept ----
__device__ __forceinline__ double log_q0(int model, const double *th, const double *mean, const double *sd) {
    double q = 0.0;
    for (int j = 0; j < PFG_MAX_THETA; ++j) {
        if (!moves(model, j)) continue;
        const double r = th[j] - mean[j];
        q = q + (-((r * r) / (2.0 * (sd[j] * sd[j]))) - ::log(sd[j] * 2.5066282746310002));      // sqrt(2 pi)
    }
    return q;
}

__global__ void smc_logtarget_kernel(int model, int B, const double *__restrict__ theta, const double *__restrict__ ll_cur,
                                     pfg_prior_hyper hy, const double *__restrict__ q0_mean, const double *__restrict__ q0_sd,
                                     double *__restrict__ h) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double *th = theta + (size_t)b * PFG_MAX_THETA;
    h[b] = (ll_cur[b] + logprior_value(model, th, hy)) - log_q0(model, th, q0_mean, q0_sd);
}

// pmmh_accept_kernel's step (never init) at the temperature *phi; log_alpha_out (may be NULL): every chain's log alpha
__global__ void smc_accept_kernel(int model, int B, double *__restrict__ theta, const double *__restrict__ theta_prop,
                                  const int32_t *__restrict__ valid, const double *__restrict__ outs,
                                  double *__restrict__ ll_cur, uint64_t *__restrict__ n_accept, pfg_prior_hyper hy,
                                  const double *__restrict__ q0_mean, const double *__restrict__ q0_sd,
                                  const double *__restrict__ phi, double *__restrict__ log_alpha_out, uint64_t seed,
                                  uint64_t chain_offset, const uint64_t *step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double ll_prop = outs[(size_t)b * PFG_OUT_DOUBLES + 4];
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    const double *tp = theta_prop + (size_t)b * PFG_MAX_THETA;
    const double f = *phi;
    const double d_post = (ll_prop + logprior_value(model, tp, hy)) - (ll_cur[b] + logprior_value(model, th, hy));
    const double d_q0 = log_q0(model, tp, q0_mean, q0_sd) - log_q0(model, th, q0_mean, q0_sd);
    const double log_alpha = f * d_post + (1.0 - f) * d_q0;
    if (log_alpha_out) log_alpha_out[b] = log_alpha;
    const bool finite = fabs(ll_prop) < INFINITY;        // false for a NaN as well
    metropolis(make_key(seed, chain_offset, b, step_ctr), kTagPmmh | kUniform, valid[b] != 0 && finite, log_alpha, th, tp,
               ll_cur + b, ll_prop, n_accept + b);
}

// ---- pMALA: the proposal's mean and log-density, propose, accept ----
// the mean of the proposal from a with drift d: a_j + (s_j^2 / 2) d_j
__device__ __forceinline__ double pmala_mean(double a, double s, double d) { return a + (0.5 * (s * s)) * d; }
// log q(b | a, g), d = d(a, g), less the constant of the scales
__device__ __forceinline__ double pmala_log_q(int model, const double *b, const double *a, const double *d, const double *s) {
    double q = 0.0;
    for (int j = 0; j < PFG_MAX_THETA; ++j) {
        if (!moves(model, j)) continue;
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
    double z[4], d[PFG_MAX_THETA], p[PFG_MAX_THETA];
    normals4(make_key(seed, chain_offset, b, step_ctr), kTagPmala | kNormals0, kTagPmala | kNormals1, z);
    drift(model, th, grad_cur + (size_t)b * PFG_MAX_THETA, hy, d);
    for (int j = 0; j < PFG_MAX_THETA; ++j)
        if (moves(model, j)) p[j] = pmala_mean(th[j], scale[j], d[j]) + scale[j] * z[j];
    store_proposal(model, th, p, theta_prop + (size_t)b * PFG_MAX_THETA, valid + b);
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
    drift(model, a, g, hy, da);
    drift(model, p, gp, hy, dp);
    const double q_fwd = pmala_log_q(model, p, a, da, s), q_rev = pmala_log_q(model, a, p, dp, s);
    const double log_alpha = (((ll_prop + logprior_value(model, p, hy)) - (ll_cur[b] + logprior_value(model, a, hy))) + q_rev) - q_fwd;
    bool finite = fabs(ll_prop) < INFINITY;              // false for a NaN as well
    for (int j = 0; j < PFG_MAX_THETA; ++j)
        if (score_used(model, j)) finite = finite && fabs(gp[j]) < INFINITY;
    if (metropolis(make_key(seed, chain_offset, b, step_ctr), kTagPmala | kUniform, valid[b] != 0 && finite, log_alpha, th, p,
                   ll_cur + b, ll_prop, n_accept + b))
        for (int j = 0; j < PFG_MAX_THETA; ++j) gc[j] = gp[j];
}

// ---- the entry points: one prologue, one epilogue ----
// What every entry point checks of its arguments (`what` names it): the context, the pointers it will use, the model id,
// the chain count.
int check_args(pfg_ctx *ctx, const char *what, int model, int B, std::initializer_list<const void *> pointers) {
    if (!ctx) return PFG_ERR_INVALID;
    for (const void *p : pointers)
        if (!p) return fail(ctx, PFG_ERR_INVALID, std::string(what) + ": NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (B < 0) return fail(ctx, PFG_ERR_INVALID, std::string(what) + ": B must be >= 0");
    return PFG_OK;
}
// ... and an update rule besides (B <= 0: no chains, not an error).  lgssm_only: how SGRLD and Gibbs refuse other models'
// chains (the reference's one preconditioner and conjugate prior).  The Gibbs rules have no step size: the defaults pass.
int check_update(pfg_ctx *ctx, const char *what, int model, const double *theta, const double *outs,
                 const pfg_prior_hyper *hyper, const char *lgssm_only = nullptr, double epsilon = 1.0, double Tscale = 1.0) {
    if (const int rc = check_args(ctx, what, model, 0, {theta, outs, hyper})) return rc;
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

int pfg_sgd_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs, const pfg_prior_hyper *hyper,
                          double epsilon, double Tscale, uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_update(ctx, __func__, model, theta, outs, hyper, nullptr, epsilon, Tscale)) return rc;
    return run_update(ctx, B, step_ctr, hip_stream, optim_update_kernel, model, B, theta, outs, *hyper, epsilon, Tscale,
                      (double *)nullptr);
}

int pfg_adagrad_update_device(pfg_ctx *ctx, int model, int B, double *theta, double *moment, const double *outs,
                              const pfg_prior_hyper *hyper, double epsilon, double Tscale, uint64_t *step_ctr,
                              void *hip_stream) {
    if (const int rc = check_update(ctx, __func__, model, theta, outs, hyper, nullptr, epsilon, Tscale)) return rc;
    if (!moment) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": NULL argument");
    return run_update(ctx, B, step_ctr, hip_stream, optim_update_kernel, model, B, theta, outs, *hyper, epsilon, Tscale, moment);
}

int pfg_sgld_cv_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs, const double *outs_centre,
                              const double *centre_grad, const pfg_prior_hyper *hyper, double epsilon, double Tscale,
                              uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_update(ctx, __func__, model, theta, outs, hyper, nullptr, epsilon, Tscale)) return rc;
    if (!outs_centre || !centre_grad) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": NULL argument");
    return run_update(ctx, B, step_ctr, hip_stream, sgld_cv_update_kernel, model, B, theta, outs, outs_centre, centre_grad,
                      *hyper, epsilon, Tscale, seed, chain_offset, (const uint64_t *)step_ctr);
}

int pfg_cv_accumulate_device(pfg_ctx *ctx, int B, const double *outs, double *acc, int repeat, int num_repeats,
                             uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_args(ctx, __func__, 0, B, {outs, acc})) return rc;
    if (num_repeats < 1 || repeat < 0 || repeat >= num_repeats)
        return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": need 0 <= repeat < num_repeats");
    return run_update(ctx, B, step_ctr, hip_stream, cv_accumulate_kernel, B, outs, acc, repeat, num_repeats);
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
    return run_update(ctx, B, step_ctr, hip_stream, pgibbs_update_kernel, (int)PFG_MODEL_LGSSM, B, theta, outs, *hyper, seed,
                      chain_offset, (const uint64_t *)step_ctr);
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

int pfg_logprior_device(pfg_ctx *ctx, int model, int B, const double *theta, const pfg_prior_hyper *hyper, double *logprior,
                        void *hip_stream) {
    if (const int rc = check_args(ctx, __func__, model, B, {theta, hyper, logprior})) return rc;
    return run_update(ctx, B, nullptr, hip_stream, logprior_kernel, model, B, theta, *hyper, logprior);
}

// (the propose steps do not bump: the accept step that closes a PMMH or pMALA step advances the counter, unless init)
int pfg_pmmh_propose_device(pfg_ctx *ctx, int model, int B, const double *theta, double *theta_prop, int32_t *valid,
                            const double *scale, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr,
                            void *hip_stream) {
    if (const int rc = check_args(ctx, __func__, model, B, {theta, theta_prop, valid, scale})) return rc;
    return run_update(ctx, B, nullptr, hip_stream, pmmh_propose_kernel, model, B, theta, theta_prop, valid, scale, seed,
                      chain_offset, step_ctr);
}

int pfg_pmmh_accept_device(pfg_ctx *ctx, int model, int B, double *theta, const double *theta_prop, const int32_t *valid,
                           const double *outs, double *ll_cur, uint64_t *n_accept, const pfg_prior_hyper *hyper, int init,
                           uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_args(ctx, __func__, model, B, {theta, theta_prop, valid, outs, ll_cur, n_accept, hyper})) return rc;
    return run_update(ctx, B, init ? nullptr : step_ctr, hip_stream, pmmh_accept_kernel, model, B, theta, theta_prop, valid,
                      outs, ll_cur, n_accept, *hyper, init, seed, chain_offset, (const uint64_t *)step_ctr);
}

int pfg_smc_logtarget_device(pfg_ctx *ctx, int model, int B, const double *theta, const double *ll_cur,
                             const pfg_prior_hyper *hyper, const double *q0_mean, const double *q0_sd, double *h,
                             void *hip_stream) {
    if (const int rc = check_args(ctx, __func__, model, B, {theta, ll_cur, hyper, q0_mean, q0_sd, h})) return rc;
    return run_update(ctx, B, nullptr, hip_stream, smc_logtarget_kernel, model, B, theta, ll_cur, *hyper, q0_mean, q0_sd, h);
}

int pfg_smc_accept_device(pfg_ctx *ctx, int model, int B, double *theta, const double *theta_prop, const int32_t *valid,
                          const double *outs, double *ll_cur, uint64_t *n_accept, const pfg_prior_hyper *hyper,
                          const double *q0_mean, const double *q0_sd, const double *phi, double *log_alpha, uint64_t seed,
                          uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_args(ctx, __func__, model, B, {theta, theta_prop, valid, outs, ll_cur, n_accept, hyper, q0_mean,
                                                            q0_sd, phi}))
        return rc;
    return run_update(ctx, B, step_ctr, hip_stream, smc_accept_kernel, model, B, theta, theta_prop, valid, outs, ll_cur,
                      n_accept, *hyper, q0_mean, q0_sd, phi, log_alpha, seed, chain_offset, (const uint64_t *)step_ctr);
}

int pfg_pmala_propose_device(pfg_ctx *ctx, int model, int B, const double *theta, const double *grad_cur, double *theta_prop,
                             int32_t *valid, const double *scale, const pfg_prior_hyper *hyper, uint64_t seed,
                             uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_args(ctx, __func__, model, B, {theta, grad_cur, theta_prop, valid, scale, hyper})) return rc;
    return run_update(ctx, B, nullptr, hip_stream, pmala_propose_kernel, model, B, theta, grad_cur, theta_prop, valid, scale,
                      *hyper, seed, chain_offset, step_ctr);
}

int pfg_pmala_accept_device(pfg_ctx *ctx, int model, int B, double *theta, const double *theta_prop, const int32_t *valid,
                            const double *outs, double *ll_cur, double *grad_cur, uint64_t *n_accept,
                            const pfg_prior_hyper *hyper, const double *scale, int init, uint64_t seed, uint64_t chain_offset,
                            uint64_t *step_ctr, void *hip_stream) {
    if (const int rc = check_args(ctx, __func__, model, B, {theta, theta_prop, valid, outs, ll_cur, grad_cur, n_accept, hyper, scale}))
        return rc;
    return run_update(ctx, B, init ? nullptr : step_ctr, hip_stream, pmala_accept_kernel, model, B, theta, theta_prop, valid,
                      outs, ll_cur, grad_cur, n_accept, *hyper, scale, init, seed, chain_offset, (const uint64_t *)step_ctr);
}
