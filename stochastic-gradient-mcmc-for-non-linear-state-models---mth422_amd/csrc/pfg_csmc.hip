// Conditional SMC with ancestor sampling (CSMC-AS; Andrieu, Doucet and Holenstein 2010, Lindsten, Jordan and Schon 2014):
// the path move of particle Gibbs for SVM and LGSSM.  EXTENSION: the reference has no path sampler for SVM.  One workgroup
// per chain, f64, N <= 1024: 64 threads x 2 particles (one wave: no s_barrier, see block_sync) for N <= 128, 256 x 4 above.
// Particle i = tid * PPT + k belongs to thread tid, slot k, so a thread's particles are neighbours in the CDF.
//   target   the law the filters and FFBS target: x_{-1} ~ N(prior_mean, prior_var) whatever theta, x_t | x_{t-1} ~ f_theta,
//            weight g_theta(y_t | x_t); proposal = the prior kernel, multinomial resampling at every step.
//   t = 0    particles 0 .. N-2 draw x_{-1}, then x_0 ~ f(. | x_{-1}); particle N-1 is x*_0; log-weight log g(y_0 | x_0).
//   t >= 1   LDS: the parents' states, the CDF of w_i = exp(lw_i - max lw) and, beside it, the CDF of the ancestor weights
//            v_i = exp((lw_i + ld_i) - max (lw + ld)), ld_i = log f(x*_t | x_{t-1}^i) less its constant (backward_log_ratio,
//            the PaRIS transition log-density).  A free particle searches the first CDF with u W (smallest j with cdf[j] >
//            u W, clamped to N-1), gathers x_{t-1}^j and takes particle_step; particle N-1 is x*_t and searches the second
//            CDF with its own uniform: ancestor sampling.
//   history  the states x_t^i (f64) then the parents a_t^i (u16; row 0 unused) go to the chain's HBM scratch, [T][N] each,
//            with vector stores; the parents also stay in LDS when T N <= 8192 entries.
//   path     k ~ W_{T-1}, then thread 0 traces back: x'_t = x_t^k, k = a_t^k, T dependent loads (LDS when the history is
//            there), writes x' over the chain's path and sums the record out[0..7] on the way: LGSSM the PFG_STAT_GIBBS
//            layout [sum_{t>=1} x_{t-1}^2, sum_{t>=1} x_t x_{t-1}, sum_{t>=1} x_t^2, sum_t x_t^2, sum_t y_t x_t, sum_t y_t^2,
//            T, 0]; SVM the same three transition sums, out[3] = sum_t y_t^2 exp(-x_t), out[4] = out[5] = 0, out[6] = T.
//   has_ref  0: all N particles are free -- a bootstrap filter with stored genealogy, the init pass; the path is not read.
//   degenerate  a weight sum or ancestor-weight sum that is zero or not finite: the chain keeps its path (the identity move
//            is invariant), the record is recomputed from it, *n_degenerate += 1; nothing is written to the path.  With
//            has_ref = 0 there is no path to keep: the record is NaN.  A descriptor that is invalid (a NULL array, T < 1, N
//            outside [2, the launch's shape], a prior variance that is not positive) gets a NaN record and the count too.
// Draws: Philox4x32-10 under key (seed_lo, seed_hi), counter {gid_lo, step_lo, t ^ (step_hi ^ gid_hi), tag}, gid =
// chain_offset + b, step = *step_ctr -- the chain key (pfg_chain_filter.hpp), drawn with the time step XORed into the third
// word and the particle in the tag:
//   0x43530000 | i  free particle i.  t = 0: normal_pair(r.x, r.y) -> the normals of x_{-1} and x_0;
//                   t >= 1: uniform53(r.x, r.y) -> its resampling uniform, normal_pair(r.z, r.w) -> z, the first: its state normal
//   0x43531000      uniform53(r.x, r.y) -> the ancestor-sampling uniform of step t
//   0x43532000      uniform53(r.x, r.y) -> the uniform of the final index k (t = T)
// Disjoint from every tag pfg_chains.hip lists.  TRACED (the twin a traced launch runs) records, when the pointers are set,
// every particle's parent, the reference particle's sampled ancestor, the normalised weights and k; the production
// instantiation does not read the trace pointers.  Built with -ffp-contract=off; ocml exp / log (no LDS tables).
#include "pfg_chain_filter.hpp"

using namespace pfg_host;

namespace {

constexpr uint32_t kTagParticle = 0x43530000u, kTagAncestor = 0x43531000u, kTagFinal = 0x43532000u;
constexpr int kHistEntries = 8192;      // parents kept in LDS: 16 KB

template <int MODEL, int NT, int PPT, bool TRACED>
__global__ __launch_bounds__(NT) void csmc_kernel(const pfg_csmc_problem *__restrict__ probs, uint64_t seed,
                                                  uint64_t chain_offset, const uint64_t *__restrict__ step_ctr) {
    constexpr int NMAX = NT * PPT, NW = NT / pfg::WAVE;
    __shared__ double xs[NMAX], cdf[NMAX], cdf2[NMAX];
    __shared__ double red_max[2][NW], red_sum[2][NW];
    __shared__ uint16_t hist[kHistEntries];

    const pfg_csmc_problem &P = probs[blockIdx.x];
    const int tid = threadIdx.x;
    const int T = P.T, N = P.N;
    const bool has_ref = P.has_ref != 0;
    const double prior_mean = P.prior_mean, prior_var = P.prior_var;
    if (!(pfg::chain_filter_usable(P, NMAX) && P.scratch && P.n_degenerate && P.path)) {
        if (tid < PFG_OUT_DOUBLES && P.out) P.out[tid] = NAN;
        if (tid == 0 && P.n_degenerate) *P.n_degenerate += 1;
        return;
    }
    const pfg::Consts<double> c = pfg::make_consts<MODEL, double>(P.theta);
    const pfg::Math<double, false> mth = {};
    const auto y = pfg::global_ptr(P.y);
    const auto ref = pfg::global_ptr(P.path);
    const auto sx = pfg::global_ptr(static_cast<double *>(P.scratch));
    const auto sa = pfg::global_ptr(reinterpret_cast<uint16_t *>(static_cast<double *>(P.scratch) + (size_t)T * N));
    const bool hist_lds = (size_t)T * N <= (size_t)kHistEntries;
    const pfg::ChainKey key = pfg::make_key(seed, chain_offset, (int)blockIdx.x, step_ctr);
    const int i0 = tid * PPT;
    const int ref_i = has_ref ? N - 1 : -1;      // the reference particle's index (none: every particle is free)
    const double sd0 = ::sqrt(prior_var);

    // ---- t = 0
    double x[PPT], lw[PPT];
    {
        const double y0 = y[0];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = i0 + k;
            x[k] = 0.0; lw[k] = -INFINITY;
            if (i >= N) continue;
            if (i == ref_i) {
                x[k] = ref[0];
                lw[k] = pfg::emission_logw<MODEL>(c, mth, x[k], y0);
            } else {
                const pfg::u32x4 r = key.draw_at(0, kTagParticle | (uint32_t)i);
                double za, zb, add[pfg::ModelDims<MODEL>::H];
                mth.normal_pair(r.x, r.y, za, zb);
                const double xm1 = prior_mean + sd0 * za;
                pfg::particle_step<MODEL, PFG_KERNEL_PRIOR, PFG_STAT_NONE>(c, mth, &xm1, y0, zb, &x[k], lw[k], add);
            }
            sx[i] = x[k];
        }
    }

    // ---- t = 1 .. T-1: resample, propagate; t = T: the weights of the last step and the final index
    bool degenerate = false;
    double Wlast = 0.0;
    for (int t = 1; t <= T; ++t) {
        const bool anc_step = has_ref && t < T;
        const double xstar = anc_step ? ref[t] : 0.0;
        // (A) the two maxima, one reduction
        double l2[PPT], m[2] = {-INFINITY, -INFINITY};
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            l2[k] = -INFINITY;
            if (i0 + k >= N) continue;
            m[0] = lw[k] > m[0] ? lw[k] : m[0];
            if (anc_step) {
                l2[k] = lw[k] + pfg::backward_log_ratio<MODEL>(c, mth, &x[k], &xstar);
                m[1] = l2[k] > m[1] ? l2[k] : m[1];
            }
        }
        pfg::block_max(red_max, m, anc_step);
        // (B) the two CDFs: a thread's running sums, one scan of the threads' totals
        double wv[PPT], cs[PPT], cv[PPT], run[2] = {0.0, 0.0}, off[2], tot[2];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const bool valid = i0 + k < N;
            wv[k] = valid ? mth.exp(lw[k] - m[0]) : 0.0;
            run[0] += wv[k];
            cs[k] = run[0];
            if (anc_step) run[1] += valid ? mth.exp(l2[k] - m[1]) : 0.0;
            cv[k] = run[1];
        }
        pfg::block_cdf(red_sum, run, off, tot, anc_step);
        const double W = tot[0], V = tot[1];
        // every thread holds the same W and V: the branch is uniform over the workgroup
        if (!(W > 0.0 && W < INFINITY) || (anc_step && !(V > 0.0 && V < INFINITY))) { degenerate = true; break; }
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = i0 + k;
            if (i >= N) continue;
            xs[i] = x[k];
            cdf[i] = cs[k] + off[0];
            if (anc_step) cdf2[i] = cv[k] + off[1];
            if (TRACED && P.trace_w) P.trace_w[(size_t)(t - 1) * N + i] = wv[k] / W;
        }
        pfg::block_sync<NW>();
        if (t == T) { Wlast = W; break; }
        // (C) parents, children
        const double yt = y[t];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = i0 + k;
            if (i >= N) continue;
            int j;
            double xn, lwn;
            if (i == ref_i) {
                const pfg::u32x4 r = key.draw_at(t, kTagAncestor);
                j = pfg::cdf_search(cdf2, N, pfg::uniform53(r.x, r.y) * V);
                xn = xstar;
                lwn = pfg::emission_logw<MODEL>(c, mth, xn, yt);
                if (TRACED && P.trace_ref_anc) P.trace_ref_anc[t] = j;
            } else {
                const pfg::u32x4 r = key.draw_at(t, kTagParticle | (uint32_t)i);
                j = pfg::cdf_search(cdf, N, pfg::uniform53(r.x, r.y) * W);
                const double xp = xs[j];
                double z, unused, add[pfg::ModelDims<MODEL>::H];
                mth.normal_pair(r.z, r.w, z, unused);
                pfg::particle_step<MODEL, PFG_KERNEL_PRIOR, PFG_STAT_NONE>(c, mth, &xp, yt, z, &xn, lwn, add);
            }
            x[k] = xn; lw[k] = lwn;
            sx[(size_t)t * N + i] = xn;
            sa[(size_t)t * N + i] = (uint16_t)j;
            if (hist_lds) hist[t * N + i] = (uint16_t)j;
            if (TRACED && P.trace_anc) P.trace_anc[(size_t)t * N + i] = j;
        }
        pfg::block_sync<NW>();       // the parents' states and both CDFs are free for the next step
    }

    // ---- the new path: thread 0 reads what the whole workgroup stored
    __threadfence_block();
    __syncthreads();
    if (tid != 0) return;
    double *out = P.out;
    if (degenerate) {
        *P.n_degenerate += 1;
        if (!has_ref) {
            for (int q = 0; q < PFG_OUT_DOUBLES; ++q) out[q] = NAN;
            return;
        }
    }
    int kk = 0;
    if (!degenerate) {
        const pfg::u32x4 r = key.draw_at(T, kTagFinal);
        kk = pfg::cdf_search(cdf, N, pfg::uniform53(r.x, r.y) * Wlast);
        if (TRACED && P.trace_k) P.trace_k[0] = kk;
    }
    // x'_t, t descending: the recorded lineage (written over the path), or the path the chain keeps
    auto state = [&](int t) -> double {
        if (degenerate) return ref[t];
        const double v = sx[(size_t)t * N + kk];
        if (t > 0) kk = hist_lds ? (int)hist[t * N + kk] : (int)sa[(size_t)t * N + kk];
        P.path[t] = v;
        return v;
    };
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto emission = [&](int t, double xt) {
        const double yt = y[t];
        if (MODEL == PFG_MODEL_SVM) {
            s[3] += (yt * yt) * ::exp(-xt);
        } else {
            s[3] += xt * xt;
            s[4] += yt * xt;
            s[5] += yt * yt;
        }
    };
    double xt = state(T - 1);
    emission(T - 1, xt);
    for (int t = T - 2; t >= 0; --t) {
        const double xp = state(t);
        s[0] += xp * xp;            // the transition of time t + 1
        s[1] += xt * xp;
        s[2] += xt * xt;
        emission(t, xp);
        xt = xp;
    }
    for (int q = 0; q < 6; ++q) out[q] = s[q];
    out[6] = (double)T;
    out[7] = 0.0;
}

}  // namespace

int64_t pfg_csmc_scratch_bytes(int T, int N) {
    if (!chain_filter_domain(T, N)) return -1;
    return round_up_256((int64_t)T * (int64_t)N * 10);          // states f64 [T][N], then parents u16 [T][N]
}

int pfg_csmc_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_csmc_problem *problems, uint64_t seed,
                    uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced) {
    const int rc = check_chain_filter_launch(ctx, __func__, "the conditional sweep is built for SVM and LGSSM (GARCH's prior has "
                                             "no conjugate draw to pair it with)", model, dtype, n_max, B, problems);
    if (rc != PFG_OK || B == 0) return rc;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    dispatch_chain_filter(model, traced != 0, n_max, [&](auto m, auto nt, auto ppt, auto tr) {
        hipLaunchKernelGGL((csmc_kernel<decltype(m)::value, decltype(nt)::value, decltype(ppt)::value, decltype(tr)::value>),
                           dim3((unsigned)B), dim3(decltype(nt)::value), 0, (hipStream_t)hip_stream, problems, seed, chain_offset,
                           step_ctr);
    });
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}
