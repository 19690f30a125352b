// The population kernels of density-tempered SMC over resident PMMH chains (Del Moral, Doucet and Jasra 2006; Duan and Fulop
// 2015): the B chains of an ensemble are one interacting population that a stage reweights, resamples ACROSS chains and
// moves.  The moves are the ensemble's own launches closed by the tempered accept step of pfg_chains.hip, which also
// computes h; here are the three kernels that see the whole population.  All f64, built with -ffp-contract=off, every result
// a pure function of the inputs and (seed, stage).
//   temper   one workgroup of 1024 threads (16 waves): the population is 2 .. 2^20 numbers and the search some 60 dependent
//            reductions, each a few exp per thread -- a barrier across workgroups per round would cost more than the
//            arithmetic.  Thread t owns the contiguous chains [t K, (t + 1) K), K = ceil(B / 1024), so its partial sums are
//            neighbours in the CDF; maxima, sums and CDF offsets are block_max / block_cdf of pfg_chain_filter.hpp for 16
//            waves.  Every thread holds the same phi, delta and sums: every branch is uniform over the workgroup.
//              w_i(d)  = exp(d (h_i - h_max)), 0 for h_i = -inf          ESS(d) = (sum w_i)^2 / sum w_i^2
//              delta   = 1 - phi if ESS(1 - phi) >= tau B (the last stage: phi' = 1 exactly), otherwise the lower end of 60
//                        rounds of bisection on [0, 1 - phi] (ESS(delta) >= tau B always holds); phi' = phi + delta
//              incr    = delta h_max + log(W / B), W = cdf[B - 1], cdf the running sum of w(delta) in chain order
//              parent  child r takes the smallest j with cdf[j] > ((r + u) / B) W, B - 1 when there is none (cdf_search)
//              u       uniform53(r.x, r.y) of Philox4x32-10, counter {stage_lo, stage_hi, 0, 0x534D0001}, key seed ^ 0x534D4353
//            status: 1 no h is finite, 2 some h is NaN or +inf, 4 delta ended at exactly 0, 8 phi is not in [0, 1); with a
//            status other than 0 nothing but the status is stored.
//   gather   theta rows and the estimates by parent into a second pair of arrays, then back (two launches on one stream: a
//            row may be the parent of a child in any other workgroup).
//   scale    one workgroup of 1024 threads, the same ownership: per theta slot the mean, then the variance about it (two
//            passes, each summed in the fixed order of block_cdf), sd_j = sqrt(sum (x - mean)^2 / B); scale[j] = c sd_j for a
//            slot the caller names (bit j of `slots`: those its proposal moves), unless sd_j is 0 or not finite: then, and
//            for every other slot, scale[j] stays.
#include "pfg_chain_filter.hpp"

using namespace pfg_host;

namespace {

constexpr int kNT = 1024, kNW = kNT / pfg::WAVE;
constexpr int kMinB = 2, kMaxB = 1 << 20;
constexpr int kBisections = 60;
constexpr uint32_t kTagSmc = 0x534D0001u;
constexpr uint64_t kSeedSmc = 0x534D4353ull;

__global__ __launch_bounds__(kNT) void smc_temper_kernel(int B, const double *__restrict__ h, double *phi_io, double tau,
                                                         uint64_t seed, uint64_t stage, double *__restrict__ result,
                                                         int32_t *__restrict__ status, int32_t *__restrict__ parent,
                                                         double *cdf) {
    // red_s is double-buffered by the round's parity: a wave one round ahead writes the other half, and it cannot be two
    // ahead, since the barrier of the round between needs every wave to have read this one
    __shared__ double red_m[2][kNW], red_s[2][2][kNW], w_sh;
    const int tid = threadIdx.x;
    const int K = (B + kNT - 1) / kNT;
    const int i0 = tid * K < B ? tid * K : B, i1 = i0 + K < B ? i0 + K : B;     // (a thread past the population: i0 = i1 = B)
    const double phi = *phi_io;

    // the maximum, and whether any h is NaN or +inf (a NaN never wins a comparison: it is counted apart)
    double m[2] = {-INFINITY, 0.0};
    for (int i = i0; i < i1; ++i) {
        const double v = h[i];
        if (v != v || v == INFINITY) m[1] = 1.0;
        else m[0] = v > m[0] ? v : m[0];
    }
    pfg::block_max<kNW, 2>(red_m, m);
    const double hmax = m[0];
    int bad = 0;
    if (!(phi >= 0.0 && phi < 1.0)) bad |= 8;
    if (m[1] != 0.0) bad |= 2;
    else if (hmax == -INFINITY) bad |= 1;
    if (bad) {
        if (tid == 0) *status = bad;
        return;
    }

    auto weight = [&](double d, double v) { return v == -INFINITY ? 0.0 : ::exp(d * (v - hmax)); };
    int parity = 0;
    // sum w and sum w^2 at d, the same in every thread
    auto sums = [&](double d, double &s1, double &s2) {
        double run[2] = {0.0, 0.0}, off[2], tot[2];
        for (int i = i0; i < i1; ++i) {
            const double w = weight(d, h[i]);
            run[0] += w;
            run[1] += w * w;
        }
        pfg::block_cdf<kNW, 2>(red_s[parity], run, off, tot);
        parity ^= 1;
        s1 = tot[0];
        s2 = tot[1];
    };
    const double want = tau * (double)B, rest = 1.0 - phi;
    double s1, s2, delta = rest;
    sums(rest, s1, s2);
    const bool last = (s1 * s1) / s2 >= want;
    if (!last) {
        double lo = 0.0, hi = rest;
        for (int k = 0; k < kBisections; ++k) {
            const double mid = 0.5 * (lo + hi);
            sums(mid, s1, s2);
            if ((s1 * s1) / s2 >= want) lo = mid; else hi = mid;
        }
        delta = lo;
    }
    if (delta == 0.0) {
        if (tid == 0) *status = 4;
        return;
    }

    // the CDF at delta in chain order: a thread's running sums, then the offset of the threads before it
    double run[2] = {0.0, 0.0}, off[2], tot[2];
    for (int i = i0; i < i1; ++i) {
        const double w = weight(delta, h[i]);
        run[0] += w;
        run[1] += w * w;
        cdf[i] = run[0];
    }
    pfg::block_cdf<kNW, 2>(red_s[parity], run, off, tot);
    for (int i = i0; i < i1; ++i) {
        const double c = off[0] + cdf[i];
        cdf[i] = c;
        if (i == B - 1) w_sh = c;
    }
    pfg::block_sync<kNW>();          // the CDF (global memory, one workgroup) and W before the searches
    const double W = w_sh;
    const pfg::u32x4 r4 = pfg::philox4x32_10({(uint32_t)stage, (uint32_t)(stage >> 32), 0u, kTagSmc},
                                             (uint32_t)(seed ^ kSeedSmc), (uint32_t)((seed ^ kSeedSmc) >> 32));
    const double u = pfg::uniform53(r4.x, r4.y);
    // a thread's children are neighbours and their targets ascend: the answer of one search bounds the next from below
    int j = 0;
    for (int r = i0; r < i1; ++r) {
        const double target = (((double)r + u) / (double)B) * W;
        if (r == i0) {
            j = pfg::cdf_search(cdf, B, target);
        } else {
            int probes = 0;
            while (probes < 3 && j < B - 1 && !(cdf[j] > target)) { ++j; ++probes; }
            if (j < B - 1 && !(cdf[j] > target)) j = pfg::cdf_search(cdf, B, target, j + 1);
        }
        parent[r] = j;
    }
    if (tid == 0) {
        const double phi_new = last ? 1.0 : phi + delta;
        result[0] = phi_new;
        result[1] = delta;
        result[2] = delta * hmax + ::log(W / (double)B);
        result[3] = (tot[0] * tot[0]) / tot[1];
        result[4] = u;
        result[5] = W;
        result[6] = hmax;
        result[7] = 0.0;
        *phi_io = phi_new;
        *status = 0;
    }
}

__global__ void smc_gather_kernel(int B, const int32_t *__restrict__ parent, const double *__restrict__ theta,
                                  const double *__restrict__ ll, double *__restrict__ theta_to, double *__restrict__ ll_to) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int p = parent[b];
    if (p < 0 || p >= B) p = b;         // (never with parents of smc_temper_kernel: no read outside the arrays whatever comes)
    for (int j = 0; j < PFG_MAX_THETA; ++j) theta_to[(size_t)b * PFG_MAX_THETA + j] = theta[(size_t)p * PFG_MAX_THETA + j];
    ll_to[b] = ll[p];
}

__global__ void smc_copy_kernel(int B, const double *__restrict__ theta, const double *__restrict__ ll,
                                double *__restrict__ theta_to, double *__restrict__ ll_to) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    for (int j = 0; j < PFG_MAX_THETA; ++j) theta_to[(size_t)b * PFG_MAX_THETA + j] = theta[(size_t)b * PFG_MAX_THETA + j];
    ll_to[b] = ll[b];
}

// slots: bit j set = theta slot j takes a new scale (the caller names the slots its proposal moves)
__global__ __launch_bounds__(kNT) void smc_scale_kernel(int B, const double *__restrict__ theta, uint32_t slots, double c,
                                                        double *__restrict__ scale) {
    __shared__ double red_a[PFG_MAX_THETA][kNW], red_b[PFG_MAX_THETA][kNW];
    const int tid = threadIdx.x;
    const int K = (B + kNT - 1) / kNT;
    const int i0 = tid * K < B ? tid * K : B, i1 = i0 + K < B ? i0 + K : B;
    double run[PFG_MAX_THETA], off[PFG_MAX_THETA], tot[PFG_MAX_THETA], mean[PFG_MAX_THETA];
    for (int j = 0; j < PFG_MAX_THETA; ++j) run[j] = 0.0;
    for (int i = i0; i < i1; ++i)
        for (int j = 0; j < PFG_MAX_THETA; ++j) run[j] += theta[(size_t)i * PFG_MAX_THETA + j];
    pfg::block_cdf<kNW, PFG_MAX_THETA>(red_a, run, off, tot);
    for (int j = 0; j < PFG_MAX_THETA; ++j) { mean[j] = tot[j] / (double)B; run[j] = 0.0; }
    for (int i = i0; i < i1; ++i)
        for (int j = 0; j < PFG_MAX_THETA; ++j) {
            const double d = theta[(size_t)i * PFG_MAX_THETA + j] - mean[j];
            run[j] += d * d;
        }
    pfg::block_cdf<kNW, PFG_MAX_THETA>(red_b, run, off, tot);
    if (tid < PFG_MAX_THETA && ((slots >> tid) & 1u)) {
        const double sd = ::sqrt(tot[tid] / (double)B);
        if (sd > 0.0 && sd < INFINITY) scale[tid] = c * sd;
    }
}

int check_population(pfg_ctx *ctx, const char *what, int B, std::initializer_list<const void *> pointers) {
    if (!ctx) return PFG_ERR_INVALID;
    if (B < kMinB || B > kMaxB)
        return fail(ctx, PFG_ERR_INVALID, std::string(what) + ": a population is 2 <= B <= 2^20 chains, got " + std::to_string(B));
    for (const void *p : pointers)
        if (!p) return fail(ctx, PFG_ERR_INVALID, std::string(what) + ": NULL argument");
    return PFG_OK;
}

}  // namespace

int64_t pfg_smc_scratch_bytes(int B) {
    if (B < kMinB || B > kMaxB) return -1;
    return round_up_256((int64_t)B * 8);            // the CDF [B] f64
}

int pfg_smc_temper_device(pfg_ctx *ctx, int B, const double *h, double *phi, double ess_target, uint64_t seed, uint64_t stage,
                          double *result, int32_t *status, int32_t *parent, void *scratch, void *hip_stream) {
    if (const int rc = check_population(ctx, __func__, B, {h, phi, result, status, parent, scratch})) return rc;
    if (!(ess_target > 0.0 && ess_target < 1.0))
        return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": ess_target must lie in (0, 1)");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(smc_temper_kernel, dim3(1), dim3(kNT), 0, (hipStream_t)hip_stream, B, h, phi, ess_target, seed, stage,
                       result, status, parent, (double *)scratch);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

int pfg_smc_gather_device(pfg_ctx *ctx, int B, const int32_t *parent, double *theta, double *ll, double *theta_tmp,
                          double *ll_tmp, void *hip_stream) {
    if (const int rc = check_population(ctx, __func__, B, {parent, theta, ll, theta_tmp, ll_tmp})) return rc;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid((B + 127) / 128), block(128);
    hipLaunchKernelGGL(smc_gather_kernel, grid, block, 0, (hipStream_t)hip_stream, B, parent, (const double *)theta,
                       (const double *)ll, theta_tmp, ll_tmp);
    hipLaunchKernelGGL(smc_copy_kernel, grid, block, 0, (hipStream_t)hip_stream, B, (const double *)theta_tmp,
                       (const double *)ll_tmp, theta, ll);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

int pfg_smc_scale_device(pfg_ctx *ctx, int B, const double *theta, uint32_t slots, double factor, double *scale,
                         void *hip_stream) {
    if (const int rc = check_population(ctx, __func__, B, {theta, scale})) return rc;
    if (slots >> PFG_MAX_THETA) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": slots names a slot past PFG_MAX_THETA");
    if (!(factor > 0.0 && factor < INFINITY)) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": factor must be > 0");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(smc_scale_kernel, dim3(1), dim3(kNT), 0, (hipStream_t)hip_stream, B, theta, slots, factor, scale);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}
