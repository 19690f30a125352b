// The population kernels of SMC^2 over resident PMMH chains (Chopin, Jacob and Papaspiliopoulos 2013; Fulop and Li 2013): the
// B chains of an ensemble are one weighted population that takes the observations chunk by chunk.  Every chain carries its
// filter's particle system (one row: x [N][NS], then logw [N]); a stage extends every filter by the chunk (the ensemble's own
// warm-started launch), reweights the chains by the chunk's likelihood estimates and, when the ESS falls below the target,
// resamples ACROSS chains -- rows, theta and estimates by parent -- and moves them by PMMH on the prefix.  Here are the three
// kernels that see the population; the filter launches and the PMMH pair are the ensemble's, unchanged.  All f64, built with
// -ffp-contract=off, every result a pure function of the inputs and (seed, stage).
//   reweight one workgroup of 1024 threads, pfg_smc.hip's ownership (thread t owns the contiguous chains [t K, (t + 1) K),
//            K = ceil(B / 1024)) and its reductions (block_max / block_cdf of pfg_chain_filter.hpp for 16 waves):
//              v_i     = (logw_i - max logw) + incr_i           a logw or incr of -inf: a zero weight
//              incr    = v_max + log(sum e^(v_i - v_max) / sum e^(logw_i - max logw))
//              ESS     = (sum e^(v_i - v_max))^2 / sum e^(2 (v_i - v_max))
//              ESS < tau B:   parent of child r = the smallest j with cdf[j] > ((r + u) / B) W, B - 1 when there is none (cdf the
//                             running sum of e^(v - v_max) in chain order, W = cdf[B - 1]), logw = 0
//              otherwise:     parent = identity, logw = v - v_max
//              u       uniform53(r.x, r.y) of Philox4x32-10, counter {stage_lo, stage_hi, 0, 0x534D0001}, key seed ^ 0x534D4353:
//                      the temperature kernel's key
//            status: 1 no v is finite, 2 some logw or incr is NaN or +inf, 4 B is not in 2 .. 2^20; with a status other than 0
//            nothing but the status is stored.
//   gather   one workgroup of 256 threads per chain: row b of dst = row parent[b] of src, 16 bytes per lane and access, the
//            stores aligned (a scalar head and tail where a row does not start or end on 16 bytes); src and dst never alias,
//            so no order between rows is needed.  theta and the estimates go by parent as in tempering: the entry point ends
//            in pfg_smc_gather_device.
//   adopt    one workgroup per chain: a chain whose acceptance count moved since `seen` copies its row fresh -> cur and
//            takes the count -- cpm_commit_kernel's rule with a copy in place of the selector flip.
#include "pfg_chain_filter.hpp"
#include "pfg_seq_checks.hpp"

using namespace pfg_host;

namespace {

constexpr int kNT = 1024, kNW = kNT / pfg::WAVE;
constexpr int kMinB = pfg_seq::kMinB, kMaxB = pfg_seq::kMaxB;
constexpr int kRowNT = 256;
constexpr uint32_t kTagSmc = 0x534D0001u;
constexpr uint64_t kSeedSmc = 0x534D4353ull;

__global__ __launch_bounds__(kNT) void seq_reweight_kernel(int B, double *logw, const double *__restrict__ incr, int64_t stride,
                                                           double tau, uint64_t seed, uint64_t stage, double *__restrict__ record,
                                                           int32_t *__restrict__ status, int32_t *__restrict__ parent,
                                                           double *cdf) {
    __shared__ double red_m[2][kNW], red_v[1][kNW], red_s[3][kNW], w_sh;
    const int tid = threadIdx.x;
    if (B < kMinB || B > kMaxB) {                // (uniform; no array is read)
        if (tid == 0) *status = 4;
        return;
    }
    const int K = (B + kNT - 1) / kNT;
    const int i0 = tid * K < B ? tid * K : B, i1 = i0 + K < B ? i0 + K : B;     // (a thread past the population: i0 = i1 = B)

    // the maximum of logw, and whether any logw or incr is NaN or +inf (a NaN never wins a comparison: it is counted apart)
    double m[2] = {-INFINITY, 0.0};
    for (int i = i0; i < i1; ++i) {
        const double l = logw[i], a = incr[(int64_t)i * stride];
        if (l != l || l == INFINITY || a != a || a == INFINITY) m[1] = 1.0;
        else m[0] = l > m[0] ? l : m[0];
    }
    pfg::block_max<kNW, 2>(red_m, m);
    const double lmax = m[0];
    if (m[1] != 0.0 || lmax == -INFINITY) {
        if (tid == 0) *status = m[1] != 0.0 ? 2 : 1;
        return;
    }
    auto value = [&](int i) {
        const double l = logw[i], a = incr[(int64_t)i * stride];
        return l == -INFINITY || a == -INFINITY ? -INFINITY : (l - lmax) + a;
    };
    double vm[1] = {-INFINITY};
    for (int i = i0; i < i1; ++i) {
        const double v = value(i);
        vm[0] = v > vm[0] ? v : vm[0];
    }
    pfg::block_max<kNW, 1>(red_v, vm);
    const double vmax = vm[0];
    if (vmax == -INFINITY) {
        if (tid == 0) *status = 1;
        return;
    }

    // sum e^(v - vmax) with its running values in chain order (the CDF), sum e^(2 (v - vmax)), sum e^(logw - lmax)
    double run[3] = {0.0, 0.0, 0.0}, off[3], tot[3];
    for (int i = i0; i < i1; ++i) {
        const double v = value(i), l = logw[i];
        const double w = v == -INFINITY ? 0.0 : ::exp(v - vmax);
        run[0] += w;
        run[1] += w * w;
        run[2] += l == -INFINITY ? 0.0 : ::exp(l - lmax);
        cdf[i] = run[0];
    }
    pfg::block_cdf<kNW, 3>(red_s, run, off, tot);
    const double ess = (tot[0] * tot[0]) / tot[1];
    const bool resample = ess < tau * (double)B;
    const pfg::u32x4 r4 = pfg::philox4x32_10({(uint32_t)stage, (uint32_t)(stage >> 32), 0u, kTagSmc},
                                             (uint32_t)(seed ^ kSeedSmc), (uint32_t)((seed ^ kSeedSmc) >> 32));
    const double u = pfg::uniform53(r4.x, r4.y);
    double W = tot[0];
    if (resample) {
        for (int i = i0; i < i1; ++i) {
            const double c = off[0] + cdf[i];
            cdf[i] = c;
            if (i == B - 1) w_sh = c;
        }
        pfg::block_sync<kNW>();          // the CDF (global memory, one workgroup) and W before the searches
        W = w_sh;
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
            logw[r] = 0.0;
        }
    } else {
        for (int i = i0; i < i1; ++i) {
            const double v = value(i);          // (its own logw[i] is still the old one: a thread writes only what it owns)
            parent[i] = i;
            logw[i] = v == -INFINITY ? -INFINITY : v - vmax;
        }
    }
    if (tid == 0) {
        record[0] = vmax + ::log(tot[0] / tot[2]);
        record[1] = ess;
        record[2] = resample ? 1.0 : 0.0;
        record[3] = u;
        record[4] = vmax;
        record[5] = W;
        record[6] = lmax;
        record[7] = 0.0;
        *status = 0;
    }
}

// a pair of doubles wherever 8 bytes are aligned: a row of odd length puts every second row of src off 16 bytes
struct __attribute__((aligned(8))) pair8 { double a, b; };

// dst[0 .. n) = src[0 .. n) by the workgroup: the stores 16-byte aligned, one scalar head and tail where dst needs them
__device__ __forceinline__ void copy_row(double *__restrict__ dst, const double *__restrict__ src, int64_t n) {
    const int64_t head = (((uintptr_t)dst >> 3) & 1) && n > 0 ? 1 : 0;
    const int64_t pairs = (n - head) >> 1;
    if (threadIdx.x == 0 && head) dst[0] = src[0];
    const pair8 *s2 = (const pair8 *)(src + head);
    double2 *d2 = (double2 *)(dst + head);
    int64_t q = threadIdx.x;
    for (; q + 3 * kRowNT < pairs; q += 4 * kRowNT) {           // four loads in flight per lane before the first store
        const pair8 v0 = s2[q], v1 = s2[q + kRowNT], v2 = s2[q + 2 * kRowNT], v3 = s2[q + 3 * kRowNT];
        d2[q] = make_double2(v0.a, v0.b);
        d2[q + kRowNT] = make_double2(v1.a, v1.b);
        d2[q + 2 * kRowNT] = make_double2(v2.a, v2.b);
        d2[q + 3 * kRowNT] = make_double2(v3.a, v3.b);
    }
    for (; q < pairs; q += kRowNT) {
        const pair8 v = s2[q];
        d2[q] = make_double2(v.a, v.b);
    }
    const int64_t done = head + 2 * pairs;
    if (threadIdx.x == 0 && done < n) dst[done] = src[done];
}

__global__ __launch_bounds__(kRowNT) void seq_gather_kernel(int B, const int32_t *__restrict__ parent, int64_t row,
                                                            const double *__restrict__ src, double *__restrict__ dst) {
    const int b = blockIdx.x;
    int p = parent[b];
    if (p < 0 || p >= B) p = b;         // (never with parents of seq_reweight_kernel: no read outside the arrays whatever comes)
    copy_row(dst + (size_t)b * row, src + (size_t)p * row, row);
}

__global__ __launch_bounds__(kRowNT) void seq_adopt_kernel(const uint64_t *__restrict__ n_accept, uint64_t *seen, int64_t row,
                                                           double *__restrict__ cur, const double *__restrict__ fresh) {
    const int b = blockIdx.x;
    const uint64_t n = n_accept[b];
    const bool moved = n != seen[b];            // uniform over the workgroup
    __syncthreads();                            // every thread has read seen[b] before thread 0 stores it
    if (!moved) return;
    copy_row(cur + (size_t)b * row, fresh + (size_t)b * row, row);
    if (threadIdx.x == 0) seen[b] = n;
}

}  // namespace

namespace {

int refuse(pfg_ctx *ctx, const char *what, int clause, int B, int64_t row_doubles) {
    const std::string who = std::string(what) + ": ";
    switch (clause) {
    case pfg_seq::BAD_B: return fail(ctx, PFG_ERR_INVALID, who + "a population is 2 <= B <= 2^20 chains, got " + std::to_string(B));
    case pfg_seq::BAD_ROW: return fail(ctx, PFG_ERR_INVALID, who + "row_doubles must be >= 1 and B * row_doubles <= 2^40, got " +
                                                                 std::to_string(row_doubles));
    case pfg_seq::NULL_ARGUMENT: return fail(ctx, PFG_ERR_INVALID, who + "NULL argument");
    case pfg_seq::ALIAS: return fail(ctx, PFG_ERR_INVALID, who + "the two row arrays must not alias");
    case pfg_seq::BAD_STRIDE: return fail(ctx, PFG_ERR_INVALID, who + "incr_stride must be >= 0");
    case pfg_seq::BAD_TARGET: return fail(ctx, PFG_ERR_INVALID, who + "ess_target must lie in (0, 1]");
    }
    return PFG_OK;
}

}  // namespace

int pfg_seq_reweight_device(pfg_ctx *ctx, int B, double *logw, const double *incr, int64_t incr_stride, double ess_target,
                            uint64_t seed, uint64_t stage, double *record, int32_t *status, int32_t *parent, void *scratch,
                            void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    const void *pointers[] = {logw, incr, record, status, parent, scratch};
    if (const int clause = pfg_seq::check_reweight(incr_stride, ess_target, pointers, 6)) return refuse(ctx, __func__, clause, B, 0);
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    // (a B outside 2 .. 2^20 is the kernel's to report: status 4 and no other access)
    hipLaunchKernelGGL(seq_reweight_kernel, dim3(1), dim3(kNT), 0, (hipStream_t)hip_stream, B, logw, incr, incr_stride, ess_target,
                       seed, stage, record, status, parent, (double *)scratch);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

int pfg_seq_gather_device(pfg_ctx *ctx, int B, const int32_t *parent, int64_t row_doubles, const double *src, double *dst,
                          double *theta, double *theta_tmp, double *ll, double *ll_tmp, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    const void *pointers[] = {parent, src, dst, theta, theta_tmp, ll, ll_tmp};
    if (const int clause = pfg_seq::check_rows(B, row_doubles, pointers, 7, src, dst)) return refuse(ctx, __func__, clause, B, row_doubles);
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(seq_gather_kernel, dim3(B), dim3(kRowNT), 0, (hipStream_t)hip_stream, B, parent, row_doubles, src, dst);
    PFG_HIP(ctx, hipGetLastError());
    return pfg_smc_gather_device(ctx, B, parent, theta, ll, theta_tmp, ll_tmp, hip_stream);       // theta and ll: tempering's
}

int pfg_seq_adopt_device(pfg_ctx *ctx, int B, const uint64_t *n_accept, uint64_t *seen, int64_t row_doubles, double *cur,
                         const double *fresh, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    const void *pointers[] = {n_accept, seen, cur, fresh};
    if (const int clause = pfg_seq::check_rows(B, row_doubles, pointers, 4, cur, fresh)) return refuse(ctx, __func__, clause, B, row_doubles);
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(seq_adopt_kernel, dim3(B), dim3(kRowNT), 0, (hipStream_t)hip_stream, n_accept, seen, row_doubles, cur, fresh);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}
