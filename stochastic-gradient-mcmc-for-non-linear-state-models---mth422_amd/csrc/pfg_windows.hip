// The windows of resident chains: one per chain and step, or several -- the reference's minibatch_size windows in each of
// num_sequences sequences (sgmcmc_sampler.py:390-425, 1249-1283), for ChainEnsemble(minibatch_size=..., num_sequences=...).
//   sample_windows_kernel        one lane per chain: the chain's one window of S steps in a series of T.
//   sample_windows_multi_kernel  one wave per chain: choose the chain's sequences (num_sequences = K distinct ones in
//                                random order, or all of them in index order), then write the W = K_eff M window
//                                descriptors of the chain, window w = k M + m being the m-th window in the k-th chosen
//                                sequence, and each window's sequence length.  Keyed draws (see pfgrad.h).
//   reduce_windows_kernel        one lane per chain: the W window records -> one record, in the reference's order of
//                                operations (within a sequence, across sequences, then the T_total / S rescaling).
// The two samplers' Philox counter and key layouts differ and both are pinned by the tests' host mirror: each stays as it
// is.  The start draw and the clamped descriptor are written out in both: shared helpers changed their instructions.
// None is on the critical path: the particle filter of the C W windows is.  Built with -ffp-contract=off, so the
// reduction is the exact sequence of IEEE operations the reference's loops perform.
#include "pfg_host.hpp"
#include "pfg_math.hpp"

using namespace pfg_host;

namespace {

constexpr int kSampleNT = 64;
constexpr int kReduceNT = 128;
constexpr int kReduceCols = 5;      // out[0..3] score columns, out[4] log-likelihood
constexpr uint32_t kSeqTag = 0x53000000u, kWinTag = 0x57000000u;    // "S": sequence draw j, "W": window w (< 2^24)

__global__ void sample_windows_kernel(int B, pfg_dev_problem *__restrict__ probs, const double *__restrict__ y,
                                      const double *__restrict__ wtab, int T, int S, int buffer, int strict,
                                      uint64_t seed, uint64_t chain_offset, const uint64_t *__restrict__ step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint64_t chain = chain_offset + (uint64_t)b, ctr = step_ctr ? *step_ctr : 0ull;
    const pfg::u32x4 r = pfg::philox4x32_10({(uint32_t)chain, (uint32_t)(chain >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32)},
                                            (uint32_t)seed ^ 0x57494E44u, (uint32_t)(seed >> 32));   // "WIND"
    const uint32_t range = strict ? (uint32_t)(T / S) : (uint32_t)(T - S + 1);
    // 64 random bits times the range, high part: bias < range / 2^64
    const uint64_t bits = ((uint64_t)r.x << 32) | r.y;
    const int idx = (int)__umul64hi(bits, (uint64_t)range);
    const int start = strict ? idx * S : idx;
    // in 64 bits: start + S + buffer overflows int for any buffer the entry point accepts (as sample_windows_multi_kernel)
    const int64_t left = start - buffer > 0 ? (int64_t)start - buffer : 0;
    const int64_t right = (int64_t)start + S + buffer < T ? (int64_t)start + S + buffer : T;
    pfg_dev_problem &P = probs[b];
    P.y = y + left;
    P.T = (int)(right - left);
    P.t1 = (int)(start - left);
    P.tL = (int)(start + S - left);
    P.weights = wtab ? wtab + (size_t)start * S : nullptr;
}

__global__ __launch_bounds__(kSampleNT) void sample_windows_multi_kernel(
    int W, int n_seq, const int64_t *__restrict__ bounds, const int64_t *__restrict__ woffs, int K, int M,
    pfg_dev_problem *__restrict__ probs, int32_t *__restrict__ seq_len, const double *__restrict__ y,
    const double *__restrict__ wtab, int S, int buffer, int strict, uint64_t seed, uint64_t chain_offset,
    const uint64_t *__restrict__ step_ctr) {
    __shared__ int chosen[PFG_MAX_DRAWN_SEQUENCES];
    __shared__ int sorted[PFG_MAX_DRAWN_SEQUENCES];
    const int c = blockIdx.x;
    const uint64_t gid = chain_offset + (uint64_t)c, ctr = step_ctr ? *step_ctr : 0ull;
    const uint32_t c1 = (uint32_t)(gid >> 32) ^ (uint32_t)(ctr >> 32);
    auto draw = [&](uint32_t idx) {
        const pfg::u32x4 r = pfg::philox4x32_10({(uint32_t)gid, c1, (uint32_t)ctr, idx}, (uint32_t)seed, (uint32_t)(seed >> 32));
        return ((uint64_t)r.x << 32) | r.y;       // 64 random bits; times a range, high part: bias < range / 2^64
    };
    if (K > 0) {
        if (threadIdx.x == 0) {
            // draw j is uniform over the n_seq - j sequences not chosen yet: the r-th of them is found by walking the
            // chosen ones in ascending order.  The ordered K-tuple has the law of np.random.choice(n_seq, K, replace=False).
            for (int j = 0; j < K; ++j) {
                int r = (int)__umul64hi(draw(kSeqTag | (uint32_t)j), (uint64_t)(n_seq - j));
                int i = 0;
                for (; i < j && sorted[i] <= r; ++i) ++r;
                for (int q = j; q > i; --q) sorted[q] = sorted[q - 1];
                sorted[i] = r;
                chosen[j] = r;
            }
        }
        __syncthreads();
    }
    for (int w = threadIdx.x; w < W; w += kSampleNT) {
        const int k = w / M;
        const int seq = K > 0 ? chosen[k] : k;
        const int64_t lo = bounds[seq];
        const int Tk = (int)(bounds[seq + 1] - lo);
        const bool whole = S < 1 || Tk - S <= 0;
        int start = 0, len = Tk;
        if (!whole) {
            const uint32_t range = strict ? (uint32_t)(Tk / S) : (uint32_t)(Tk - S + 1);
            const int idx = (int)__umul64hi(draw(kWinTag | (uint32_t)w), (uint64_t)range);
            start = strict ? idx * S : idx;
            len = S;
        }
        const int64_t left = start - buffer > 0 ? (int64_t)start - buffer : 0;
        const int64_t right = (int64_t)start + len + buffer < Tk ? (int64_t)start + len + buffer : Tk;
        const size_t i = (size_t)c * W + w;
        pfg_dev_problem &P = probs[i];
        P.y = y + lo + left;
        P.T = (int)(right - left);
        P.t1 = (int)(start - left);
        P.tL = (int)(start + len - left);
        P.weights = (whole || !wtab) ? nullptr : wtab + (woffs ? woffs[seq] : 0) + (size_t)start * S;
        seq_len[i] = Tk;
    }
}

__global__ __launch_bounds__(kReduceNT) void reduce_windows_kernel(int C, int K, int M, const double *__restrict__ win,
                                                                   const int32_t *__restrict__ seq_len, int rescale,
                                                                   double T_total, double *__restrict__ outs) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const size_t W = (size_t)K * M;
    const double *g = win + (size_t)c * W * PFG_OUT_DOUBLES;
    const double Md = (double)M;
    double acc[kReduceCols], S = 0.0;
    for (int k = 0; k < K; ++k) {
        // sgmcmc_sampler.py:411-418: part = 0; part += g * 1.0 / minibatch_size, window by window
        double part[kReduceCols];
        for (int j = 0; j < kReduceCols; ++j) part[j] = 0.0;
        for (int m = 0; m < M; ++m) {
            const double *r = g + ((size_t)k * M + m) * PFG_OUT_DOUBLES;
            for (int j = 0; j < kReduceCols; ++j) part[j] = part[j] + (r[j] * 1.0) / Md;
        }
        // :1264-1277: the first sequence's part as is, the others added in choice order
        for (int j = 0; j < kReduceCols; ++j) acc[j] = k == 0 ? part[j] : acc[j] + part[j];
        if (rescale) S = S + (double)seq_len[(size_t)c * W + (size_t)k * M];
    }
    double *o = outs + (size_t)c * PFG_OUT_DOUBLES;
    // :1278-1282: acc * T_total / S
    for (int j = 0; j < kReduceCols; ++j) o[j] = rescale ? (acc[j] * T_total) / S : acc[j];
    for (int j = kReduceCols; j < PFG_OUT_DOUBLES; ++j) o[j] = 0.0;
}

}  // namespace

int pfg_sample_windows_device(pfg_ctx *ctx, int B, pfg_dev_problem *dev_probs, const double *y_dev,
                              const double *weights_table_dev, int T, int S, int buffer, int strict,
                              uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (B <= 0) return PFG_OK;
    if (!dev_probs || !y_dev) return fail(ctx, PFG_ERR_INVALID, "pfg_sample_windows_device: NULL argument");
    if (S < 1 || S > T || buffer < 0) return fail(ctx, PFG_ERR_INVALID, "need 1 <= S <= T and buffer >= 0");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(sample_windows_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)hip_stream, B,
                       dev_probs, y_dev, weights_table_dev, T, S, buffer, strict, seed, chain_offset, step_ctr);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

int pfg_sample_windows_multi_device(pfg_ctx *ctx, int C, int n_seq, const int64_t *seq_bounds_dev,
                                    const int64_t *weight_offsets_dev, int num_sequences, int M,
                                    pfg_dev_problem *dev_probs, int32_t *seq_len_dev, const double *y_dev,
                                    const double *weights_dev, int S, int buffer, int strict, uint64_t seed,
                                    uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (n_seq < 1) return fail(ctx, PFG_ERR_INVALID, "pfg_sample_windows_multi_device: need n_seq >= 1");
    if (num_sequences != -1 && (num_sequences < 1 || num_sequences > n_seq))
        return fail(ctx, PFG_ERR_INVALID, "num_sequences must be -1 or in 1.." + std::to_string(n_seq) + ", got " +
                                              std::to_string(num_sequences));
    if (num_sequences > PFG_MAX_DRAWN_SEQUENCES)
        return fail(ctx, PFG_ERR_UNSUPPORTED, "num_sequences = " + std::to_string(num_sequences) + " > " +
                                                  std::to_string(PFG_MAX_DRAWN_SEQUENCES) + " drawn sequences per chain");
    if (M < 1) return fail(ctx, PFG_ERR_INVALID, "minibatch_size must be >= 1");
    const int64_t W = (int64_t)(num_sequences == -1 ? n_seq : num_sequences) * M;
    if (W >= (int64_t(1) << 24)) return fail(ctx, PFG_ERR_UNSUPPORTED, "more than 2^24 - 1 windows per chain");
    if (strict && S < 1) return fail(ctx, PFG_ERR_INVALID, "the strict partition needs S >= 1");
    if (buffer < 0) return fail(ctx, PFG_ERR_INVALID, "buffer must be >= 0");
    if (C <= 0) return PFG_OK;
    if (!dev_probs || !seq_len_dev || !y_dev || !seq_bounds_dev)
        return fail(ctx, PFG_ERR_INVALID, "pfg_sample_windows_multi_device: NULL argument");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(sample_windows_multi_kernel, dim3(C), dim3(kSampleNT), 0, (hipStream_t)hip_stream, (int)W, n_seq,
                       seq_bounds_dev, weight_offsets_dev, num_sequences == -1 ? 0 : num_sequences, M, dev_probs,
                       seq_len_dev, y_dev, weights_dev, S, buffer, strict, seed, chain_offset, step_ctr);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

int pfg_reduce_windows_device(pfg_ctx *ctx, int C, int num_seq_windows, int M, const double *win_outs,
                              const int32_t *seq_len_dev, int rescale, double T_total, double *outs, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (num_seq_windows < 1 || M < 1) return fail(ctx, PFG_ERR_INVALID, "pfg_reduce_windows_device: need K >= 1 and M >= 1");
    if (rescale && !(T_total > 0.0)) return fail(ctx, PFG_ERR_INVALID, "pfg_reduce_windows_device: T_total must be > 0");
    if (C <= 0) return PFG_OK;
    if (!win_outs || !outs || (rescale && !seq_len_dev))
        return fail(ctx, PFG_ERR_INVALID, "pfg_reduce_windows_device: NULL argument");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(reduce_windows_kernel, dim3((C + kReduceNT - 1) / kReduceNT), dim3(kReduceNT), 0,
                       (hipStream_t)hip_stream, C, num_seq_windows, M, win_outs, seq_len_dev, rescale ? 1 : 0, T_total, outs);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}
