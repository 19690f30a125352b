// What the kernels that run one chain per lane or per workgroup share: the chain key of every draw (pfg_chains.hip,
// pfg_csmc.hip, pfg_cpm.hip, pfg_sqmc.hip) and, for the filters with one workgroup per chain, f64, N <= 1024 (pfg_csmc.hip,
// pfg_cpm.hip, pfg_sqmc.hip), the device pieces -- emission_logw, cdf_search, the descriptor check, the workgroup maximum and
// CDF offsets, the sort by state of the two filters that resample in the order of the states and the way their score
// instantiations carry a particle's additive statistic through that sort (stat_publish, stat_at, stat_advance) -- and the host
// pieces: the entry point's argument check, the (model, traced, n_max) -> instantiation dispatch and the sizing helpers.
// Each file keeps its tags, its LDS, its phase structure and what it does with a descriptor it refuses.
#pragma once
#include <type_traits>

#include "pfg_host.hpp"
#include "pfg_models.hpp"
#include "pfg_reg_kernel.hpp"

namespace pfg {

// ---- the key: the draws of chain gid = chain_offset + b at step = *step_ctr (0 for a NULL counter) are Philox4x32-10 of the
// counter {gid_lo, step_lo, step_hi ^ gid_hi, tag} under key (seed_lo, seed_hi); draw_at XORs a row or time index into the
// third word.  A draw is a pure function of its key.
struct ChainKey {
    uint32_t gid, c1, c2, k0, k1;
    __device__ __forceinline__ u32x4 draw_tag(uint32_t tag) const { return philox4x32_10({gid, c1, c2, tag}, k0, k1); }
    __device__ __forceinline__ u32x4 draw_at(uint32_t index, uint32_t tag) const { return philox4x32_10({gid, c1, index ^ c2, tag}, k0, k1); }
};
__device__ __forceinline__ ChainKey make_key(uint64_t seed, uint64_t chain_offset, int b, const uint64_t *step_ctr) {
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    return {(uint32_t)gid, (uint32_t)step, (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32), (uint32_t)seed, (uint32_t)(seed >> 32)};
}
__device__ __forceinline__ double uniform53(uint32_t a, uint32_t b) {      // (0, 1)
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

// ---- one workgroup per chain
// log g(y | x) of a given state: particle_step's expressions (svm/kernels.py:56-62, lgssm/kernels.py:58-62)
template <int MODEL, typename MATH>
__device__ __forceinline__ double emission_logw(const Consts<double> &c, const MATH &mth, double x, double y) {
    if (MODEL == PFG_MODEL_SVM) return svm_logw(c, x, mth.exp_finite(-x), y * y);
    const double diff = y - c.C * x;
    return (c.c0 + (-0.5 * (diff * diff)) * c.Rinv) + c.logLRinv;
}

// smallest j in [from, N-1] with cdf[j] > target, N-1 when there is none
__device__ __forceinline__ int cdf_search(const double *cdf, int N, double target, int from = 0) {
    int lo = from, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the fields every chain-filter descriptor has: arrays in place, T >= 1, 2 <= N <= the launch's shape, a positive finite
// prior variance, a finite prior mean.  A kernel ANDs in its own pointers and refuses in its own way
template <typename PROBLEM>
__device__ __forceinline__ bool chain_filter_usable(const PROBLEM &P, int nmax) {
    return P.theta && P.y && P.out && P.T >= 1 && P.N >= 2 && P.N <= nmax && P.prior_var > 0.0 && P.prior_var < INFINITY &&
           isfinite(P.prior_mean);
}

// The two reductions of a workgroup of NW waves over K values per thread, each under one barrier, through red [K][NW] in
// LDS.  `rest` (uniform over the workgroup) false: only value 0 is wanted, the others skip their wave reduction.  One wave:
// no barrier, no LDS.
// m[k] -> its maximum over the workgroup
template <int NW, int K>
__device__ __forceinline__ void block_max(double (&red)[K][NW], double *m, bool rest = true) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    m[0] = wave_max(m[0]);
    for (int k = 1; k < K; ++k)
        if (rest) m[k] = wave_max(m[k]);
    if (NW > 1) {
        if (lane == 0)
            for (int k = 0; k < K; ++k) red[k][wave] = m[k];
        block_sync<NW>();
#pragma unroll
        for (int w = 0; w < NW; ++w)
            for (int k = 0; k < K; ++k) m[k] = red[k][w] > m[k] ? red[k][w] : m[k];
    }
}
// run[k], the thread's sum -> off[k], the sum over the threads before it, and tot[k], the workgroup's: a wave scan, then the
// waves' totals added in ascending order
template <int NW, int K>
__device__ __forceinline__ void block_cdf(double (&red)[K][NW], const double *run, double *off, double *tot, bool rest = true) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    double inc[K];
    for (int k = 0; k < K; ++k) {
        inc[k] = k == 0 || rest ? wave_incl_scan(run[k]) : 0.0;
        off[k] = inc[k] - run[k];
        tot[k] = bcast_lane63(inc[k]);
    }
    if (NW > 1) {
        if (lane == WAVE - 1)
            for (int k = 0; k < K; ++k) red[k][wave] = inc[k];
        block_sync<NW>();
        double before[K];
        for (int k = 0; k < K; ++k) { tot[k] = 0.0; before[k] = 0.0; }
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            for (int k = 0; k < K; ++k) {
                if (w == wave) before[k] = tot[k];
                tot[k] += red[k][w];
            }
        }
        for (int k = 0; k < K; ++k) off[k] += before[k];
    }
}

// ---- the sort of the filters that resample in the order of the states (pfg_cpm.hip, pfg_sqmc.hip)
// (xa, ia) before (xb, ib) in the order of the sort
__device__ __forceinline__ bool key_less(double xa, int ia, double xb, int ib) { return xa < xb || (xa == xb && ia < ib); }

// The N (state, log-weight) pairs of a workgroup of NT threads x PPT particles, particle i = tid * PPT + k, ascending by
// (state, particle index): a total order.  Afterwards sx holds the sorted states and si sorted position -> particle.
//   one wave (NT == 64)  a rank sort: a particle's position is the number of keys before its own, N broadcast LDS reads per
//                        thread and no barrier.  The caller has stored the keys in particle order in `keys` and synchronised;
//                        x, lw: the thread's own particles.  Distinct states need one comparison per pair; equal ones collide
//                        on a position, which the read-back sees, and the whole wave then ranks again with the index as the
//                        tie-break.  slw: the log-weights by sorted position.
//   otherwise            a bitonic network over npad, the next power of two, in LDS, a barrier per stage.  The caller has stored
//                        sx[i], si[i] = i for i < npad (the padding: +inf keys) and synchronised; slw (the caller's, by
//                        particle) is not touched.
template <int NT, int PPT>
__device__ __forceinline__ void sort_by_state(int N, int npad, const double *x, const double *lw, const double *keys, double *sx,
                                              double *slw, int *si) {
    constexpr int NW = NT / WAVE;
    const int tid = threadIdx.x, i0 = tid * PPT;
    if constexpr (NW == 1) {
        auto scatter = [&](const int *rank) {
#pragma unroll
            for (int k = 0; k < PPT; ++k)
                if (i0 + k < N) { sx[rank[k]] = x[k]; slw[rank[k]] = lw[k]; si[rank[k]] = i0 + k; }
            block_sync<NW>();
        };
        int rank[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) rank[k] = 0;
        for (int j = 0; j < N; ++j) {
            const double xj = keys[j];
#pragma unroll
            for (int k = 0; k < PPT; ++k) rank[k] += xj < x[k] ? 1 : 0;
        }
        scatter(rank);
        bool clash = false;
#pragma unroll
        for (int k = 0; k < PPT; ++k)
            if (i0 + k < N) clash = clash || si[rank[k]] != i0 + k;
        if (__any(clash)) {         // uniform over the wave
            block_sync<NW>();
#pragma unroll
            for (int k = 0; k < PPT; ++k) rank[k] = 0;
            for (int j = 0; j < N; ++j) {
                const double xj = keys[j];
#pragma unroll
                for (int k = 0; k < PPT; ++k) rank[k] += key_less(xj, j, x[k], i0 + k) ? 1 : 0;
            }
            scatter(rank);
        }
    } else {
        for (int kk = 2; kk <= npad; kk <<= 1) {
            for (int j = kk >> 1; j > 0; j >>= 1) {
                for (int q = tid; q < (npad >> 1); q += NT) {
                    const int a = ((q & ~(j - 1)) << 1) | (q & (j - 1)), b = a | j;
                    const bool up = (a & kk) == 0;
                    const double xa = sx[a], xb = sx[b];
                    const int ia = si[a], ib = si[b];
                    const bool swap = up ? key_less(xb, ib, xa, ia) : key_less(xa, ia, xb, ib);
                    if (swap) { sx[a] = xb; sx[b] = xa; si[a] = ib; si[b] = ia; }
                }
                block_sync<NW>();
            }
        }
    }
}

// ---- the additive statistic of the two sorted filters (STAT = PFG_STAT_SCORE: Poyiadjis' O(N) recursion, with the fixed-lag
// shrinkage of Nemeth, Sherlock and Fearnhead 2016 for lambduh < 1)
// Every particle carries alpha [H] in registers beside (x, lw).  The sort moves (state, index) pairs only, so alpha goes to LDS
// BY PARTICLE, sa[h * NMAX + i], in the phase that stores the keys (the barrier that orders those stores orders these), and
// whoever needs the alpha at a sorted position reads it through si: the weighted sums S ride on block_cdf's K = 1 + H values,
// a child gathers its parent's.  Both filters keep sa until the barrier that frees sx and the CDF.
template <int NMAX, int PPT, int H>
__device__ __forceinline__ void stat_publish(int N, const double (&alpha)[PPT][H], double *sa) {
    const int i0 = threadIdx.x * PPT;
#pragma unroll
    for (int k = 0; k < PPT; ++k)
        if (i0 + k < N) {
#pragma unroll
            for (int h = 0; h < H; ++h) sa[h * NMAX + i0 + k] = alpha[k][h];
        }
}
// a [H] = the alpha of the particle at sorted position p < N.  An entry that names no particle has none, 0: a padding entry of
// the bitonic network, or a slot the rank sort never wrote -- NaN states can leave either at p < N, and the chain is then
// degenerate whatever is read here; the unsigned compare keeps the read inside sa all the same
template <int NMAX, int H>
__device__ __forceinline__ void stat_at(const double *sa, const int *si, int N, int p, double *a) {
    const unsigned i = (unsigned)si[p];
#pragma unroll
    for (int h = 0; h < H; ++h) a[h] = i < (unsigned)N ? sa[h * NMAX + i] : 0.0;
}
// alpha_child = lambduh alpha_parent + (1 - lambduh) S + add; lambduh == 1 is the plain recursion and does not read S
template <int H>
__device__ __forceinline__ void stat_advance(double lambduh, const double *parent, const double *S, const double *add,
                                             double *alpha) {
#pragma unroll
    for (int h = 0; h < H; ++h)
        alpha[h] = lambduh == 1.0 ? parent[h] + add[h] : (lambduh * parent[h] + (1.0 - lambduh) * S[h]) + add[h];
}

}  // namespace pfg

namespace pfg_host {

constexpr int kChainFilterMaxN = 1024;

inline int64_t round_up_256(int64_t bytes) { return (bytes + 255) / 256 * 256; }
// the domain of the per-chain sizing queries (pfg_csmc_scratch_bytes, pfg_cpm_aux_bytes)
inline bool chain_filter_domain(int T, int N) { return T >= 1 && N >= 2 && N <= kChainFilterMaxN; }

// The argument checks of an entry point that launches one workgroup per chain: SVM | LGSSM, f64, 2 <= n_max <= 1024.
// garch_clause: why the family has no GARCH instantiation.  PFG_OK: go on (B may still be 0)
inline int check_chain_filter_launch(pfg_ctx *ctx, const char *func, const char *garch_clause, int model, int dtype, int n_max,
                                     int B, const void *problems) {
    if (!ctx) return PFG_ERR_INVALID;
    const std::string who = std::string(func) + ": ";
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (model == PFG_MODEL_GARCH) return fail(ctx, PFG_ERR_UNSUPPORTED, who + garch_clause);
    if (dtype != PFG_F64) return fail(ctx, PFG_ERR_UNSUPPORTED, who + "f64 only");
    if (n_max > kChainFilterMaxN || n_max < 2)
        return fail(ctx, PFG_ERR_UNSUPPORTED, who + "2 <= N <= 1024 particles (one workgroup per chain), got " + std::to_string(n_max));
    if (B < 0) return fail(ctx, PFG_ERR_INVALID, who + "B must be >= 0");
    if (!problems) return fail(ctx, PFG_ERR_INVALID, who + "NULL argument");
    return PFG_OK;
}

// (model, traced, n_max) -> f(MODEL, NT, PPT, TRACED) as std::integral_constants: one wave of 64 threads x 2 particles up to
// N = 128, 256 x 4 above
template <typename F>
void dispatch_chain_filter(int model, bool traced, int n_max, F &&f) {
    auto shape = [&](auto m, auto tr) {
        if (n_max <= 128) f(m, std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{}, tr);
        else f(m, std::integral_constant<int, 256>{}, std::integral_constant<int, 4>{}, tr);
    };
    auto twin = [&](auto m) {
        if (traced) shape(m, std::true_type{});
        else shape(m, std::false_type{});
    };
    if (model == PFG_MODEL_SVM) twin(std::integral_constant<int, PFG_MODEL_SVM>{});
    else twin(std::integral_constant<int, PFG_MODEL_LGSSM>{});
}

}  // namespace pfg_host
