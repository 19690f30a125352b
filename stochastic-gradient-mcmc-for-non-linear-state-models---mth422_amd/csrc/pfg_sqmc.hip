// The filter of sequential quasi-Monte Carlo (Gerber and Chopin 2015) for SVM and LGSSM, as the estimate of PMMH chains.
// EXTENSION: the reference has no particle MCMC and no quasi-Monte Carlo.  The particles are sorted by state, and the N
// (resampling, move) pairs of a timestep are ONE randomised Sobol' point set in [0, 1)^2 instead of 2N independent draws: the
// log-likelihood estimate itself gets less noisy at a given N.  Every point is uniform under the randomisation, so the estimate
// is unbiased and PMMH on it is exact for every N.  The chain carries nothing beyond PMMH's state.  One workgroup per chain,
// f64, N = 2^m with 2 <= N <= 1024: 64 threads x 2 particles (one wave: no s_barrier, see block_sync) for n_max <= 128,
// 256 x 4 above.  Particle (child) i = tid * PPT + k belongs to thread tid, slot k.
//   target   the law the filters target: x_{-1} ~ N(prior_mean, prior_var) whatever theta, x_t | x_{t-1} ~ f_theta, weight
//            g_theta(y_t | x_t); proposal = the prior kernel, resampling at every step t >= 1.
//   points   index i in [0, N): a_i = bitreverse32(i), the van der Corput point; b_i = XOR over the set bits k of i of V_k,
//            V_0 = 0x80000000, V_{k+1} = V_k ^ (V_k >> 1), the second Sobol' dimension.  The first 2^m of them are a (0, m, 2)-net.
//   shift    row r = 0 .. T (row 0 serves x_{-1}, row t+1 step t): ONE Philox4x32-10 draw of the chain key
//            (pfg_chain_filter.hpp) at (r, 0x53510000) gives (s_a, s_b, l_a, l_b).  U52 = ((a_i ^ s_a) << 20) | (l_a >> 12),
//            u = (U52 + 0.5) 2^-52; V52 and v likewise from b_i, s_b, l_b: both exact in double, v in (0, 1).  A random digital
//            shift: it keeps the net and makes every point uniform.  Tag 0x53510000 is disjoint from every tag pfg_chains.hip
//            lists, from pfg_csmc.hip's 0x4353.... and from pfg_cpm.hip's 0x43500000 .. 0x43500100.
//   rank     the rank of point i in u-order is k = (a_i ^ s_a) >> (32 - m), a bijection: sorted position k takes point
//            i(k) = bitreverse_m(k ^ (s_a >> (32 - m))), and u_(k) = (k + delta) / N with one delta in (0, 1) per row,
//            delta = ((((s_a & (2^(32-m) - 1)) << 20) | (l_a >> 12)) + 0.5) 2^(m-52) -- a systematic comb, exact in double.
//   normals  z = Phi^-1(v) by ocml's normcdfinv.
//   row 0    x_{-1}^i = prior_mean + sqrt(prior_var) Phi^-1(v_i), the particle index as the point index; u is not used.
//   t = 0    the particles in ascending order of (x_{-1}, index); the child at position k moves from the parent at position k
//            with z of row 1's point i(k) (equal weights: no search); lw = log g(y_0 | x_0).
//   t >= 1   sort ascending by (state, index) (pfg::sort_by_state); the CDF of exp(lw - max lw) in that order; child k searches
//            with u_(k) W for the smallest j with cdf[j] > target, clamped to N-1; it gathers the sorted state at j and moves
//            with z of row t+1's point i(k).  No resampling after the last weight.
//   out      out[4] = sum_t log((1 / N) sum_i w_t^i) with the Gaussian constants log g carries; every other slot 0.
//   STAT     PFG_STAT_NONE: the above, what pfg_sqmc_device launches.  PFG_STAT_SCORE (pfg_sqmc_score_device) carries the O(N)
//            additive statistic through the sort and the gather exactly as pfg_cpm.hip does (see there; the pieces are
//            pfg::stat_publish, stat_at and stat_advance of pfg_chain_filter.hpp): at t = 0 the parent of the child at position k
//            is the x_{-1} at sorted position k.  out[h] = the weighted mean of the last step's alpha for h < H; out[4] and the
//            trace arrays are bitwise STAT_NONE's.
//   degenerate  a weight sum that is zero or not finite: out[4] = -inf, which pmmh_accept_kernel rejects.  Every thread holds
//            the same sum: the branch is uniform.
//   refused  a NULL array, T < 1, N not a power of two in [2, the launch's shape], a prior variance that is not positive: a
//            NaN record and no other store.
// TRACED (the twin a traced launch runs) records, when the pointers are set, trace_anc [T][N] each child's parent in sorted
// coordinates (row 0: -1), trace_ll [T] the per-step increments of out[4] and trace_z [T+1][N] the normals as used (row 0 in
// particle order, the later rows in child order); the production instantiation does not read the trace pointers.  Both write
// the same out.  Built with -ffp-contract=off; ocml exp / log / normcdfinv (no LDS tables).
#include "pfg_chain_filter.hpp"

using namespace pfg_host;

namespace {

constexpr uint32_t kTagSqmc = 0x53510000u;

// b_i, the second Sobol' coordinate of index i < 1024 as a 32-bit fraction
__device__ __forceinline__ uint32_t sobol2(uint32_t i) {
    uint32_t b = 0u, v = 0x80000000u;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        b ^= ((i >> k) & 1u) ? v : 0u;
        v ^= v >> 1;
    }
    return b;
}

// (hi << 20 | lo >> 12) + 0.5 as a double: 52 bits and the half, exact
__device__ __forceinline__ double grid52(uint32_t hi, uint32_t lo) {
    return (double)(((uint64_t)hi << 20) | (uint64_t)(lo >> 12)) + 0.5;
}

// Phi^-1 on the midpoint grid, ONE copy per kernel: inlined at its three call sites times PPT, ocml's normcdfinv (branches,
// each with a table of fp64 coefficients) took the kernels to 452 .. 490 VGPRs, one wave per SIMD
__device__ __attribute__((noinline)) double inverse_normal_cdf(double v) { return ::normcdfinv(v); }

template <int MODEL, int NT, int PPT, bool TRACED, int STAT>
__global__ __launch_bounds__(NT) void sqmc_kernel(const pfg_sqmc_problem *__restrict__ probs, double lambduh, uint64_t seed,
                                                  uint64_t chain_offset, const uint64_t *__restrict__ step_ctr) {
    static_assert(STAT == PFG_STAT_NONE || STAT == PFG_STAT_SCORE, "out[4] alone, or the score beside it");
    constexpr int NMAX = NT * PPT, NW = NT / pfg::WAVE, H = pfg::ModelDims<MODEL>::H;
    constexpr bool ONE_WAVE = NW == 1, SCORE = STAT == PFG_STAT_SCORE;
    constexpr int K = SCORE ? 1 + H : 1;        // what block_cdf sums: the weights, and the weighted alpha columns
    // sorted states; log-weights (by particle under the bitonic sort, by sorted position under the rank sort); the CDF in
    // sorted order; sorted position -> particle
    __shared__ double sx[NMAX], slw[NMAX], cdf[NMAX];
    __shared__ int si[NMAX];
    __shared__ double red_max[1][NW], red_sum[K][NW];
    __shared__ double sa[SCORE ? H * NMAX : 1];         // alpha by particle (pfg::stat_publish)

    const pfg_sqmc_problem &P = probs[blockIdx.x];
    const int tid = threadIdx.x;
    const int T = P.T, N = P.N;
    const double prior_mean = P.prior_mean, prior_var = P.prior_var;
    if (!(pfg::chain_filter_usable(P, NMAX) && (N & (N - 1)) == 0)) {
        if (tid < PFG_OUT_DOUBLES && P.out) P.out[tid] = NAN;
        return;
    }
    const pfg::Consts<double> c = pfg::make_consts<MODEL, double>(P.theta);
    const pfg::Math<double, false> mth = {};
    const auto y = pfg::global_ptr(P.y);
    const pfg::ChainKey key = pfg::make_key(seed, chain_offset, (int)blockIdx.x, step_ctr);
    const int i0 = tid * PPT;
    const int m = 31 - __clz(N);                // N = 2^m, 1 <= m <= 10
    const double sd0 = ::sqrt(prior_var);
    const double two_m52 = 2.220446049250313e-16;       // 2^-52

    // z of point i under the shift (s_b, l_b) of a row
    auto point_z = [&](const pfg::u32x4 &r, uint32_t i) -> double {
        return inverse_normal_cdf(grid52(sobol2(i) ^ r.y, r.w) * two_m52);
    };
    // the point that has rank k in the u-order of a row
    auto point_of_rank = [&](const pfg::u32x4 &r, int k) -> uint32_t {
        return __brev((uint32_t)k ^ (r.x >> (32 - m))) >> (32 - m);
    };
    double alpha[PPT][H], S[H];             // SCORE: the particles' statistics; the weighted mean of the step before
#pragma unroll
    for (int h = 0; h < H; ++h) S[h] = 0.0;
    // the particles (x, lw) into LDS as sort_by_state wants them (SCORE, from t = 1 on: their alpha too), then the sort; sx
    // is sorted afterwards
    auto sort = [&](const double *x, const double *lw, bool with_alpha) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = i0 + k;
            if (i < N) {
                if (ONE_WAVE) cdf[i] = x[k];        // the keys in particle order (the CDF is not built yet)
                else { sx[i] = x[k]; slw[i] = lw[k]; si[i] = i; }
            }
        }
        if (SCORE && with_alpha) pfg::stat_publish<NMAX, PPT, H>(N, alpha, sa);
        pfg::block_sync<NW>();
        pfg::sort_by_state<NT, PPT>(N, N, x, lw, cdf, sx, slw, si);
    };

    // ---- t = 0
    double x[PPT], lw[PPT], z[PPT];
    {
        const pfg::u32x4 r0 = key.draw_at(0u, kTagSqmc), r1 = key.draw_at(1u, kTagSqmc);
        double xm1[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            xm1[k] = 0.0; lw[k] = 0.0;
            if (i0 + k >= N) continue;
            const double zm1 = point_z(r0, (uint32_t)(i0 + k));
            xm1[k] = prior_mean + sd0 * zm1;
            if (TRACED && P.trace_z) P.trace_z[i0 + k] = zm1;
        }
        sort(xm1, lw, false);
        const double y0 = y[0];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            x[k] = 0.0; lw[k] = -INFINITY; z[k] = 0.0;
#pragma unroll
            for (int h = 0; h < H; ++h) alpha[k][h] = 0.0;
            if (i0 + k >= N) continue;
            const double xp = sx[i0 + k];
            z[k] = point_z(r1, point_of_rank(r1, i0 + k));
            pfg::particle_step<MODEL, PFG_KERNEL_PRIOR, STAT>(c, mth, &xp, y0, z[k], &x[k], lw[k], alpha[k]);
            if (TRACED && P.trace_z) P.trace_z[(size_t)N + i0 + k] = z[k];
            if (TRACED && P.trace_anc) P.trace_anc[i0 + k] = -1;
        }
        pfg::block_sync<NW>();       // the sorted states are free for the next step
    }

    // ---- t = 1 .. T-1: the weights of step t-1, sort, resample, propagate; t = T: the weights of the last step
    bool degenerate = false;
    double ll = 0.0;
    const double logN = ::log((double)N);
    for (int t = 1; t <= T; ++t) {
        // (A) the normals of step t and the comb's offset; the maximum
        double delta = 0.0;
        if (t < T) {
            const pfg::u32x4 r = key.draw_at((uint32_t)(t + 1), kTagSqmc);
#pragma unroll
            for (int k = 0; k < PPT; ++k)
                if (i0 + k < N) z[k] = point_z(r, point_of_rank(r, i0 + k));
            delta = grid52(r.x & ((1u << (32 - m)) - 1u), r.z) * ::ldexp(1.0, m - 52);
        }
        // a NaN state or log-weight makes the maximum +inf, hence the weight sum zero or NaN: the chain is degenerate whatever
        // order the sort below leaves such particles in
        double ma = -INFINITY;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            if (i0 + k < N) {
                const double l = (lw[k] != lw[k] || x[k] != x[k]) ? INFINITY : lw[k];
                ma = l > ma ? l : ma;
            }
        }
        pfg::block_max(red_max, &ma);
        // (S) the sort: the last step's weights need no order (their sum does not depend on it)
        if (t < T) sort(x, lw, true);
        // (B) the CDF in sorted order: a thread's running sums, one scan of the threads' totals
        // SCORE: the sums of w alpha beside it, in the same order; lambduh == 1 reads them after the last step only
        const bool want_S = SCORE && (t == T || lambduh != 1.0);
        double cs[PPT], run[K];
#pragma unroll
        for (int q = 0; q < K; ++q) run[q] = 0.0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = i0 + k;
            double w = 0.0;
            if (p < N) {
                double l = lw[k];           // the last step: particle order
                if (t < T) l = ONE_WAVE ? slw[p] : slw[si[p]];
                w = mth.exp(l - ma);
                if (want_S) {
                    double a[H];
                    if (t < T) pfg::stat_at<NMAX, H>(sa, si, N, p, a);
#pragma unroll
                    for (int h = 0; h < H; ++h) run[SCORE ? 1 + h : 0] += w * (t < T ? a[h] : alpha[k][h]);
                }
            }
            run[0] += w;
            cs[k] = run[0];
        }
        double offs[K], tot[K];
        pfg::block_cdf(red_sum, run, offs, tot, want_S);
        const double off = offs[0], W = tot[0];
        // every thread holds the same W: the branch is uniform over the workgroup
        if (!(W > 0.0 && W < INFINITY)) { degenerate = true; break; }
        const double incr = (ma + ::log(W)) - logN;
        ll += incr;
        if (TRACED && P.trace_ll && tid == 0) P.trace_ll[t - 1] = incr;
        if (want_S) {
#pragma unroll
            for (int h = 0; h < H; ++h) S[h] = tot[SCORE ? 1 + h : 0] / W;
        }
        if (t == T) break;
#pragma unroll
        for (int k = 0; k < PPT; ++k)
            if (i0 + k < N) cdf[i0 + k] = cs[k] + off;
        pfg::block_sync<NW>();
        // (C) parents, children
        // a thread's children are neighbours and their targets ascend, so the answer of one search bounds the next from
        // below: a few probes from there (the CDF does not decrease, so this is the same smallest j), then bisection
        const double yt = y[t];
        int j = 0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int r = i0 + k;
            if (r >= N) continue;
            const double target = (((double)r + delta) / (double)N) * W;
            if (k == 0) {
                j = pfg::cdf_search(cdf, N, target);
            } else {
                int probes = 0;
                while (probes < 3 && j < N - 1 && !(cdf[j] > target)) { ++j; ++probes; }
                if (j < N - 1 && !(cdf[j] > target)) j = pfg::cdf_search(cdf, N, target, j + 1);
            }
            const double xp = sx[j];
            double add[H], ap[H];
            if (SCORE) pfg::stat_at<NMAX, H>(sa, si, N, j, ap);
            pfg::particle_step<MODEL, PFG_KERNEL_PRIOR, STAT>(c, mth, &xp, yt, z[k], &x[k], lw[k], add);
            if (SCORE) pfg::stat_advance<H>(lambduh, ap, S, add, alpha[k]);
            if (TRACED && P.trace_anc) P.trace_anc[(size_t)t * N + r] = j;
            if (TRACED && P.trace_z) P.trace_z[(size_t)(t + 1) * N + r] = z[k];
        }
        pfg::block_sync<NW>();       // the sorted states and the CDF are free for the next step
    }
    // out[h] = S_{T-1}[h], the weighted mean of the last step's statistics (a degenerate chain: 0)
    double mine = 0.0;
    if (SCORE && !degenerate) {
#pragma unroll
        for (int h = 0; h < H; ++h) mine = tid == h ? S[h] : mine;
    }
    if (tid < PFG_OUT_DOUBLES) P.out[tid] = tid == 4 ? (degenerate ? -INFINITY : ll) : mine;
}

// the two entry points: the checks, then the STAT instantiation of (model, traced, n_max)
template <int STAT>
int launch_sqmc(pfg_ctx *ctx, const char *func, int model, int dtype, int n_max, int B, const pfg_sqmc_problem *problems,
                double lambduh, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced) {
    const int rc = check_chain_filter_launch(ctx, func, "the SQMC filter is built for SVM and LGSSM (the sort orders a "
                                             "scalar state)", model, dtype, n_max, B, problems);
    if (rc != PFG_OK) return rc;
    if (!(lambduh > 0.0 && lambduh <= 1.0)) return fail(ctx, PFG_ERR_INVALID, std::string(func) + ": lambduh must lie in (0, 1]");
    if (B == 0) return PFG_OK;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    dispatch_chain_filter(model, traced != 0, n_max, [&](auto m, auto nt, auto ppt, auto tr) {
        hipLaunchKernelGGL((sqmc_kernel<decltype(m)::value, decltype(nt)::value, decltype(ppt)::value, decltype(tr)::value, STAT>),
                           dim3((unsigned)B), dim3(decltype(nt)::value), 0, (hipStream_t)hip_stream, problems, lambduh, seed,
                           chain_offset, step_ctr);
    });
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

}  // namespace

int pfg_sqmc_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_sqmc_problem *problems, uint64_t seed,
                    uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced) {
    return launch_sqmc<PFG_STAT_NONE>(ctx, __func__, model, dtype, n_max, B, problems, 1.0, seed, chain_offset, step_ctr, hip_stream,
                                      traced);
}

int pfg_sqmc_score_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_sqmc_problem *problems, double lambduh,
                          uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced) {
    return launch_sqmc<PFG_STAT_SCORE>(ctx, __func__, model, dtype, n_max, B, problems, lambduh, seed, chain_offset, step_ctr,
                                       hip_stream, traced);
}
