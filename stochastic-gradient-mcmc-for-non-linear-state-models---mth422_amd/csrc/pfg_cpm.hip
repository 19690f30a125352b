// The filter of correlated pseudo-marginal PMMH (Deligiannidis, Doucet and Pitt 2018) for SVM and LGSSM.  EXTENSION: the
// reference has no particle MCMC.  The log-likelihood estimate is a deterministic function of theta and of an array U of
// standard normals that the chain carries as part of its state; a step proposes U' = rho U + sqrt(1 - rho^2) eps beside
// theta', so the two estimates in the accept ratio are correlated and their difference is far less noisy than two
// independent estimates'.  U -> U' is reversible with respect to N(0, I) and the estimate is unbiased under it, so the
// chain is exact for every N and every rho in [0, 1).  One workgroup per chain, f64, N <= 1024: 64 threads x 2 particles
// (one wave: no s_barrier, see block_sync) for N <= 128, 256 x 4 above.  Particle i = tid * PPT + k belongs to thread
// tid, slot k.
//   target   the law the filters target: x_{-1} ~ N(prior_mean, prior_var) whatever theta, x_t | x_{t-1} ~ f_theta, weight
//            g_theta(y_t | x_t); proposal = the prior kernel, resampling at every step t >= 1.
//   U        [T+1][N+1] f64 per buffer.  Row 0, columns 0 .. N-1: the normals of x_{-1}.  Row t+1, columns 0 .. N-1: the state
//            normals of step t; column N: the resampling normal of step t.  (Column N of rows 0 and 1 is carried along and
//            never read by the filter.)  A chain owns two buffers u0, u1 and a selector *which: the kernel reads
//            U = u[*which & 1], writes U' to the other one and filters on U'.  rho == 0 never reads U: the init pass.
//   eps      entry (row, col): Philox4x32-10 under key (seed_lo, seed_hi), counter {gid_lo, step_lo, row ^ (step_hi ^
//            gid_hi), 0x43500000 | (col >> 2)}, gid = chain_offset + b, step = *step_ctr -- the chain key (pfg_chain_filter.hpp)
//            drawn with the row XORed into the third word.  One draw r serves four columns: normal_pair(r.x, r.y) -> columns 4q, 4q + 1,
//            normal_pair(r.z, r.w) -> columns 4q + 2, 4q + 3.  Tags 0x43500000 .. 0x43500100: disjoint from every tag
//            pfg_chains.hip lists.  U' = rho * U + sqrt(1 - rho * rho) * eps (rho == 0: eps itself).
//   t = 0    x_{-1}^i = prior_mean + sqrt(prior_var) U'[0][i], x_0^i = particle_step(x_{-1}^i, U'[1][i]), lw = log g(y_0 | x_0).
//   t >= 1   the smoothness the correlation needs (a small move of U moves the estimate little) comes from resampling in
//            the order of the states:
//              sort     (pfg::sort_by_state, pfg_chain_filter.hpp: shared with pfg_sqmc.hip)
//                       the N (state, log-weight) pairs ascending by (state, original index): a total order.  One wave: a
//                       rank sort, a particle's position is the number of keys before its own (N broadcast LDS reads per
//                       thread, no barrier; equal states are seen as a collision and ranked again with the index).  256 x 4: a
//                       bitonic network over the next power of two in LDS, the padding carries +inf keys and zero weight.
//              cdf      of exp(lw - max lw) in sorted order.
//              search   child r takes ((r + u) / N) W with u = min(Phi(U'[t+1][N]), 1 - 2^-53), Phi(z) = erfc(-z / sqrt 2) / 2:
//                       systematic resampling on one uniform.  The smallest j with cdf[j] > target, clamped to N-1.
//              move     child r gathers the state at sorted position j and takes particle_step with U'[t+1][r].
//   out      out[4] = sum_t log((1 / N) sum_i w_t^i) with the Gaussian constants log g carries; every other slot 0.
//   STAT     PFG_STAT_NONE: the above, what pfg_cpm_device launches.  PFG_STAT_SCORE (pfg_cpm_score_device: the drift of particle
//            MALA on this filter) carries Poyiadjis' O(N) additive statistic through the sort and the gather: alpha [H] per
//            particle in registers beside (x, lw), alpha = add(x_{-1} -> x_0, y_0) at t = 0 and, for the child r of the parent at
//            sorted position j, alpha_r = lambduh alpha_j + (1 - lambduh) S + add(x_j -> x_r, y_t), S = sum_i w_i alpha_i / sum_i w_i
//            under the weights of the CDF (lambduh == 1 does not read S: the plain recursion; lambduh < 1: the fixed-lag
//            shrinkage of Nemeth, Sherlock and Fearnhead 2016).  alpha goes to LDS by particle with the keys (sa; pfg::stat_publish)
//            and is read through si (pfg::stat_at); the sums of w alpha are block_cdf's values 1 .. H, so they cost no barrier.
//            out[h] = S of the last step for h < H, 0 above and for a degenerate chain.  The weight arithmetic is the same
//            instructions in the same order: out[4], U' and the trace arrays are bitwise STAT_NONE's.
//   degenerate  a weight sum that is zero or not finite: out[4] = -inf, which pmmh_accept_kernel rejects; the rest of U' is
//            still written (a finite array: NaN never enters U).  Every thread holds the same sum: the branch is uniform.
//   refused  a NULL array, T < 1, N outside [2, the launch's shape], a prior variance that is not positive: a NaN record and
//            no other store.
// TRACED (the twin a traced launch runs) records, when the pointers are set, each child's parent in sorted coordinates and
// the per-step increments of out[4]; the production instantiation does not read the trace pointers.  Both write the same
// out[4] and the same U'.  Built with -ffp-contract=off; ocml exp / log / erfc (no LDS tables).
#include "pfg_chain_filter.hpp"

using namespace pfg_host;

namespace {

constexpr uint32_t kTagCpm = 0x43500000u;      // | column >> 2

template <int MODEL, int NT, int PPT, bool TRACED, int STAT>
__global__ __launch_bounds__(NT) void cpm_kernel(const pfg_cpm_problem *__restrict__ probs, double rho, double lambduh,
                                                 uint64_t seed, uint64_t chain_offset, const uint64_t *__restrict__ step_ctr) {
    static_assert(PPT == 2 || PPT == 4, "a thread's columns lie in one Philox draw");
    static_assert(STAT == PFG_STAT_NONE || STAT == PFG_STAT_SCORE, "out[4] alone, or the score beside it");
    constexpr int NMAX = NT * PPT, NW = NT / pfg::WAVE, H = pfg::ModelDims<MODEL>::H;
    constexpr bool ONE_WAVE = NW == 1, SCORE = STAT == PFG_STAT_SCORE;
    constexpr int K = SCORE ? 1 + H : 1;        // what block_cdf sums: the weights, and the weighted alpha columns
    // sorted states; log-weights (by particle under the bitonic sort, by sorted position under the rank sort); the CDF in
    // sorted order; sorted position -> particle
    __shared__ double sx[NMAX], slw[NMAX], cdf[NMAX];
    __shared__ int si[NMAX];
    __shared__ double red_max[1][NW], red_sum[K][NW], u_sh;
    __shared__ double sa[SCORE ? H * NMAX : 1];         // alpha by particle (pfg::stat_publish)

    const pfg_cpm_problem &P = probs[blockIdx.x];
    const int tid = threadIdx.x;
    const int T = P.T, N = P.N;
    const double prior_mean = P.prior_mean, prior_var = P.prior_var;
    if (!(pfg::chain_filter_usable(P, NMAX) && P.u0 && P.u1 && P.which)) {
        if (tid < PFG_OUT_DOUBLES && P.out) P.out[tid] = NAN;
        return;
    }
    const pfg::Consts<double> c = pfg::make_consts<MODEL, double>(P.theta);
    const pfg::Math<double, false> mth = {};
    const auto y = pfg::global_ptr(P.y);
    const int cur = *P.which & 1;
    const auto uc = pfg::global_ptr(static_cast<const double *>(cur ? P.u1 : P.u0));
    const auto un = pfg::global_ptr(cur ? P.u0 : P.u1);
    const pfg::ChainKey key = pfg::make_key(seed, chain_offset, (int)blockIdx.x, step_ctr);
    // the draw that holds eps (row, col)
    auto draw = [&](int row, int col) { return key.draw_at((uint32_t)row, kTagCpm | ((uint32_t)col >> 2)); };
    const int i0 = tid * PPT, ld = N + 1;
    const double srho = ::sqrt(1.0 - rho * rho);
    const double sd0 = ::sqrt(prior_var);
    int npad = 2;
    while (npad < N) npad <<= 1;

    // U'[row][col] from eps and, for rho != 0, U[row][col]; stored
    auto mix = [&](int row, int col, double eps) -> double {
        const size_t at = (size_t)row * ld + col;
        const double v = rho == 0.0 ? eps : rho * uc[at] + srho * eps;
        un[at] = v;
        return v;
    };
    // Column N of a row belongs to the last thread when that one has no particle (N <= NMAX - PPT): it then runs the same
    // instructions as the others, on another column, and no lane waits for an extra normal_pair.  Otherwise thread 0 takes it
    // as a second draw.
    const bool spare = (NT - 1) * PPT >= N;
    const int owner = spare ? NT - 1 : 0;
    // the thread's PPT entries of a row (columns i0 .. i0 + PPT - 1 below N) into z; column N's owner returns that entry
    auto propose_row = [&](int row, double *z) -> double {
        double last = 0.0;
        const bool mine = spare && tid == owner;
        if (i0 < N || mine) {
            const int c0 = mine ? N : i0;
            const pfg::u32x4 r = draw(row, c0);
#pragma unroll
            for (int k = 0; k < PPT; k += 2) {
                const bool second = ((c0 + k) >> 1) & 1;
                double ea, eb;
                mth.normal_pair(second ? r.z : r.x, second ? r.w : r.y, ea, eb);
                if (mine) {
                    if (k == 0) last = mix(row, N, (N & 1) ? eb : ea);
                } else {
                    if (i0 + k < N) z[k] = mix(row, i0 + k, ea);
                    if (i0 + k + 1 < N) z[k + 1] = mix(row, i0 + k + 1, eb);
                }
            }
        }
        if (!spare && tid == 0) {
            const pfg::u32x4 r = draw(row, N);
            const bool second = (N >> 1) & 1;
            double ea, eb;
            mth.normal_pair(second ? r.z : r.x, second ? r.w : r.y, ea, eb);
            last = mix(row, N, (N & 1) ? eb : ea);
        }
        return last;
    };

    // ---- t = 0
    double x[PPT], lw[PPT], z[PPT];
    double alpha[PPT][H], S[H];             // SCORE: the particles' statistics; the weighted mean of the step before
#pragma unroll
    for (int h = 0; h < H; ++h) S[h] = 0.0;
    {
        double zm1[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) { zm1[k] = 0.0; z[k] = 0.0; }
        propose_row(0, zm1);
        propose_row(1, z);
        const double y0 = y[0];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            x[k] = 0.0; lw[k] = -INFINITY;
#pragma unroll
            for (int h = 0; h < H; ++h) alpha[k][h] = 0.0;
            if (i0 + k >= N) continue;
            const double xm1 = prior_mean + sd0 * zm1[k];
            pfg::particle_step<MODEL, PFG_KERNEL_PRIOR, STAT>(c, mth, &xm1, y0, z[k], &x[k], lw[k], alpha[k]);
        }
    }

    // ---- t = 1 .. T-1: the weights of step t-1, sort, resample, propagate; t = T: the weights of the last step
    bool degenerate = false;
    double ll = 0.0;
    const double logN = ::log((double)N);
    int t = 1;
    for (; t <= T; ++t) {
        // (A) the normals of step t; the maximum; the particles into LDS in particle order
        if (t < T) {
            const double zr = propose_row(t + 1, z);
            if (tid == owner) {
                const double phi = 0.5 * ::erfc(-zr / 1.4142135623730951);
                u_sh = phi < (1.0 - 1.1102230246251565e-16) ? phi : (1.0 - 1.1102230246251565e-16);
            }
        }
        // a NaN state or log-weight makes the maximum +inf, hence the weight sum zero or NaN: the chain is degenerate whatever
        // order the sort below leaves such particles in
        double ma = -INFINITY;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = i0 + k;
            if (i < N) {
                const double l = (lw[k] != lw[k] || x[k] != x[k]) ? INFINITY : lw[k];
                ma = l > ma ? l : ma;
                if (t < T) {
                    if (ONE_WAVE) cdf[i] = x[k];        // the keys in particle order (the CDF is not built yet)
                    else { sx[i] = x[k]; slw[i] = lw[k]; si[i] = i; }
                }
            } else if (!ONE_WAVE && t < T && i < npad) {
                sx[i] = INFINITY; slw[i] = -INFINITY; si[i] = i;
            }
        }
        if (SCORE && t < T) pfg::stat_publish<NMAX, PPT, H>(N, alpha, sa);
        pfg::block_max(red_max, &ma);
        if (ONE_WAVE) pfg::block_sync<NW>();      // the keys' stores before the sort's reads (256 x 4: block_max's barrier)
        // (S) the sort: the last step's weights need no order (their sum does not depend on it).  -DPFG_CPM_NO_SORT: a
        // diagnostic build that leaves it out, to time what it costs (tools/cpm_time.py); never the library's
#ifndef PFG_CPM_NO_SORT
        // (pfg::sort_by_state: a rank sort in one wave, a bitonic network over the next power of two under 256 x 4)
        if (t < T) pfg::sort_by_state<NT, PPT>(N, npad, x, lw, cdf, sx, slw, si);
#else
        if (t < T && ONE_WAVE) {
#pragma unroll
            for (int k = 0; k < PPT; ++k)
                if (i0 + k < N) { sx[i0 + k] = x[k]; slw[i0 + k] = lw[k]; }
            pfg::block_sync<NW>();
        }
#endif
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
                if (t < T) {
                    if (ONE_WAVE) l = slw[p];
                    else { const int i = si[p]; l = i < N ? slw[i] : -INFINITY; }
                }
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
        const double yt = y[t], u = u_sh;
        int j = 0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int r = i0 + k;
            if (r >= N) continue;
            const double target = (((double)r + u) / (double)N) * W;
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
        }
        pfg::block_sync<NW>();       // the sorted states and the CDF are free for the next step
    }
    // a degenerate chain: the rows of U' the loop did not reach (row t + 1 is written when step t begins)
    if (degenerate)
        for (int row = t + 2; row <= T; ++row) propose_row(row, z);
    // out[h] = S_{T-1}[h], the weighted mean of the last step's statistics (a degenerate chain: 0)
    double mine = 0.0;
    if (SCORE && !degenerate) {
#pragma unroll
        for (int h = 0; h < H; ++h) mine = tid == h ? S[h] : mine;
    }
    if (tid < PFG_OUT_DOUBLES) P.out[tid] = tid == 4 ? (degenerate ? -INFINITY : ll) : mine;
}

// One lane per chain, after the accept step: a chain whose acceptance count moved (or every chain: init) now reads the
// buffer the filter wrote
__global__ void cpm_commit_kernel(int B, const uint64_t *__restrict__ n_accept, uint64_t *__restrict__ seen,
                                  int32_t *__restrict__ which, int init) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (init || n_accept[b] != seen[b]) { which[b] ^= 1; seen[b] = n_accept[b]; }
}

}  // namespace

int64_t pfg_cpm_aux_bytes(int T, int N) {
    if (!chain_filter_domain(T, N)) return -1;
    return round_up_256(((int64_t)T + 1) * ((int64_t)N + 1) * 8);          // U [T+1][N+1] f64
}

namespace {

// the two entry points: the checks, then the STAT instantiation of (model, traced, n_max)
template <int STAT>
int launch_cpm(pfg_ctx *ctx, const char *func, int model, int dtype, int n_max, int B, const pfg_cpm_problem *problems, double rho,
               double lambduh, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced) {
    const int rc = check_chain_filter_launch(ctx, func, "the correlated filter is built for SVM and LGSSM (the sort orders a "
                                             "scalar state)", model, dtype, n_max, B, problems);
    if (rc != PFG_OK) return rc;
    if (!(rho >= 0.0 && rho < 1.0)) return fail(ctx, PFG_ERR_INVALID, std::string(func) + ": rho must lie in [0, 1)");
    if (!(lambduh > 0.0 && lambduh <= 1.0)) return fail(ctx, PFG_ERR_INVALID, std::string(func) + ": lambduh must lie in (0, 1]");
    if (B == 0) return PFG_OK;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    dispatch_chain_filter(model, traced != 0, n_max, [&](auto m, auto nt, auto ppt, auto tr) {
        hipLaunchKernelGGL((cpm_kernel<decltype(m)::value, decltype(nt)::value, decltype(ppt)::value, decltype(tr)::value, STAT>),
                           dim3((unsigned)B), dim3(decltype(nt)::value), 0, (hipStream_t)hip_stream, problems, rho, lambduh, seed,
                           chain_offset, step_ctr);
    });
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

}  // namespace

int pfg_cpm_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_cpm_problem *problems, double rho,
                   uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced) {
    return launch_cpm<PFG_STAT_NONE>(ctx, __func__, model, dtype, n_max, B, problems, rho, 1.0, seed, chain_offset, step_ctr,
                                     hip_stream, traced);
}

int pfg_cpm_score_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_cpm_problem *problems, double rho,
                         double lambduh, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream,
                         int traced) {
    return launch_cpm<PFG_STAT_SCORE>(ctx, __func__, model, dtype, n_max, B, problems, rho, lambduh, seed, chain_offset, step_ctr,
                                      hip_stream, traced);
}

int pfg_cpm_commit_device(pfg_ctx *ctx, int B, const uint64_t *n_accept, uint64_t *seen, int32_t *which, int init,
                          void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (B < 0) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": B must be >= 0");
    if (!n_accept || !seen || !which) return fail(ctx, PFG_ERR_INVALID, std::string(__func__) + ": NULL argument");
    if (B == 0) return PFG_OK;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(cpm_commit_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)hip_stream, B, n_accept, seen, which,
                       init);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}
