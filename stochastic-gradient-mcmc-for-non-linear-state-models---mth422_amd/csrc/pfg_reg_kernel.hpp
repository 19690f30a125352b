// libpfgrad device code: pf_reg_kernel, the LDS-resident particle filter (N <= 4096) incl. its PaRIS, systematic-,
// stratified- and adaptive-resampling and O(N^2) instantiations.  Its build switches, derived compile-time switches and its one LDS layout: pfg_reg_traits.hpp.
#pragma once
#include "pfg_reg_traits.hpp"

namespace pfg {

// LDS-resident kernel: N <= NT*PPT particles; particle i = k*NT + tid belongs to thread tid,
// slot k.  Only the log-weights live in registers across timesteps; particles and statistics
// live in LDS as struct-of-arrays over the particle axis (lane i <-> particle i: conflict-free).
//   LDS: cdf | buf0 {x[NS][NLS], stats[H][NLS]} | buf1 (PP only) | reduction scratch | math tables | PaRIS / O(N^2) tail:
//   RegTraits::layout says where each starts and what aliases what
// PP = ping-pong state buffers: children are written to the other buffer, so no barrier is
// needed between gathering parents and publishing children (3 barriers per timestep, and a
// slot's parent state dies as soon as its child is computed).  PP = false keeps ONE buffer
// (larger N fits in 160 KiB) at the price of a 4th barrier and of holding all gathered
// parents in registers across it.
// workgroup barrier; a one-wave workgroup only needs its own LDS accesses kept in program order (the LDS
// executes a wave's instructions in order): no s_barrier, no drain of the LDS queue
template <int NW> __device__ __forceinline__ void block_sync() {
    if (NW == 1) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}
// 1 / x by v_rcp_f64 + two Newton steps instead of the IEEE division sequence
__device__ __forceinline__ double rcp_newton2(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

template <int MODEL, int KERNEL, typename REAL, int NT, int PPT, int RNG, bool PP, int MODE = 0, bool TRACE = true, bool SCORE1 = false>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RegTraits<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, MODE>::OCC_MIN, RegTraits<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, MODE>::OCC_MAX))) void pf_reg_kernel(const pfg_dev_problem *__restrict__ probs) {
    using TR = RegTraits<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, MODE>;
    constexpr int NS = TR::NS, H = TR::H, NW = TR::NW;
    static_assert(!TR::LWL || PP, "PaRIS / O(N^2) need the parents intact while children are built: ping-pong buffers");
    static_assert(!TR::SYSTEMATIC || RNG == PFG_RNG_DEVICE, "systematic resampling draws its offset on the device");
    extern __shared__ __align__(16) unsigned char smem[];

    const pfg_dev_problem &P = probs[blockIdx.x];
    const int N = P.N, T = P.T, t1 = P.t1, tL = P.tL;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    // SCORE1 (PFG_SMOOTHER_POYIADJIS_N launches of the 1024 x 4 unit): the Poyiadjis O(N) score only -- the filter, the
    // lambda != 1 shrinkage and the other statistics compiled out (config 4: 10.56 -> 10.07 ms, no spilled VGPR; the
    // 256 x 4 unit gains 0.5 %, the 512 x 2 one loses 2 %: profiles/r04_ab_score1_twin.txt).  A descriptor that is not
    // (NEMETH, lambduh = 1, SCORE) gets NaNs, loudly, instead of another estimator's numbers.
    constexpr bool ONLY_SCORE1 = PFG_EXP_PLAIN || SCORE1;
    if constexpr (SCORE1) {
        if (P.smoother != PFG_SMOOTHER_NEMETH || P.lambduh != 1.0 || P.stat != PFG_STAT_SCORE) {
            if (threadIdx.x < PFG_OUT_DOUBLES && P.out) P.out[threadIdx.x] = __builtin_nan("");
            return;
        }
    }
    // ADAPTIVE (pfg_launch_device_adaptive, flagged batches of pfg_run_batch): a descriptor that does not ask for it -- or
    // asks for a recursion this instantiation has no skip path for -- gets NaNs, as in the score-only twins
    if constexpr (TR::ADAPTIVE) {
        if (!(P.flags & PFG_FLAG_ADAPTIVE_RESAMPLING) || P.smoother != PFG_SMOOTHER_NEMETH || P.stat == PFG_STAT_PREDICTIVE) {
            if (threadIdx.x < PFG_OUT_DOUBLES && P.out) P.out[threadIdx.x] = __builtin_nan("");
            return;
        }
    }
    [[maybe_unused]] const double tauN = TR::ADAPTIVE ? (double)ess_threshold_of(P.reserved) * (double)N : 0.0;
    const bool is_filter = !ONLY_SCORE1 && (P.smoother == PFG_SMOOTHER_FILTER);
    const int stat = ONLY_SCORE1 ? (int)PFG_STAT_SCORE : P.stat;
    const double lam_d = ONLY_SCORE1 ? 1.0 : is_filter ? 0.0 : ((P.smoother == PFG_SMOOTHER_PARIS || TR::N2) ? 1.0 : P.lambduh);
    const REAL lam = (REAL)lam_d, oml = (REAL)(1.0 - lam_d);
    const bool needS_every = is_filter || (lam_d != 1.0);
    // RAWSCORE: a plain window whose statistic is the score carries it as raw sums (see PFG_OPT_RAWSCORE); window-uniform
    [[maybe_unused]] const bool raw_score = TR::RAWSCORE && !needS_every && stat == PFG_STAT_SCORE;
    const gptr<const double> yv = global_ptr(P.y);
    const gptr<const double> wv = global_ptr(P.weights);
    const gptr<const double> uv = global_ptr(P.u);
    const gptr<const double> zv = global_ptr(P.z);

    // every pointer into the LDS block comes from the one layout the host sized it with (RegTraits::layout)
    const int NLS = TR::FAST ? TR::layout(0).NLS : TR::layout(N).NLS;
    double *cdf = reg_lds_ptr<double, TR, &RegLdsLayout::cdf>(smem, N);
    uint32_t *cdfu = reg_lds_ptr<uint32_t, TR, &RegLdsLayout::cdf>(smem, N);         // BLK: 32-bit fixed point
    REAL *cur = reg_lds_ptr<REAL, TR, &RegLdsLayout::buf0>(smem, N), *nxt = reg_lds_ptr<REAL, TR, &RegLdsLayout::buf1>(smem, N);
    // element index of component d of particle i
    auto sidx = [&](int d, int i) -> size_t { return TR::sidx(NLS, d, i); };
    double *red_scan = reg_lds_ptr<double, TR, &RegLdsLayout::red_scan>(smem, N);
    double *red_max = reg_lds_ptr<double, TR, &RegLdsLayout::red_max>(smem, N);
    float *red_maxf = reinterpret_cast<float *>(red_max);
    double *red_S = reg_lds_ptr<double, TR, &RegLdsLayout::red_S>(smem, N);
    double *red_W0 = reg_lds_ptr<double, TR, &RegLdsLayout::red_W0>(smem, N);
    const double invN = 1.0 / (double)N;
    double *tabmem = reg_lds_ptr<double, TR, &RegLdsLayout::tab>(smem, N);
    REAL *lwL = reg_lds_ptr<REAL, TR, &RegLdsLayout::lwL>(smem, N);                   // PaRIS / O(N^2) only, like the next four
    int *paris_queue = reg_lds_ptr<int, TR, &RegLdsLayout::queue>(smem, N);
    int *paris_wq0 = reg_lds_ptr<int, TR, &RegLdsLayout::wq0>(smem, N), *paris_wq1 = reg_lds_ptr<int, TR, &RegLdsLayout::wq1>(smem, N);
    int *paris_Jres = reg_lds_ptr<int, TR, &RegLdsLayout::Jres>(smem, N);

    Math<REAL, TR::TAB> mth;
    mth.t.e2 = tabmem;
    mth.t.lg = reinterpret_cast<const double2 *>(tabmem + TAB_E2);
    mth.t.sc = reinterpret_cast<const double2 *>(tabmem + TAB_E2 + 2 * TAB_LG);
    if constexpr (TR::TABMEM) mth.t.e2g = (gptr<const double>)ExpTabMem<TR::EXPTAB_TAG>::e2;
    if (tab_bytes<REAL, RNG, TR::TAB>() > 0) tab_fill(tabmem, RNG == PFG_RNG_DEVICE, tid, NT);
    if (TR::FAST && !TR::BLK) {
#pragma unroll
        for (int k = 0; k < PPT; ++k)
            if (k * NT + tid >= N) cdf[cdf_phys(k * NT + tid)] = 2.0;      // sentinel: never <= u
    }
    __syncthreads();

    const Consts<REAL> c = make_consts<MODEL, REAL>(P.theta);
    int np2 = 1;
    while (np2 < N) np2 <<= 1;
    // measurement hooks (pfg_dev_problem.stamps): shader-clock / 100 MHz stamps at start and end;
    // per-phase cycle sums only in diagnostic builds
    if (P.stamps && tid == 0) { P.stamps[0] = __builtin_amdgcn_s_memtime(); P.stamps[1] = __builtin_amdgcn_s_memrealtime(); }
#ifdef PFG_PHASE_STAMPS
    unsigned long long ph_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long ph_prev = __builtin_amdgcn_s_memtime();
#define PFG_PH(i) { const unsigned long long ph_now = __builtin_amdgcn_s_memtime(); ph_acc[i] += ph_now - ph_prev; ph_prev = ph_now; }
#define PFG_MARK(s)
#elif defined(PFG_ISA_MARKERS)
    // tools/isa_histogram.py: phase boundaries and rarely-executed regions as comments in the ISA listing
#define PFG_PH(i) asm volatile("; PFG_PHASE " #i);
#define PFG_MARK(s) asm volatile("; PFG_MARK " s);
#else
#define PFG_PH(i)
#define PFG_MARK(s)
#endif

    LaneRng rng = {};
    if (RNG == PFG_RNG_DEVICE)
        rng = lane_rng_init(P.seed, P.stream, P.step_ctr ? *P.step_ctr : 0ull, (uint32_t)tid);
    // PPT standard normals for this thread's slots (device RNG)
    auto draw_normals = [&](REAL *zz) {
#pragma unroll
        for (int k = 0; k < PPT; k += 2) {
            REAL a, b;
            mth.normal_pair(rng.next(), rng.next(), a, b);
            zz[k] = a;
            if (k + 1 < PPT) zz[k + 1] = b;
        }
    };

    REAL lw[PPT];
    long long paris_cursor = 0;            // PaRIS in the reference's stream order: doubles of P.paris_stream consumed so far
    bool paris_overflow = false;           // ... and whether the stream ran out (the host retries with a longer one)
    // RAW (PFG_FLAG_PARIS_RAW_STREAM, PaRIS REPLAY): P.paris_stream is the window's WHOLE np.random stream as doubles
    // (RandomState.random_sample): the kernel takes from it, in np.random's order, the N resampling uniforms of a timestep,
    // its N normals and the backward sampling's uniforms -- one launch for a window whose consumption is data dependent.
    // The normals are NumPy's legacy Gaussians (legacy_gauss: Marsaglia's polar method on pairs of doubles, the second
    // variate of a pair cached for the next call): accept / reject is exact fp64 arithmetic (no contraction in the REPLAY
    // units), so the CONSUMPTION is the reference's to the double; the values go through this device's log (<= 1 ulp from
    // the host libm's), within the REPLAY tolerance.
    const bool raw = TR::RAWCAP && (P.flags & PFG_FLAG_PARIS_RAW_STREAM) != 0 && P.paris_stream != nullptr;
    bool carry_has = false;                // a cached second variate is pending (workgroup-uniform); its value sits in red_W0[1]
    double *const zbuf = reinterpret_cast<double *>(paris_queue);          // [N] normals of the current call (queue scratch is free then)
    long long *const raw_slots = reinterpret_cast<long long *>(red_W0 + 2);  // [0] cut-off attempt of a call, [1] stream position of the cached pair
    [[maybe_unused]] auto legacy_normals = [&]() {
        const gptr<const double> strm = global_ptr(P.paris_stream);
        const long long cap = P.paris_stream_len;
        const unsigned long long ltm = (1ull << lane) - 1ull;
        int *const wc = reinterpret_cast<int *>(red_scan);                 // [PPT][NW] accepted attempts per (slot, wave)
        const int produced0 = carry_has ? 1 : 0;
        __syncthreads();                                                   // queue scratch / red_scan of the previous phase are done with
        if (carry_has && tid == 0) zbuf[0] = red_W0[1];
        const int need = (N - produced0 + 1) >> 1;                         // pairs to accept
        const long long base = paris_cursor;
        int acc = 0;
        for (int round = 0; acc < need && !paris_overflow; ++round) {
            double x1[PPT], x2[PPT], r2[PPT];
            bool fl[PPT];
            int rank[PPT];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const long long p = base + 2 * ((long long)round * (NT * PPT) + k * NT + tid);
                const bool in = p + 1 < cap;
                const double d0 = in ? strm[p] : 0.5, d1 = in ? strm[p + 1] : 0.5;
                x1[k] = 2.0 * d0 - 1.0;
                x2[k] = 2.0 * d1 - 1.0;
                r2[k] = x1[k] * x1[k] + x2[k] * x2[k];
                fl[k] = in && !(r2[k] >= 1.0 || r2[k] == 0.0);
                const unsigned long long mk = __ballot(fl[k]);
                rank[k] = __popcll(mk & ltm);
                if (lane == 0) wc[k * NW + wave] = __popcll(mk);
            }
            __syncthreads();
            int S = 0;
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    if (w == wave) rank[k] += S;
                    S += wc[k * NW + w];
                }
            }
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int q = acc + rank[k];
                if (fl[k] && q < need) {
                    const double f = sqrt(-2.0 * log(r2[k]) / r2[k]);
                    const int i0 = produced0 + 2 * q;
                    zbuf[i0] = f * x2[k];                                  // returned by this call of legacy_gauss
                    const long long j = (long long)round * (NT * PPT) + k * NT + tid;
                    if (i0 + 1 < N) zbuf[i0 + 1] = f * x1[k];              // the cached one, returned by the next call
                    else { red_W0[1] = f * x1[k]; raw_slots[1] = base + 2 * j; }
                    if (q == need - 1) raw_slots[0] = j;
                }
            }
            acc += S;
            if (acc < need && base + 2 * ((long long)(round + 1) * (NT * PPT)) + 1 >= cap) paris_overflow = true;
            __syncthreads();
        }
        if (need > 0 && !paris_overflow) paris_cursor = base + 2 * (raw_slots[0] + 1);
        carry_has = ((N - produced0) & 1) != 0;
    };
    if (TR::RAWCAP && raw && (P.flags & PFG_FLAG_PARIS_RAW_CARRY)) {          // the generator came with a cached Gaussian: stream[0]
        carry_has = true;
        if (tid == 0) red_W0[1] = P.paris_stream[0];
        paris_cursor = 1;
    }
    // ---- x0 (kernels.py:83-100, garch/kernels.py:7-18) or warm start ------------------
    {
        double pv = P.prior_var;
        if (MODEL == PFG_MODEL_GARCH && (P.flags & PFG_FLAG_GARCH_STATIONARY_PRIOR))
            pv = (double)c.alpha / (1.0 - (double)c.beta - (double)c.gamma);
        const double sd = sqrt(pv);
        REAL z0[PPT];
        if (RNG == PFG_RNG_DEVICE) draw_normals(z0);
        if constexpr (TR::RAWCAP) { if (raw && !P.init_x) legacy_normals(); }
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = k * NT + tid;
            lw[k] = (REAL)0;
            if (i < N) {
                REAL x[NS], s[H];
#pragma unroll
                for (int d = 0; d < NS; ++d) x[d] = (REAL)0;
#pragma unroll
                for (int h = 0; h < H; ++h) s[h] = (REAL)0;
                if (P.init_x) {
#pragma unroll
                    for (int d = 0; d < NS; ++d) x[d] = (REAL)P.init_x[(size_t)i * NS + d];
                    lw[k] = (REAL)P.init_logw[i];
                    if (P.init_stats && !is_filter) {
#pragma unroll
                        for (int h = 0; h < H; ++h) s[h] = (REAL)P.init_stats[(size_t)i * H + h];
                    }
                } else {
                    const double z = (RNG == PFG_RNG_REPLAY) ? ((TR::RAWCAP && raw) ? zbuf[i] : P.z0[i]) : (double)z0[k];
                    x[0] = (REAL)(P.prior_mean + sd * z);
                    if (RNG == PFG_RNG_DEVICE && PFG_TR(P.trace_x) && P.rec_z0) P.rec_z0[i] = z;
                }
#pragma unroll
                for (int d = 0; d < NS; ++d) cur[sidx(d, i)] = x[d];
                if constexpr (TR::RAWSCORE) {
                    REAL r[H];
#pragma unroll
                    for (int h = 0; h < H; ++h) r[h] = s[h];
                    if (raw_score && P.init_x && P.init_stats) raw_score_in(c, s, r);      // Cw = 0 (zeros stay +0 without it)
#pragma unroll
                    for (int h = 0; h < H; ++h) cur[sidx((NS + h), i)] = r[h];
                } else {
#pragma unroll
                for (int h = 0; h < H; ++h) cur[sidx((NS + h), i)] = s[h];
                }
                if (PFG_TR(P.trace_x)) {
#pragma unroll
                    for (int d = 0; d < NS; ++d) P.trace_x[(size_t)i * NS + d] = (double)x[d];
                    P.trace_logw[i] = (double)lw[k];
                    if (P.trace_stats && !is_filter) {
#pragma unroll
                        for (int h = 0; h < H; ++h) P.trace_stats[(size_t)i * H + h] = (double)s[h];
                    }
                }
            } else if (TR::ADAPTIVE && TR::FAST) {
                // a slot beyond N reads its OWN cell on a step that does not resample (no other thread's): give it a value
#pragma unroll
                for (int d = 0; d < NS + H; ++d) cur[sidx(d, i)] = (REAL)0;
            }
        }
    }

    double ll = 0.0, wt_prev = 1.0, tie = 1.0;
    [[maybe_unused]] double Cw = 0.0;       // RAWSCORE: the window weights of the statistic steps so far
    double ll_W = 1.0, ll_w = 0.0;          // LAZYLL: lane t % 64 of wave 0 holds step t's (W, w, m)
    float ll_m = 0.0f;
    double filt[H], S[H];
#pragma unroll
    for (int h = 0; h < H; ++h) { filt[h] = 0.0; S[h] = 0.0; }
    double m = 0.0, W = (double)N;
    // slots beyond N: log-weight -inf (weight exactly 0, never an ancestor); their lanes run the
    // same straight-line code on clamped indices and only their stores are masked.
    bool valid[PPT];
    int own[PPT];                       // own particle index, clamped for reads
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        valid[k] = (k * NT + tid) < N;
        own[k] = valid[k] ? (k * NT + tid) : (N - 1);
        if (!valid[k]) lw[k] = -INFINITY;
    }
    const int last = N - 1;
    [[maybe_unused]] float m_next = 0.0f;
    if constexpr (TR::STALE) {
        // the shift of t = 0 is the exact maximum; the second barrier keeps the loop's first write of red_maxf behind
        // every wave's read
        float ml = (float)lw[0];
#pragma unroll
        for (int k = 1; k < PPT; ++k) ml = fmaxf(ml, (float)lw[k]);
        ml = wave_max(ml);
        if (lane == 0) red_maxf[wave] = ml;
        block_sync<NW>();
        float mm = red_maxf[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) mm = fmaxf(mm, red_maxf[w]);
        m = uniform_f64((double)mm);
        block_sync<NW>();
        if constexpr (TR::SHIFTFOLD) {          // the log-weights cross every loop edge as lw - shift
#pragma unroll
            for (int k = 0; k < PPT; ++k) lw[k] -= (REAL)m;
        }
    }

    for (int t = 0; t <= T; ++t) {
        [[maybe_unused]] double uu_raw[PPT];
        [[maybe_unused]] REAL zz_raw[PPT];
        if constexpr (TR::RAWCAP) {
            if (raw && t < T) {
                // np.random's order within a timestep: N uniforms (np.random.choice), N normals (Kernel.rv), then the
                // backward sampling's draws (at the end of this iteration)
                const gptr<const double> strm = global_ptr(P.paris_stream);
                if (paris_cursor + N > P.paris_stream_len) paris_overflow = true;
#pragma unroll
                for (int k = 0; k < PPT; ++k) uu_raw[k] = paris_overflow ? 0.5 : strm[paris_cursor + own[k]];
                if (!paris_overflow) paris_cursor += N;
                legacy_normals();
#pragma unroll
                for (int k = 0; k < PPT; ++k) zz_raw[k] = (REAL)zbuf[own[k]];
            }
        }
        // ---- (A) block max of the current log weights  (log_normalize, pf.py:374-377) ----
        // (SUMSHIFT: none -- the next shift comes from the scan total behind barrier 2; SHIFTFOLD alone: the maximum of lw - shift)
        [[maybe_unused]] float ml = 0.0f;
        if constexpr (!TR::SUMSHIFT) {
            ml = (float)lw[0];
#pragma unroll
            for (int k = 1; k < PPT; ++k) ml = fmaxf(ml, (float)lw[k]);
            ml = wave_max(ml);
            if (NW > 1 && lane == 0) red_maxf[wave] = ml;
        }
        PFG_PH(0)
        if constexpr (!TR::STALE) block_sync<NW>();                                 // barrier 1
        PFG_PH(1)
        if constexpr (!TR::STALE) {
            float mm = NW > 1 ? red_maxf[0] : ml;     // one wave: its maximum IS the block maximum, no LDS round trip
#pragma unroll
            for (int w = 1; w < NW; ++w) mm = fmaxf(mm, red_maxf[w]);
            m = uniform_f64((double)mm);      // f32-rounded max: a valid shift for log_normalize (see wave_max)
        }
        // ---- (B) unnormalised weights, (C) prefix scan + weighted statistic sums --------
        const bool needS = needS_every || (t == T);
        double cs[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const REAL a = TR::SHIFTFOLD ? lw[k] : (REAL)(lw[k] - (REAL)m);
            if constexpr (TR::HOT_B != 0) cs[k] = (double)mth.template exp_hot<TR::HOT_B>(a);      // (STALE: REAL is double)
            else cs[k] = (double)mth.exp(a);                                                        // exp(-inf) = 0
        }
        if (needS) {
            PFG_MARK("cold needS")
#pragma unroll
            for (int h = 0; h < H; ++h) {
                double part = 0.0;
#pragma unroll
                for (int k = 0; k < PPT; ++k) part += (double)cur[sidx((NS + h), own[k])] * cs[k];
                part = wave_sum(part);
                if (lane == 0) red_S[h * NW + wave] = part;
            }
        }
        if constexpr (TR::ADAPTIVE) {
            // sum of w^2 for the effective sample size: rides on this reduction phase, one LDS slot per wave, no barrier of its own
            if (t < T) {
                double q2 = 0.0;
#pragma unroll
                for (int k = 0; k < PPT; ++k) q2 += cs[k] * cs[k];
                q2 = wave_sum(q2);
                if (lane == 0) red_W0[4 + wave] = q2;
            }
        }
        double wave_inc = 0.0;          // BLK: this wave's inclusive scan (lane 63 = the wave total)
        float es[PPT];                  // SORTED: inclusive prefix of the exponential spacings of this thread's children (in-wave
                                        // sums < 2^9 in f32: good to 1e-5 of a spacing, half the registers across barrier 2 and a
                                        // 6-instruction wave scan; the cross-wave offsets and the normalisation are f64)
        uint32_t us[PPT];               // SORTED: the sorted uniforms as 32-bit fixed point
        if (TR::BLK) {
#pragma unroll
            for (int k = 1; k < PPT; ++k) cs[k] += cs[k - 1];
            const double inc = wave_incl_scan(cs[PPT - 1]);
            const double exc = inc - cs[PPT - 1];
#pragma unroll
            for (int k = 0; k < PPT; ++k) cs[k] += exc;
            if (NW > 1 && lane == WAVE - 1) red_scan[wave] = inc;
            wave_inc = inc;
            if (TR::SORTED && t < T) {
                // exponential spacings of this thread's (valid) children, thread-local prefix + one wave scan; the
                // (N+1)-th spacing rides in the last wave's total
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const float e = spacing_f32(rng.next());
                    es[k] = (valid[k] ? e : 0.0f) + (k > 0 ? es[k - 1] : 0.0f);
                }
                const float eincf = wave_incl_scan_f32(es[PPT - 1]);
                const float eexc = eincf - es[PPT - 1];
#pragma unroll
                for (int k = 0; k < PPT; ++k) es[k] += eexc;
                if (lane == WAVE - 1) {
                    double einc = (double)eincf;
                    if (wave == NW - 1) einc += (double)spacing_f32(rng.next());
                    red_scan[NW + wave] = einc;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                cs[k] = wave_incl_scan(cs[k]);
                if (lane == WAVE - 1) red_scan[k * NW + wave] = cs[k];
            }
        }
        if (RNG != PFG_RNG_REPLAY && TR::SYSTEMATIC && tid == 0) red_W0[0] = u01_32(rng.next());
        // this step's randomness: REPLAY loads are issued here so that their latency overlaps the
        // barrier; device draws happen right before their use (keeps register pressure down).  (Loading a timestep
        // ahead was measured, round 3: a lone window 2.90 -> 2.85 ms, 768 windows 6.85 -> 7.60 ms -- the registers
        // cost more than the latency; the REPLAY kernel's distance to the device units is its fp64 CDF and search.)
        double uu[PPT];
        REAL zz[PPT];
        if (t < T && RNG == PFG_RNG_REPLAY) {
            if (TR::RAWCAP && raw) {
#pragma unroll
                for (int k = 0; k < PPT; ++k) { uu[k] = uu_raw[k]; zz[k] = zz_raw[k]; }
            } else {
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    uu[k] = uv[(size_t)t * N + own[k]];
                    zz[k] = (REAL)zv[(size_t)t * N + own[k]];
                }
            }
        }
        PFG_PH(2)
        block_sync<NW>();                                                       // barrier 2
        PFG_PH(3)
        if (TR::BLK && NW == 1) {
            // one wave: no other totals to add, W is the scan's last lane
            W = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(wave_inc), WAVE - 1),
                                 __builtin_amdgcn_readlane(__double2loint(wave_inc), WAVE - 1));
        } else if (TR::BLK) {
            // NW wave totals: exclusive prefix by a DPP scan over the first lanes
            const double tot = (lane < NW) ? red_scan[lane] : 0.0;
            double inc = tot;
            inc += dpp_shr0_f64<0x111>(inc);
            inc += dpp_shr0_f64<0x112>(inc);
            if (NW > 4) { inc += dpp_shr0_f64<0x114>(inc); inc += dpp_shr0_f64<0x118>(inc); }
            const double exc = inc - tot;
            const double off = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(exc), wave),
                                                __builtin_amdgcn_readlane(__double2loint(exc), wave));
#pragma unroll
            for (int k = 0; k < PPT; ++k) cs[k] += off;
            W = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(inc), NW - 1),
                                 __builtin_amdgcn_readlane(__double2loint(inc), NW - 1));
            if constexpr (TR::STALE) {
                bool retry;
                if constexpr (TR::SUMSHIFT) {
                    // the range guard on W's high word (every wave holds the same bits): 2^-728 <= W < 2^728, see PFG_OPT_SUMSHIFT
                    constexpr uint32_t W_LO = (uint32_t)(1023 - 728) << 20, W_HI = (uint32_t)(1023 + 728) << 20;
                    retry = t > 0 && !((uint32_t)__double2hiint(W) - W_LO < W_HI - W_LO);
                } else {
                    // this step's exact maximum: the next step's shift, and the range guard of this one (NaN, +-inf fail it)
                    float mm = red_maxf[0];
#pragma unroll
                    for (int w = 1; w < NW; ++w) mm = fmaxf(mm, red_maxf[w]);
                    if constexpr (TR::SHIFTFOLD) mm += (float)m;
                    m_next = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, mm)));
                    retry = t > 0 && !(fabsf(m_next - (float)m) <= 512.0f);
                }
                if (retry) {
                    PFG_MARK("cold stale-shift-retry")
                    block_sync<NW>();
                    if constexpr (!TR::SUMSHIFT) m = uniform_f64((double)m_next);
                    const REAL y_p = (REAL)yv[t - 1], y2_p = y_p * y_p;
                    REAL lwk[PPT];
#pragma unroll
                    for (int k = 0; k < PPT; ++k) {
                        const REAL x1 = cur[sidx(0, own[k])];
                        lwk[k] = valid[k] ? svm_logw(c, x1, mth.exp_finite(-x1), y2_p) : (REAL)(-INFINITY);
                        if constexpr (!TR::SUMSHIFT) cs[k] = (double)mth.exp((REAL)(lwk[k] - (REAL)m));
                    }
                    if constexpr (TR::SUMSHIFT) {
                        // the exact block maximum as the shift, as in the t = 0 prologue (red_maxf is idle in the T-loop: every
                        // earlier read of it lies behind at least this retry's first barrier)
                        float rl = (float)lwk[0];
#pragma unroll
                        for (int k = 1; k < PPT; ++k) rl = fmaxf(rl, (float)lwk[k]);
                        rl = wave_max(rl);
                        if (lane == 0) red_maxf[wave] = rl;
                        block_sync<NW>();
                        float mm = red_maxf[0];
#pragma unroll
                        for (int w = 1; w < NW; ++w) mm = fmaxf(mm, red_maxf[w]);
                        m = uniform_f64((double)mm);
#pragma unroll
                        for (int k = 0; k < PPT; ++k) cs[k] = (double)mth.exp((REAL)(lwk[k] - (REAL)m));
                    }
                    if constexpr (TR::SHIFTFOLD) {          // final_logw of a retry at t = T
#pragma unroll
                        for (int k = 0; k < PPT; ++k) lw[k] = lwk[k] - (REAL)m;
                    }
                    if (needS) {
#pragma unroll
                        for (int h = 0; h < H; ++h) {
                            double part = 0.0;
#pragma unroll
                            for (int k = 0; k < PPT; ++k) part += (double)cur[sidx((NS + h), own[k])] * cs[k];
                            part = wave_sum(part);
                            if (lane == 0) red_S[h * NW + wave] = part;
                        }
                    }
#pragma unroll
                    for (int k = 1; k < PPT; ++k) cs[k] += cs[k - 1];
                    const double inc2 = wave_incl_scan(cs[PPT - 1]);
                    const double exc2 = inc2 - cs[PPT - 1];
#pragma unroll
                    for (int k = 0; k < PPT; ++k) cs[k] += exc2;
                    if (lane == WAVE - 1) red_scan[wave] = inc2;
                    block_sync<NW>();
                    const double tot2 = (lane < NW) ? red_scan[lane] : 0.0;
                    double incw = tot2;
                    incw += dpp_shr0_f64<0x111>(incw);
                    incw += dpp_shr0_f64<0x112>(incw);
                    const double excw = incw - tot2;
                    const double off2 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(excw), wave),
                                                         __builtin_amdgcn_readlane(__double2loint(excw), wave));
#pragma unroll
                    for (int k = 0; k < PPT; ++k) cs[k] += off2;
                    W = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(incw), NW - 1),
                                         __builtin_amdgcn_readlane(__double2loint(incw), NW - 1));
                }
                if constexpr (TR::SUMSHIFT) {
                    // the next shift: s + ln2 * e, W = f 2^e with f in [0.5, 1) -- the f32 value within ln 2 above the step's
                    // log-sum-exp.  (W out of range at t = 0 or after the retry: whatever comes out is caught by the next guard)
                    const int e = (int)(((uint32_t)__double2hiint(W) >> 20) & 0x7ffu) - 1022;
                    const float sn = fmaf((float)e, 0.693147180559945f, (float)m);
                    m_next = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sn)));
                }
            }
            if (TR::SORTED && t < T) {
                const double totE = (lane < NW) ? red_scan[NW + lane] : 0.0;
                double incE = totE;
                incE += dpp_shr0_f64<0x111>(incE);
                incE += dpp_shr0_f64<0x112>(incE);
                incE += dpp_shr0_f64<0x114>(incE);
                incE += dpp_shr0_f64<0x118>(incE);
                const double excE = incE - totE;
                const double offE = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(excE), wave),
                                                     __builtin_amdgcn_readlane(__double2loint(excE), wave));
                const double Etot = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(incE), NW - 1),
                                                     __builtin_amdgcn_readlane(__double2loint(incE), NW - 1));
                const double fe = uniform_f64(rcp_newton2(Etot) * 4294967296.0);
#pragma unroll
                for (int k = 0; k < PPT; ++k) us[k] = cvt_u32_sat(((double)es[k] + offE) * fe);
            }
        } else if (PPT * NW <= 16) {
            // lane j < PPT*NW holds total j; exclusive prefix by a 16-lane DPP scan; each thread
            // picks its PPT offsets and the grand total with v_readlane (uniform indices)
            double tot = (lane < PPT * NW) ? red_scan[lane] : 0.0;
            double inc = tot;
            inc += dpp_shr0_f64<0x111>(inc);
            inc += dpp_shr0_f64<0x112>(inc);
            inc += dpp_shr0_f64<0x114>(inc);
            inc += dpp_shr0_f64<0x118>(inc);
            const double exc = inc - tot;
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int j = k * NW + wave;
                cs[k] += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(exc), j),
                                          __builtin_amdgcn_readlane(__double2loint(exc), j));
            }
            W = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(inc), PPT * NW - 1),
                                 __builtin_amdgcn_readlane(__double2loint(inc), PPT * NW - 1));
        } else {
            double run = 0.0;
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                double off = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    off = (w == wave) ? run : off;
                    run += red_scan[k * NW + w];
                }
                cs[k] += off;
            }
            W = uniform_f64(run);
        }
        const double invW = uniform_f64(PFG_OPT_RCPW ? rcp_newton2(W) : 1.0 / W);
        // ADAPTIVE: resample iff ESS = W^2 / sum w^2 < tau N.  Workgroup-uniform by construction: every wave adds the same NW
        // LDS slots in the same order, W is the same scan of the same LDS totals in every wave, and the result is made scalar
        // -- barriers 3 and 4 are skipped under it
        [[maybe_unused]] bool resample = true;
        if constexpr (TR::ADAPTIVE) {
            if (t < T) {
                double W2 = red_W0[4];
#pragma unroll
                for (int w = 1; w < NW; ++w) W2 += red_W0[4 + w];
                resample = __builtin_amdgcn_readfirstlane((int)(W * W < tauN * W2)) != 0;
            }
        }
        if (needS) {
            PFG_MARK("cold needS")
#pragma unroll
            for (int h = 0; h < H; ++h) {
                double acc = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) acc += red_S[h * NW + w];
                S[h] = uniform_f64(acc * invW);
            }
        }
        // log-likelihood increment of the step that produced these weights
        // (buffered_smoother.py:124-126): log(mean(exp(logw))) = m + log(W/N).  Wave 0 only.
        if (wave == 0) {
            PFG_MARK("w0.25 wave0-loglik")
            const bool counts = t > 0 && (t - 1) >= t1 && (t - 1) < tL;
            if (TR::LAZYLL) {
                const bool mine = lane == (t & (WAVE - 1));
                ll_W = mine ? W : ll_W;
                ll_w = mine ? (counts ? wt_prev : 0.0) : ll_w;
                ll_m = mine ? (float)m : ll_m;          // m is an f32 value
                // (TWINLESS_LL -- STRATIFIED, SYSTEMATIC, N2, ...: one instantiation serves traced and production launches, so a
                // traced running value must not move the flushes -- the parked terms are summed for the trace alone and `ll` is
                // bitwise the production one)
                const bool due = (t & (WAVE - 1)) == WAVE - 1 || t == T;
                if (due || (!TR::TWINLESS_LL && PFG_TR(P.trace_ll))) {
                    PFG_MARK("cold loglik-flush")
                    const double term = ll_w * ((double)ll_m + (double)mth.log((REAL)(ll_W * invN)));
                    ll = uniform_f64(ll + wave_sum(term));
                    ll_w = 0.0;
                } else if (TR::TWINLESS_LL && PFG_TR(P.trace_ll)) {
                    const double term = ll_w * ((double)ll_m + (double)mth.log((REAL)(ll_W * invN)));
                    const double run = ll + wave_sum(term);
                    if (tid == 0) P.trace_ll[t] = run;
                }
                if ((due || !TR::TWINLESS_LL) && PFG_TR(P.trace_ll) && tid == 0) P.trace_ll[t] = ll;
            } else {
                if (counts) ll = uniform_f64(ll + wt_prev * (m + log(W / (double)N)));
                if (PFG_TR(P.trace_ll) && tid == 0) P.trace_ll[t] = ll;
            }
        }
        if (is_filter && t > 0) {
            PFG_MARK("cold filter")
#pragma unroll
            for (int h = 0; h < H; ++h) filt[h] = uniform_f64(filt[h] + S[h]);
        }
        if (t == T) break;
        if constexpr (TR::STALE) m = uniform_f64((double)m_next);      // the log-likelihood above used the shift W was formed with

        // ---- (D) normalised CDF to LDS (RandomState.choice: cumsum, /= last) -------------
        const double y_t = yv[t];
        const bool inside = (t >= t1) && (t < tL);
        const double wt = (inside && wv) ? wv[t - t1] : 1.0;
        const bool use_stat = inside && (stat != PFG_STAT_NONE);
        const bool plain = !needS_every;                 // not filter and lambda == 1
        if (!TR::ADAPTIVE || resample) {            // (ADAPTIVE: phases D and E only on a step that resamples)
        if (TR::BLK) {
            // all PPT positions: slots beyond N carry weight 0 (flat CDF, never selected)
            {
                const double fixs = invW * 4294967296.0;
#pragma unroll
                for (int k = 0; k < PPT; ++k)
                    cdfu[cdf_phys(tid * PPT + k)] = cvt_u32_sat(cs[k] * fixs);
            }
        } else {
#pragma unroll
            for (int k = 0; k < PPT; ++k)
                if (valid[k]) {
                    cdf[TR::FAST ? cdf_phys(k * NT + tid) : k * NT + tid] = cs[k] * invW;
                    if (TR::PARIS || TR::N2) lwL[k * NT + tid] = lw[k];
                }
        }
        PFG_PH(4)
        block_sync<NW>();                                                       // barrier 3
        PFG_PH(5)
        if (TR::PRIO == 1) __builtin_amdgcn_s_setprio(2);                           // the LDS-heavy phases E, F: see PRIO
        if (TR::PRIO == 2) __builtin_amdgcn_s_setprio(0);

        // ---- (E) ancestors: smallest j with cdf[j] > u (searchsorted 'right').  Branch-free:
        // probes past the end read cdf[N-1] (= 1 > u), the final clamp covers rounding.
        if (RNG != PFG_RNG_REPLAY) {
            if (TR::SYSTEMATIC) {
                // extension: one uniform per timestep (drawn by thread 0 before barrier 2)
                const double u0 = red_W0[0];
#pragma unroll
                for (int k = 0; k < PPT; ++k) uu[k] = ((double)(k * NT + tid) + u0) * invN;
                if (PFG_TR(P.trace_x) && P.rec_ud) {          // test instrumentation, as for STRATIFIED
#pragma unroll
                    for (int k = 0; k < PPT; ++k)
                        if (valid[k]) P.rec_ud[(size_t)t * N + k * NT + tid] = uu[k];
                }
            } else if (TR::STRATIFIED) {
                // extension: child r = k NT + tid searches with (r + U_r) / N, U_r from the lane that owns it
#pragma unroll
                for (int k = 0; k < PPT; ++k) uu[k] = ((double)(k * NT + tid) + u01_32(rng.next())) * invN;
                if (PFG_TR(P.trace_x) && P.rec_ud) {          // test instrumentation: the uniforms this launch searched with
#pragma unroll
                    for (int k = 0; k < PPT; ++k)
                        if (valid[k]) P.rec_ud[(size_t)t * N + k * NT + tid] = uu[k];
                }
            } else if (!TR::BLK) {
#pragma unroll
                for (int k = 0; k < PPT; ++k) uu[k] = u01_32(rng.next());
                if (TR::ADAPTIVE && PFG_TR(P.trace_x) && P.rec_ud) {      // test instrumentation, as for STRATIFIED
#pragma unroll
                    for (int k = 0; k < PPT; ++k)
                        if (valid[k]) P.rec_ud[(size_t)t * N + k * NT + tid] = uu[k];
                }
            }
        } else if (TR::STRATIFIED) {
            // REPLAY: U_r is the caller's u[t][r]; one addition and one IEEE division (pfgrad.h, PFG_SMOOTHER_NEMETH_STRATIFIED)
#pragma unroll
            for (int k = 0; k < PPT; ++k) uu[k] = ((double)(k * NT + tid) + uu[k]) / (double)N;
        }
        }
        int anc[PPT];
        [[maybe_unused]] uint32_t gaddr[PPT];       // GADDR: byte offset of the parent's record in a state array
#pragma unroll
        for (int k = 0; k < PPT; ++k) { anc[k] = 0; gaddr[k] = 0u; }
        if (!TR::ADAPTIVE || resample) {
        if (TR::BLK) {
            uint32_t ua[PPT];
#pragma unroll
            for (int k = 0; k < PPT; ++k) ua[k] = TR::SORTED ? us[k] : rng.next();
#ifdef PFG_EXP_EVENWORDS
            // knock-out (timing only, NOT a valid resampler): evenly spaced words in CDF order -- what sorted uniforms
            // would do to the LDS bank conflicts of the search and the gathers, without their cost
#pragma unroll
            for (int k = 0; k < PPT; ++k) ua[k] = (uint32_t)(((uint64_t)(tid * PPT + k) << 32) / (uint64_t)(NT * PPT)) + (ua[k] >> 12);
#endif
            if (PFG_TR(P.trace_x) && P.rec_u) {           // test instrumentation: the words this launch searched with
#pragma unroll
                for (int k = 0; k < PPT; ++k)
                    if (valid[k]) P.rec_u[(size_t)t * N + k * NT + tid] = ua[k];
            }
            // the search runs on BYTE offsets into the CDF (the LDS address itself: probe offsets fold into the
            // ds_read immediates and a level costs compare + select + add, no address arithmetic)
            using lds_u32 = const __attribute__((address_space(3))) uint32_t;
            const uint32_t cdf_base = (uint32_t)(uintptr_t)(lds_u32 *)cdfu;
            uint32_t off[PPT];
#pragma unroll
            for (int k = 0; k < PPT; ++k) off[k] = cdf_base;
            constexpr int FIRST_STEP = TR::PIVOTS ? 128 : (NT * PPT) >> 1;
            if constexpr (TR::PIVOTS) {
                const uint32_t p511 = __builtin_amdgcn_readfirstlane(cdfu[cdf_phys(511)]);
                const uint32_t p255 = __builtin_amdgcn_readfirstlane(cdfu[cdf_phys(255)]);
                const uint32_t p767 = __builtin_amdgcn_readfirstlane(cdfu[cdf_phys(767)]);
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const bool g1 = p511 <= ua[k];
                    const uint32_t t2 = g1 ? p767 : p255;
                    const bool g2 = t2 <= ua[k];
                    off[k] += (g1 ? 4u * (512 + 16) : 0u) + (g2 ? 4u * (256 + 8) : 0u);
                }
            }
#pragma unroll
            for (int step = FIRST_STEP; step >= 1; step >>= 1) {
                const int probe = step - 1 + (step >= 32 ? (step >> 5) - 1 : 0);
                const int adv = step + (step >> 5);
                uint32_t cv[PPT];
#pragma unroll
                for (int k = 0; k < PPT; ++k) cv[k] = *(lds_u32 *)(uintptr_t)(off[k] + 4u * probe);
                if constexpr (PFG_OPT_SEL32 && NT >= 512) {
                // the advanced offset is formed while the probe is in flight; compare + select in the VOP2 forms
                // (v_cmp_le_u32 vcc / v_cndmask_b32 with the implicit vcc).  The compiler's own lowering selects
                // between 0 and the advance with the VOP3 form, which reads vcc as an SGPR operand: two wait states
                // behind the compare, 22 s_nop per lane-timestep in this loop.  Measured (ms per bench launch, with /
                // without): 512 x 2 GARCH 2.86 / 2.95, 1024 x 4 12.68 / 12.76, one wave 1.73 / 1.73, but 256 x 4 SVM
                // 52.3 / 51.5 -- there the glued pairs keep the scheduler from weaving the generator's integer work
                // into the search, which hides more than the wait states cost; so only for NT >= 512.
                uint32_t cand[PPT];
#pragma unroll
                for (int k = 0; k < PPT; ++k) cand[k] = off[k] + 4u * adv;
#pragma unroll
                for (int k = 0; k < PPT; ++k)
                    asm("v_cmp_le_u32_e32 vcc, %1, %2\n\tv_cndmask_b32_e32 %0, %3, %4, vcc"
                        : "=v"(off[k]) : "v"(cv[k]), "v"(ua[k]), "v"(off[k]), "v"(cand[k]) : "vcc");
                } else {
#pragma unroll
                for (int k = 0; k < PPT; ++k) off[k] += (cv[k] <= ua[k]) ? 4u * adv : 0u;
                }
            }
            if constexpr (TR::GADDR) {
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const uint32_t rel = off[k] - cdf_base;
                    // p4 = rel - 4 q in ONE multiply-add (the compiler's own form is shift, mask, subtract)
                    const uint32_t q = __umul24(rel, 993u) >> 17;
                    uint32_t p4;
                    asm("v_mad_i32_i24 %0, %1, -4, %2" : "=v"(p4) : "v"(q), "v"(rel));
                    const uint32_t a = __umul24(p4, 1025u) & 0x3ff0u;
                    gaddr[k] = min(a, 16u * (uint32_t)last);
                    if constexpr (TRACE) anc[k] = (int)(gaddr[k] >> 4);
                }
            } else
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                uint32_t p = (off[k] - cdf_base) >> 2;
                p -= __umul24(p, 993u) >> 15;                                   // physical -> CDF position (p < 2^15)
                anc[k] = (int)(((p << (NT == 256 ? 8 : (NT == 512 ? 9 : (NT == 1024 ? 10 : 6)))) & (uint32_t)((PPT - 1) * NT)) | (p >> TR::LOG_PPT));   // -> particle index
            }
        } else if (TR::FAST) {
            // sentinel-padded cdf, physical positions: log2(NT*PPT) fixed probes whose offsets
            // fold into the ds_read immediates; logical index recovered once at the end
            // on byte offsets, like the 32-bit search above (the LDS address is the search variable)
            using lds_f64 = const __attribute__((address_space(3))) double;
            const uint32_t cdf_base = (uint32_t)(uintptr_t)(lds_f64 *)cdf;
            uint32_t off[PPT];
#pragma unroll
            for (int k = 0; k < PPT; ++k) off[k] = cdf_base;
#pragma unroll
            for (int step = (NT * PPT) >> 1; step >= 1; step >>= 1) {
                const int probe = step - 1 + (step >= 32 ? (step >> 5) - 1 : 0);
                const int adv = step + (step >> 5);
                double cv[PPT];
#pragma unroll
                for (int k = 0; k < PPT; ++k) cv[k] = *(lds_f64 *)(uintptr_t)(off[k] + 8u * probe);
#pragma unroll
                for (int k = 0; k < PPT; ++k) off[k] += (cv[k] <= uu[k]) ? 8u * adv : 0u;
            }
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const uint32_t p = (off[k] - cdf_base) >> 3;
                anc[k] = (int)(p - (__umul24(p, 993u) >> 15));                  // p - p/33 (exact for p < 32768)
            }
        } else {
            for (int step = np2 >> 1; step >= 1; step >>= 1) {
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    int idx = anc[k] + step - 1;
                    idx = idx < last ? idx : last;
                    anc[k] += (cdf[idx] <= uu[k]) ? step : 0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PPT; ++k) anc[k] = anc[k] < last ? anc[k] : last;
        if constexpr (TR::GADDR && TRACE) {
            // GADDR gathers by address: the index exists for the trace alone and is stored at once, not held across phases F-H
            if (P.trace_x && P.trace_anc) {
#pragma unroll
                for (int k = 0; k < PPT; ++k)
                    if (valid[k]) P.trace_anc[(size_t)t * N + k * NT + tid] = anc[k];
            }
        }
#ifdef PFG_EXP_OWNGATHER
        // knock-out (timing / counters only, NOT a valid resampler): the real search runs (its result is kept alive), but
        // every child gathers its OWN slot -- conflict-free lane <-> particle reads: what is left of SQ_LDS_BANK_CONFLICT is
        // the search's share (profiles/r04_lds_conflict_split.txt)
#pragma unroll
        for (int k = 0; k < PPT; ++k) { asm volatile("" :: "v"(anc[k])); anc[k] = valid[k] ? k * NT + tid : 0; }
#endif
        if (RNG == PFG_RNG_REPLAY) {
            // near-tie margin: how close u came to flipping an ancestor index
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const double hi = cdf[TR::FAST ? cdf_phys(anc[k]) : anc[k]] - uu[k];
                const double lo = anc[k] > 0 ? uu[k] - cdf[TR::FAST ? cdf_phys(anc[k] - 1) : anc[k] - 1] : 1.0;
                const double mg = hi < lo ? hi : lo;
                tie = (valid[k] && mg < tie) ? mg : tie;
            }
        }
        } else {
            // ADAPTIVE, ESS >= tau N: child i is parent i -- thread and particle coincide, so the state is read from and
            // written to this thread's own cells (slots beyond N: their own cell too) and no barrier orders anything
#pragma unroll
            for (int k = 0; k < PPT; ++k) { anc[k] = (TR::FAST || valid[k]) ? k * NT + tid : last; gaddr[k] = 0u; }
        }
        // ... and its log-weight carries on: base = (logw - m) - log(sum exp(logw - m)) + log N, in the log domain
        [[maybe_unused]] double lse = 0.0, lgN = 0.0;
        if constexpr (TR::ADAPTIVE) {
            if (!resample) { lse = uniform_f64(log(W)); lgN = uniform_f64(log((double)N)); }
        }
        PFG_PH(6)
        // ---- (F) gather parents, (G) propose / weight / statistic, (H) publish children ---
        auto slots = [&](auto stat_tag) {
            constexpr int STAT = decltype(stat_tag)::value;
            if (STAT != PFG_STAT_SCORE) { PFG_MARK("cold sufficient-statistics") }
            REAL xp[PPT][NS], sp[PPT][H];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                if constexpr (TR::PAIRED) {
                    typedef double dv2 __attribute__((ext_vector_type(2)));
                    REAL rec[NS + H];
#pragma unroll
                    for (int p = 0; p < (NS + H) / 2; ++p) {
                        dv2 v;
                        if constexpr (TR::GADDR) {
                            using lds_byte = const __attribute__((address_space(3))) unsigned char;
                            v = *(const __attribute__((address_space(3))) dv2 *)((lds_byte *)cur + gaddr[k] + (uint32_t)(p * 16 * NLS));
                        } else {
                            v = *reinterpret_cast<const dv2 *>(&cur[sidx(2 * p, anc[k])]);
                        }
                        rec[2 * p] = (REAL)v.x; rec[2 * p + 1] = (REAL)v.y;
                    }
#pragma unroll
                    for (int d = 0; d < NS; ++d) xp[k][d] = rec[d];
#pragma unroll
                    for (int h = 0; h < H; ++h) sp[k][h] = rec[NS + h];
                } else {
#pragma unroll
                for (int d = 0; d < NS; ++d) xp[k][d] = cur[sidx(d, anc[k])];
#pragma unroll
                for (int h = 0; h < H; ++h) sp[k][h] = cur[sidx((NS + h), anc[k])];
                }
            }
            PFG_PH(7)
            if (TR::PRIO == 1) __builtin_amdgcn_s_setprio(0);
            if (TR::PRIO == 2) __builtin_amdgcn_s_setprio(2);
            if (!PP && (!TR::ADAPTIVE || resample)) block_sync<NW>();           // barrier 4 (single buffer)
            PFG_PH(8)
            if (RNG != PFG_RNG_REPLAY) {
                draw_normals(zz);
                if (PFG_TR(P.trace_x) && P.rec_z) {
#pragma unroll
                    for (int k = 0; k < PPT; ++k)
                        if (valid[k]) P.rec_z[(size_t)t * N + k * NT + tid] = (double)zz[k];
                }
            }
            // One straight-line block per case: the case is uniform, so it is decided once per timestep and
            // not per particle, and the stores of a FAST layout are unconditional (a slot beyond N has its own
            // LDS cell and weight 0) -- the PPT particle chains stay in one basic block for the scheduler.
#if PFG_OPT_SHIFTFOLD
            // SHIFTFOLD (A/B builds; the closures of every kernel of such a build capture one more variable): m is already the next
            // step's shift here; the children's log-weights are born as lw - m, the shift riding in svm_logw's constant (one add per
            // timestep, wave-uniform: scalar registers)
            [[maybe_unused]] REAL k0_shifted = (REAL)0;
            if constexpr (TR::SHIFTFOLD) k0_shifted = (REAL)uniform_f64((double)(c.c0 + c.logLRinv) - m);
#endif
            auto children = [&](auto upd_tag) {
                constexpr int UPD = decltype(upd_tag)::value;      // 0 plain + statistic, 1 plain, no statistic, 2 general
                // RAWSCORE: plain + statistic with STAT = score IS the statistic step of a raw window; the step hands out the raw factors
                constexpr bool RAWUPD = TR::RAWSCORE && STAT == PFG_STAT_SCORE && UPD == 0;
                [[maybe_unused]] constexpr int TUNE = RAWUPD ? TR::STEP_TUNE : (TR::STEP_TUNE & ~PFG_STEP_RAWSCORE);
                if (UPD == 1) { PFG_MARK("cold children-outside-window") }
                if (UPD == 2) { PFG_MARK("cold children-general") }
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    REAL xn[NS], add[H], lwn;
#ifdef PFG_FAST_ALGEBRA
#if PFG_OPT_SHIFTFOLD
                    if constexpr (TR::STEP_TUNE != 0) particle_step_svm_tuned<STAT, TUNE>(c, mth, xp[k], (REAL)y_t, zz[k], xn, lwn, add, k0_shifted);
#else
                    if constexpr (TR::STEP_TUNE != 0) particle_step_svm_tuned<STAT, TUNE>(c, mth, xp[k], (REAL)y_t, zz[k], xn, lwn, add, (REAL)0);
#endif
                    else
#endif
                    particle_step<MODEL, KERNEL, STAT, REAL>(c, mth, xp[k], (REAL)y_t, zz[k], xn, lwn, add);
                    if constexpr (TR::ADAPTIVE) {
                        if (!resample) lwn = (REAL)(((((double)lw[k] - m) - lse) + lgN) + (double)lwn);
                    }
                    lw[k] = valid[k] ? lwn : (REAL)(-INFINITY);
                    if constexpr (RAWUPD) {
                        // raw sums: r0 += (w_t y^2) e, r1 += (w_t z) z, r2 += (w_t z) xp
                        const REAL y2 = (REAL)y_t * (REAL)y_t, wy2 = (REAL)wt * y2;     // wave-uniform: once per timestep
                        const REAL zw = (REAL)wt * add[1];
                        sp[k][0] = fma(wy2, add[0], sp[k][0]);
                        sp[k][1] = fma(zw, add[1], sp[k][1]);
                        sp[k][2] = fma(zw, add[2], sp[k][2]);
                    } else if (UPD == 0) {
                        // Poyiadjis O(N), lambda = 1: 1*s[a] + 0*S + w_t h = s[a] + w_t h exactly
#pragma unroll
                        for (int h = 0; h < H; ++h) sp[k][h] = sp[k][h] + add[h] * (REAL)wt;
                    } else if (UPD == 2) {
#pragma unroll
                        for (int h = 0; h < H; ++h) {
                            const REAL a = use_stat ? add[h] * (REAL)wt : (REAL)0;
                            // pf.py:175-179 / :78-80
                            const REAL sm = (lam * sp[k][h] + oml * (REAL)S[h]) + a;
                            sp[k][h] = is_filter ? a : sm;
                        }
                    }
                    // (1024 threads: the guarded store keeps the particles in separate blocks -- 19 instead of 27
                    // spilled registers at the 128-VGPR cap, 13.1 instead of 14.5 ms per config-4 launch)
                    if ((TR::FAST && NT < 1024) || valid[k]) {
                        const int i = k * NT + tid;
                        if constexpr (TR::PAIRED) {
                            typedef double dv2 __attribute__((ext_vector_type(2)));
                            REAL rec[NS + H];
#pragma unroll
                            for (int d = 0; d < NS; ++d) rec[d] = xn[d];
#pragma unroll
                            for (int h = 0; h < H; ++h) rec[NS + h] = sp[k][h];
#pragma unroll
                            for (int p = 0; p < (NS + H) / 2; ++p) {
                                dv2 v;
                                v.x = (double)rec[2 * p]; v.y = (double)rec[2 * p + 1];
                                *reinterpret_cast<dv2 *>(&nxt[sidx(2 * p, i)]) = v;
                            }
                        } else {
#pragma unroll
                        for (int d = 0; d < NS; ++d) nxt[sidx(d, i)] = xn[d];
#pragma unroll
                        for (int h = 0; h < H; ++h) nxt[sidx((NS + h), i)] = sp[k][h];
                        }
                    }
                }
            };
            if (!plain) children(std::integral_constant<int, 2>{});
            else if (use_stat) children(std::integral_constant<int, 0>{});
            else children(std::integral_constant<int, 1>{});
        };
        // PaRIS (pf.py:183-341): children are proposed from the filter's ancestors as above, then
        // every child draws Ntilde parents from the backward kernel  w_k q(child | x_k)  by
        // accept-reject against the filter weights (exact categorical fallback after
        // max_accept_reject rounds) and averages  stats[J] + w_t h(x_J, child)  over them.
        auto paris_slots = [&](auto stat_tag) {
            constexpr int STAT = decltype(stat_tag)::value;
            const int Nt = P.Ntilde, R = P.max_accept_reject;
            const double *__restrict__ const pidx = P.paris_idx_u;
            const double *__restrict__ const pacc = P.paris_acc_u;
            const double *__restrict__ const pman = P.paris_man_u;
            int *queue = paris_queue;                               // [<= N] children left to the fallback
            int *qcount = reinterpret_cast<int *>(red_max) + NW;    // behind the NW floats of red_maxf
            // ---- 1. propose every child from its filter ancestor and publish x' -------------
            if (RNG != PFG_RNG_REPLAY) {
                draw_normals(zz);
                if (PFG_TR(P.trace_x) && P.rec_z) {       // test instrumentation, as in the plain kernel
#pragma unroll
                    for (int k = 0; k < PPT; ++k)
                        if (valid[k]) P.rec_z[(size_t)t * N + k * NT + tid] = (double)zz[k];
                }
            }
            REAL xn[PPT][NS], lwn[PPT], aux[PPT], sacc[PPT][H];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                REAL xp[NS], add[H];
#pragma unroll
                for (int d = 0; d < NS; ++d) xp[d] = cur[sidx(d, anc[k])];
                particle_step<MODEL, KERNEL, STAT, REAL>(c, mth, xp, (REAL)y_t, zz[k], xn[k], lwn[k], add);
                aux[k] = (MODEL == PFG_MODEL_SVM) ? mth.exp(-xn[k][0]) : (REAL)0;
#pragma unroll
                for (int h = 0; h < H; ++h) sacc[k][h] = (REAL)0;
                if (valid[k]) {
#pragma unroll
                    for (int d = 0; d < NS; ++d) nxt[sidx(d, k * NT + tid)] = xn[k][d];
                }
            }
            // wave-local work queues of pending children (this wave's NT*PPT/NW slots of two [NL]
            // arrays) and the accepted parent of every child of the current backward draw
            int *const wq0 = paris_wq0 + wave * (PPT * WAVE);
            int *const wq1 = paris_wq1 + wave * (PPT * WAVE);
            int *const Jres = paris_Jres;
            const unsigned long long ltmask = (1ull << lane) - 1ull;
            const bool ordered = RNG == PFG_RNG_REPLAY && P.paris_stream != nullptr;
            for (int j = 0; j < Nt; ++j) {
                // ---- 2. accept-reject against the filter weights, up to R rounds per child ------
                // Pending children sit compacted in a wave-local queue.  While more than half a
                // wave is pending each lane tries one candidate for one child per pass; below that
                // a child gets K = 2^k <= 64/pending CONSECUTIVE rounds in one pass (K lanes, the
                // first accepting round wins -- exactly the sequential outcome, also on replayed
                // pools), so the long tail of rounds costs a handful of passes.
                int *qa = wq0, *qb = wq1;
                int cnt = 0;
                if (!ordered) {
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const unsigned long long mk = __ballot(valid[k]);
                    if (valid[k]) qa[cnt + __popcll(mk & ltmask)] = k * NT + tid;
                    cnt += __popcll(mk);
                }
                }
                auto candidate = [&](int child, int round, bool act, int &Iout) {
                    double u1, u2;
                    if (RNG == PFG_RNG_REPLAY) {
                        const size_t at = (((size_t)t * Nt + j) * R + (act ? round : 0)) * N + child;
                        u1 = pidx[at]; u2 = pacc[at];
                    } else { u1 = u01_32(rng.next()); u2 = u01_32(rng.next()); }
                    int I = 0;
#pragma unroll
                    for (int step = (NT * PPT) >> 1; step >= 1; step >>= 1) {
                        const int probe = step - 1 + (step >= 32 ? (step >> 5) - 1 : 0);
                        I += (cdf[I + probe] <= u1) ? step + (step >> 5) : 0;
                    }
                    I -= (I * 993) >> 15;
                    I = I < last ? I : last;
                    REAL xI[NS], xc[NS];
#pragma unroll
                    for (int d = 0; d < NS; ++d) { xI[d] = cur[sidx(d, I)]; xc[d] = nxt[sidx(d, child)]; }
                    const double thr = (double)mth.exp(backward_log_ratio<MODEL, REAL>(c, mth, xI, xc));
                    Iout = I;
                    return act && u2 <= thr;
                };
                int r0 = 0;
                while (cnt > 0 && r0 < R) {                       // wave-uniform
                    __builtin_amdgcn_wave_barrier();
                    int ncnt = 0;
                    if (cnt > WAVE / 2) {
                        for (int e0 = 0; e0 < cnt; e0 += WAVE) {
                            const int e = e0 + lane;
                            const bool act = e < cnt;
                            const int child = qa[act ? e : 0];
                            int I;
                            const bool acc = candidate(child, r0, act, I);
                            if (acc) Jres[child] = I;
                            const bool rej = act && !acc;
                            const unsigned long long mk = __ballot(rej);
                            if (rej) qb[ncnt + __popcll(mk & ltmask)] = child;
                            ncnt += __popcll(mk);
                        }
                        r0 += 1;
                    } else {
                        int logK = 1;
                        while ((cnt << (logK + 1)) <= WAVE) ++logK;           // cnt * 2^logK <= 64
                        const int K = 1 << logK;
                        const int e = lane >> logK, o = lane & (K - 1);
                        const bool have = e < cnt;
                        const bool act = have && (r0 + o) < R;
                        const int child = qa[have ? e : 0];
                        int I;
                        const bool acc = candidate(child, r0 + o, act, I);
                        const unsigned long long am = __ballot(acc);
                        const unsigned long long segmask = (K >= 64) ? ~0ull : ((1ull << K) - 1ull);
                        const unsigned long long seg = (am >> (e << logK)) & segmask;
                        const int first = __ffsll((long long)seg) - 1;       // lowest accepting round
                        if (acc && o == first) Jres[child] = I;
                        const bool rej = have && o == 0 && seg == 0ull;
                        const unsigned long long mk = __ballot(rej);
                        if (rej) qb[__popcll(mk & ltmask)] = child;
                        ncnt = __popcll(mk);
                        r0 += K;
                    }
                    { int *tq = qa; qa = qb; qb = tq; }
                    cnt = ncnt;
                }
                // ---- 3. children still pending: exact categorical draw, one child per wave at a
                //         time over all parents -------------------------------------------------------
                if (tid == 0) *qcount = 0;
                __syncthreads();
                if (ordered) {
                    // ---- 2'. the REFERENCE's consumption order (pf.py:260-341): one sequential stream of uniforms.  Round
                    // r of draw j takes len(L) doubles for np.random.choice and len(L) for np.random.rand, the k-th
                    // pending child IN INDEX ORDER gets the k-th of each; once at most manual_sample_threshold children
                    // are left (or after max_accept_reject rounds) each of them takes one double, in index order, for its
                    // exact categorical draw.  The rank of a pending child = a workgroup-wide exclusive count of the
                    // pending flags in particle-index order (slot-major: particle k * NT + tid).  accept_reject = False
                    // (pf.py:226-236): no rounds, child i's draw j takes double i * Ntilde + j of the timestep's N * Ntilde (the cursor
                    // moves on by N * Ntilde behind the last draw).
                    const gptr<const double> strm = global_ptr(P.paris_stream);       // global_load: see global_ptr
                    const long long cap = P.paris_stream_len;
                    const bool noar = (P.flags & PFG_FLAG_PARIS_NO_ACCEPT_REJECT) != 0;
                    const int mthr = P.paris_manual_threshold;
                    int *const wcnt = paris_wq0;                       // [PPT][NW] pending children per (slot, wave)
                    bool pend[PPT];
#pragma unroll
                    for (int k = 0; k < PPT; ++k) pend[k] = valid[k];
                    int S = 0, rank[PPT];
                    for (int round = 0;; ++round) {
#pragma unroll
                        for (int k = 0; k < PPT; ++k) {
                            const unsigned long long mk = __ballot(pend[k]);
                            rank[k] = __popcll(mk & ltmask);
                            if (lane == 0) wcnt[k * NW + wave] = __popcll(mk);
                        }
                        __syncthreads();
                        S = 0;
#pragma unroll
                        for (int k = 0; k < PPT; ++k) {
#pragma unroll
                            for (int w = 0; w < NW; ++w) {
                                if (w == wave) rank[k] += S;
                                S += wcnt[k * NW + w];
                            }
                        }
                        __syncthreads();                                // wcnt is rewritten by the next round
                        if (S == 0 || noar || S <= mthr || round >= R || paris_overflow) break;
                        if (paris_cursor + 2ll * S > cap) { paris_overflow = true; break; }
                        // A round is a dependent chain: HBM latency of the two uniforms, ten LDS probes, gather, exp.  All four
                        // slots of a thread walk it TOGETHER (loads first, the searches level by level, branch-free; a slot
                        // that is not pending searches with u = -1 and ends at parent 0): one after the other, behind an
                        // `if (!pend[k]) continue`, a round cost 8 us.
                        double u1v[PPT], u2v[PPT];
#pragma unroll
                        for (int k = 0; k < PPT; ++k) {
                            u1v[k] = pend[k] ? strm[paris_cursor + rank[k]] : -1.0;
                            u2v[k] = pend[k] ? strm[paris_cursor + S + rank[k]] : 2.0;
                        }
                        int Iv[PPT];
#pragma unroll
                        for (int k = 0; k < PPT; ++k) Iv[k] = 0;
#pragma unroll
                        for (int step = (NT * PPT) >> 1; step >= 1; step >>= 1) {
                            const int probe = step - 1 + (step >= 32 ? (step >> 5) - 1 : 0);
#pragma unroll
                            for (int k = 0; k < PPT; ++k) Iv[k] += (cdf[Iv[k] + probe] <= u1v[k]) ? step + (step >> 5) : 0;
                        }
#pragma unroll
                        for (int k = 0; k < PPT; ++k) {
                            int I = Iv[k];
                            I -= (I * 993) >> 15;
                            I = I < last ? I : last;
                            REAL xI[NS];
#pragma unroll
                            for (int d = 0; d < NS; ++d) xI[d] = cur[sidx(d, I)];
                            const double thr = (double)mth.exp(backward_log_ratio<MODEL, REAL>(c, mth, xI, xn[k]));
                            if (pend[k] && u2v[k] <= thr) { Jres[k * NT + tid] = I; pend[k] = false; }
                        }
                        paris_cursor += 2ll * S;
                    }
                    // the children still pending, in index order: queue position = rank
                    if (S > 0 && !noar && paris_cursor + S > cap) paris_overflow = true;
                    if (S > 0 && noar && paris_cursor + (long long)N * Nt > cap) paris_overflow = true;
                    if (!paris_overflow) {
#pragma unroll
                        for (int k = 0; k < PPT; ++k) {
                            if (!pend[k]) continue;
                            const int i = k * NT + tid;
                            queue[rank[k]] = i;
                            const double um = noar ? strm[paris_cursor + (long long)i * Nt + j] : strm[paris_cursor + rank[k]];
                            nxt[sidx(NS, i)] = (REAL)um;
                        }
                        if (tid == 0) *qcount = S;
                        if (!noar) paris_cursor += S;
                    } else {
#pragma unroll
                        for (int k = 0; k < PPT; ++k)
                            if (pend[k]) Jres[k * NT + tid] = 0;            // the host discards an overflowed window
                    }
                }
                for (int e0 = 0; e0 < cnt; e0 += WAVE) {
                    const int e = e0 + lane;
                    if (e < cnt) {
                        const int i = qa[e];
                        queue[atomicAdd(qcount, 1)] = i;
                        // the child's fallback uniform rides in its (still unused) statistic slot
                        const double um = (RNG == PFG_RNG_REPLAY) ? pman[((size_t)t * Nt + j) * N + i]
                                                                  : u01_32(rng.next());
                        nxt[sidx(NS, i)] = (REAL)um;
                    }
                }
                __syncthreads();
                const int nq = *qcount;
                // one pending child per WAVE at a time: lane handles parents lane, lane+64, ...
                // (wave-local max / total / ordered cumulative count: no workgroup barrier inside)
                constexpr int MAXC = NT * PPT / WAVE;
                const int nchunk = (N + WAVE - 1) / WAVE;
                for (int e = wave; e < nq; e += NW) {
                    const int ci = queue[e];
                    REAL xc[NS];
#pragma unroll
                    for (int d = 0; d < NS; ++d) xc[d] = nxt[sidx(d, ci)];
                    const double um = (double)nxt[sidx(NS, ci)];
                    if constexpr (RNG == PFG_RNG_DEVICE) {
                        // Device generator: any enumeration of the parents is a valid categorical
                        // sampler, so enumerate LANE-major (lane's parents lane, lane+64, ...): per-lane
                        // running sums, ONE wave scan over the lane totals, then the owning lane
                        // resolves its own <= MAXC entries -- no per-chunk wave reductions (they are
                        // dependent DPP chains with nothing to overlap: one wave per SIMD here).
                        // fp64 shifts by the block maximum m of the parents' log-weights (the
                        // backward ratio is <= 0, so every exponent is <= 0); f32 takes the exact max.
                        REAL mm = (REAL)m;
                        REAL lq[MAXC];
                        float mxf2 = -INFINITY;
#pragma unroll
                        for (int mI = 0; mI < MAXC; ++mI) {
                            const int q = mI * WAVE + lane;
                            const int qq = q < N ? q : last;
                            REAL xq[NS];
#pragma unroll
                            for (int d = 0; d < NS; ++d) xq[d] = cur[sidx(d, qq)];
                            lq[mI] = (q < N && mI < nchunk) ? lwL[qq] + backward_log_ratio<MODEL, REAL>(c, mth, xq, xc)
                                                            : (REAL)(-INFINITY);
                            mxf2 = fmaxf(mxf2, (float)lq[mI]);
                        }
                        if (sizeof(REAL) == 4) mm = (REAL)wave_max(mxf2);
                        double evl[MAXC], tl = 0.0;
#pragma unroll
                        for (int mI = 0; mI < MAXC; ++mI) {
                            evl[mI] = (double)mth.exp((REAL)(lq[mI] - mm));       // exp(-inf) = 0
                            tl += evl[mI];
                        }
                        const double incl = wave_incl_scan(tl);
                        const double target = um * bcast_lane63(incl);
                        int Lsel = (int)wave_sum(incl <= target ? 1.0 : 0.0);
                        Lsel = __builtin_amdgcn_readfirstlane(Lsel < WAVE - 1 ? Lsel : WAVE - 1);
                        const double loc = target - (incl - tl);                  // this lane's local target
                        double run = 0.0;
                        int msel = 0;
                        bool found = false;
#pragma unroll
                        for (int mI = 0; mI < MAXC; ++mI) {
                            run += evl[mI];
                            const bool here = !found && run > loc;
                            msel = here ? mI : msel;
                            found = found || here;
                        }
                        int res = msel * WAVE + lane;
                        res = __builtin_amdgcn_readlane(res, Lsel);
                        if (lane == 0) Jres[ci] = res < last ? res : last;
                        continue;
                    }
                    REAL l[MAXC];
                    float mxf = -INFINITY;
#pragma unroll
                    for (int mI = 0; mI < MAXC; ++mI) {
                        const int q = mI * WAVE + lane;
                        const int qq = q < N ? q : last;
                        REAL xq[NS];
#pragma unroll
                        for (int d = 0; d < NS; ++d) xq[d] = cur[sidx(d, qq)];
                        l[mI] = (q < N) ? lwL[qq] + backward_log_ratio<MODEL, REAL>(c, mth, xq, xc) : (REAL)(-INFINITY);
                        mxf = fmaxf(mxf, (float)l[mI]);
                        if (mI + 1 >= nchunk) break;
                    }
                    const REAL mm = (REAL)wave_max(mxf);
                    // chunk m = parents [64m, 64m+64): independent wave sums (pipelined), then the
                    // chunk holding the target is scanned once -- index order as np.random.choice
                    double ev[MAXC], csum[MAXC], tot = 0.0;
#pragma unroll
                    for (int mI = 0; mI < MAXC; ++mI) {
                        ev[mI] = (mI < nchunk) ? (double)mth.exp((REAL)(l[mI] - mm)) : 0.0;
                        csum[mI] = wave_sum(ev[mI]);
                        tot += csum[mI];
                    }
                    const double target = um * tot;
                    double before = 0.0, evsel = 0.0, run = 0.0;
                    int msel = nchunk - 1;
                    bool found = false;
#pragma unroll
                    for (int mI = 0; mI < MAXC; ++mI) {
                        const bool here = !found && mI < nchunk && (run + csum[mI] > target || mI == nchunk - 1);
                        if (here) { msel = mI; before = run; found = true; }
                        evsel = here ? ev[mI] : evsel;
                        run += csum[mI];
                    }
                    const double inc = wave_incl_scan(evsel) + before;
                    int cnt = ((msel * WAVE + lane) < N && inc <= target) ? 1 : 0;
                    cnt = msel * WAVE + (int)wave_sum((double)cnt);
                    if (lane == 0) Jres[ci] = cnt < last ? cnt : last;
                }
                __syncthreads();
                // ---- 4. rewired parent: stats[J] + w_t h(x_J, child) ----------------------------
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const int Jk = valid[k] ? Jres[k * NT + tid] : 0;
                    if (PFG_TR(P.trace_x) && P.trace_paris_J && valid[k])
                        P.trace_paris_J[((size_t)t * Nt + j) * N + k * NT + tid] = Jk;
                    REAL xJ[NS], aj[H];
#pragma unroll
                    for (int d = 0; d < NS; ++d) xJ[d] = cur[sidx(d, Jk)];
                    additive_stat<MODEL, STAT, REAL>(c, xJ, xn[k], (REAL)y_t, aux[k], aj);
#pragma unroll
                    for (int h = 0; h < H; ++h) {
                        const REAL a = use_stat ? aj[h] * (REAL)wt : (REAL)0;
                        sacc[k][h] += cur[sidx((NS + h), Jk)] + a;
                    }
                }
                __syncthreads();                // queue / statistic-slot scratch free for the next j
            }
            if (ordered && (P.flags & PFG_FLAG_PARIS_NO_ACCEPT_REJECT) && !paris_overflow) paris_cursor += (long long)N * Nt;
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                lw[k] = valid[k] ? lwn[k] : (REAL)(-INFINITY);
                if (valid[k]) {
#pragma unroll
                    for (int h = 0; h < H; ++h) nxt[sidx((NS + h), k * NT + tid)] = sacc[k][h] / (REAL)Nt;
                }
            }
        };
        // Poyiadjis O(N^2) (pf.py:84-136): children are proposed from the filter's ancestors, then
        // every child averages  stats_j + w_t h(x_j, child)  over ALL parents j with the backward
        // weights  log_normalize(logw_j + log q(child | x_j)).  Every lane walks the parents in the
        // same order (LDS broadcast reads); two passes: exact per-child maximum, then exp-sums.
        // No barrier inside: parents are read from `cur` (published behind barrier 3), children go to `nxt`; in the
        // one-wave instantiation (64 x 2) barrier 3 itself is program order, so a timestep has no s_barrier at all.
        // The sweep is skipped while it cannot change anything (PFG_OPT_N2SKIP): before t1 of a window that starts
        // without init_stats every parent's statistics are +0.0 and the step adds nothing, so every child's are
        // num / den = (sum_j e_j (0 + 0)) / den = +0.0 for any finite weights -- written directly.  Steps of the right
        // buffer (t >= tL) carry non-zero statistics and keep the sweep.
        auto n2_slots = [&](auto stat_tag) {
            constexpr int STAT = decltype(stat_tag)::value;
            if (RNG != PFG_RNG_REPLAY) {
                draw_normals(zz);
                if (PFG_TR(P.trace_x) && P.rec_z) {       // test instrumentation, as in the plain kernel
#pragma unroll
                    for (int k = 0; k < PPT; ++k)
                        if (valid[k]) P.rec_z[(size_t)t * N + k * NT + tid] = (double)zz[k];
                }
            }
            REAL xn[PPT][NS], lwn[PPT], aux[PPT];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                REAL xp[NS], add[H];
#pragma unroll
                for (int d = 0; d < NS; ++d) xp[d] = cur[sidx(d, anc[k])];
                particle_step<MODEL, KERNEL, STAT, REAL>(c, mth, xp, (REAL)y_t, zz[k], xn[k], lwn[k], add);
                aux[k] = (MODEL == PFG_MODEL_SVM) ? mth.exp(-xn[k][0]) : (REAL)0;
                if (valid[k]) {
#pragma unroll
                    for (int d = 0; d < NS; ++d) nxt[sidx(d, k * NT + tid)] = xn[k][d];
                }
            }
            if (PFG_OPT_N2SKIP && t < t1 && !(P.init_x && P.init_stats)) {      // workgroup-uniform
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    lw[k] = valid[k] ? lwn[k] : (REAL)(-INFINITY);
                    if (valid[k]) {
#pragma unroll
                        for (int h = 0; h < H; ++h) nxt[sidx((NS + h), k * NT + tid)] = (REAL)0;
                    }
                }
                return;
            }
            REAL mx[PPT];
#pragma unroll
            for (int k = 0; k < PPT; ++k) mx[k] = (REAL)(-INFINITY);
#pragma unroll 2
            for (int j = 0; j < N; ++j) {
                REAL xj[NS];
#pragma unroll
                for (int d = 0; d < NS; ++d) xj[d] = cur[sidx(d, j)];
                const REAL lj = lwL[j];
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const REAL v = lj + backward_log_ratio<MODEL, REAL>(c, mth, xj, xn[k]);
                    mx[k] = v > mx[k] ? v : mx[k];
                }
            }
            REAL den[PPT], num[PPT][H];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                den[k] = (REAL)0;
#pragma unroll
                for (int h = 0; h < H; ++h) num[k][h] = (REAL)0;
            }
#pragma unroll 2
            for (int j = 0; j < N; ++j) {
                REAL xj[NS], sj[H];
#pragma unroll
                for (int d = 0; d < NS; ++d) xj[d] = cur[sidx(d, j)];
#pragma unroll
                for (int h = 0; h < H; ++h) sj[h] = cur[sidx((NS + h), j)];
                const REAL lj = lwL[j];
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const REAL e = mth.exp((lj + backward_log_ratio<MODEL, REAL>(c, mth, xj, xn[k])) - mx[k]);
                    REAL aj[H];
                    additive_stat<MODEL, STAT, REAL>(c, xj, xn[k], (REAL)y_t, aux[k], aj);
                    den[k] += e;
#pragma unroll
                    for (int h = 0; h < H; ++h) {
                        const REAL a = use_stat ? aj[h] * (REAL)wt : (REAL)0;
                        num[k][h] += e * (sj[h] + a);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                lw[k] = valid[k] ? lwn[k] : (REAL)(-INFINITY);
                if (valid[k]) {
#pragma unroll
                    for (int h = 0; h < H; ++h) nxt[sidx((NS + h), k * NT + tid)] = num[k][h] / den[k];
                }
            }
        };
        bool did_paris = false;
        if constexpr (TR::N2) {
            if (stat == PFG_STAT_SCORE) n2_slots(std::integral_constant<int, PFG_STAT_SCORE>{});
            else n2_slots(std::integral_constant<int, PFG_STAT_SUFF>{});
            did_paris = true;
        }
        if constexpr (TR::PARIS) {
            if (P.smoother == PFG_SMOOTHER_PARIS) {
                if (stat == PFG_STAT_SCORE) paris_slots(std::integral_constant<int, PFG_STAT_SCORE>{});
                else paris_slots(std::integral_constant<int, PFG_STAT_SUFF>{});
                did_paris = true;
            }
        }
        if (!did_paris) {
            if (stat == PFG_STAT_SCORE) slots(std::integral_constant<int, PFG_STAT_SCORE>{});
            else slots(std::integral_constant<int, PFG_STAT_SUFF>{});
        }
        if constexpr (TR::RAWSCORE) {
            if (raw_score && use_stat) Cw = uniform_f64(Cw + wt);
        }
        if (PFG_TR(P.trace_x)) {
            // own children back from LDS (written by this thread: no barrier needed)
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                if (valid[k]) {
                    const int i = k * NT + tid;
                    const size_t row = (size_t)(t + 1) * N + i;
                    if constexpr (!(TR::GADDR && TRACE)) {          // GADDR: stored behind the search
                    if (P.trace_anc) P.trace_anc[(size_t)t * N + i] = anc[k];
                    }
#pragma unroll
                    for (int d = 0; d < NS; ++d) P.trace_x[row * NS + d] = (double)nxt[sidx(d, i)];
                    P.trace_logw[row] = TR::SHIFTFOLD ? (double)lw[k] + m : (double)lw[k];
                    if (P.trace_stats && !is_filter) {
                        if constexpr (TR::RAWSCORE) {          // a raw window's slots leave in the score's scale, with this step's Cw
                            REAL r[H], sv[H];
#pragma unroll
                            for (int h = 0; h < H; ++h) r[h] = sv[h] = nxt[sidx((NS + h), i)];
                            if (raw_score) raw_score_out(c, (REAL)Cw, r, sv);
#pragma unroll
                            for (int h = 0; h < H; ++h) P.trace_stats[row * H + h] = (double)sv[h];
                        } else {
#pragma unroll
                        for (int h = 0; h < H; ++h)
                            P.trace_stats[row * H + h] = (double)nxt[sidx((NS + h), i)];
                        }
                    }
                }
            }
        }
        if (PP) { REAL *tmp = cur; cur = nxt; nxt = tmp; }
        wt_prev = wt;
        PFG_PH(9)
    }
    if (P.stamps && tid == 0) { P.stamps[2] = __builtin_amdgcn_s_memtime(); P.stamps[3] = __builtin_amdgcn_s_memrealtime(); }
#ifdef PFG_PHASE_STAMPS
    if (P.stamps && lane == 0) {
#pragma unroll
        for (int q = 0; q < 10; ++q) atomicAdd(reinterpret_cast<unsigned long long *>(P.stamps) + 4 + q, ph_acc[q]);
    }
#endif
#undef PFG_PH
#undef PFG_MARK

    // ---- outputs --------------------------------------------------------------------
    if (RNG == PFG_RNG_REPLAY && P.out) {
        tie = -wave_max(-tie);
        if (lane == 0) red_max[wave] = tie;
        __syncthreads();
        tie = red_max[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) tie = red_max[w] < tie ? red_max[w] : tie;
    }
    if (TR::PARIS && tid == 0 && P.paris_consumed) {
        P.paris_consumed[0] = paris_overflow ? -1ll : paris_cursor;
        // RAW: a cached Gaussian is pending -> how far back from the end of the consumption its pair of doubles starts
        P.paris_consumed[1] = (TR::RAWCAP && raw && carry_has && !paris_overflow) ? paris_cursor - raw_slots[1] : 0ll;
    }
    if constexpr (TR::RAWSCORE) {
        // the weighted sums of t == T ran over raw slots: to the score's scale, once
        if (raw_score) {
            REAL r[H], sv[H];
#pragma unroll
            for (int h = 0; h < H; ++h) r[h] = (REAL)S[h];
            raw_score_out(c, (REAL)Cw, r, sv);
#pragma unroll
            for (int h = 0; h < H; ++h) S[h] = (double)sv[h];
        }
    }
    if (tid == 0 && P.out) {
#pragma unroll
        for (int h = 0; h < PFG_MAX_STAT; ++h) P.out[h] = 0.0;
#pragma unroll
        for (int h = 0; h < H; ++h) P.out[h] = is_filter ? filt[h] : S[h];
        P.out[4] = ll;
        P.out[5] = W;
        P.out[6] = m;
        P.out[7] = tie;
    }
    if (P.final_x) {
        // own entries of the current buffer: written by this thread, no barrier needed
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = k * NT + tid;
            if (i < N) {
#pragma unroll
                for (int d = 0; d < NS; ++d) P.final_x[(size_t)i * NS + d] = (double)cur[sidx(d, i)];
                if (P.final_logw) P.final_logw[i] = TR::SHIFTFOLD ? (double)lw[k] + m : (double)lw[k];
                if (P.final_stats && !is_filter) {
                    if constexpr (TR::RAWSCORE) {
                        REAL r[H], sv[H];
#pragma unroll
                        for (int h = 0; h < H; ++h) r[h] = sv[h] = cur[sidx((NS + h), i)];
                        if (raw_score) raw_score_out(c, (REAL)Cw, r, sv);
#pragma unroll
                        for (int h = 0; h < H; ++h) P.final_stats[(size_t)i * H + h] = (double)sv[h];
                    } else {
#pragma unroll
                    for (int h = 0; h < H; ++h)
                        P.final_stats[(size_t)i * H + h] = (double)cur[sidx((NS + h), i)];
                    }
                }
            }
        }
    }
}

}  // namespace pfg
