// Kernel launch templates of libpfgrad.so.  Included ONLY by the instantiation units
// (pfg_inst_*.hip), each of which instantiates launch_mkr for one (model, proposal kernel, generator).
// They map a LaunchPlan (make_plan in pfg_plan.hip) onto an instantiation and choose nothing themselves.
#pragma once
#include <mutex>
#include "pfg_host.hpp"
#include "pfg_device.hpp"

namespace pfg_host {

// Dynamic LDS above 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize; set it once per kernel and
// CONTEXT (again only if a larger size is asked for), not on every launch.  The attribute belongs to the
// (function, device) pair and a context is bound to one device; a context is used by one thread at a time.
#define PFG_ENSURE_LDS(ctx, kern, lds)                                                                    \
    do {                                                                                                  \
        if ((lds) > 64 * 1024) {                                                                          \
            size_t &pfg_lds_set_ = (ctx)->lds_set[reinterpret_cast<const void *>(kern)];                  \
            if ((lds) > pfg_lds_set_) {                                                                   \
                PFG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern),                    \
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds))); \
                pfg_lds_set_ = (lds);                                                                     \
            }                                                                                             \
        }                                                                                                 \
    } while (0)

// ---- whole-GPU window (pfg_grid_kernel.hpp): init, then per timestep [REPLAY: the reference's CDF] + the step kernel,
// then finish; T_max + 2 (REPLAY: 5 T_max + 2) launches on `st`, no host synchronisation in between.  Every window of the
// batch must fall into the same tile class (pfg::grid_ppt(N)); windows shorter than t_max leave their launches at once.
// phase: PFG_GRID_ALL = init, every timestep, finish; PFG_GRID_INIT / PFG_GRID_FINISH alone; t >= 0: timestep t alone
// (callers that put events or graph nodes between the launches)
constexpr int PFG_GRID_ALL = -1, PFG_GRID_INIT = -2, PFG_GRID_FINISH = -3;
template <int MODEL, int KERNEL, typename REAL, int RNG, int NT, int PPT, int KMAX>
int launch_grid_ppt(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    constexpr int NW = NT / pfg::WAVE;
    const int phase = p.phase;
    const dim3 grid((unsigned)p.tiles, (unsigned)B), blk(NT);
    const size_t red_bytes = (size_t)(4 * PPT * NW + 16 + PFG_MAX_STAT * NW) * 8;
    const size_t lds_init = red_bytes + pfg::tab_bytes<REAL, RNG, (RNG == PFG_RNG_DEVICE)>();
    const size_t lds_fin = (size_t)(pfg::GRID_MAX_TILES + 1) * 8 + red_bytes;
    auto k_init = pfg::pfg_grid_init_kernel<MODEL, KERNEL, REAL, RNG, NT, PPT>;
    auto k_fin = pfg::pfg_grid_finish_kernel<MODEL, REAL, RNG, NT, PPT>;
    const int t_lo = phase >= 0 ? phase : 0, t_hi = phase >= 0 ? phase + 1 : (phase == PFG_GRID_ALL ? p.t_max : 0);
    if (phase == PFG_GRID_ALL || phase == PFG_GRID_INIT) hipLaunchKernelGGL(k_init, grid, blk, lds_init, st, dp);
    if constexpr (RNG == PFG_RNG_REPLAY) {
        // the plan sizes the step kernel's LDS from grid_coarse_reserve(n_max) <= GRID_COARSE_MAX coarse entries
        static_assert(pfg::grid_step_lds_bytes<NT, PPT, REAL, RNG>(pfg::GRID_COARSE_MAX) <= kLdsLimit,
                      "a full coarse table must fit the REPLAY step kernel's LDS");
        auto k_step = pfg::pfg_grid_step_kernel<MODEL, KERNEL, REAL, RNG, NT, PPT>;
        PFG_ENSURE_LDS(ctx, k_step, p.lds);
        // the reference's CDF: four launches that spread the particle axis over the GPU (cdf_single: the lone-workgroup
        // kernel, A/B and cross-check)
        const unsigned n16 = (unsigned)((p.n_max + 16383) / 16384), n4 = (unsigned)((p.n_max + pfg::CDF_BLK - 1) / pfg::CDF_BLK);
        for (int t = t_lo; t < t_hi; ++t) {
            if (p.cdf_single) {
                hipLaunchKernelGGL((pfg::pfg_grid_cdf_kernel<MODEL, REAL>), dim3((unsigned)B), dim3(pfg::CDF_NT), 0, st, dp, t);
            } else {
                hipLaunchKernelGGL((pfg::pfg_grid_cdf_sum_kernel<MODEL, REAL>), dim3(n16, (unsigned)B), dim3(pfg::CDF_NT), 0, st, dp, t);
                hipLaunchKernelGGL((pfg::pfg_grid_cdf_class_kernel<MODEL, REAL>), dim3(n4, (unsigned)B), dim3(pfg::CDF_NT), 0, st, dp, t);
                hipLaunchKernelGGL((pfg::pfg_grid_cdf_chain_kernel<MODEL, REAL>), dim3((unsigned)B), dim3(pfg::WAVE), 0, st, dp, t);
                hipLaunchKernelGGL((pfg::pfg_grid_cdf_apply_kernel<MODEL, REAL>), dim3(n4, (unsigned)B), dim3(pfg::CDF_NT), 0, st, dp, t);
            }
            hipLaunchKernelGGL(k_step, grid, blk, p.lds, st, dp, t);
        }
    } else {
        // score1: the score-only twin of the step kernel (PFG_SMOOTHER_POYIADJIS_N)
        auto k_step = p.score1 ? pfg::pfg_grid_step_dev_kernel<MODEL, KERNEL, REAL, NT, PPT, KMAX, true>
                               : pfg::pfg_grid_step_dev_kernel<MODEL, KERNEL, REAL, NT, PPT, KMAX>;
        PFG_ENSURE_LDS(ctx, k_step, p.lds);
        for (int t = t_lo; t < t_hi; ++t) hipLaunchKernelGGL(k_step, grid, blk, p.lds, st, dp, t);
    }
    if (phase == PFG_GRID_ALL || phase == PFG_GRID_FINISH) hipLaunchKernelGGL(k_fin, grid, blk, lds_fin, st, dp);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

using pf_kernel_t = void (*)(const pfg_dev_problem *);

inline int launch_kernel(pfg_ctx *ctx, pf_kernel_t kern, int nt, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    PFG_ENSURE_LDS(ctx, kern, p.lds);
    hipLaunchKernelGGL(kern, dim3(B), dim3(nt), p.lds, st, dp);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

// (The launchers below reference their kernels in a fixed order, which is the order the kernels take in the code
// object; the compiler's register allocation has been seen to depend on it.)

// The exp table in device memory (pfg::ExpTabMem<TAG>, read by the RegTraits::TABMEM kernels of this unit) is filled ONCE per
// device and process, by the first launch that needs it: the fill kernel goes onto that launch's stream and the host waits
// for it there before it marks the device, so the table is complete before any reader is enqueued on any stream -- and, as
// nothing writes it again, it never changes under a running kernel.  A stream that is being captured cannot be waited on:
// the first TABMEM launch of a device must be an eager one (ChainEnsemble runs an eager step before it captures).
template <int TAG>
int ensure_exp_tab_mem(pfg_ctx *ctx, hipStream_t st) {
    static std::mutex mu;
    static std::vector<char> filled;
    std::lock_guard<std::mutex> lock(mu);
    if ((size_t)ctx->device < filled.size() && filled[(size_t)ctx->device]) return PFG_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    PFG_HIP(ctx, hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(ctx, PFG_ERR_INVALID, "the first launch of this kernel on a device fills its exp table and cannot be captured: run one eager launch first");
    hipLaunchKernelGGL(pfg::exp_tab_mem_fill_kernel<TAG>, dim3(1), dim3(pfg::TAB_E2_ACC), 0, st);
    PFG_HIP(ctx, hipGetLastError());
    PFG_HIP(ctx, hipStreamSynchronize(st));
    if (filled.size() <= (size_t)ctx->device) filled.resize((size_t)ctx->device + 1, 0);
    filled[(size_t)ctx->device] = 1;
    return PFG_OK;
}

// an LDS-resident kernel; traced = the descriptors may carry trace_* / rec_* buffers: the TRACE = true instantiation,
// otherwise the twin with the trace instrumentation compiled out (device generator: what bench.py times; REPLAY: the
// drop-in Sampler's launch)
template <int MODEL, int KERNEL, typename REAL, int NT, int PPT, int RNG, bool PP, int MODE, bool TRACE = true, bool SCORE1 = false>
int launch_one_t(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    using TR = pfg::RegTraits<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, MODE>;
    if constexpr (TR::TABMEM) {
        if (const int rc = ensure_exp_tab_mem<TR::EXPTAB_TAG>(ctx, st)) return rc;
    }
    return launch_kernel(ctx, pfg::pf_reg_kernel<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, MODE, TRACE, SCORE1>, NT, p, B, dp, st);
}
template <int MODEL, int KERNEL, typename REAL, int NT, int PPT, int RNG, bool PP>
int launch_one(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    if constexpr (reg_score1_twin(MODEL, RNG, sizeof(REAL) == 8, NT, PPT, PP))
        if (p.score1) return launch_one_t<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, pfg::MODE_PLAIN, false, true>(ctx, p, B, dp, st);
    if (!p.traced) return launch_one_t<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, pfg::MODE_PLAIN, false>(ctx, p, B, dp, st);
    return launch_one_t<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, pfg::MODE_PLAIN, true>(ctx, p, B, dp, st);
}
template <int MODEL, int KERNEL, typename REAL, int RNG>
int launch_v(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
#define PFG_ENTRY(NT_, PPT_, PP_)                                                                 \
    if constexpr (reg_entry_built(MODEL, RNG, sizeof(REAL) == 8, NT_, PPT_, PP_))                \
        if (p.nt == NT_ && p.ppt == PPT_ && p.pp == PP_) return launch_one<MODEL, KERNEL, REAL, NT_, PPT_, RNG, PP_>(ctx, p, B, dp, st);
    PFG_ENTRY(256, 1, true) PFG_ENTRY(256, 4, true) PFG_ENTRY(256, 4, false) PFG_ENTRY(1024, 1, true) PFG_ENTRY(64, 2, true)
    PFG_ENTRY(1024, 4, false) PFG_ENTRY(64, 4, true) PFG_ENTRY(512, 2, false)
    // one wave per window on ONE state buffer (a wave's LDS accesses execute in order: the gather of a step is over
    // before its stores are issued, the fourth "barrier" is free) -- half the LDS per window
    PFG_ENTRY(64, 2, false) PFG_ENTRY(64, 4, false)
#undef PFG_ENTRY
    return fail(ctx, PFG_ERR_INVALID, "the launch plan names no kernel of this unit");
}

// PaRIS (MODE_PARIS) / O(N^2) Poyiadjis (MODE_N2) instantiations: the ping-pong 256 x ppt variants with the parents'
// log-weights in LDS, or (nt = MEM_NT) the large-N kernel's PaRIS instantiation (second log-weight array; state in the
// HBM scratch, descriptors carry one); or one wave per window (nt = 64, 2 particles per lane, N <= 128: paris64x2 / n2_64x2)
template <int MODEL, int KERNEL, typename REAL, int RNG, int MODE>
int launch_paris(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    if (p.nt == 256 && p.ppt == 1) return launch_one_t<MODEL, KERNEL, REAL, 256, 1, RNG, true, MODE>(ctx, p, B, dp, st);
    if (p.nt == 256) return launch_one_t<MODEL, KERNEL, REAL, 256, 4, RNG, true, MODE>(ctx, p, B, dp, st);
    if (p.nt == pfg::MEM_NT) {
        if (RNG != PFG_RNG_DEVICE || !p.record) return launch_kernel(ctx, pfg::pf_mem_kernel<MODEL, KERNEL, REAL, RNG, true>, pfg::MEM_NT, p, B, dp, st);
        if constexpr (RNG == PFG_RNG_DEVICE)        // a traced launch: the twin that also writes out its draws (rec_z0, rec_z, rec_ud)
            return launch_kernel(ctx, pfg::pf_mem_kernel<MODEL, KERNEL, REAL, RNG, /*PARIS*/ true, /*LW4*/ false, /*SCORE1*/ false, /*STRAT*/ false,
                                                         /*ADAPT*/ false, /*RECORD*/ true>, pfg::MEM_NT, p, B, dp, st);
    }
    if (p.nt == 64 && p.ppt == 2) return launch_one_t<MODEL, KERNEL, REAL, 64, 2, RNG, true, MODE>(ctx, p, B, dp, st);
    return fail(ctx, PFG_ERR_INVALID, "the launch plan names no PaRIS / O(N^2) kernel of this unit");
}

// large-N kernel: lw4 = the log-weights in registers, score1 = its score-only twin
template <int MODEL, int KERNEL, typename REAL, int RNG>
int launch_mem(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    if (p.score1) return launch_kernel(ctx, pfg::pf_mem_kernel<MODEL, KERNEL, REAL, RNG, false, true, true>, pfg::MEM_NT, p, B, dp, st);
    if (p.lw4) return launch_kernel(ctx, pfg::pf_mem_kernel<MODEL, KERNEL, REAL, RNG, false, true>, pfg::MEM_NT, p, B, dp, st);
    return launch_kernel(ctx, pfg::pf_mem_kernel<MODEL, KERNEL, REAL, RNG>, pfg::MEM_NT, p, B, dp, st);
}

// large-N kernel, device-RNG fast path (thread-major CDF, unrolled search, two chunks in flight) for np2 slots
template <int MODEL, int KERNEL, typename REAL, int NP2>
int launch_big_one(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    return launch_kernel(ctx, pfg::pf_big_kernel<MODEL, KERNEL, REAL, NP2>, pfg::MEM_NT, p, B, dp, st);
}
template <int MODEL, int KERNEL, typename REAL>
int launch_big(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    if (p.np2 == 4096) return launch_big_one<MODEL, KERNEL, REAL, 4096>(ctx, p, B, dp, st);
    return launch_big_one<MODEL, KERNEL, REAL, 16384>(ctx, p, B, dp, st);
}

// a resampling scheme other than multinomial (MODE_SYSTEMATIC / MODE_STRATIFIED / MODE_ADAPTIVE; Scheme in pfg_host.hpp):
// the 256 x 4 LDS-resident instantiation (single buffer in fp64, ping-pong in f32; one instantiation that honours trace
// buffers serves traced and production launches) and, where the scheme has them, the twins of the kernels that serve
// multinomial windows above N = 1024: the large-N kernel's (REPLAY) or the fast large-N kernel's (device generator)
template <int MODEL, int KERNEL, typename REAL, int RNG, int MODE>
int launch_scheme(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    constexpr bool STRAT = MODE == pfg::MODE_STRATIFIED, ADAPT = MODE == pfg::MODE_ADAPTIVE;
    if (p.np2 == 0 && p.nt == 256)
        return launch_one_t<MODEL, KERNEL, REAL, 256, 4, RNG, sizeof(REAL) == 4, MODE>(ctx, p, B, dp, st);
    if constexpr (!STRAT && !ADAPT) {
        return fail(ctx, PFG_ERR_INVALID, "the launch plan names no kernel of this unit");
    } else if constexpr (RNG == PFG_RNG_REPLAY) {
        if (p.lw4) return launch_kernel(ctx, pfg::pf_mem_kernel<MODEL, KERNEL, REAL, RNG, /*PARIS*/ false, /*LW4*/ true, /*SCORE1*/ false, STRAT, ADAPT>, pfg::MEM_NT, p, B, dp, st);
        return launch_kernel(ctx, pfg::pf_mem_kernel<MODEL, KERNEL, REAL, RNG, /*PARIS*/ false, /*LW4*/ false, /*SCORE1*/ false, STRAT, ADAPT>, pfg::MEM_NT, p, B, dp, st);
    } else {
        if (p.np2 == 4096) return launch_kernel(ctx, pfg::pf_big_kernel<MODEL, KERNEL, REAL, 4096, STRAT, ADAPT>, pfg::MEM_NT, p, B, dp, st);
        return launch_kernel(ctx, pfg::pf_big_kernel<MODEL, KERNEL, REAL, 16384, STRAT, ADAPT>, pfg::MEM_NT, p, B, dp, st);
    }
}

// every kernel of one (model, proposal kernel, generator): explicitly instantiated in
// pfg_inst_<model>_<kernel>_<rng>.hip.  The DEVICE-generator units are compiled with
// -ffp-contract=fast (no operation-order parity to keep there), the REPLAY units with
// -ffp-contract=off (the reference's NumPy operation order).
template <int MODEL, int KERNEL, int RNG>
int launch_mkr(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st) {
    constexpr bool dev = RNG == PFG_RNG_DEVICE;
    switch (p.family) {
        case Family::Systematic:    // built for the device generator: single buffer in fp64, ping-pong in f32
            if constexpr (dev) {
                if (p.f64) return launch_scheme<MODEL, KERNEL, double, RNG, pfg::MODE_SYSTEMATIC>(ctx, p, B, dp, st);
                return launch_scheme<MODEL, KERNEL, float, RNG, pfg::MODE_SYSTEMATIC>(ctx, p, B, dp, st);
            }
            break;
        case Family::Big:
            if constexpr (dev) return p.f64 ? launch_big<MODEL, KERNEL, double>(ctx, p, B, dp, st) : launch_big<MODEL, KERNEL, float>(ctx, p, B, dp, st);
            break;
        case Family::N2:
            if (p.f64) return launch_paris<MODEL, KERNEL, double, RNG, pfg::MODE_N2>(ctx, p, B, dp, st);
            return launch_paris<MODEL, KERNEL, float, RNG, pfg::MODE_N2>(ctx, p, B, dp, st);
        case Family::Paris:
            if (p.f64) return launch_paris<MODEL, KERNEL, double, RNG, pfg::MODE_PARIS>(ctx, p, B, dp, st);
            return launch_paris<MODEL, KERNEL, float, RNG, pfg::MODE_PARIS>(ctx, p, B, dp, st);
        case Family::Mem:
            if (p.f64) return launch_mem<MODEL, KERNEL, double, RNG>(ctx, p, B, dp, st);
            return launch_mem<MODEL, KERNEL, float, RNG>(ctx, p, B, dp, st);
        case Family::Reg:
            if (p.f64) return launch_v<MODEL, KERNEL, double, RNG>(ctx, p, B, dp, st);
            return launch_v<MODEL, KERNEL, float, RNG>(ctx, p, B, dp, st);
        case Family::Grid:
#define PFG_GRID_CASE(REAL_)                                                                                          \
    (p.ppt == 4 ? launch_grid_ppt<MODEL, KERNEL, REAL_, RNG, pfg::GRID_NT, 4, 2>(ctx, p, B, dp, st)                  \
     : p.kmax == 2 ? launch_grid_ppt<MODEL, KERNEL, REAL_, RNG, pfg::GRID_NT, 8, 2>(ctx, p, B, dp, st)               \
                   : launch_grid_ppt<MODEL, KERNEL, REAL_, RNG, pfg::GRID_NT, 8, 8>(ctx, p, B, dp, st))
            if (p.f64) return PFG_GRID_CASE(double);
            return PFG_GRID_CASE(float);
#undef PFG_GRID_CASE
        case Family::Stratified:    // (last: the kernels above keep their places in the code object)
            return p.f64 ? launch_scheme<MODEL, KERNEL, double, RNG, pfg::MODE_STRATIFIED>(ctx, p, B, dp, st)
                         : launch_scheme<MODEL, KERNEL, float, RNG, pfg::MODE_STRATIFIED>(ctx, p, B, dp, st);
        case Family::Adaptive:      // (behind Stratified, for the same reason)
            return p.f64 ? launch_scheme<MODEL, KERNEL, double, RNG, pfg::MODE_ADAPTIVE>(ctx, p, B, dp, st)
                         : launch_scheme<MODEL, KERNEL, float, RNG, pfg::MODE_ADAPTIVE>(ctx, p, B, dp, st);
        case Family::None:
            break;
    }
    return fail(ctx, PFG_ERR_INVALID, "the launch plan names no kernel of this unit");
}

}  // namespace pfg_host
