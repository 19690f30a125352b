// libpfgrad.so: host side of the C ABI declared in include/pfgrad.h + kernel dispatch.
// The particle-filter kernels are instantiated in pfg_inst_*.hip (one unit per model x proposal
// kernel, compiled in parallel by sgmcmc_ssm_amd/_build.py); this unit holds the dispatcher, the
// small update / window / KSD kernels and the extern "C" entry points.  pfg_run_batch (host buffers) checks every
// window, plans the launch, then describes each window's buffers once (describe_window): sizing the arenas, staging the
// inputs and fetching the outputs are loops over those descriptions.
#include <mutex>
#include <unordered_map>
#include "pfg_host.hpp"
#include "pfg_device.hpp"
#include "pfg_elementwise.hpp"

using namespace pfg_host;

namespace pfg_host {
extern template int launch_mkr<PFG_MODEL_SVM, PFG_KERNEL_PRIOR, PFG_RNG_REPLAY>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_SVM, PFG_KERNEL_PRIOR, PFG_RNG_DEVICE>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_GARCH, PFG_KERNEL_PRIOR, PFG_RNG_REPLAY>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_GARCH, PFG_KERNEL_PRIOR, PFG_RNG_DEVICE>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_GARCH, PFG_KERNEL_OPTIMAL, PFG_RNG_REPLAY>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_GARCH, PFG_KERNEL_OPTIMAL, PFG_RNG_DEVICE>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_LGSSM, PFG_KERNEL_PRIOR, PFG_RNG_REPLAY>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_LGSSM, PFG_KERNEL_PRIOR, PFG_RNG_DEVICE>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_LGSSM, PFG_KERNEL_OPTIMAL, PFG_RNG_REPLAY>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
extern template int launch_mkr<PFG_MODEL_LGSSM, PFG_KERNEL_OPTIMAL, PFG_RNG_DEVICE>(pfg_ctx *, const LaunchPlan &, int, const pfg_dev_problem *, hipStream_t);
}  // namespace pfg_host

namespace {

template <int V> using int_c = std::integral_constant<int, V>;

// runtime (model, kernel, dtype, rng) -> f(int_c<MODEL>, int_c<KERNEL>, REAL(), int_c<RNG>): the one place where the ids
// become template arguments.  An id outside its enum takes the last branch (LGSSM, optimal, f32, REPLAY), which is what
// the unchecked queries pfg_variant_name / pfg_scratch_bytes have always computed for it.
template <typename F>
auto with_types(int model, int kernel, int dtype, int rng, F &&f) {
    auto g = [&](auto m, auto k, auto real) {
        return rng == PFG_RNG_DEVICE ? f(m, k, real, int_c<PFG_RNG_DEVICE>()) : f(m, k, real, int_c<PFG_RNG_REPLAY>());
    };
    auto d = [&](auto m, auto k) { return dtype == PFG_F64 ? g(m, k, double()) : g(m, k, float()); };
    auto kk = [&](auto m) { return kernel == PFG_KERNEL_PRIOR ? d(m, int_c<PFG_KERNEL_PRIOR>()) : d(m, int_c<PFG_KERNEL_OPTIMAL>()); };
    return model == PFG_MODEL_SVM ? d(int_c<PFG_MODEL_SVM>(), int_c<PFG_KERNEL_PRIOR>())
           : model == PFG_MODEL_GARCH ? kk(int_c<PFG_MODEL_GARCH>()) : kk(int_c<PFG_MODEL_LGSSM>());
}
// the same, where the proposal kernel does not matter (sizes)
template <typename F>
auto with_types(int model, int dtype, int rng, F &&f) { return with_types(model, PFG_KERNEL_PRIOR, dtype, rng, f); }

// dynamic LDS of the LDS-resident kernel (NT, PPT, PP, MODE).  Evaluated in this unit, built without PFG_FAST_ALGEBRA:
// the largest math tables any build of the kernel units carries.
template <int NT, int PPT, bool PP, int MODE = pfg::MODE_PLAIN>
size_t reg_lds(int model, int dtype, int rng, int N) {
    return with_types(model, dtype, rng, [&](auto m, auto, auto real, auto g) {
        return pfg::reg_kernel_lds_bytes<decltype(m)::value, decltype(real), NT, PPT, decltype(g)::value, PP, MODE>(N);
    });
}

// ---- kernel variants ----------------------------------------------------------------
// pp = ping-pong LDS state buffers (3 barriers/step); single buffer fits larger N (4 barriers).  tag1: the name of the
// score-only twin, where a unit has one (reg_score1_twin).
struct Variant { int NT, PPT; bool pp; const char *tag, *tag1; size_t (*lds)(int, int, int, int); };
template <int NT, int PPT, bool PP>
constexpr Variant entry(const char *tag, const char *tag1 = nullptr) { return {NT, PPT, PP, tag, tag1, reg_lds<NT, PPT, PP>}; }
const Variant kVariants[] = { entry<256, 1, true>("wg256x1"), entry<256, 4, true>("wg256x4", "wg256x4_score1"),
                              entry<256, 4, false>("wg256x4s", "wg256x4s_score1"),
                              // latency variant: one particle per thread, 16 waves on one CU; picked for
                              // small batches (fewer windows than a quarter of the CUs), never by order
                              entry<1024, 1, true>("wg1024x1", "wg1024x1_score1"),
                              // 1024 < N <= 4096 with the device generator when the state fits LDS
                              // (32-bit CDF): SVM fp64, every model in f32
                              entry<1024, 4, false>("wg1024x4s", "wg1024x4s_score1"),
                              // N <= 128: one wave per window (barriers and cross-wave reductions degenerate)
                              entry<64, 2, true>("wg64x2", "wg64x2_score1"),
                              // GARCH fp64: six LDS arrays allow two workgroups per CU; eight waves each
                              // put four waves on a SIMD (256x4: two)
                              entry<512, 2, false>("wg512x2s"),
                              // 128 < N <= 256, many windows: still one wave per window, four particles per lane
                              entry<64, 4, true>("wg64x4"),
                              // one wave per window, single state buffer
                              entry<64, 2, false>("wg64x2s", "wg64x2s_score1"), entry<64, 4, false>("wg64x4s") };
// Measured and not kept (round 3, BASELINE config 4, 512 chains, ms per launch): the 4096 LDS slots of N <= 4096 in
// fewer, wider threads -- 512 x 8 (2 waves per SIMD, 251 VGPRs, no spills) 12.99, 256 x 16 (1 wave per SIMD, 256 VGPRs +
// 176 AGPRs) 16.14, against 12.73 for 1024 x 4 at its 128-VGPR cap (16 spilled VGPRs): LDS holds ONE such workgroup per
// CU, so its own 16 waves are all the latency hiding a CU has, and they are worth more than the registers.
constexpr int kLds4096Variant = 4, kTinyVariant = 5, kGarchVariant = 6, kTiny4Variant = 7;
// device generator: the one-wave variants on a single state buffer (half the LDS per window: 18 instead of 11 windows
// per CU for LGSSM N = 100; 16384 windows of BASELINE config 1 in 1.86 instead of 2.25 ms)
constexpr int kTinySingleVariant = 8, kTiny4SingleVariant = 9;
constexpr int kLatencyVariant = 3, kLatencyBatch = 64;
constexpr int kNumVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));
// the LDS-resident PaRIS variants (ping-pong state, the parents' log-weights in LDS); paris64x2: one wave per window
struct ParisVariant { int NT, PPT; const char *tag; size_t (*lds)(int, int, int, int); };
const ParisVariant kParisVariants[] = { {64, 2, "paris64x2", reg_lds<64, 2, true, pfg::MODE_PARIS>},
                                        {256, 1, "paris256x1", reg_lds<256, 1, true, pfg::MODE_PARIS>},
                                        {256, 4, "paris256x4", reg_lds<256, 4, true, pfg::MODE_PARIS>} };

int state_dim(int model) { return model == PFG_MODEL_GARCH ? 2 : 1; }
int stat_dim(int model) { return model == PFG_MODEL_SVM ? 3 : 4; }
int theta_dim(int model) { return model == PFG_MODEL_SVM ? 3 : 4; }

// The kernel of a plain batch (no PaRIS / systematic / O(N^2)) of `batch` windows of up to n_max particles: Reg with the
// kVariants index v, Mem, Grid, or None above every kernel.  force = PFGRAD_VARIANT: <tag> forces a variant (tuning /
// tests) when it can hold n_max.
Family pick_plain(int model, int dtype, int rng, int n_max, int batch, const char *force, int &v) {
    auto fits = [&](int i) { return kVariants[i].lds(model, dtype, rng, n_max) <= kLdsLimit; };
    auto holds = [&](int i) { return n_max <= kVariants[i].NT * kVariants[i].PPT && fits(i); };
    auto reg = [&](int i) { v = i; return Family::Reg; };
    if (force) {
        if (!std::strcmp(force, "mem1024") && n_max <= pfg::MEM_MAX_N) return Family::Mem;
        // "big": the large-N kernels also where an LDS-resident variant would fit (A/B timing)
        if (!std::strcmp(force, "big") && rng == PFG_RNG_DEVICE && n_max > 1024 && n_max <= pfg::MEM_MAX_N) return Family::Mem;
        for (int i = 0; i < kNumVariants; ++i)
            if (!std::strcmp(force, kVariants[i].tag) && holds(i)) return reg(i);
    }
    // preference order: fp64 N<=1024 runs best on the single-buffer 256x4 variant at 3
    // workgroups per CU; f32 on ping-pong.  N > 1024 goes to the large-N kernel: 1024-thread
    // register-resident variants spill at the 128-VGPR cap and measured 3-5x slower than it.
    // N <= 128, many windows: one wave per window (2048 LGSSM N=100 T=200 chains: 1.07 -> 0.57 ms);
    // a lone window is quicker on the four waves of wg256x1 (0.34 vs 0.38 ms)
    if (n_max <= 128 && batch > kLatencyBatch && fits(kTinyVariant))
        return reg(rng == PFG_RNG_DEVICE ? kTinySingleVariant : kTinyVariant);
    if (n_max > 128 && n_max <= 256 && batch > kLatencyBatch && rng == PFG_RNG_DEVICE && fits(kTiny4Variant))
        return reg(kTiny4SingleVariant);
    if (batch <= kLatencyBatch && n_max > 256 && n_max <= 1024 && fits(kLatencyVariant)) return reg(kLatencyVariant);
    // GARCH fp64, device generator, 256 < N <= 1024: LDS holds two workgroups per CU either way; 512 threads x 2
    // particles put four waves on a SIMD instead of two (8192 windows of config 3: 1.99 -> 1.87 ms)
    if (model == PFG_MODEL_GARCH && dtype == PFG_F64 && rng == PFG_RNG_DEVICE && n_max > 256 && n_max <= 1024 && fits(kGarchVariant))
        return reg(kGarchVariant);
    const int order_f64[] = {0, 2, 1}, order_f32[] = {0, 1, 2};
    for (int i : dtype == PFG_F64 ? order_f64 : order_f32)
        if (holds(i)) return reg(i);
    if (rng == PFG_RNG_DEVICE && n_max <= 4096 && fits(kLds4096Variant)) return reg(kLds4096Variant);
    if (n_max <= pfg::MEM_MAX_N) return Family::Mem;
    if (n_max <= pfg::GRID_MAX_N) return Family::Grid;     // one window over the whole GPU (pfg_grid_kernel.hpp)
    return Family::None;
}

// Who asks for a plan: the queries pfg_variant_name / pfg_scratch_bytes (a large batch of plain windows), pfg_run_batch
// (N above the one-workgroup kernels, or PFGRAD_VARIANT=grid, runs as whole-GPU windows), pfg_launch_device* (one-workgroup
// kernels only) and pfg_launch_device_grid* (whole-GPU windows).
enum class Caller { Query, Batch, Device, Grid };

LaunchPlan refuse(LaunchPlan &p, int rc, std::string msg) {
    p.rc = rc;
    p.err = std::move(msg);
    return std::move(p);
}

// Which kernel runs a batch of B windows of up to n_max particles, with what LDS and scratch, under which name.  smoother
// as the dispatcher receives it: PFG_SMOOTHER_POYIADJIS_N states that every window is (NEMETH, lambduh = 1, score) -- the
// same kernels as NEMETH, except where a unit has a twin specialised to that estimator.  traced: the descriptors may carry
// trace_* / rec_* buffers (the plain LDS-resident kernels exist as a production twin that ignores them, see
// pfg_reg_kernel.hpp; every other kernel always honours them).  predictive: the windows ask for the predictive statistic,
// which only the general large-N kernel computes.  The environment variables PFGRAD_VARIANT, PFGRAD_NO_SCORE1 and
// PFGRAD_CDF_SINGLE are read here and nowhere else.
LaunchPlan make_plan(Caller caller, int model, int dtype, int rng, int smoother, int n_max, int B, bool traced,
                     bool predictive = false, int t_max = 0, int phase = -1) {
    LaunchPlan p;
    p.f64 = dtype == PFG_F64;
    p.n_max = n_max; p.t_max = t_max; p.phase = phase;
    auto score1_on = [&] {          // PFGRAD_NO_SCORE1=1 (A/B timing): the general kernel for these launches too
        if (smoother != PFG_SMOOTHER_POYIADJIS_N) return false;
        const char *off = std::getenv("PFGRAD_NO_SCORE1");
        return !(off && off[0] == '1');
    };
    auto mem_lds = [&] { return with_types(model, dtype, rng, [&](auto, auto, auto real, auto g) { return pfg::mem_kernel_lds_bytes<decltype(real), decltype(g)::value>(n_max); }); };
    auto mem_scratch = [&](bool paris) {
        return (with_types(model, dtype, rng, [&](auto m, auto, auto real, auto) {
                    return pfg::mem_kernel_scratch_bytes<decltype(m)::value, decltype(real)>(n_max, paris);
                }) + 255) / 256 * 256;
    };
    const char *force = std::getenv("PFGRAD_VARIANT");
    int v = -1;
    if (caller == Caller::Grid) p.family = Family::Grid;
    else if (smoother == PFG_SMOOTHER_KALMAN) p.family = Family::Kalman;
    else if (smoother == PFG_SMOOTHER_KALMAN_FFBS) p.family = Family::KalmanFfbs;
    else if (smoother == PFG_SMOOTHER_PARIS) p.family = Family::Paris;
    else if (smoother == PFG_SMOOTHER_NEMETH_SYSTEMATIC) p.family = Family::Systematic;
    else if (smoother == PFG_SMOOTHER_POYIADJIS_N2) p.family = Family::N2;
    else if (predictive && n_max <= pfg::MEM_MAX_N) p.family = Family::Mem;
    else {
        p.family = pick_plain(model, dtype, rng, n_max, B, force, v);
        if (p.family == Family::None)
            return refuse(p, PFG_ERR_UNSUPPORTED, "N = " + std::to_string(n_max) + " exceeds the supported maximum of " + std::to_string(pfg::GRID_MAX_N));
        if (p.family == Family::Grid && caller == Caller::Device)
            return refuse(p, PFG_ERR_UNSUPPORTED, "N = " + std::to_string(n_max) + " > " + std::to_string(pfg::MEM_MAX_N) +
                                                      " runs as a whole-GPU window, one launch per timestep: use pfg_launch_device_grid (it needs T_max)");
        // PFGRAD_VARIANT=grid: the whole-GPU window also where a one-workgroup kernel would serve (tests, A/B timing)
        if (caller == Caller::Batch && !predictive && force && !std::strcmp(force, "grid")) p.family = Family::Grid;
        // N > 1024 with the device generator: the fast large-N kernel, unless PFGRAD_VARIANT=mem1024 asks for the general
        // one (A/B timing, tests; a predictive batch has taken the general one above)
        if (p.family == Family::Mem && rng == PFG_RNG_DEVICE && !(force && !std::strcmp(force, "mem1024"))) p.family = Family::Big;
    }
    switch (p.family) {
        case Family::Reg: {
            const Variant &e = kVariants[v];
            p.nt = e.NT; p.ppt = e.PPT; p.pp = e.pp;
            p.traced = traced;
            p.lds = e.lds(model, dtype, rng, n_max);
            p.name = e.tag;
            if (!reg_entry_built(model, rng, p.f64, e.NT, e.PPT, e.pp)) return refuse(p, PFG_ERR_UNSUPPORTED, "no kernel variant");
            p.score1 = !traced && reg_score1_twin(model, rng, p.f64, e.NT, e.PPT, e.pp) && score1_on();
            if (p.score1) p.name = e.tag1;
            break;
        }
        case Family::Mem:
            // the log-weights in registers: N <= 4096, and no window asks for the predictive statistic
            p.lw4 = !predictive && n_max <= 4096;
            // its score-only twin (GARCH: unmeasured here, +8 % in the LDS-resident REPLAY unit)
            p.score1 = p.lw4 && !traced && p.f64 && model != PFG_MODEL_GARCH && score1_on();
            p.name = p.score1 ? "mem1024_score1" : "mem1024";
            p.lds = mem_lds();
            p.scratch = mem_scratch(false);
            break;
        case Family::Big:
            p.np2 = n_max <= 4096 ? 4096 : 16384;
            p.name = p.np2 == 4096 ? "big4096" : "big16384";
            p.lds = with_types(model, dtype, rng, [&](auto, auto, auto real, auto) { return pfg::big_kernel_lds_bytes<decltype(real)>(p.np2); });
            p.scratch = mem_scratch(false);         // (what the general kernel needs: the fast path uses less)
            break;
        case Family::Paris:
        case Family::N2: {
            const bool paris = p.family == Family::Paris;
            const std::string pf = paris ? "pf = 'paris'" : "pf = 'poyiadjis_N2'";
            if (paris) {
                // PaRIS in one wave per window (64 threads x 2 particles, N <= 128): picked like wg64x2s for plain
                // windows -- device generator, more than kLatencyBatch windows; REPLAY, lone windows and N > 128 keep
                // the 256-thread variants.
                // PFGRAD_VARIANT=<tag> forces any PaRIS LDS-resident variant that holds n_max (tests, A/B timing).
                const ParisVariant *pv = nullptr;
                for (const ParisVariant &e : kParisVariants)
                    if (force && !std::strcmp(force, e.tag) && n_max <= e.NT * e.PPT) pv = &e;
                if (!pv && n_max <= 128 && rng == PFG_RNG_DEVICE && B > kLatencyBatch) pv = &kParisVariants[0];
                if (pv) {
                    p.nt = pv->NT; p.ppt = pv->PPT; p.name = pv->tag;
                    p.lds = pv->lds(model, dtype, rng, n_max);
                    if (p.lds > kLdsLimit)
                        return refuse(p, PFG_ERR_UNSUPPORTED, pf + ": N = " + std::to_string(n_max) + " does not fit the LDS-resident variant");
                    break;
                }
            }
            if (n_max <= 1024) {
                p.nt = 256; p.ppt = n_max <= 256 ? 1 : 4;
                p.name = paris ? (p.ppt == 1 ? "paris256x1" : "paris256x4") : (p.ppt == 1 ? "n2_256x1" : "n2_256x4");
                p.lds = (paris ? (p.ppt == 1 ? reg_lds<256, 1, true, pfg::MODE_PARIS> : reg_lds<256, 4, true, pfg::MODE_PARIS>)
                               : (p.ppt == 1 ? reg_lds<256, 1, true, pfg::MODE_N2> : reg_lds<256, 4, true, pfg::MODE_N2>))(model, dtype, rng, n_max);
                if (p.lds > kLdsLimit)
                    return refuse(p, PFG_ERR_UNSUPPORTED, pf + ": N = " + std::to_string(n_max) + " does not fit the LDS-resident variant");
                break;
            }
            // the large-N kernel's PaRIS instantiation (also its O(N^2) sweep): state in the HBM scratch
            p.name = paris ? "paris_mem1024" : "n2_mem1024";
            p.scratch = mem_scratch(true);
            if (n_max > pfg::MEM_MAX_N)
                return refuse(p, PFG_ERR_UNSUPPORTED, pf + " is implemented for N <= 16384 (N = " + std::to_string(n_max) + ")");
            p.nt = pfg::MEM_NT;
            p.lds = mem_lds();
            break;
        }
        case Family::Systematic:        // the 256 x 4 default variants of fp64 / f32
            p.name = "systematic256x4";
            p.nt = 256; p.ppt = 4; p.pp = !p.f64;
            if (rng != PFG_RNG_DEVICE) return refuse(p, PFG_ERR_UNSUPPORTED, "systematic resampling needs the DEVICE rng");
            if (n_max > 1024) return refuse(p, PFG_ERR_UNSUPPORTED, "systematic resampling is built for N <= 1024");
            p.lds = (p.f64 ? reg_lds<256, 4, false, pfg::MODE_SYSTEMATIC> : reg_lds<256, 4, true, pfg::MODE_SYSTEMATIC>)(model, dtype, rng, n_max);
            if (p.lds > kLdsLimit) return refuse(p, PFG_ERR_UNSUPPORTED, "systematic resampling: state does not fit LDS");
            break;
        case Family::Grid: {
            // every window of the batch must fall into the same tile class; NEMETH / FILTER with the score, sufficient or
            // no statistic
            p.ppt = pfg::grid_ppt(n_max); p.kmax = pfg::grid_kmax(n_max);
            p.score1 = rng == PFG_RNG_DEVICE && score1_on();
            p.name = p.ppt == 8 ? (p.score1 ? "grid2048_score1" : "grid2048") : (p.score1 ? "grid1024_score1" : "grid1024");
            if (n_max > pfg::GRID_MAX_N)
                return refuse(p, PFG_ERR_UNSUPPORTED, "N = " + std::to_string(n_max) + " exceeds the supported maximum of " + std::to_string(pfg::GRID_MAX_N));
            // REPLAY: PFGRAD_CDF_SINGLE=1 computes the reference's CDF with the lone-workgroup kernel (A/B and cross-check)
            const char *single = std::getenv("PFGRAD_CDF_SINGLE");
            p.cdf_single = single && single[0] == '1';
            with_types(model, dtype, rng, [&](auto m, auto, auto real, auto g) {
                using REAL = decltype(real);
                const pfg::GridLayout L = pfg::grid_layout<decltype(m)::value, REAL>(n_max, rng == PFG_RNG_REPLAY);
                p.tiles = L.G;
                p.scratch = L.bytes;
                if (rng == PFG_RNG_REPLAY)      // the timestep kernel's LDS: the coarse table of any window N <= n_max fits CR(n_max)
                    p.lds = p.ppt == 4 ? pfg::grid_step_lds_bytes<pfg::GRID_NT, 4, REAL, decltype(g)::value>(L.CR)
                                       : pfg::grid_step_lds_bytes<pfg::GRID_NT, 8, REAL, decltype(g)::value>(L.CR);
                else
                    p.lds = 8 * (p.ppt == 4 ? pfg::grid_dev_lds_doubles<pfg::GRID_NT, 4>(L.G) : pfg::grid_dev_lds_doubles<pfg::GRID_NT, 8>(L.G));
                return 0;
            });
            break;
        }
        case Family::Kalman:
            // n_max = the longest window [t1, tL) of the batch: the backward messages stored per window
            p.name = "kalman";
            p.traced = false;
            p.scratch = (16 * ((size_t)n_max + 1) + 255) / 256 * 256;
            break;
        case Family::KalmanFfbs:
            // n_max = the most paths of a window (the workgroup: one lane per path, lanes loop beyond 256); t_max = the
            // longest buffer, whose forward messages are stored per window
            p.name = "kalman_ffbs";
            p.traced = true;        // trace_x = the sampled paths
            p.nt = n_max <= 64 ? 64 : n_max <= 128 ? 128 : 256;
            p.scratch = (16 * ((size_t)t_max + 1) + 255) / 256 * 256;
            break;
        case Family::None:
            break;
    }
    return p;
}

// The ids a batch of `smoother` windows is built for.  The exact Kalman score ignores the proposal kernel and the
// generator; FFBS ignores the proposal kernel, its normals come from REPLAY z or the DEVICE generator.
int check_ids(pfg_ctx *ctx, int smoother, int model, int kernel, int dtype, int rng) {
    if (smoother == PFG_SMOOTHER_KALMAN || smoother == PFG_SMOOTHER_KALMAN_FFBS) {
        const bool ffbs = smoother == PFG_SMOOTHER_KALMAN_FFBS;
        const std::string what = ffbs ? "FFBS latent paths (kind = 'complete') are" : "the exact Kalman score (kind = 'marginal') is";
        if (model != PFG_MODEL_LGSSM) return fail(ctx, PFG_ERR_UNSUPPORTED, what + " built for LGSSM only");
        if (dtype != PFG_F64) return fail(ctx, PFG_ERR_UNSUPPORTED, what + " built for dtype f64 only");
        if (!ffbs) return PFG_OK;
    } else {
        if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
        if (kernel != PFG_KERNEL_PRIOR && kernel != PFG_KERNEL_OPTIMAL)
            return fail(ctx, PFG_ERR_INVALID, "Unrecoginized kernel id");
        if (model == PFG_MODEL_SVM && kernel == PFG_KERNEL_OPTIMAL)
            return fail(ctx, PFG_ERR_UNSUPPORTED, "SVM optimal kernel not analytic");   // svm/helper.py:62
        if (dtype != PFG_F64 && dtype != PFG_F32) return fail(ctx, PFG_ERR_INVALID, "bad dtype");
    }
    if (rng != PFG_RNG_REPLAY && rng != PFG_RNG_DEVICE) return fail(ctx, PFG_ERR_INVALID, "bad rng mode");
    return PFG_OK;
}

// B windows of the descriptors dp on st, as planned: the kernel's name becomes pfg_last_variant once it is chosen
int launch(pfg_ctx *ctx, const LaunchPlan &p, int model, int kernel, int rng, int B, const pfg_dev_problem *dp, hipStream_t st) {
    if (p.family == Family::Grid && B > 65535) return fail(ctx, PFG_ERR_INVALID, "at most 65535 whole-GPU windows per launch");
    if (p.name) {
        ctx->last_variant = p.name;
        ctx->last_traced = p.traced;
    }
    if (p.rc) return fail(ctx, p.rc, p.err);
    if (p.family == Family::Kalman) return launch_kalman(ctx, p, B, dp, st);
    if (p.family == Family::KalmanFfbs) return launch_ffbs(ctx, p, rng, B, dp, st);
    return with_types(model, kernel, PFG_F64, rng, [&](auto m, auto k, auto, auto g) {
        return launch_mkr<decltype(m)::value, decltype(k)::value, decltype(g)::value>(ctx, p, B, dp, st);
    });
}

int dispatch(pfg_ctx *ctx, Caller caller, int model, int kernel, int dtype, int rng, int smoother, int n_max, int B,
             const pfg_dev_problem *dp, hipStream_t st, bool traced = false, int t_max = 0, int phase = -1) {
    const int rc = check_ids(ctx, smoother, model, kernel, dtype, rng);
    if (rc) return rc;
    if (B <= 0) return PFG_OK;
    if (n_max < 1 && smoother != PFG_SMOOTHER_KALMAN) return fail(ctx, PFG_ERR_INVALID, "N must be >= 1");
    if (caller == Caller::Grid && t_max < 0) return fail(ctx, PFG_ERR_INVALID, "T_max must be >= 0");
    return launch(ctx, make_plan(caller, model, dtype, rng, smoother, n_max, B, traced, false, t_max, phase), model, kernel, rng, B, dp, st);
}

// ---- SGLD update for resident chains ---------------------------------------------------
__device__ __forceinline__ double reflect_chol(double L) { return L < 0.0 ? sqrt(L * L + 1e-16) : L; }

// momentum == nullptr: SGLD.  Otherwise SGHMC with friction alpha: the increment d of each
// variable becomes v <- (1 - alpha) v + drift + sqrt(alpha) * noise (noise ~ N(0, 2 eps / T)).
__global__ void sgld_update_kernel(int model, int B, double *__restrict__ theta,
                                   const double *__restrict__ outs, pfg_prior_hyper hy, double eps,
                                   double Tscale, uint64_t seed, uint64_t chain_offset,
                                   const uint64_t *step_ctr, double *__restrict__ momentum, double alpha) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double *th = theta + (size_t)b * PFG_MAX_THETA;
    const double *g = outs + (size_t)b * PFG_OUT_DOUBLES;
    const uint64_t step = step_ctr ? *step_ctr : 0ull;
    const uint64_t gid = chain_offset + (uint64_t)b;
    const uint32_t c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32) ^ (uint32_t)(gid >> 32);
    pfg::u32x4 r0 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x5A11u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    pfg::u32x4 r1 = pfg::philox4x32_10({(uint32_t)gid, c1, c2, 0x5A12u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double nsd = sqrt(1.0 / Tscale) * sqrt(2.0 * eps) * (momentum ? sqrt(alpha) : 1.0);
    double *mv = momentum ? momentum + (size_t)b * PFG_MAX_THETA : nullptr;
    // one variable's increment: SGLD drift + noise, or the SGHMC momentum recursion
    auto incr = [&](int slot, double drift, double noise) {
        const double d = drift + noise;
        if (!mv) return d;
        const double v = (1.0 - alpha) * mv[slot] + d;
        mv[slot] = v;
        return v;
    };
    double nz[4];
    const pfg::Math<double, false> mth = {};
    mth.normal_pair(r0.x, r0.y, nz[0], nz[1]);
    mth.normal_pair(r1.x, r1.y, nz[2], nz[3]);
    if (model == PFG_MODEL_SVM || model == PFG_MODEL_LGSSM) {
        const bool lg = model == PFG_MODEL_LGSSM;
        double A = th[0], C = lg ? th[1] : 1.0, LQ = th[lg ? 2 : 1], LR = th[lg ? 3 : 2];
        double Qinv = LQ * LQ + 1e-16, Rinv = LR * LR + 1e-16;
        // score columns: SVM [LR, LQ, A]; LGSSM [LR, LQ, C, A]
        double gLR = g[0], gLQ = g[1], gC = lg ? g[2] : 0.0, gA = g[lg ? 3 : 2];
        // grad_logprior: covariance.py:272-284 (n = 1), matrices.py:597-607
        double pLQ = (hy.df_Qinv - 2.0) / LQ - LQ / hy.scale_Qinv;
        double pLR = (hy.df_Rinv - 2.0) / LR - LR / hy.scale_Rinv;
        double pA = -1.0 * (Qinv * (A - hy.mean_A)) / hy.var_col_A;
        double pC = -1.0 * (Rinv * (C - hy.mean_C)) / hy.var_col_C;
        int j = 0;
        A += incr(0, eps * ((pA + gA) / Tscale), nsd * nz[j]); ++j;
        if (lg) { C += incr(1, eps * ((pC + gC) / Tscale), nsd * nz[j]); ++j; }
        LQ += incr(lg ? 2 : 1, eps * ((pLQ + gLQ) / Tscale), nsd * nz[j]); ++j;
        LR += incr(lg ? 3 : 2, eps * ((pLR + gLR) / Tscale), nsd * nz[j]); ++j;
        // project_parameters: _utils.py:165-170, covariance.py:68-80, lgssm/parameters.py:39-42
        double aa = fabs(A);
        if (aa > 0.9999) A *= 0.9999 / aa;
        if (lg) C = 1.0;
        LQ = reflect_chol(LQ); LR = reflect_chol(LR);
        th[0] = A;
        if (lg) { th[1] = C; th[2] = LQ; th[3] = LR; } else { th[1] = LQ; th[2] = LR; }
    } else {
        double lmu = th[0], lphi = th[1], llam = th[2], LR = th[3];
        double mu = exp(lmu), phi = 1.0 / (1.0 + exp(-lphi)), lam = 1.0 / (1.0 + exp(-llam));
        // garch_var.py:152-165
        double p0 = -hy.shape_mu - 1.0 + hy.scale_mu / mu;
        double p1 = ((hy.alpha_phi - 1.0) / (1.0 + phi) - (hy.beta_phi - 1.0) / (1.0 - phi)) * phi * (1.0 - phi);
        double p2 = ((hy.alpha_lambduh - 1.0) / (1.0 + lam) - (hy.beta_lambduh - 1.0) / (1.0 - lam)) * lam * (1.0 - lam);
        double pLR = (hy.df_Rinv - 2.0) / LR - LR / hy.scale_Rinv;
        // score columns [LR, log_mu, logit_phi, logit_lambduh]
        lmu += incr(0, eps * ((p0 + g[1]) / Tscale), nsd * nz[0]);
        lphi += incr(1, eps * ((p1 + g[2]) / Tscale), nsd * nz[1]);
        llam += incr(2, eps * ((p2 + g[3]) / Tscale), nsd * nz[2]);
        LR += incr(3, eps * ((pLR + g[0]) / Tscale), nsd * nz[3]);
        th[0] = lmu; th[1] = lphi; th[2] = llam; th[3] = reflect_chol(LR);
    }
}

__global__ void bump_counter_kernel(uint64_t *ctr) { *ctr += 1; }

// window starts for resident chains (see pfg_sample_windows_device)
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

// ---- IMQ kernel Stein discrepancy: all K^2 pairs, row i per workgroup-stride, f64 ----------
constexpr int KSD_MAX_D = 8;
__global__ __launch_bounds__(256) void imq_ksd_kernel(int K, int d, const double *__restrict__ x,
                                                      const double *__restrict__ g, double c2, double beta,
                                                      double *__restrict__ partial) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = blockIdx.x; i < K; i += gridDim.x) {
        double xi[KSD_MAX_D], gi[KSD_MAX_D];
        for (int k = 0; k < d; ++k) { xi[k] = x[(size_t)i * d + k]; gi[k] = g[(size_t)i * d + k]; }
        for (int j = threadIdx.x; j < K; j += blockDim.x) {
            double diff2 = 0.0, gg = 0.0, g0d = 0.0, g1d = 0.0;
            for (int k = 0; k < d; ++k) {
                const double df = xi[k] - x[(size_t)j * d + k];
                const double gj = g[(size_t)j * d + k];
                diff2 += df * df; gg += gi[k] * gj; g0d += gi[k] * -df; g1d += gj * df;
            }
            const double base = diff2 + c2;
            const double bb = pow(base, -beta);
            const double coeff = -2.0 * beta * (bb / base);
            acc += gg * bb + g0d * coeff + g1d * coeff + (-(double)d + 2.0 * (beta + 1.0) * diff2 / base) * coeff;
        }
    }
    acc = pfg::wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- elementwise sufficient statistics: second pass over the recorded trajectory (pfg_elementwise.hpp) ----
int elementwise_pass(pfg_ctx *ctx, const pfg_problem &q, const double *theta_dev, const double *tx, const double *tlw, const int32_t *par, int Nt,
                     size_t Wd, double *S0, double *S1, double *Sbar, double *w, double *mean, double *stats) {
    const int N = q.N, T = q.T, NS = state_dim(q.model);
    const int tL = q.tL < q.T ? q.tL : q.T;
    const double lam = q.smoother == PFG_SMOOTHER_NEMETH ? q.lambduh : 1.0;
    hipStream_t st = ctx->stream;
    PFG_HIP(ctx, hipMemsetAsync(S0, 0, (size_t)N * Wd * 8, st));
    double *cur = S0, *nxt = S1;
    const dim3 cgrid((unsigned)((Wd + 255) / 256)), sgrid((unsigned)((Wd + 255) / 256), (unsigned)N);
    for (int t = 0; t < T; ++t) {
        if (lam != 1.0) {
            hipLaunchKernelGGL(pfg::ews_softmax_kernel, dim3(1), dim3(1024), 0, st, N, tlw + (size_t)t * N, w);
            hipLaunchKernelGGL(pfg::ews_colsum_kernel, cgrid, dim3(256), 0, st, N, (int)Wd, cur, w, Sbar);
        }
        const bool inside = t >= q.t1 && t < tL;
        const int col0 = inside ? 3 * (t - q.t1) : -1;
        const double wt = (inside && q.weights) ? q.weights[t - q.t1] : 1.0;
        const int32_t *pt = par + (size_t)t * Nt * N;
        const double *xt = tx + (size_t)t * N * NS, *xn = tx + (size_t)(t + 1) * N * NS;
        if (q.smoother == PFG_SMOOTHER_POYIADJIS_N2) {
            const double *lwt = tlw + (size_t)t * N;
            if (q.model == PFG_MODEL_GARCH)
                hipLaunchKernelGGL(pfg::ews_n2_step_kernel<PFG_MODEL_GARCH>, dim3(N), dim3(256), 0, st, N, (int)Wd, wt, col0, theta_dev, xt, lwt, xn, cur, nxt);
            else if (q.model == PFG_MODEL_LGSSM)
                hipLaunchKernelGGL(pfg::ews_n2_step_kernel<PFG_MODEL_LGSSM>, dim3(N), dim3(256), 0, st, N, (int)Wd, wt, col0, theta_dev, xt, lwt, xn, cur, nxt);
            else
                hipLaunchKernelGGL(pfg::ews_n2_step_kernel<PFG_MODEL_SVM>, dim3(N), dim3(256), 0, st, N, (int)Wd, wt, col0, theta_dev, xt, lwt, xn, cur, nxt);
        } else if (q.model == PFG_MODEL_GARCH)
            hipLaunchKernelGGL(pfg::ews_step_kernel<PFG_MODEL_GARCH>, sgrid, dim3(256), 0, st, N, (int)Wd, Nt, lam, wt, col0, pt, xt, xn, Sbar, cur, nxt);
        else
            hipLaunchKernelGGL(pfg::ews_step_kernel<PFG_MODEL_SVM>, sgrid, dim3(256), 0, st, N, (int)Wd, Nt, lam, wt, col0, pt, xt, xn, Sbar, cur, nxt);
        double *tmp = cur; cur = nxt; nxt = tmp;
    }
    hipLaunchKernelGGL(pfg::ews_softmax_kernel, dim3(1), dim3(1024), 0, st, N, tlw + (size_t)T * N, w);
    hipLaunchKernelGGL(pfg::ews_colsum_kernel, cgrid, dim3(256), 0, st, N, (int)Wd, cur, w, mean);
    if (stats) PFG_HIP(ctx, hipMemcpyAsync(stats, cur, (size_t)N * Wd * 8, hipMemcpyDeviceToDevice, st));
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

}  // namespace

// ======================================================================================
// C ABI
// ======================================================================================
// ---- caller-registered pinned host ranges (pfg_host_register) -------------------------------------
namespace {
constexpr size_t kDirectMinDoubles = (size_t)1 << 16;     // inputs at least this long are staged from registered pages directly
struct HostRange { const char *lo, *hi; };
std::mutex g_host_mu;
std::vector<HostRange> g_host_ranges;
bool host_registered(const void *p, size_t bytes) {
    const char *a = static_cast<const char *>(p);
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (const HostRange &r : g_host_ranges)
        if (a >= r.lo && a + bytes <= r.hi) return true;
    return false;
}

// ---- pfg_run_batch: validation, the batch summary, one description of every buffer ---------------------------------
// One window of a batch whose first window is `first` (everything `first` decides is shared by the batch): PFG_OK, or
// the first rule it breaks.
int check_window(pfg_ctx *ctx, const pfg_problem &q, const pfg_result &r, const pfg_problem &first, int b) {
    const std::string id = "problem " + std::to_string(b) + ": ";
    auto bad = [&](int code, const char *msg) { return fail(ctx, code, id + msg); };
    const int model = first.model, dtype = first.dtype, rng = first.rng;
    const bool kalman = first.smoother == PFG_SMOOTHER_KALMAN;     // the exact score: no particles, no streams
    const bool ffbs = first.smoother == PFG_SMOOTHER_KALMAN_FFBS;  // FFBS paths: N paths, REPLAY normals in z only
    auto mixed = [&](int s) { return (q.smoother == s) != (first.smoother == s); };   // s is all or none of a batch
    if (q.model != model || q.kernel != first.kernel || q.dtype != dtype || q.rng != rng)
        return bad(PFG_ERR_INVALID, "model/kernel/dtype/rng must match across a batch");
    if (q.N < 1 && !kalman) return bad(PFG_ERR_INVALID, "N must be >= 1");
    if (q.T < 0) return bad(PFG_ERR_INVALID, "T must be >= 0");
    if (q.t1 < 0 || q.tL < q.t1) return bad(PFG_ERR_INVALID, "need 0 <= t1 <= tL");
    if ((q.smoother < PFG_SMOOTHER_NEMETH || q.smoother > PFG_SMOOTHER_POYIADJIS_N2) && q.smoother != PFG_SMOOTHER_KALMAN &&
        q.smoother != PFG_SMOOTHER_KALMAN_FFBS)
        return bad(PFG_ERR_INVALID, "Unrecognized pf (smoother id)");
    if (mixed(PFG_SMOOTHER_KALMAN_FFBS)) return bad(PFG_ERR_INVALID, "FFBS latent paths cannot share a batch with other smoothers");
    if (mixed(PFG_SMOOTHER_KALMAN)) return bad(PFG_ERR_INVALID, "the exact Kalman score cannot share a batch with particle filters");
    if (kalman || ffbs) {       // the exact LGSSM passes: a forward message from the prior, no particles
        if (q.t1 > q.T) return bad(PFG_ERR_INVALID, "need t1 <= T");
        if (!(q.prior_var > 0.0) || !std::isfinite(q.prior_var) || !std::isfinite(q.prior_mean))
            return bad(PFG_ERR_INVALID, "the forward message needs a finite precision > 0 (prior_var = 1 / precision)");
        if (q.init_x || q.elementwise || q.paris_stream ||
            (ffbs ? q.stat != PFG_STAT_SCORE && q.stat != PFG_STAT_NONE && q.stat != PFG_STAT_GIBBS : q.stat == PFG_STAT_PREDICTIVE))
            return bad(PFG_ERR_INVALID, ffbs ? "FFBS latent paths take no warm start or elementwise statistic; stat is score, none or gibbs"
                                             : "the exact Kalman score takes no warm start, elementwise or predictive statistic");
        if (r.x_T || r.logw_T || r.stats_T || (kalman && r.trace_x) || r.trace_logw || r.trace_stats || r.trace_ll || r.trace_anc ||
            r.rec_u || r.rec_z || r.rec_z0 || r.rec_ud || r.ew_mean || r.ew_stats)
            return bad(PFG_ERR_INVALID, ffbs ? "FFBS latent paths have no particles: only the result record and trace_x (the paths)"
                                             : "the exact Kalman score has no particles: only the result record");
        if (ffbs && rng == PFG_RNG_REPLAY && q.T > 0 && !q.z) return bad(PFG_ERR_INVALID, "REPLAY FFBS needs z (T N normals)");
        if (ffbs && q.stat == PFG_STAT_GIBBS && q.N != 1)
            return bad(PFG_ERR_INVALID, "the Gibbs statistic (PFG_STAT_GIBBS) is of one path: N must be 1");
    }
    if (mixed(PFG_SMOOTHER_POYIADJIS_N2)) return bad(PFG_ERR_INVALID, "pf = 'poyiadjis_N2' cannot share a batch with other smoothers");
    if (q.smoother == PFG_SMOOTHER_POYIADJIS_N2 && q.N > pfg::MEM_MAX_N)
        return bad(PFG_ERR_UNSUPPORTED, "pf = 'poyiadjis_N2' is implemented for N <= 16384");
    if (q.smoother == PFG_SMOOTHER_POYIADJIS_N2 && q.elementwise && q.N > 4096)
        return bad(PFG_ERR_UNSUPPORTED, "elementwise statistics with pf = 'poyiadjis_N2' are implemented for N <= 4096");
    if (q.smoother == PFG_SMOOTHER_POYIADJIS_N2 && q.stat == PFG_STAT_PREDICTIVE)
        return bad(PFG_ERR_INVALID, "Only can use pf = 'filter' since we are filtering");
    if (mixed(PFG_SMOOTHER_PARIS)) return bad(PFG_ERR_INVALID, "pf = 'paris' cannot share a batch with other smoothers");
    if (q.smoother == PFG_SMOOTHER_PARIS) {
        if (q.Ntilde < 1 || q.Ntilde > 64) return bad(PFG_ERR_INVALID, "Ntilde must be in [1, 64]");
        if (q.max_accept_reject < 0) return bad(PFG_ERR_INVALID, "max_accept_reject must be >= 0");
        if (q.paris_stream) {
            if (rng != PFG_RNG_REPLAY) return bad(PFG_ERR_INVALID, "paris_stream is a REPLAY input");
            if (q.paris_idx_u || q.paris_acc_u || q.paris_man_u)
                return bad(PFG_ERR_INVALID, "paris_stream replaces the addressed pools paris_idx_u / acc_u / man_u");
            if (q.paris_stream_len < 0 || q.paris_manual_threshold < 0)
                return bad(PFG_ERR_INVALID, "paris_stream_len and paris_manual_threshold must be >= 0");
            if (q.N > pfg::MEM_MAX_N) return bad(PFG_ERR_UNSUPPORTED, "pf = 'paris' is implemented for N <= 16384");
            if ((q.flags & PFG_FLAG_PARIS_RAW_STREAM) && dtype != PFG_F64)
                return bad(PFG_ERR_UNSUPPORTED, "PFG_FLAG_PARIS_RAW_STREAM is built for dtype f64 (it reproduces np.random's doubles)");
            if ((q.flags & PFG_FLAG_PARIS_RAW_STREAM) && (q.z0 || q.u || q.z))
                return bad(PFG_ERR_INVALID, "PFG_FLAG_PARIS_RAW_STREAM draws z0 / u / z from paris_stream: they must be NULL");
            if ((q.flags & PFG_FLAG_PARIS_RAW_CARRY) && (!(q.flags & PFG_FLAG_PARIS_RAW_STREAM) || q.paris_stream_len < 1))
                return bad(PFG_ERR_INVALID, "PFG_FLAG_PARIS_RAW_CARRY needs PFG_FLAG_PARIS_RAW_STREAM and the cached Gaussian in paris_stream[0]");
            if ((q.flags & PFG_FLAG_PARIS_RAW_CARRY) && q.init_x && q.T == 0)
                return bad(PFG_ERR_INVALID, "PFG_FLAG_PARIS_RAW_CARRY with a warm start and T = 0 draws no normal: nothing to carry the cached Gaussian through");
        } else if (rng == PFG_RNG_REPLAY && (!q.paris_man_u || (q.max_accept_reject > 0 && (!q.paris_idx_u || !q.paris_acc_u)))) {
            return bad(PFG_ERR_INVALID, "REPLAY paris needs the paris_* uniform pools or paris_stream");
        }
        if ((q.flags & (PFG_FLAG_PARIS_RAW_STREAM | PFG_FLAG_PARIS_RAW_CARRY)) && !q.paris_stream)
            return bad(PFG_ERR_INVALID, "PFG_FLAG_PARIS_RAW_STREAM needs paris_stream");
        if ((q.flags & PFG_FLAG_PARIS_NO_ACCEPT_REJECT) && !q.paris_stream)
            return bad(PFG_ERR_UNSUPPORTED, "PaRIS with accept_reject = False is built for the REPLAY stream order (paris_stream)");
    } else if (q.paris_stream) {
        return bad(PFG_ERR_INVALID, "paris_stream needs pf = 'paris'");
    }
    if ((q.stat < PFG_STAT_SCORE || q.stat > PFG_STAT_PREDICTIVE) && !(ffbs && q.stat == PFG_STAT_GIBBS))
        return bad(PFG_ERR_INVALID, "bad stat id");
    if ((q.stat == PFG_STAT_PREDICTIVE) != (first.stat == PFG_STAT_PREDICTIVE))
        return bad(PFG_ERR_INVALID, "the predictive statistic cannot share a batch with others");
    if (q.stat == PFG_STAT_PREDICTIVE) {
        if (q.smoother != PFG_SMOOTHER_FILTER)                                  // svm/helper.py:209-210
            return bad(PFG_ERR_INVALID, "Only can use pf = 'filter' since we are filtering");
        if (q.num_steps_ahead < 0 || q.num_steps_ahead >= PFG_MAX_PRED) return bad(PFG_ERR_INVALID, "num_steps_ahead must be in [0, 15]");
        if (q.N > pfg::MEM_MAX_N) return bad(PFG_ERR_UNSUPPORTED, "N exceeds the supported maximum of 16384");
        if (rng == PFG_RNG_REPLAY && model != PFG_MODEL_LGSSM && q.T > 0 && !q.pred_z)
            return bad(PFG_ERR_INVALID, "REPLAY predictive needs the pred_z pool");
    }
    if (!q.theta) return bad(PFG_ERR_INVALID, "theta is NULL");
    if (q.T > 0 && !q.y) return bad(PFG_ERR_INVALID, "observations are NULL");
    const bool raw_stream = q.smoother == PFG_SMOOTHER_PARIS && (q.flags & PFG_FLAG_PARIS_RAW_STREAM) != 0;
    const bool streams = rng == PFG_RNG_REPLAY && !raw_stream && !kalman && !ffbs;
    if (streams && !q.init_x && !q.z0) return bad(PFG_ERR_INVALID, "REPLAY needs z0");
    if (streams && q.T > 0 && (!q.u || !q.z)) return bad(PFG_ERR_INVALID, "REPLAY needs u and z");
    if (q.init_x && !q.init_logw) return bad(PFG_ERR_INVALID, "init_x needs init_logw");
    if (mixed(PFG_SMOOTHER_NEMETH_SYSTEMATIC))
        return bad(PFG_ERR_INVALID, "systematic resampling cannot share a batch with other smoothers");
    if (q.smoother == PFG_SMOOTHER_NEMETH_SYSTEMATIC && (rng != PFG_RNG_DEVICE || q.N > 1024))
        return bad(PFG_ERR_UNSUPPORTED, "systematic resampling needs the DEVICE rng and N <= 1024");
    if (!(q.prior_var >= 0.0) && !(q.flags & PFG_FLAG_GARCH_STATIONARY_PRIOR) && !q.init_x)
        return bad(PFG_ERR_INVALID, "prior_var must be >= 0");
    if (model == PFG_MODEL_SVM && std::fabs(q.theta[0]) > 1.0) {
        char buf[160];
        snprintf(buf, sizeof buf, "Current AR parameter is |A| = %.17g > 1\nTry calling project_parameters?", std::fabs(q.theta[0]));
        return fail(ctx, PFG_ERR_NUMERIC, buf);                                   // svm/kernels.py:6-11
    }
    if (q.elementwise) {
        if (q.smoother != PFG_SMOOTHER_NEMETH && q.smoother != PFG_SMOOTHER_PARIS && q.smoother != PFG_SMOOTHER_POYIADJIS_N2)
            return bad(PFG_ERR_UNSUPPORTED, "elementwise statistics are built for pf = 'poyiadjis_N' | 'nemeth' | 'paris' | 'poyiadjis_N2'");
        if (q.stat == PFG_STAT_PREDICTIVE) return bad(PFG_ERR_INVALID, "elementwise statistics do not combine with the predictive statistic");
        if (!r.ew_mean) return bad(PFG_ERR_INVALID, "elementwise needs ew_mean");
        if (r.trace_x || r.trace_logw || r.trace_stats || r.trace_anc || r.rec_u || r.rec_z || r.rec_z0 || r.rec_ud)
            return bad(PFG_ERR_INVALID, "elementwise statistics cannot be combined with trace outputs");
        if ((q.tL < q.T ? q.tL : q.T) - q.t1 < 1) return bad(PFG_ERR_INVALID, "elementwise needs a non-empty window [t1, tL)");
    } else if (r.ew_mean || r.ew_stats) {
        return bad(PFG_ERR_INVALID, "ew_mean / ew_stats need pfg_problem.elementwise");
    }
    if ((r.rec_u || r.rec_z || r.rec_z0 || r.rec_ud) && (rng != PFG_RNG_DEVICE || !r.trace_x))
        return bad(PFG_ERR_INVALID, "rec_u / rec_z / rec_z0 record the DEVICE generator's draws and need trace_x");
    if (r.trace_anc && !r.trace_x) return bad(PFG_ERR_INVALID, "trace_anc needs trace_x");
    if ((r.logw_T || r.stats_T) && !r.x_T) return bad(PFG_ERR_INVALID, "logw_T/stats_T need x_T");
    if (!ffbs && (r.trace_logw == nullptr) != (r.trace_x == nullptr)) return bad(PFG_ERR_INVALID, "trace_x and trace_logw go together");
    if (r.trace_stats && !r.trace_x) return bad(PFG_ERR_INVALID, "trace_stats needs trace_x");
    return PFG_OK;
}

// What the plan needs of a valid batch: the longest window (Kalman: of steps [t1, tL), else of particles), the longest
// FFBS buffer, whether any window records a trajectory, and the smoother to plan for.
struct BatchSummary { int n_max = 0, t_max = 0; bool traced = false; int smoother = PFG_SMOOTHER_NEMETH; };
BatchSummary summarize(int B, const pfg_problem *ps, const pfg_result *rs) {
    BatchSummary s;
    bool score1 = true;         // every window the Poyiadjis O(N) score: units with a twin specialised to it run that
    for (int b = 0; b < B; ++b) {
        const pfg_problem &q = ps[b];
        const pfg_result &r = rs[b];
        s.traced = s.traced || r.trace_x || r.trace_ll || r.rec_u || r.rec_z || r.rec_z0 || r.rec_ud || q.elementwise;
        score1 = score1 && q.smoother == PFG_SMOOTHER_NEMETH && q.lambduh == 1.0 && q.stat == PFG_STAT_SCORE;
        const int n = q.smoother == PFG_SMOOTHER_KALMAN ? (q.tL < q.T ? q.tL : q.T) - q.t1 : q.N;
        s.n_max = n > s.n_max ? n : s.n_max;
        if (q.smoother == PFG_SMOOTHER_KALMAN_FFBS) s.t_max = q.T > s.t_max ? q.T : s.t_max;
    }
    // the smoothers with kernels of their own fill whole batches; the rest run the plain kernels
    const int s0 = ps[0].smoother;
    if (s0 == PFG_SMOOTHER_PARIS || s0 == PFG_SMOOTHER_NEMETH_SYSTEMATIC || s0 == PFG_SMOOTHER_POYIADJIS_N2 ||
        s0 == PFG_SMOOTHER_KALMAN || s0 == PFG_SMOOTHER_KALMAN_FFBS)
        s.smoother = s0;
    else if (score1 && !s.traced)
        s.smoother = PFG_SMOOTHER_POYIADJIS_N;
    return s;
}

// The buffers of a batch, laid out window after window in the device arenas (offsets in doubles).  Each is described
// once, here, by describe_window; sizing, staging and fetching are loops over the pieces.
struct Layout {
    std::vector<Piece> &pieces;
    size_t n[3] = {0, 0, 0};        // doubles of the In, Out and Work arenas
    size_t n_host = 0;              // doubles of the pinned staging arena
    // observations / window weights that many windows share (same host pointer and length) are staged once: 12288
    // chains on one series would otherwise carry 98 MB of copies of the same 8 KB
    std::unordered_map<const double *, std::pair<size_t, size_t>> shared;     // source -> (length, offset)

    template <typename T>
    void add(T *&slot, Piece::Arena a, size_t at, size_t len, const double *src = nullptr, void *dst = nullptr,
             size_t bytes = 0, Piece::Copy copy = Piece::None) {
        pieces.push_back({&slot, src, dst, at, len, bytes, a, copy});
    }
    // an input of len doubles at src (none if either is 0); big inputs in caller-registered pinned memory
    // (pfg_host_register) go to the device straight from there, everything else through the staging arena
    template <typename T> void in(T *&slot, const double *src, size_t len) {
        if (!src || len == 0) return;
        const bool direct = len >= kDirectMinDoubles && host_registered(src, len * 8);
        if (!direct) n_host += len;
        add(slot, Piece::In, n[Piece::In], len, src, nullptr, 0, direct ? Piece::Direct : Piece::Staged);
        n[Piece::In] += len;
    }
    template <typename T> void in_shared(T *&slot, const double *src, size_t len) {
        if (!src || len == 0) return;
        auto it = shared.find(src);
        if (it != shared.end() && it->second.first == len) return add(slot, Piece::In, it->second.second, len);
        shared[src] = {len, n[Piece::In]};
        in(slot, src, len);
    }
    template <typename T> void out(T *&slot, size_t len, void *dst = nullptr, size_t bytes = 0) {
        add(slot, Piece::Out, n[Piece::Out], len, nullptr, dst, bytes);
        n[Piece::Out] += len;
    }
    // an output the caller asked for (dst non-NULL): len doubles of the arena, `bytes` of them fetched
    template <typename D, typename T> void want(D *dst, T *&slot, size_t len, size_t bytes) { if (dst) out(slot, len, dst, bytes); }
    template <typename T> void want(double *dst, T *&slot, size_t len) { want(dst, slot, len, len * 8); }
    template <typename T> void work(T *&slot, size_t len) {
        add(slot, Piece::Work, n[Piece::Work], len);
        n[Piece::Work] += len;
    }
};

// the elementwise pass's device-only statistic matrices (its traces are the descriptor's trace_x / trace_logw and
// trace_anc or trace_paris_J, redirected into the work arena)
struct EwPlan { double *S0, *S1, *Sbar, *w, *mean, *stats; size_t Wd; int Nt; };
constexpr int kOwnDoubles = PFG_MAX_THETA + 1;      // h_own per window: theta padded, the step counter

// Window q's buffers in arena order -- inputs: the series and weights (shared across the batch), theta, the REPLAY
// streams, the warm start, the PaRIS pools or stream, the predictive draws, the step counter; outputs: the PaRIS stream
// counts, the predictive statistic, the result record, then what r asks for -- and its descriptor's scalars.
void describe_window(Layout &L, const pfg_problem &q, pfg_result &r, pfg_dev_problem &d, EwPlan &e, double *own) {
    const int NS = state_dim(q.model), H = stat_dim(q.model), P = theta_dim(q.model);
    const size_t N = q.N, T = q.T, TN = T * N;
    const int tL = q.tL < q.T ? q.tL : q.T;
    const bool replay = q.rng == PFG_RNG_REPLAY, paris = q.smoother == PFG_SMOOTHER_PARIS;
    L.in_shared(d.y, q.y, T);
    L.in_shared(d.weights, q.weights, tL > q.t1 ? (size_t)(tL - q.t1) : 0);
    for (int j = 0; j < PFG_MAX_THETA; ++j) own[j] = j < P ? q.theta[j] : 0.0;
    L.in(d.theta, own, PFG_MAX_THETA);
    if (replay && q.smoother == PFG_SMOOTHER_KALMAN_FFBS) {
        L.in(d.z, q.z, TN);
    } else if (replay && q.smoother != PFG_SMOOTHER_KALMAN) {
        L.in(d.z0, q.z0, N);
        L.in(d.u, q.u, TN);
        L.in(d.z, q.z, TN);
    }
    if (q.init_x) {
        L.in(d.init_x, q.init_x, N * NS);
        L.in(d.init_logw, q.init_logw, N);
        L.in(d.init_stats, q.init_stats, N * H);
    }
    if (paris) {
        d.Ntilde = q.Ntilde; d.max_accept_reject = q.max_accept_reject;
        if (replay) {
            L.in(d.paris_idx_u, q.paris_idx_u, TN * q.Ntilde * q.max_accept_reject);
            L.in(d.paris_acc_u, q.paris_acc_u, TN * q.Ntilde * q.max_accept_reject);
            L.in(d.paris_man_u, q.paris_man_u, TN * q.Ntilde);
            if (q.paris_stream) {
                if (q.paris_stream_len > 0) L.in(d.paris_stream, q.paris_stream, q.paris_stream_len);
                else L.add(d.paris_stream, Piece::In, 0, 0);        // an empty stream is still "stream order" (non-NULL)
                d.paris_stream_len = q.paris_stream_len;
                d.paris_manual_threshold = q.paris_manual_threshold;
                L.out(d.paris_consumed, 2);                         // the consumed count, the carry-back distance
            }
        }
    }
    if (q.stat == PFG_STAT_PREDICTIVE) {
        d.num_steps_ahead = q.num_steps_ahead;
        if (replay && q.model != PFG_MODEL_LGSSM) L.in(d.pred_z, q.pred_z, TN * (q.num_steps_ahead + 1));
        L.want(r.pred, d.pred_out, PFG_MAX_PRED);
    }
    static_assert(offsetof(pfg_result, loglik) == offsetof(pfg_result, mean_stat) + PFG_MAX_STAT * 8, "record = mean_stat, loglik");
    if (q.stat == PFG_STAT_GIBBS) L.want(r.pred, d.out, PFG_OUT_DOUBLES);      // the whole record: 7 statistics
    else L.want(r.mean_stat, d.out, PFG_OUT_DOUBLES, (PFG_MAX_STAT + 1) * 8);
    L.want(r.x_T, d.final_x, N * NS);
    L.want(r.logw_T, d.final_logw, N);
    L.want(r.stats_T, d.final_stats, N * H);
    L.want(r.trace_x, d.trace_x, (T + (q.smoother == PFG_SMOOTHER_KALMAN_FFBS ? 0 : 1)) * N * NS);   // FFBS: the paths [T][N]
    L.want(r.trace_logw, d.trace_logw, (T + 1) * N);
    L.want(r.trace_stats, d.trace_stats, (T + 1) * N * H);
    L.want(r.trace_ll, d.trace_ll, T + 1);
    L.want(r.trace_anc, d.trace_anc, (TN + 1) / 2, TN * 4);         // int32 pairs in f64 slots
    if (q.elementwise) {
        e.Wd = 3 * (size_t)(tL - q.t1);
        e.Nt = paris ? q.Ntilde : 1;
        L.work(d.trace_x, (T + 1) * N * NS);
        L.work(d.trace_logw, (T + 1) * N);
        L.work(paris ? d.trace_paris_J : d.trace_anc, (TN * e.Nt + 1) / 2);
        L.work(e.S0, N * e.Wd);
        L.work(e.S1, N * e.Wd);
        L.work(e.Sbar, e.Wd);
        L.work(e.w, N);
        L.want(r.ew_mean, e.mean, e.Wd);
        L.want(r.ew_stats, e.stats, N * e.Wd);
    }
    L.want(r.rec_u, d.rec_u, (TN + 1) / 2, TN * 4);
    L.want(r.rec_z, d.rec_z, TN);
    L.want(r.rec_z0, d.rec_z0, N);
    L.want(r.rec_ud, d.rec_ud, TN);
    if (q.step) {       // the step counter of this window, as a resident chain would read it from HBM
        std::memcpy(own + PFG_MAX_THETA, &q.step, 8);
        L.in(d.step_ctr, own + PFG_MAX_THETA, 1);
    }
    d.prior_mean = q.prior_mean; d.prior_var = q.prior_var; d.lambduh = q.lambduh;
    d.seed = q.seed; d.stream = q.stream;
    d.T = q.T; d.t1 = q.t1; d.tL = tL; d.N = q.N;
    d.smoother = q.smoother; d.stat = q.stat; d.flags = q.flags;
}
}  // namespace

extern "C" {

int pfg_version(void) { return PFG_VERSION; }

int pfg_host_register(void *ptr, size_t bytes) {
    if (!ptr || bytes == 0) return PFG_ERR_INVALID;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        const char *a = static_cast<const char *>(ptr);
        for (const HostRange &r : g_host_ranges)
            if (a < r.hi && a + bytes > r.lo) return PFG_ERR_INVALID;      // overlaps a registered range
    }
    if (hipHostRegister(ptr, bytes, hipHostRegisterPortable) != hipSuccess) {
        (void)hipGetLastError();
        return PFG_ERR_DEVICE;
    }
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_ranges.push_back({static_cast<const char *>(ptr), static_cast<const char *>(ptr) + bytes});
    return PFG_OK;
}

int pfg_host_unregister(void *ptr) {
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_ranges.begin();
        for (; it != g_host_ranges.end(); ++it)
            if (it->lo == static_cast<const char *>(ptr)) break;
        if (it == g_host_ranges.end()) return PFG_ERR_INVALID;
        g_host_ranges.erase(it);
    }
    if (hipHostUnregister(ptr) != hipSuccess) {
        (void)hipGetLastError();
        return PFG_ERR_DEVICE;
    }
    return PFG_OK;
}

int pfg_struct_size(int which) {
    switch (which) {
        case 0: return (int)sizeof(pfg_problem);
        case 1: return (int)sizeof(pfg_result);
        case 2: return (int)sizeof(pfg_dev_problem);
        case 3: return (int)sizeof(pfg_prior_hyper);
    }
    return -1;
}

const char *pfg_last_error(pfg_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int pfg_create(pfg_ctx **out, int device_id) {
    if (!out) return fail(nullptr, PFG_ERR_INVALID, "pfg_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, PFG_ERR_DEVICE, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, PFG_ERR_INVALID, "pfg_create: bad device id");
    pfg_ctx *ctx = new (std::nothrow) pfg_ctx();
    if (!ctx) return fail(nullptr, PFG_ERR_NOMEM, "pfg_create: out of host memory");
    ctx->device = device_id;
    if ((e = hipSetDevice(device_id)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
        std::string m = std::string("pfg_create: ") + hipGetErrorString(e);
        delete ctx;
        return fail(nullptr, PFG_ERR_DEVICE, m);
    }
    *out = ctx;
    return PFG_OK;
}

void pfg_destroy(pfg_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    ctx->in.release(); ctx->out.release(); ctx->desc.release(); ctx->scratch.release(); ctx->work.release(); ctx->h_in.release(); ctx->h_out.release();
    delete ctx;
}

const char *pfg_last_variant(pfg_ctx *ctx) { return ctx ? ctx->last_variant : "none"; }

int pfg_last_traced(pfg_ctx *ctx) { return ctx ? (ctx->last_traced ? 1 : 0) : -1; }

void *pfg_ctx_stream(pfg_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int pfg_synchronize(pfg_ctx *ctx) {
    if (!ctx) return PFG_ERR_INVALID;
    PFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PFG_OK;
}

// both for a large batch of plain windows: never the latency variant or a twin
int64_t pfg_scratch_bytes(int model, int dtype, int rng, int N) {
    if (model < 0 || model > 2 || N < 1) return -1;
    const LaunchPlan p = make_plan(Caller::Query, model, dtype, rng, PFG_SMOOTHER_NEMETH, N, 1 << 30, false);
    return p.name ? (int64_t)p.scratch : -1;
}

int64_t pfg_scratch_bytes_smoother(int model, int dtype, int rng, int smoother, int N) {
    if (model < 0 || model > 2 || N < 1 || smoother < PFG_SMOOTHER_NEMETH || smoother > PFG_SMOOTHER_POYIADJIS_N) return -1;
    const LaunchPlan p = make_plan(Caller::Device, model, dtype, rng, smoother, N, 1 << 30, false);
    return p.rc || !p.name ? -1 : (int64_t)p.scratch;
}

const char *pfg_variant_name(int model, int kernel, int dtype, int rng, int n_max) {
    (void)kernel;
    const LaunchPlan p = make_plan(Caller::Query, model, dtype, rng, PFG_SMOOTHER_NEMETH, n_max, 1 << 30, false);
    return p.name ? p.name : "none";
}

int pfg_launch_device(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int B,
                      const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!dev_probs && B > 0) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device: dev_probs is NULL");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    return dispatch(ctx, Caller::Device, model, kernel, dtype, rng, PFG_SMOOTHER_NEMETH, n_max, B, dev_probs, (hipStream_t)hip_stream);
}

int pfg_launch_device_traced(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother, int n_max, int B,
                             const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!dev_probs && B > 0) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_traced: dev_probs is NULL");
    if (smoother < PFG_SMOOTHER_NEMETH || smoother > PFG_SMOOTHER_POYIADJIS_N)
        return fail(ctx, PFG_ERR_INVALID, "Unrecognized pf (smoother id)");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    return dispatch(ctx, Caller::Device, model, kernel, dtype, rng, smoother, n_max, B, dev_probs, (hipStream_t)hip_stream, true);
}

int pfg_launch_device_smoother(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother, int n_max,
                               int B, const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!dev_probs && B > 0) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_smoother: dev_probs is NULL");
    if (smoother < PFG_SMOOTHER_NEMETH || smoother > PFG_SMOOTHER_KALMAN_FFBS)
        return fail(ctx, PFG_ERR_INVALID, "Unrecognized pf (smoother id)");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    return dispatch(ctx, Caller::Device, model, kernel, dtype, rng, smoother, n_max, B, dev_probs, (hipStream_t)hip_stream);
}

int pfg_launch_device_grid(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int T_max, int B,
                           const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!dev_probs && B > 0) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid: dev_probs is NULL");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    return dispatch(ctx, Caller::Grid, model, kernel, dtype, rng, PFG_SMOOTHER_NEMETH, n_max, B, dev_probs, (hipStream_t)hip_stream, true, T_max);
}

int pfg_launch_device_grid_smoother(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother, int n_max, int T_max,
                                    int phase, int B, const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!dev_probs && B > 0) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid_smoother: dev_probs is NULL");
    if (smoother != PFG_SMOOTHER_NEMETH && smoother != PFG_SMOOTHER_FILTER && smoother != PFG_SMOOTHER_POYIADJIS_N)
        return fail(ctx, PFG_ERR_UNSUPPORTED, "whole-GPU windows are built for NEMETH / FILTER / POYIADJIS_N");
    if (phase < PFG_GRID_PHASE_FINISH) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid_smoother: phase must be PFG_GRID_PHASE_ALL, a timestep >= 0, PFG_GRID_PHASE_INIT or PFG_GRID_PHASE_FINISH");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    return dispatch(ctx, Caller::Grid, model, kernel, dtype, rng, smoother, n_max, B, dev_probs, (hipStream_t)hip_stream, true,
                    phase == PFG_GRID_PHASE_ALL ? T_max : 0, phase);
}

int pfg_launch_device_grid_phase(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int phase, int B,
                                 const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!dev_probs && B > 0) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid_phase: dev_probs is NULL");
    if (phase < PFG_GRID_PHASE_FINISH) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid_phase: phase must be a timestep >= 0, PFG_GRID_PHASE_INIT or PFG_GRID_PHASE_FINISH");
    if (phase == -1) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid_phase: use pfg_launch_device_grid for the whole window");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    return dispatch(ctx, Caller::Grid, model, kernel, dtype, rng, PFG_SMOOTHER_NEMETH, n_max, B, dev_probs, (hipStream_t)hip_stream, true, 0, phase);
}

int pfg_sghmc_update_device(pfg_ctx *ctx, int model, int B, double *theta, double *momentum, const double *outs,
                            const pfg_prior_hyper *hyper, double epsilon, double alpha, double Tscale,
                            uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream);

int pfg_sgld_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                           const pfg_prior_hyper *hyper, double epsilon, double Tscale, uint64_t seed,
                           uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    return pfg_sghmc_update_device(ctx, model, B, theta, nullptr, outs, hyper, epsilon, 1.0, Tscale, seed,
                                   chain_offset, step_ctr, hip_stream);
}

int pfg_sghmc_update_device(pfg_ctx *ctx, int model, int B, double *theta, double *momentum, const double *outs,
                            const pfg_prior_hyper *hyper, double epsilon, double alpha, double Tscale,
                            uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!(alpha > 0.0 && alpha <= 1.0)) return fail(ctx, PFG_ERR_INVALID, "SGHMC friction alpha must be in (0, 1]");
    if (!theta || !outs || !hyper) return fail(ctx, PFG_ERR_INVALID, "pfg_sgld_update_device: NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    if (!(epsilon > 0.0) || !(Tscale > 0.0)) return fail(ctx, PFG_ERR_INVALID, "epsilon and Tscale must be > 0");
    if (B <= 0) return PFG_OK;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(sgld_update_kernel, dim3((B + 127) / 128), dim3(128), 0, st, model, B, theta, outs,
                       *hyper, epsilon, Tscale, seed, chain_offset, (const uint64_t *)step_ctr, momentum, alpha);
    if (step_ctr) hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, st, step_ctr);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

// the checks the SGRLD and Gibbs updates share: LGSSM chains only (the reference's one preconditioner and conjugate prior)
static int check_lgssm_update(pfg_ctx *ctx, const char *what, bool sgrld, int model, const double *theta,
                              const double *outs, const pfg_prior_hyper *hyper) {
    if (!theta || !outs || !hyper) return fail(ctx, PFG_ERR_INVALID, std::string(what) + ": NULL argument");
    if (model < 0 || model > 2) return fail(ctx, PFG_ERR_INVALID, "Unrecognized model id");
    const char *sampler = model == PFG_MODEL_SVM ? "SVMSampler" : "GARCHSampler";
    if (model != PFG_MODEL_LGSSM && sgrld)          // sgmcmc_sampler.py:643-646
        return fail(ctx, PFG_ERR_UNSUPPORTED, std::string(what) + ": No Default Preconditioner for " + sampler);
    if (model != PFG_MODEL_LGSSM)
        return fail(ctx, PFG_ERR_UNSUPPORTED, std::string(what) + ": no conjugate Gibbs draw for " + sampler);
    return PFG_OK;
}

int pfg_sgrld_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                            const pfg_prior_hyper *hyper, double epsilon, double Tscale,
                            uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    const int rc = check_lgssm_update(ctx, "pfg_sgrld_update_device", true, model, theta, outs, hyper);
    if (rc) return rc;
    if (!(epsilon > 0.0) || !(Tscale > 0.0)) return fail(ctx, PFG_ERR_INVALID, "epsilon and Tscale must be > 0");
    if (B <= 0) return PFG_OK;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const int lrc = launch_sgrld_update(ctx, B, theta, outs, *hyper, epsilon, Tscale, seed, chain_offset, step_ctr, st);
    if (lrc) return lrc;
    if (step_ctr) hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, st, step_ctr);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

int pfg_gibbs_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                            const pfg_prior_hyper *hyper, uint64_t seed, uint64_t chain_offset,
                            uint64_t *step_ctr, void *hip_stream) {
    if (!ctx) return PFG_ERR_INVALID;
    const int rc = check_lgssm_update(ctx, "pfg_gibbs_update_device", false, model, theta, outs, hyper);
    if (rc) return rc;
    if (B <= 0) return PFG_OK;
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const int lrc = launch_gibbs_update(ctx, B, theta, outs, *hyper, seed, chain_offset, step_ctr, st);
    if (lrc) return lrc;
    if (step_ctr) hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, st, step_ctr);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

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

int pfg_imq_ksd(pfg_ctx *ctx, int K, int d, const double *x, const double *g, double c, double beta,
                double *ksd_out) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!x || !g || !ksd_out) return fail(ctx, PFG_ERR_INVALID, "pfg_imq_ksd: NULL argument");
    if (K < 1 || d < 1 || d > KSD_MAX_D) return fail(ctx, PFG_ERR_INVALID, "pfg_imq_ksd: need K >= 1 and 1 <= d <= 8");
    if (!(beta > 0.0 && beta < 1.0)) return fail(ctx, PFG_ERR_INVALID, "pfg_imq_ksd: beta must be in (0,1)");
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)K * d;
    const int nblk = K < 1024 ? K : 1024;
    PFG_HIP(ctx, ctx->in.ensure(2 * n * 8));
    PFG_HIP(ctx, ctx->out.ensure((size_t)nblk * 8));
    double *dx = static_cast<double *>(ctx->in.ptr), *dg = dx + n;
    PFG_HIP(ctx, hipMemcpyAsync(dx, x, n * 8, hipMemcpyHostToDevice, ctx->stream));
    PFG_HIP(ctx, hipMemcpyAsync(dg, g, n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(imq_ksd_kernel, dim3(nblk), dim3(256), 0, ctx->stream, K, d, dx, dg, c * c, beta,
                       static_cast<double *>(ctx->out.ptr));
    PFG_HIP(ctx, hipGetLastError());
    PFG_HIP(ctx, ctx->h_out.ensure((size_t)nblk));
    PFG_HIP(ctx, hipMemcpyAsync(ctx->h_out.data(), ctx->out.ptr, (size_t)nblk * 8, hipMemcpyDeviceToHost, ctx->stream));
    PFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double tot = 0.0;
    for (int b = 0; b < nblk; ++b) tot += ctx->h_out[b];          // fixed order: reproducible
    *ksd_out = std::sqrt(tot) / (double)K;
    return PFG_OK;
}

int pfg_run(pfg_ctx *ctx, const pfg_problem *p, pfg_result *r) { return pfg_run_batch(ctx, 1, p, r); }

int pfg_run_batch(pfg_ctx *ctx, int B, const pfg_problem *ps, pfg_result *rs) {
    if (!ctx) return PFG_ERR_INVALID;
    if (B < 0 || (B > 0 && (!ps || !rs))) return fail(ctx, PFG_ERR_INVALID, "pfg_run_batch: NULL problems/results");
    if (B == 0) return PFG_OK;
    const int model = ps[0].model, kernel = ps[0].kernel, dtype = ps[0].dtype, rng = ps[0].rng;
    int rc = check_ids(ctx, ps[0].smoother, model, kernel, dtype, rng);
    for (int b = 0; b < B && !rc; ++b) rc = check_window(ctx, ps[b], rs[b], ps[0], b);
    if (rc) return rc;

    // ---- plan ---------------------------------------------------------------------------
    const BatchSummary sum = summarize(B, ps, rs);
    const bool predictive = ps[0].stat == PFG_STAT_PREDICTIVE;   // large-N kernel only (any N)
    LaunchPlan plan = make_plan(Caller::Batch, model, dtype, rng, sum.smoother, sum.n_max, B, sum.traced, predictive, sum.t_max);
    if (plan.rc && !plan.name) return fail(ctx, plan.rc, plan.err);
    if (plan.family == Family::Grid) {
        for (int b = 0; b < B; ++b) {
            const pfg_problem &q = ps[b];
            const std::string id = "problem " + std::to_string(b) + ": ";
            if (q.smoother != PFG_SMOOTHER_NEMETH && q.smoother != PFG_SMOOTHER_FILTER)
                return fail(ctx, PFG_ERR_UNSUPPORTED, id + "N > " + std::to_string(pfg::MEM_MAX_N) + " is built for pf = 'poyiadjis_N' | 'nemeth' | 'filter'");
            if (q.elementwise) return fail(ctx, PFG_ERR_UNSUPPORTED, id + "elementwise statistics are built for N <= " + std::to_string(pfg::MEM_MAX_N));
            if (pfg::grid_ppt(q.N) != pfg::grid_ppt(sum.n_max))
                return fail(ctx, PFG_ERR_INVALID, id + "whole-GPU windows of one batch must all have N <= 524288 or all N > 524288");
            // every window lays out its own scratch from its own N inside a stride sized from n_max: never launch one
            // that would not fit (the layout is monotone in N, so this only fails if that invariant is broken)
            const size_t need = with_types(model, dtype, rng, [&](auto m, auto, auto real, auto) {
                return pfg::grid_layout<decltype(m)::value, decltype(real)>(q.N, rng == PFG_RNG_REPLAY).bytes;
            });
            if (need > plan.scratch)
                return fail(ctx, PFG_ERR_INVALID, id + "whole-GPU layout of N = " + std::to_string(q.N) + " needs " + std::to_string(need) +
                                                      " scratch bytes, more than the " + std::to_string(plan.scratch) + " planned for n_max = " +
                                                      std::to_string(sum.n_max));
            plan.t_max = q.T > plan.t_max ? q.T : plan.t_max;
        }
    }
    // every window of the batch gets n_max-sized state (the predictive statistic's buffers after it)
    const size_t pred_each = predictive ? ((size_t)sum.n_max * PFG_MAX_PRED * (dtype == PFG_F64 ? 8 : 4) + 255) / 256 * 256 : 0;
    const size_t scratch_each = plan.scratch + pred_each, n_scratch = scratch_each * (size_t)B;

    // ---- describe, allocate -------------------------------------------------------------
    Layout L{ctx->pieces};
    std::vector<EwPlan> ew;
    try {
        ctx->h_desc.assign(B, pfg_dev_problem{});
        ctx->h_own.resize((size_t)B * kOwnDoubles);
        ctx->pieces.clear();
        ew.resize(B);
        for (int b = 0; b < B; ++b) describe_window(L, ps[b], rs[b], ctx->h_desc[b], ew[b], &ctx->h_own[(size_t)b * kOwnDoubles]);
    } catch (const std::bad_alloc &) {
        return fail(ctx, PFG_ERR_NOMEM, "pfg_run_batch: out of host memory");
    }
    const size_t n_in = L.n[Piece::In], n_out = L.n[Piece::Out], n_work = L.n[Piece::Work];
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    PFG_HIP(ctx, ctx->in.ensure(n_in * 8));
    PFG_HIP(ctx, ctx->out.ensure(n_out * 8));
    PFG_HIP(ctx, ctx->desc.ensure((size_t)B * sizeof(pfg_dev_problem)));
    if (n_scratch) PFG_HIP(ctx, ctx->scratch.ensure(n_scratch));
    if (n_work) PFG_HIP(ctx, ctx->work.ensure(n_work * 8));
    double *hin = nullptr;
    try {
        if (ctx->h_in.ensure(L.n_host) == hipSuccess) {
            hin = ctx->h_in.data();
        } else {
            // the runtime refuses to page-lock that much: stage from pageable memory (slower copies, same result)
            (void)hipGetLastError();
            ctx->h_in_pageable.resize(L.n_host);
            hin = ctx->h_in_pageable.data();
        }
        if (ctx->h_out.ensure(n_out) != hipSuccess) throw std::bad_alloc();
    } catch (const std::bad_alloc &) {
        return fail(ctx, PFG_ERR_NOMEM, "pfg_run_batch: out of host memory");
    }

    // ---- stage: point every descriptor at its buffers, pack the staged inputs --------------------------------------
    // `copies` = the H2D transfers: runs of packed pieces (contiguous on both sides) and the direct pieces
    char *const base[3] = {static_cast<char *>(ctx->in.ptr), static_cast<char *>(ctx->out.ptr), static_cast<char *>(ctx->work.ptr)};
    struct Copy { size_t at; const double *src; size_t n; bool packed; };
    std::vector<Copy> copies;
    size_t oh = 0;                      // offset into the host staging arena
    for (const Piece &p : ctx->pieces) {
        void *dev = base[p.arena] + p.at * 8;
        std::memcpy(p.slot, &dev, sizeof dev);
        if (p.copy == Piece::Direct) {
            copies.push_back({p.at, p.src, p.n, false});
        } else if (p.copy == Piece::Staged) {
            std::memcpy(hin + oh, p.src, p.n * 8);
            if (!copies.empty() && copies.back().packed && copies.back().src + copies.back().n == hin + oh && copies.back().at + copies.back().n == p.at)
                copies.back().n += p.n;                   // extends the current packed run
            else
                copies.push_back({p.at, hin + oh, p.n, true});
            oh += p.n;
        }
    }
    for (int b = 0; b < B; ++b) {
        pfg_dev_problem &d = ctx->h_desc[b];
        d.scratch = n_scratch ? static_cast<void *>(static_cast<char *>(ctx->scratch.ptr) + scratch_each * (size_t)b) : nullptr;
        if (predictive) d.pred_scratch = static_cast<char *>(d.scratch) + plan.scratch;
    }

    // ---- launch, elementwise pass, fetch ------------------------------------------------
    for (const Copy &cp : copies)
        PFG_HIP(ctx, hipMemcpyAsync(static_cast<double *>(ctx->in.ptr) + cp.at, cp.src, cp.n * 8, hipMemcpyHostToDevice, ctx->stream));
    PFG_HIP(ctx, hipMemcpyAsync(ctx->desc.ptr, ctx->h_desc.data(), (size_t)B * sizeof(pfg_dev_problem),
                                hipMemcpyHostToDevice, ctx->stream));
    PFG_HIP(ctx, hipMemsetAsync(ctx->out.ptr, 0, n_out * 8, ctx->stream));
    rc = launch(ctx, plan, model, kernel, rng, B, static_cast<const pfg_dev_problem *>(ctx->desc.ptr), ctx->stream);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        if (!ps[b].elementwise) continue;
        const pfg_dev_problem &d = ctx->h_desc[b];
        const EwPlan &e = ew[b];
        rc = elementwise_pass(ctx, ps[b], d.theta, d.trace_x, d.trace_logw, ps[b].smoother == PFG_SMOOTHER_PARIS ? d.trace_paris_J : d.trace_anc, e.Nt,
                              e.Wd, e.S0, e.S1, e.Sbar, e.w, e.mean, e.stats);
        if (rc) return rc;
    }
    PFG_HIP(ctx, hipMemcpyAsync(ctx->h_out.data(), ctx->out.ptr, n_out * 8, hipMemcpyDeviceToHost, ctx->stream));
    PFG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double *hout = ctx->h_out.data();
    for (const Piece &p : ctx->pieces)
        if (p.dst) std::memcpy(p.dst, hout + p.at, p.bytes);
    for (int b = 0; b < B; ++b) {       // the PaRIS stream counts: an int64 pair into two fields of the record
        const int64_t *pc = ctx->h_desc[b].paris_consumed;
        int64_t two[2] = {0, 0};
        if (pc) std::memcpy(two, hout + (reinterpret_cast<const double *>(pc) - static_cast<const double *>(ctx->out.ptr)), 16);
        rs[b].paris_consumed = two[0];
        rs[b].paris_carry_back = (int32_t)two[1];
        rs[b].status = PFG_OK;
    }
    return PFG_OK;
}

}  // extern "C"
