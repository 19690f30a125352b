// The launch planner of libpfgrad.so: which kernel runs a batch of windows (the variant tables, pick_plain, make_plan),
// its dispatch onto the instantiation units (pfg_inst_*.hip, pfg_kalman.hip, pfg_ffbs.hip), the size and name queries and
// the pfg_launch_device* entry points.  pfg_run_batch (pfgrad.hip) plans and launches through what pfg_host.hpp declares.
#include "pfg_host.hpp"
#include "pfg_device.hpp"

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
// the LDS-resident PaRIS and O(N^2) Poyiadjis variants (ping-pong state, the parents' log-weights in LDS), in the same
// order; paris64x2 / n2_64x2: one wave per window
struct ParisVariant { int NT, PPT; const char *tag; size_t (*lds)(int, int, int, int); };
const ParisVariant kParisVariants[] = { {64, 2, "paris64x2", reg_lds<64, 2, true, pfg::MODE_PARIS>},
                                        {256, 1, "paris256x1", reg_lds<256, 1, true, pfg::MODE_PARIS>},
                                        {256, 4, "paris256x4", reg_lds<256, 4, true, pfg::MODE_PARIS>} };
const ParisVariant kN2Variants[] = { {64, 2, "n2_64x2", reg_lds<64, 2, true, pfg::MODE_N2>},
                                     {256, 1, "n2_256x1", reg_lds<256, 1, true, pfg::MODE_N2>},
                                     {256, 4, "n2_256x4", reg_lds<256, 4, true, pfg::MODE_N2>} };
constexpr int kOneWaveSmoother = 0, kNumSmootherVariants = 3;
static_assert(sizeof(kParisVariants) == sizeof(kN2Variants) && sizeof(kN2Variants) / sizeof(kN2Variants[0]) == kNumSmootherVariants,
              "one table per smoother, the same shapes in the same order");

// The kernel of a plain batch (no PaRIS / systematic / stratified / O(N^2)) of `batch` windows of up to n_max particles: Reg with the
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

LaunchPlan refuse(LaunchPlan &p, int rc, std::string msg) {
    p.rc = rc;
    p.err = std::move(msg);
    return std::move(p);
}

template <int MODE>
size_t scheme_big_lds(int model, int dtype, int rng, int np2) {
    return with_types(model, dtype, rng, [&](auto, auto, auto real, auto) {
        return pfg::big_kernel_lds_bytes<decltype(real), MODE == pfg::MODE_STRATIFIED, MODE == pfg::MODE_ADAPTIVE>(np2);
    });
}
template <int MODE>
size_t scheme_unit_lds(int model, int dtype, int rng, int N) {
    return (dtype == PFG_F64 ? reg_lds<256, 4, false, MODE> : reg_lds<256, 4, true, MODE>)(model, dtype, rng, N);
}
const Scheme kSchemes[] = {
    // the resampling schemes other than multinomial, in the order of Resampling: the fields of Scheme (pfg_host.hpp).
    // (Systematic windows never ask for the predictive or elementwise statistics: check_window refuses both for the id.)
    {Family::Systematic, "systematic", pfg::MODE_SYSTEMATIC, 1024, "", true, false, false,
     "systematic256x4", nullptr, nullptr, nullptr, scheme_unit_lds<pfg::MODE_SYSTEMATIC>, scheme_big_lds<pfg::MODE_SYSTEMATIC>},
    {Family::Stratified, "stratified", pfg::MODE_STRATIFIED, pfg::MEM_MAX_N, "", false, true, false, "stratified256x4",
     "big4096_stratified", "big16384_stratified", "mem1024_stratified", scheme_unit_lds<pfg::MODE_STRATIFIED>, scheme_big_lds<pfg::MODE_STRATIFIED>},
    {Family::Adaptive, "adaptive", pfg::MODE_ADAPTIVE, pfg::MEM_MAX_N, " (no whole-GPU windows)", false, true, true, "adaptive256x4",
     "big4096_adaptive", "big16384_adaptive", "mem1024_adaptive", scheme_unit_lds<pfg::MODE_ADAPTIVE>, scheme_big_lds<pfg::MODE_ADAPTIVE>},
};

}  // namespace

namespace pfg_host {

const Scheme &scheme_of(Resampling r) { return kSchemes[(int)r - 1]; }

// Which kernel runs a batch of B windows of up to n_max particles, with what LDS and scratch, under which name.  smoother
// as the dispatcher receives it: PFG_SMOOTHER_POYIADJIS_N states that every window is (NEMETH, lambduh = 1, score) -- the
// same kernels as NEMETH, except where a unit has a twin specialised to that estimator.  traced: the descriptors may carry
// trace_* / rec_* buffers (the plain LDS-resident kernels exist as a production twin that ignores them, see
// pfg_reg_kernel.hpp; every other kernel always honours them).  predictive: the windows ask for the predictive statistic,
// which only the general large-N kernel computes.  elementwise: a window of the batch asks for elementwise statistics (the
// one-wave O(N^2) variant is not picked for those).  The environment variables PFGRAD_VARIANT, PFGRAD_NO_SCORE1 and
// PFGRAD_CDF_SINGLE are read here and nowhere else.
LaunchPlan make_plan(const PlanRequest &r) {
    const Caller caller = r.caller;
    const int model = r.model, dtype = r.dtype, rng = r.rng, smoother = r.smoother, n_max = r.n_max, B = r.B, t_max = r.t_max, phase = r.phase;
    const bool traced = r.traced, predictive = r.predictive, elementwise = r.elementwise;
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
    else if (r.resampling != Resampling::Multinomial) p.family = scheme_of(r.resampling).family;
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
            // One wave per window (64 threads x 2 particles, N <= 128; paris64x2 / n2_64x2): picked like wg64x2s for plain
            // windows -- device generator, more than kLatencyBatch windows; REPLAY, small batches and N > 128 keep the
            // 256-thread variants, and so do O(N^2) windows with elementwise statistics.
            // PFGRAD_VARIANT=<tag> forces any LDS-resident variant of the smoother that holds n_max (tests, A/B timing).
            const ParisVariant *const table = paris ? kParisVariants : kN2Variants, *pv = nullptr;
            for (int i = 0; i < kNumSmootherVariants; ++i)
                if (force && !std::strcmp(force, table[i].tag) && n_max <= table[i].NT * table[i].PPT) pv = &table[i];
            if (!pv && n_max <= 128 && rng == PFG_RNG_DEVICE && B > kLatencyBatch && (paris || !elementwise)) pv = &table[kOneWaveSmoother];
            if (!pv && n_max <= 1024) pv = &table[n_max <= 256 ? 1 : 2];
            if (pv) {
                p.nt = pv->NT; p.ppt = pv->PPT; p.name = pv->tag;
                p.lds = pv->lds(model, dtype, rng, n_max);
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
            // both instantiations honour trace_* buffers; the draws are written by the twin a traced launch runs
            p.record = traced && rng == PFG_RNG_DEVICE;
            break;
        }
        case Family::Systematic:
        case Family::Stratified:
        case Family::Adaptive: {
            // a row of kSchemes: up to three size classes, each a twin of the kernel that serves multinomial windows of
            // that size (256 x 4: single buffer in fp64, ping-pong in f32)
            const Scheme &s = scheme_of(r.resampling);
            const std::string what = std::string(s.what) + " resampling";
            if (predictive && s.no_predictive) return refuse(p, PFG_ERR_UNSUPPORTED, what + " is not built for the predictive statistic");
            if (elementwise && s.no_elementwise) return refuse(p, PFG_ERR_UNSUPPORTED, what + " is not built for elementwise statistics");
            // (a scheme that ends with the 256 x 4 unit names it in its refusals too: pfg_last_variant of a refused launch)
            const bool unit = n_max <= 1024 || s.n_limit <= 1024;
            if (unit) {
                p.name = s.unit;
                p.nt = 256; p.ppt = 4; p.pp = !p.f64;
            }
            if (s.device_only && rng != PFG_RNG_DEVICE) return refuse(p, PFG_ERR_UNSUPPORTED, what + " needs the DEVICE rng");
            if (n_max > s.n_limit) return refuse(p, PFG_ERR_UNSUPPORTED, what + " is built for N <= " + std::to_string(s.n_limit) + s.limit_note);
            if (unit) {
                p.lds = s.unit_lds(model, dtype, rng, n_max);
                if (p.lds > kLdsLimit) return refuse(p, PFG_ERR_UNSUPPORTED, what + ": state does not fit LDS");
                break;
            }
            p.nt = pfg::MEM_NT;
            p.scratch = mem_scratch(false);
            if (rng == PFG_RNG_DEVICE) {
                p.np2 = n_max <= 4096 ? 4096 : 16384;
                p.name = p.np2 == 4096 ? s.big4096 : s.big16384;
                p.lds = s.big_lds(model, dtype, rng, p.np2);
            } else {
                p.lw4 = n_max <= 4096;
                p.name = s.mem;
                p.lds = mem_lds();
            }
            break;
        }
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

// A whole-GPU batch of pfg_run_batch: the smoothers built for it, one tile class, every window's layout inside the stride
int check_grid_batch(pfg_ctx *ctx, LaunchPlan &plan, int B, const pfg_problem *ps) {
    const int model = ps[0].model, dtype = ps[0].dtype, rng = ps[0].rng;
    for (int b = 0; b < B; ++b) {
        const pfg_problem &q = ps[b];
        const std::string id = "problem " + std::to_string(b) + ": ";
        if (q.smoother != PFG_SMOOTHER_NEMETH && q.smoother != PFG_SMOOTHER_FILTER)
            return fail(ctx, PFG_ERR_UNSUPPORTED, id + "N > " + std::to_string(pfg::MEM_MAX_N) + " is built for pf = 'poyiadjis_N' | 'nemeth' | 'filter'");
        if (q.elementwise) return fail(ctx, PFG_ERR_UNSUPPORTED, id + "elementwise statistics are built for N <= " + std::to_string(pfg::MEM_MAX_N));
        if (pfg::grid_ppt(q.N) != pfg::grid_ppt(plan.n_max))
            return fail(ctx, PFG_ERR_INVALID, id + "whole-GPU windows of one batch must all have N <= 524288 or all N > 524288");
        // every window lays out its own scratch from its own N inside a stride sized from n_max: never launch one
        // that would not fit (the layout is monotone in N, so this only fails if that invariant is broken)
        const size_t need = with_types(model, dtype, rng, [&](auto m, auto, auto real, auto) {
            return pfg::grid_layout<decltype(m)::value, decltype(real)>(q.N, rng == PFG_RNG_REPLAY).bytes;
        });
        if (need > plan.scratch)
            return fail(ctx, PFG_ERR_INVALID, id + "whole-GPU layout of N = " + std::to_string(q.N) + " needs " + std::to_string(need) +
                                                  " scratch bytes, more than the " + std::to_string(plan.scratch) + " planned for n_max = " +
                                                  std::to_string(plan.n_max));
        plan.t_max = q.T > plan.t_max ? q.T : plan.t_max;
    }
    return PFG_OK;
}

}  // namespace pfg_host

namespace {

// what every pfg_launch_device* entry point (`fn`) checks first ...
int check_entry(pfg_ctx *ctx, const char *fn, int B, const pfg_dev_problem *dev_probs) {
    if (!ctx) return PFG_ERR_INVALID;
    if (!dev_probs && B > 0) return fail(ctx, PFG_ERR_INVALID, std::string(fn) + ": dev_probs is NULL");
    return PFG_OK;
}

// the request of a query (B: a large batch) or entry point that states `smoother` (no flag: see pfg_launch_device_adaptive);
// what else differs from a query's request is set by name
PlanRequest request(Caller caller, int model, int dtype, int rng, int smoother, int n_max, int B = 1 << 30) {
    PlanRequest r;
    r.caller = caller; r.model = model; r.dtype = dtype; r.rng = rng; r.n_max = n_max; r.B = B;
    r.smoother = smoother; r.resampling = resampling_of(smoother, 0);
    return r;
}

// ... and does once its own arguments are checked
int dispatch(pfg_ctx *ctx, const PlanRequest &r, int kernel, const pfg_dev_problem *dp, hipStream_t st) {
    PFG_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = check_ids(ctx, r.smoother, r.model, kernel, r.dtype, r.rng);
    if (rc) return rc;
    if (r.B <= 0) return PFG_OK;
    if (r.n_max < 1 && r.smoother != PFG_SMOOTHER_KALMAN) return fail(ctx, PFG_ERR_INVALID, "N must be >= 1");
    if (r.caller == Caller::Grid && r.t_max < 0) return fail(ctx, PFG_ERR_INVALID, "T_max must be >= 0");
    return launch(ctx, make_plan(r), r.model, kernel, r.rng, r.B, dp, st);
}

}  // namespace

extern "C" {

// both for a large batch of plain windows: never the latency variant or a twin
int64_t pfg_scratch_bytes(int model, int dtype, int rng, int N) {
    if (model < 0 || model > 2 || N < 1) return -1;
    const LaunchPlan p = make_plan(request(Caller::Query, model, dtype, rng, PFG_SMOOTHER_NEMETH, N));
    return p.name ? (int64_t)p.scratch : -1;
}

int64_t pfg_scratch_bytes_smoother(int model, int dtype, int rng, int smoother, int N) {
    if (model < 0 || model > 2 || N < 1 || !launch_smoother_id(smoother, false)) return -1;
    const LaunchPlan p = make_plan(request(Caller::Device, model, dtype, rng, smoother, N));
    return p.rc || !p.name ? -1 : (int64_t)p.scratch;
}

const char *pfg_variant_name(int model, int kernel, int dtype, int rng, int n_max) {
    (void)kernel;
    const LaunchPlan p = make_plan(request(Caller::Query, model, dtype, rng, PFG_SMOOTHER_NEMETH, n_max));
    return p.name ? p.name : "none";
}

int pfg_launch_device(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int B,
                      const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (const int rc = check_entry(ctx, __func__, B, dev_probs)) return rc;
    return dispatch(ctx, request(Caller::Device, model, dtype, rng, PFG_SMOOTHER_NEMETH, n_max, B), kernel, dev_probs, (hipStream_t)hip_stream);
}

int pfg_launch_device_traced(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother, int n_max, int B,
                             const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (const int rc = check_entry(ctx, __func__, B, dev_probs)) return rc;
    if (!launch_smoother_id(smoother, false)) return fail(ctx, PFG_ERR_INVALID, "Unrecognized pf (smoother id)");
    PlanRequest r = request(Caller::Device, model, dtype, rng, smoother, n_max, B);
    r.traced = true;
    return dispatch(ctx, r, kernel, dev_probs, (hipStream_t)hip_stream);
}

int pfg_launch_device_smoother(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother, int n_max,
                               int B, const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (const int rc = check_entry(ctx, __func__, B, dev_probs)) return rc;
    if (!launch_smoother_id(smoother, true)) return fail(ctx, PFG_ERR_INVALID, "Unrecognized pf (smoother id)");
    return dispatch(ctx, request(Caller::Device, model, dtype, rng, smoother, n_max, B), kernel, dev_probs, (hipStream_t)hip_stream);
}

// NEMETH windows whose descriptors carry PFG_FLAG_ADAPTIVE_RESAMPLING: the launch states the scheme
int pfg_launch_device_adaptive(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int B,
                               const pfg_dev_problem *dev_probs, void *hip_stream, int traced) {
    if (const int rc = check_entry(ctx, __func__, B, dev_probs)) return rc;
    PlanRequest r = request(Caller::Device, model, dtype, rng, PFG_SMOOTHER_NEMETH, n_max, B);
    r.resampling = Resampling::Adaptive; r.traced = traced != 0;
    return dispatch(ctx, r, kernel, dev_probs, (hipStream_t)hip_stream);
}

int pfg_launch_device_grid(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int T_max, int B,
                           const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (const int rc = check_entry(ctx, __func__, B, dev_probs)) return rc;
    PlanRequest r = request(Caller::Grid, model, dtype, rng, PFG_SMOOTHER_NEMETH, n_max, B);
    r.traced = true; r.t_max = T_max;
    return dispatch(ctx, r, kernel, dev_probs, (hipStream_t)hip_stream);
}

int pfg_launch_device_grid_smoother(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother, int n_max, int T_max,
                                    int phase, int B, const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (const int rc = check_entry(ctx, __func__, B, dev_probs)) return rc;
    if (smoother != PFG_SMOOTHER_NEMETH && smoother != PFG_SMOOTHER_FILTER && smoother != PFG_SMOOTHER_POYIADJIS_N)
        return fail(ctx, PFG_ERR_UNSUPPORTED, "whole-GPU windows are built for NEMETH / FILTER / POYIADJIS_N");
    if (phase < PFG_GRID_PHASE_FINISH) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid_smoother: phase must be PFG_GRID_PHASE_ALL, a timestep >= 0, PFG_GRID_PHASE_INIT or PFG_GRID_PHASE_FINISH");
    PlanRequest r = request(Caller::Grid, model, dtype, rng, smoother, n_max, B);
    r.traced = true; r.t_max = phase == PFG_GRID_PHASE_ALL ? T_max : 0; r.phase = phase;
    return dispatch(ctx, r, kernel, dev_probs, (hipStream_t)hip_stream);
}

int pfg_launch_device_grid_phase(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int phase, int B,
                                 const pfg_dev_problem *dev_probs, void *hip_stream) {
    if (const int rc = check_entry(ctx, __func__, B, dev_probs)) return rc;
    if (phase < PFG_GRID_PHASE_FINISH) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid_phase: phase must be a timestep >= 0, PFG_GRID_PHASE_INIT or PFG_GRID_PHASE_FINISH");
    if (phase == -1) return fail(ctx, PFG_ERR_INVALID, "pfg_launch_device_grid_phase: use pfg_launch_device_grid for the whole window");
    PlanRequest r = request(Caller::Grid, model, dtype, rng, PFG_SMOOTHER_NEMETH, n_max, B);
    r.traced = true; r.phase = phase;
    return dispatch(ctx, r, kernel, dev_probs, (hipStream_t)hip_stream);
}

}  // extern "C"
