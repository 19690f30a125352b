// Host-side declarations shared by the translation units of libpfgrad.so: the context, error plumbing, the launch plan
// with what pfg_run_batch needs of the planner and the elementwise pass, and the per-(model, proposal kernel, generator)
// launch entry the ten instantiation units (pfg_inst_*.hip) define: those units compile in parallel.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "pfgrad.h"

namespace pfg_host {

inline thread_local std::string g_create_error;

struct Arena {           // growable device buffer
    void *ptr = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr; cap = 0;
        size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; cap = 0; }
};

struct HostArena {       // growable PINNED host buffer (hipHostMalloc): H2D / D2H copies from it are truly
    double *ptr = nullptr;   // asynchronous and run at link speed; a pageable std::vector is staged by the runtime
    size_t cap = 0;          // in doubles
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr; cap = 0;
        const size_t want = n + n / 4 + 512;
        void *p = nullptr;
        hipError_t e = hipHostMalloc(&p, want * sizeof(double), hipHostMallocDefault);
        if (e == hipSuccess) { ptr = static_cast<double *>(p); cap = want; }
        return e;
    }
    double *data() { return ptr; }
    double &operator[](size_t i) { return ptr[i]; }
    void release() { if (ptr) (void)hipHostFree(ptr); ptr = nullptr; cap = 0; }
};

// One buffer of a pfg_run_batch window (pfgrad.hip, describe_window): the arena it lives in, its offset and length
// there, what crosses between it and the host, and the descriptor field set to its device address once the arena
// bases are known.
struct Piece {
    enum Arena : uint8_t { In, Out, Work };
    enum Copy : uint8_t { None, Staged, Direct };   // In: packed into the staging arena, or DMA'd from registered pages
    void *slot;              // address of the device pointer to set (a pfg_dev_problem or elementwise-pass field)
    const double *src;       // In: the host source
    void *dst;               // Out: where the host result goes (NULL: read back elsewhere)
    size_t at, n;            // offset and length in the arena, doubles
    size_t bytes;            // Out: bytes fetched into dst (an int32 payload fills fewer than n * 8)
    Arena arena;
    Copy copy;
};

}  // namespace pfg_host

struct pfg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    pfg_host::Arena in, out, desc, scratch, work;      // work: device-only buffers (elementwise-statistics pass)
    pfg_host::HostArena h_in, h_out;
    std::vector<double> h_in_pageable;   // staging when the pinned arena cannot be had (hipHostMalloc refused)
    std::vector<pfg_dev_problem> h_desc;
    std::vector<pfg_host::Piece> pieces;  // pfg_run_batch: every buffer of the batch
    std::vector<double> h_own;           // pfg_run_batch: per window, theta padded to PFG_MAX_THETA and the step counter
    const char *last_variant = "none";   // tag of the kernel variant the latest dispatch launched
    bool last_traced = false;            // ... and whether that was a trace-honouring instantiation
    // largest dynamic-LDS size hipFuncAttributeMaxDynamicSharedMemorySize has been set to, per kernel: the
    // attribute is per (function, device) and a context is bound to one device
    std::unordered_map<const void *, size_t> lds_set;
};

namespace pfg_host {

inline int fail(pfg_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

#define PFG_HIP(ctx, call)                                                            \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess)                                                         \
            return fail(ctx, e_ == hipErrorOutOfMemory ? PFG_ERR_NOMEM : PFG_ERR_DEVICE, \
                        std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)

constexpr size_t kLdsLimit = 160 * 1024;

// What runs a batch: filled by make_plan (pfg_plan.hip), the one place where a kernel is chosen; launch_mkr only maps it
// onto an instantiation.
enum class Family {
    None,
    Reg,           // LDS-resident kernel, entry (nt, ppt, pp)
    Paris, N2,     // its PaRIS / O(N^2) Poyiadjis instantiations, 256 x ppt or one wave (64 x 2); nt = MEM_NT: the large-N kernel's PaRIS one
    Systematic, Stratified, Adaptive,  // the twins of a resampling scheme other than multinomial (Scheme below, one row of
                   // kSchemes in pfg_plan.hip each), in up to three size classes: the LDS-resident 256 x 4 instantiation
                   // (n_max <= 1024; np2 = 0), above it the large-N kernel's twin (REPLAY; lw4: N <= 4096) or the fast
                   // large-N kernel's twin (device generator, np2 slots)
    Mem,           // large-N kernel (state in an HBM scratch); lw4: N <= 4096, log-weights in registers
    Big,           // large-N kernel, device-generator fast path for np2 particle slots
    Grid,          // whole-GPU window above the one-workgroup kernels' maximum (pfg_grid_kernel.hpp), tile class (ppt, kmax)
    Kalman,        // exact Kalman score of LGSSM windows (PFG_SMOOTHER_KALMAN, pfg_kalman.hip): one lane per window
    KalmanFfbs,    // FFBS paths and complete-data score of LGSSM windows (PFG_SMOOTHER_KALMAN_FFBS, pfg_ffbs.hip): one
                   // workgroup of nt lanes per window, one lane per path
};

struct LaunchPlan {
    Family family = Family::None;
    bool f64 = true;
    int n_max = 0;
    int nt = 0, ppt = 0;
    bool pp = true;
    bool traced = true;          // the TRACE instantiation (pfg_last_traced)
    bool score1 = false;         // the score-only twin (PFG_SMOOTHER_POYIADJIS_N, see SCORE1 in pfg_reg_kernel.hpp)
    bool lw4 = false;
    bool record = false;         // Paris / N2 on the large-N kernel, device generator: the twin that writes rec_z0 / rec_z / rec_ud
    int np2 = 0;                 // Big
    int kmax = 0, tiles = 0, t_max = 0, phase = -1;   // Grid
    bool cdf_single = false;     // Grid, REPLAY: the lone-workgroup CDF kernel
    size_t lds = 0;              // dynamic LDS of the kernel (Grid: of its timestep kernel)
    size_t scratch = 0;          // per-window HBM scratch, bytes (0: none; Kalman: from the longest window, n_max;
                                 // KalmanFfbs: from the longest buffer, t_max)
    const char *name = nullptr;  // pfg_last_variant once the kernel is chosen
    int rc = PFG_OK;             // an error found once the kernel is chosen (name set) or before (name NULL)
    std::string err;
};

// The LDS-resident (nt, ppt, pp) entries built for a unit, and those with a score-only twin.  (Twins measured per unit,
// whole library built with -DPFG_EXP_PLAIN=1 -- device generator: 1024 x 4 -4.7 %, one wave x 2 -2.8 %, 256 x 4 -0.6 %,
// 512 x 2 +2.1 %, large-N kernel 0; REPLAY arithmetic legs: SVM 256 x 4 -5.8 %, LGSSM one wave -6.5 %, GARCH 256 x 4
// +8 %: profiles/r04_ab_score1_twin.txt; the 1024 x 1 latency variant, one window alone, SVM T = N = 1000: device
// 1.957 -> 1.814 ms, REPLAY 2.768 -> 2.623.)
constexpr bool reg_entry_built(int model, int rng, bool f64, int nt, int ppt, bool pp) {
    if ((nt == 256 && (ppt == 1 ? pp : ppt == 4)) || (pp && ((nt == 1024 && ppt == 1) || (nt == 64 && ppt == 2)))) return true;
    if (rng != PFG_RNG_DEVICE) return false;
    if (nt == 512) return ppt == 2 && !pp && model == PFG_MODEL_GARCH && f64;
    return (nt == 1024 && ppt == 4 && !pp) || (nt == 64 && (ppt == 4 || ppt == 2));
}
constexpr bool reg_score1_twin(int model, int rng, bool f64, int nt, int ppt, bool pp) {
    const bool lat = model != PFG_MODEL_GARCH && nt == 1024 && ppt == 1 && pp;
    const bool dev = rng == PFG_RNG_DEVICE && !pp && ((nt == 1024 && ppt == 4) || (nt == 64 && ppt == 2));
    const bool rep = rng == PFG_RNG_REPLAY && model != PFG_MODEL_GARCH && ((nt == 256 && ppt == 4) || (nt == 64 && ppt == 2));
    return f64 && (lat || dev || rep);
}

// Launch of the planned kernel of one (model, proposal kernel, generator): defined (and explicitly instantiated) in
// pfg_inst_*.hip via pfg_launch.hpp, declared here for the dispatcher in pfg_plan.hip.
template <int MODEL, int KERNEL, int RNG>
int launch_mkr(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st);

// Launch of the Kalman window kernel (Family::Kalman), defined in pfg_kalman.hip.
int launch_kalman(pfg_ctx *ctx, const LaunchPlan &p, int B, const pfg_dev_problem *dp, hipStream_t st);

// Launch of the FFBS window kernel (Family::KalmanFfbs), defined in pfg_ffbs.hip.
int launch_ffbs(pfg_ctx *ctx, const LaunchPlan &p, int rng, int B, const pfg_dev_problem *dp, hipStream_t st);

// ---- pfg_plan.hip.  Who asks for a plan: the queries pfg_variant_name / pfg_scratch_bytes (a large batch of plain windows), pfg_run_batch
// (N above the one-workgroup kernels, or PFGRAD_VARIANT=grid, runs as whole-GPU windows), pfg_launch_device* (one-workgroup
// kernels only) and pfg_launch_device_grid* (whole-GPU windows).
enum class Caller { Query, Batch, Device, Grid };
// How the windows of a batch resample, as their descriptors (or the launch) state it: a smoother id of its own
// (systematic, stratified) or NEMETH windows that carry PFG_FLAG_ADAPTIVE_RESAMPLING.  A scheme fills a batch.
enum class Resampling { Multinomial, Systematic, Stratified, Adaptive };
inline Resampling resampling_of(int smoother, uint32_t flags) {
    if (flags & PFG_FLAG_ADAPTIVE_RESAMPLING) return Resampling::Adaptive;
    return smoother == PFG_SMOOTHER_NEMETH_SYSTEMATIC ? Resampling::Systematic
           : smoother == PFG_SMOOTHER_NEMETH_STRATIFIED ? Resampling::Stratified : Resampling::Multinomial;
}
// What is built for a scheme other than multinomial: one row of kSchemes (pfg_plan.hip), read by make_plan and by
// pfg_run_batch's check_window.  Every scheme is a twin of the NEMETH kernels; a scheme whose n_limit is 1024 has the
// 256 x 4 unit alone.
struct Scheme {
    Family family;
    const char *what;                   // its name in messages
    int mode;                           // pfg::MODE_*
    int n_limit;                        // its largest N
    const char *limit_note;             // ... and what the refusal above it adds
    bool device_only;                   // no REPLAY stream to run it from
    bool no_predictive, no_elementwise; // refuses the predictive statistic / elementwise statistics
    const char *unit, *big4096, *big16384, *mem;                    // the variant names of its size classes
    size_t (*unit_lds)(int model, int dtype, int rng, int N);       // 256 x 4: single buffer in fp64, ping-pong in f32
    size_t (*big_lds)(int model, int dtype, int rng, int np2);
};
const Scheme &scheme_of(Resampling r);  // r != Multinomial
// a smoother id that a launch may state: those of the particle filters, and (kalman) PFG_SMOOTHER_KALMAN / KALMAN_FFBS
constexpr bool launch_smoother_id(int smoother, bool kalman) {
    return smoother >= PFG_SMOOTHER_NEMETH && (smoother <= (kalman ? PFG_SMOOTHER_KALMAN_FFBS : PFG_SMOOTHER_POYIADJIS_N) ||
                                               smoother == PFG_SMOOTHER_NEMETH_STRATIFIED);
}

// What make_plan is asked: smoother as the dispatcher receives it (PFG_SMOOTHER_POYIADJIS_N states that every window is
// (NEMETH, lambduh = 1, score)), the scheme beside it; B windows of up to n_max particles.
struct PlanRequest {
    Caller caller = Caller::Query;
    int model = 0, dtype = PFG_F64, rng = PFG_RNG_REPLAY;
    int smoother = PFG_SMOOTHER_NEMETH;
    Resampling resampling = Resampling::Multinomial;
    int n_max = 0;
    int B = 1 << 30;            // (a query: a large batch, never the latency variant)
    bool traced = false;        // the descriptors may carry trace_* / rec_* buffers
    bool predictive = false;    // the windows ask for the predictive statistic
    int t_max = 0, phase = -1;  // KalmanFfbs: the longest buffer; Grid: the longest window and the phase to launch
    bool elementwise = false;   // a window of the batch asks for elementwise statistics
};
LaunchPlan make_plan(const PlanRequest &r);
int check_ids(pfg_ctx *ctx, int smoother, int model, int kernel, int dtype, int rng);
int launch(pfg_ctx *ctx, const LaunchPlan &p, int model, int kernel, int rng, int B, const pfg_dev_problem *dp, hipStream_t st);
// pfg_run_batch, Family::Grid: what every window of a whole-GPU batch must satisfy; plan.t_max becomes the longest T
int check_grid_batch(pfg_ctx *ctx, LaunchPlan &plan, int B, const pfg_problem *ps);
inline int state_dim(int model) { return model == PFG_MODEL_GARCH ? 2 : 1; }

// ---- pfg_elementwise.hip.  The pass's device-only statistic matrices (its traces are the descriptor's trace_x /
// trace_logw and trace_anc or trace_paris_J, redirected into the work arena)
struct EwPlan { double *S0, *S1, *Sbar, *w, *mean, *stats; size_t Wd; int Nt; };
// the second pass over the trajectory that window q recorded through its descriptor d (host copy), on ctx->stream
int elementwise_pass(pfg_ctx *ctx, const pfg_problem &q, const pfg_dev_problem &d, const EwPlan &e);

}  // namespace pfg_host
