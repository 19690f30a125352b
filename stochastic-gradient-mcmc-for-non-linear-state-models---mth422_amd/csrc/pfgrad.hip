// libpfgrad.so: host side of the C ABI declared in include/pfgrad.h -- the context and registration calls and
// pfg_run / pfg_run_batch (host buffers).  pfg_run_batch checks every window, plans the launch (pfg_plan.hip), then
// describes each window's buffers once (describe_window): sizing the arenas, staging the inputs and fetching the outputs
// are loops over those descriptions.  No kernel lives here: see pfg_inst_*.hip (particle filters), pfg_chains.hip,
// pfg_windows.hip, pfg_elementwise.hip and pfg_ksd.hip.
#include <mutex>
#include "pfg_host.hpp"
#include "pfg_device.hpp"

using namespace pfg_host;

namespace {

int stat_dim(int model) { return model == PFG_MODEL_SVM ? 3 : 4; }
int theta_dim(int model) { return model == PFG_MODEL_SVM ? 3 : 4; }

// ---- caller-registered pinned host ranges (pfg_host_register) -------------------------------------
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
    // what a resampling scheme refuses, from its row of kSchemes (pfg_plan.hip); the recursions a scheme has no kernel for
    // are named (its id or flag says NEMETH)
    const Scheme &systematic = scheme_of(Resampling::Systematic), &stratified = scheme_of(Resampling::Stratified);
    auto unbuilt = [&](const Scheme &s, const std::string &rest) { return fail(ctx, PFG_ERR_UNSUPPORTED, id + s.what + " resampling " + rest); };
    auto above = [](const Scheme &s) { return "is built for N <= " + std::to_string(s.n_limit) + s.limit_note; };
    auto not_nemeth = [&](const Scheme &s, int smoother) -> int {
        const char *pf = smoother == PFG_SMOOTHER_FILTER ? "filter" : smoother == PFG_SMOOTHER_PARIS ? "paris"
                         : smoother == PFG_SMOOTHER_POYIADJIS_N2 ? "poyiadjis_N2" : nullptr;
        return pf ? unbuilt(s, std::string("is built for the NEMETH recursion, not pf = '") + pf + "'") : PFG_OK;
    };
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
        q.smoother != PFG_SMOOTHER_KALMAN_FFBS && q.smoother != PFG_SMOOTHER_NEMETH_STRATIFIED)
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
            r.rec_u || r.rec_z || r.rec_z0 || r.rec_ud || r.ew_mean || r.ew_stats || r.trace_paris_J)
            return bad(PFG_ERR_INVALID, ffbs ? "FFBS latent paths have no particles: only the result record and trace_x (the paths)"
                                             : "the exact Kalman score has no particles: only the result record");
        if (ffbs && rng == PFG_RNG_REPLAY && q.T > 0 && !q.z) return bad(PFG_ERR_INVALID, "REPLAY FFBS needs z (T N normals)");
        if (ffbs && q.stat == PFG_STAT_GIBBS && q.N != 1)
            return bad(PFG_ERR_INVALID, "the Gibbs statistic (PFG_STAT_GIBBS) is of one path: N must be 1");
    }
    // adaptive (ESS-triggered) resampling: the flag fills a batch or is absent from it; what it is not built for is named
    const bool adaptive = (q.flags & PFG_FLAG_ADAPTIVE_RESAMPLING) != 0;
    if (adaptive != ((first.flags & PFG_FLAG_ADAPTIVE_RESAMPLING) != 0))
        return bad(PFG_ERR_INVALID, "adaptive resampling (PFG_FLAG_ADAPTIVE_RESAMPLING) cannot share a batch with windows that resample at every step");
    if (adaptive) {
        const Scheme &s = scheme_of(Resampling::Adaptive);
        if (const int rc = not_nemeth(s, q.smoother)) return rc;
        if (q.smoother == PFG_SMOOTHER_NEMETH_SYSTEMATIC || q.smoother == PFG_SMOOTHER_NEMETH_STRATIFIED)
            return bad(PFG_ERR_UNSUPPORTED, "adaptive resampling is built for multinomial draws, not systematic or stratified ones");
        if (q.smoother != PFG_SMOOTHER_NEMETH) return bad(PFG_ERR_INVALID, "adaptive resampling needs a particle filter (smoother NEMETH)");
        if (s.no_predictive && q.stat == PFG_STAT_PREDICTIVE) return unbuilt(s, "is not built for the predictive statistic");
        if (s.no_elementwise && q.elementwise) return unbuilt(s, "is not built for elementwise statistics");
        if (q.N > s.n_limit) return unbuilt(s, above(s));
        const float tau = pfg::ess_threshold_of(q.reserved);
        if (!(tau > 0.0f && tau <= 1.0f)) return bad(PFG_ERR_INVALID, "ess_threshold must be in (0, 1]");
    }
    if (mixed(PFG_SMOOTHER_NEMETH_STRATIFIED)) {
        // the id says NEMETH: the recursions it has no kernel for are named, any other mix is a caller's error
        if (const int rc = not_nemeth(stratified, q.smoother == PFG_SMOOTHER_NEMETH_STRATIFIED ? first.smoother : q.smoother)) return rc;
        return bad(PFG_ERR_INVALID, "stratified resampling cannot share a batch with other smoothers");
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
    if (q.smoother == PFG_SMOOTHER_NEMETH_STRATIFIED && stratified.no_predictive && q.stat == PFG_STAT_PREDICTIVE)
        return unbuilt(stratified, "is not built for the predictive statistic");
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
    if (q.smoother == PFG_SMOOTHER_NEMETH_SYSTEMATIC && (rng != PFG_RNG_DEVICE || q.N > systematic.n_limit))
        return unbuilt(systematic, "needs the DEVICE rng and N <= " + std::to_string(systematic.n_limit));
    if (q.smoother == PFG_SMOOTHER_NEMETH_STRATIFIED && q.N > stratified.n_limit) return unbuilt(stratified, above(stratified));
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
        if (r.trace_x || r.trace_logw || r.trace_stats || r.trace_anc || r.rec_u || r.rec_z || r.rec_z0 || r.rec_ud || r.trace_paris_J)
            return bad(PFG_ERR_INVALID, "elementwise statistics cannot be combined with trace outputs");
        if ((q.tL < q.T ? q.tL : q.T) - q.t1 < 1) return bad(PFG_ERR_INVALID, "elementwise needs a non-empty window [t1, tL)");
    } else if (r.ew_mean || r.ew_stats) {
        return bad(PFG_ERR_INVALID, "ew_mean / ew_stats need pfg_problem.elementwise");
    }
    if ((r.rec_u || r.rec_z || r.rec_z0 || r.rec_ud) && (rng != PFG_RNG_DEVICE || !r.trace_x))
        return bad(PFG_ERR_INVALID, "rec_u / rec_z / rec_z0 record the DEVICE generator's draws and need trace_x");
    if (r.trace_anc && !r.trace_x) return bad(PFG_ERR_INVALID, "trace_anc needs trace_x");
    if (r.trace_paris_J && (!r.trace_x || q.smoother != PFG_SMOOTHER_PARIS))
        return bad(PFG_ERR_INVALID, "trace_paris_J needs trace_x and pf = 'paris'");
    if ((r.logw_T || r.stats_T) && !r.x_T) return bad(PFG_ERR_INVALID, "logw_T/stats_T need x_T");
    if (!ffbs && (r.trace_logw == nullptr) != (r.trace_x == nullptr)) return bad(PFG_ERR_INVALID, "trace_x and trace_logw go together");
    if (r.trace_stats && !r.trace_x) return bad(PFG_ERR_INVALID, "trace_stats needs trace_x");
    return PFG_OK;
}

// What the plan needs of a valid batch: the longest window (Kalman: of steps [t1, tL), else of particles), the longest
// FFBS buffer, whether any window records a trajectory or asks for elementwise statistics, and the smoother and
// resampling scheme to plan for.
PlanRequest summarize(int B, const pfg_problem *ps, const pfg_result *rs) {
    PlanRequest s;
    s.caller = Caller::Batch; s.model = ps[0].model; s.dtype = ps[0].dtype; s.rng = ps[0].rng; s.B = B;
    s.predictive = ps[0].stat == PFG_STAT_PREDICTIVE;   // large-N kernel only (any N)
    bool score1 = true;         // every window the Poyiadjis O(N) score: units with a twin specialised to it run that
    for (int b = 0; b < B; ++b) {
        const pfg_problem &q = ps[b];
        const pfg_result &r = rs[b];
        s.traced = s.traced || r.trace_x || r.trace_ll || r.rec_u || r.rec_z || r.rec_z0 || r.rec_ud || q.elementwise;
        s.elementwise = s.elementwise || q.elementwise;
        score1 = score1 && q.smoother == PFG_SMOOTHER_NEMETH && q.lambduh == 1.0 && q.stat == PFG_STAT_SCORE;
        const int n = q.smoother == PFG_SMOOTHER_KALMAN ? (q.tL < q.T ? q.tL : q.T) - q.t1 : q.N;
        s.n_max = n > s.n_max ? n : s.n_max;
        if (q.smoother == PFG_SMOOTHER_KALMAN_FFBS) s.t_max = q.T > s.t_max ? q.T : s.t_max;
    }
    // the smoothers with kernels of their own fill whole batches; the rest run the plain kernels
    const int s0 = ps[0].smoother;
    s.resampling = resampling_of(s0, ps[0].flags);
    if (s.resampling != Resampling::Multinomial || s0 == PFG_SMOOTHER_PARIS || s0 == PFG_SMOOTHER_POYIADJIS_N2 ||
        s0 == PFG_SMOOTHER_KALMAN || s0 == PFG_SMOOTHER_KALMAN_FFBS)     // (adaptive: NEMETH windows, checked)
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
    if (paris) L.want(r.trace_paris_J, d.trace_paris_J, (TN * q.Ntilde + 1) / 2, TN * q.Ntilde * 4);     // packed int32 likewise
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
    d.reserved = (q.flags & PFG_FLAG_ADAPTIVE_RESAMPLING) ? q.reserved : 0;      // the threshold's bits
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
        case 4: return (int)sizeof(pfg_csmc_problem);
        case 5: return (int)sizeof(pfg_cpm_problem);
        case 6: return (int)sizeof(pfg_sqmc_problem);
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
    const PlanRequest sum = summarize(B, ps, rs);
    const bool predictive = sum.predictive;
    LaunchPlan plan = make_plan(sum);
    if (plan.rc && !plan.name) return fail(ctx, plan.rc, plan.err);
    if (plan.family == Family::Grid && (rc = check_grid_batch(ctx, plan, B, ps))) return rc;
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
    for (int b = 0; b < B && !rc; ++b)
        if (ps[b].elementwise) rc = elementwise_pass(ctx, ps[b], ctx->h_desc[b], ew[b]);
    if (rc) return rc;
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
