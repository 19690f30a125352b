/*
 * pfgrad.h -- C ABI of libpfgrad.so: the buffered particle-filter score / log-likelihood
 * estimator of sgmcmc_ssm, implemented as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference is pure Python and has no FFI; this ABI is what a ctypes binding on the
 * reference side would bind in place of the call
 *     buffered_pf_wrapper(pf=..., observations=..., parameters=..., N=..., kernel=...,
 *                         additive_statistic_func=..., t1=..., tL=..., weights=...,
 *                         prior_mean=..., prior_var=...)
 * (sgmcmc_ssm/particle_filters/buffered_smoother.py:156-199, loop :12-149) as issued by
 * Helper.pf_gradient_estimate / pf_loglikelihood_estimate
 * (models/svm/helper.py:67-185, models/garch/helper.py:59-170, models/lgssm/helper.py:1016-1143).
 * Python callables (Kernel objects, additive_statistic_func) cannot cross to the device,
 * so (Kernel, statistic) pairs are replaced by enumerated ids.  See INTEGRATION.md for the
 * reference-side ctypes stub.
 *
 * Conventions: plain C, no torch types.  Every function returns 0 on success or a negative
 * pfg_status code and never throws; the message is available from pfg_last_error().
 * A pfg_ctx is not thread-safe (one per host thread / process).  Host pointers are owned by
 * the caller and must stay valid for the duration of the call; device memory allocated by
 * the library is owned by the pfg_ctx.
 */
#ifndef PFGRAD_H
#define PFGRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFG_VERSION 126          /* 0.1.26 */
#define PFG_MAX_STAT 4           /* widest additive statistic (GARCH / LGSSM score) */
#define PFG_MAX_THETA 4          /* raw parameters per model */
#define PFG_OUT_DOUBLES 8        /* doubles in one result record (see pfg_dev_problem.out) */
#define PFG_STAMP_WORDS 16       /* uint64 words behind pfg_dev_problem.stamps */
#define PFG_MAX_PRED 16          /* predictive log-likelihood leads k = 0..num_steps_ahead (<= 15) */

typedef struct pfg_ctx pfg_ctx;

/* models: theta layout = Parameters.var_dict order of the reference
 *   SVM   [A, LQinv, LRinv]                       models/svm/parameters.py:21-25
 *   GARCH [log_mu, logit_phi, logit_lambduh, LRinv] models/garch/parameters.py:19-22
 *   LGSSM [A, C, LQinv, LRinv]                    models/lgssm/parameters.py:20-25
 * score statistic column order (what pf_gradient_estimate unpacks):
 *   SVM   [LRinv, LQinv, A]                       models/svm/helper.py:121-126
 *   GARCH [LRinv, log_mu, logit_phi, logit_lambduh] models/garch/helper.py:109-115
 *   LGSSM [LRinv, LQinv, C, A]                    models/lgssm/helper.py:1136-1142        */
enum pfg_model { PFG_MODEL_SVM = 0, PFG_MODEL_GARCH = 1, PFG_MODEL_LGSSM = 2 };
/* proposal kernels: models/{svm,garch,lgssm}/kernels.py ("prior" bootstrap, "optimal") */
enum pfg_kernel { PFG_KERNEL_PRIOR = 0, PFG_KERNEL_OPTIMAL = 1 };
/* smoothers: particle_filters/pf.py:138-181 (nemeth; poyiadjis_N = lambduh 1.0), :40-82 (filter),
 * :183-341 (PaRIS: Ntilde backward-sampled parents per child by accept-reject, exact
 * categorical fallback after max_accept_reject rounds; N <= 1024 LDS-resident, up to 16384 in
 * the large-N kernel through pfg_run / pfg_run_batch, which size its scratch) */
enum pfg_smoother { PFG_SMOOTHER_NEMETH = 0, PFG_SMOOTHER_FILTER = 1, PFG_SMOOTHER_PARIS = 2,
                    /* EXTENSION (not in the reference, which resamples multinomially every step,
                     * pf.py:26-30): NEMETH with systematic resampling, u_i = (i + u0)/N with ONE
                     * uniform u0 per timestep (the next word of lane 0's keyed generator).  DEVICE rng, N <= 1024.
                     * No REPLAY stream (the reference has no such resampler); a traced launch records the uniform of
                     * every child in rec_ud, from which the oracle replays the search and the whole recursion.
                     * Its own kernel instantiation (keeps the hot path untouched). */
                    PFG_SMOOTHER_NEMETH_SYSTEMATIC = 3,
                    /* poyiadjis_smoother, the O(N^2) algorithm (pf.py:84-136): every child averages
                     * stats_j + w_t h(x_j, child) over ALL parents j with the backward weights
                     * w_j q(child | x_j), normalised per child.  N <= 1024 LDS-resident -- "n2_64x2" (one wave per
                     * window, N <= 128), "n2_256x1" (N <= 256), "n2_256x4" -- and up to 16384 in the large-N kernel
                     * ("n2_mem1024", state in the scratch).  The sweep over the parents is skipped on the steps before
                     * t1 of a window without init_stats, where its result is exactly zero.  GARCH: the reference's
                     * backward kernel (garch/kernels.py:20-37) scores only the x component of the state, so the phi /
                     * lambda scores of this smoother (and of PaRIS) differ systematically from the O(N) ones; this
                     * library reproduces the reference. */
                    PFG_SMOOTHER_POYIADJIS_N2 = 4,
                    /* LAUNCH-LEVEL id only (pfg_launch_device_smoother; never in a descriptor): the caller states that
                     * every descriptor of the batch is the Poyiadjis O(N) score -- smoother = NEMETH, lambduh = 1.0,
                     * stat = SCORE (what pf = 'poyiadjis_N' means, pf.py:139-180).  Same kernels and the same numbers
                     * as NEMETH; the 1024 x 4 (1024 < N <= 4096) and the one-wave x 2 (N <= 128, batches) fp64
                     * device-generator units, and the 256 x 4 / one-wave x 2 REPLAY units of SVM and LGSSM, run a twin
                     * with the filter, the lambda != 1 shrinkage and the other statistics compiled out (BASELINE config
                     * 4: -3.9 %, config 1: -3.8 %; seed-compatible arithmetic -4.6 % / -6.2 %, bitwise the same numbers).
                     * A descriptor that breaks the statement gets out[0..7] = NaN from that twin.  pfg_run_batch
                     * chooses it by itself when every window of the batch qualifies. */
                    PFG_SMOOTHER_POYIADJIS_N = 5,
                    /* The EXACT score of the linear Gaussian model, no particles: the reference's kind = 'marginal'
                     * gradient (sgmcmc_sampler.py:298-329; models/lgssm/helper.py:53-192, 312-420, include_init = True).
                     * Valid in descriptors and launches; model LGSSM and dtype F64 only; kernel, rng, N, lambduh,
                     * stat and the stream / seed fields are ignored.  Per window: forward Kalman messages over the
                     * left buffer [0, t1) from the message of x_{-1} given by prior_mean = mean_precision / precision,
                     * prior_var = 1 / precision (> 0), backward messages over the right buffer [tL, T) from the zero
                     * message, then the smoothed score over [t1, tL) with `weights`.  out[0..3] = the gradient in the
                     * LGSSM score column order, out[4] = sum_t w_t log Pr(y_t | y_{<t}) over [t1, tL) given the left
                     * buffer (noisy_loglikelihood(kind = 'marginal'), sgmcmc_sampler.py:147-174), out[5..7] = 0.
                     * `scratch`: 16 (tL - t1 + 1) bytes rounded up to 256 (pfg_run / pfg_run_batch allocate it;
                     * resident callers supply it).  A batch is all-Kalman or Kalman-free; no trace / final outputs. */
                    PFG_SMOOTHER_KALMAN = 6,
                    /* Forward-filtering backward-sampling of the latent path, no particles: the reference's
                     * LGSSMHelper.latent_var_sample(distr = 'joint') (models/lgssm/helper.py:650-698) and, on its paths,
                     * the complete-data score of kind = 'complete' (sgmcmc_sampler.py:330-362; helper.py:422-491).
                     * Model LGSSM and dtype F64 only; kernel and lambduh are ignored.  Per descriptor, one workgroup:
                     * the forward Kalman messages of the whole buffer [0, T) from the message of x_{-1} (prior_mean,
                     * prior_var as for PFG_SMOOTHER_KALMAN), then N = the number of paths sampled backward, one lane per
                     * path.  REPLAY: z holds T N standard normals in the reference's draw order, z[k N + s] = path s at
                     * time T-1-k (one np.random.standard_normal(T N)); z0 / u are not read.  DEVICE: the lane generator
                     * keyed by (seed, stream, *step_ctr), lane = path.  stat = SCORE: out[0..3] = the complete-data score
                     * over [t1, tL) with `weights`, averaged over the paths, in the LGSSM score column order (transition
                     * terms only where x_{t-1} is in the buffer); stat = NONE: 0; out[4..7] = 0.  trace_x (optional):
                     * the paths, [T][N] with t ascending; no other trace or final output.  `scratch`: 16 (T + 1) bytes
                     * rounded up to 256, from the whole buffer (pfg_run / pfg_run_batch allocate it; resident callers
                     * supply it).  A batch is all-FFBS or FFBS-free. */
                    PFG_SMOOTHER_KALMAN_FFBS = 7,
                    /* EXTENSION (not in the reference): NEMETH (any lambduh; poyiadjis_N is lambduh = 1.0) with STRATIFIED
                     * resampling: child r of a timestep searches the unchanged CDF with u'_r = (r + U_r) / N, one
                     * U_r ~ U[0, 1) per child, r the particle index in the reference's order.  Valid in descriptors and
                     * launches; stat = SCORE / SUFF / NONE; both generators, f64 and f32 state, N <= 16384: the 256 x 4
                     * LDS-resident instantiation "stratified256x4" for N <= 1024, above it "mem1024_stratified" (REPLAY)
                     * or "big4096_stratified" / "big16384_stratified" (DEVICE: the uniforms come out sorted, so the
                     * multinomial kernel's spacing draws and second scan are compiled out).
                     * REPLAY contract: U_r is the caller's u[t N + r] -- the stream a multinomial window consumes, so a
                     * NumPy generator is left where the multinomial call leaves it -- and, in fp64,
                     *     u' = ((double)r + u[t*N + r]) / (double)N         (one addition, one IEEE division)
                     * then the unchanged cumsum; /= last; searchsorted(side='right').  The REPLAY units are built with
                     * -ffp-contract=off: this is exactly NumPy's (np.arange(N) + u[t]) / N, and the pinned oracle fed
                     * those uniforms is the specification, ancestors included.  DEVICE: U_r is one 32-bit uniform of the
                     * lane that owns child r (rec_ud records u'_r in traced launches).
                     * A batch is all-stratified or stratified-free (INVALID); together with FILTER, PARIS or POYIADJIS_N2
                     * windows, with PFG_STAT_PREDICTIVE or with N > 16384: UNSUPPORTED, the message says which.  Whole-GPU
                     * windows and elementwise statistics are not built for it. */
                    PFG_SMOOTHER_NEMETH_STRATIFIED = 8 };
/* additive statistic: *_complete_data_loglike_gradient (score), *_sufficient_statistics, zero */
enum pfg_stat { PFG_STAT_SCORE = 0, PFG_STAT_SUFF = 1, PFG_STAT_NONE = 2,
                /* k-step-ahead predictive log-likelihoods accumulated with the filter's
                 * logsumexp update (pf.py:72-76; statistic functions svm/helper.py:352-395,
                 * lgssm/helper.py:1281-1336, garch/helper.py:374-412).  FILTER smoother only. */
                PFG_STAT_PREDICTIVE = 3,
                /* the sufficient statistics of the blocked Gibbs sampler (lgssm/helper.py:502-555) of the one path of
                 * a PFG_SMOOTHER_KALMAN_FFBS window (N = 1 only), over the whole buffer: t1, tL and the weights are
                 * ignored.  out[0..7] = [sum_{t>=1} x_{t-1}^2, sum_{t>=1} x_t x_{t-1}, sum_{t>=1} x_t^2, sum_t x_t^2,
                 * sum_t y_t x_t, sum_t y_t^2, T, 0]; pfg_run / pfg_run_batch return the record in pfg_result.pred[0..7]
                 * (mean_stat and loglik are not written).  FFBS only: another smoother refuses it as a bad stat id. */
                PFG_STAT_GIBBS = 4 };
/* particle-state arithmetic type.  Weight normalisation, CDF and search are always f64. */
enum pfg_dtype { PFG_F64 = 0, PFG_F32 = 1 };
/* REPLAY: caller supplies the NumPy legacy stream (z0[N], u[T*N], z[T*N]) -> results
 * reproduce the reference on the same seed.  DEVICE: generated in the kernel: one jsf32
 * generator per lane keyed by Philox4x32-10(seed; lane, stream, *step_ctr); 32-bit uniforms,
 * Box-Muller normals evaluated on the f32 transcendental units and widened. */
enum pfg_rng { PFG_RNG_REPLAY = 0, PFG_RNG_DEVICE = 1 };

enum pfg_status {
    PFG_OK = 0,
    PFG_ERR_INVALID = -1,      /* bad argument (message says which) */
    PFG_ERR_UNSUPPORTED = -2,  /* combination not built (e.g. SVM optimal kernel) */
    PFG_ERR_DEVICE = -3,       /* HIP runtime error */
    PFG_ERR_NOMEM = -4,
    PFG_ERR_NUMERIC = -5       /* |A| > 1 for SVM (models/svm/kernels.py:6-11) */
};

/* flags of pfg_problem / pfg_dev_problem */
#define PFG_FLAG_GARCH_STATIONARY_PRIOR 1u /* prior_var = alpha/(1-beta-gamma) (garch/helper.py:324-327) */
#define PFG_FLAG_PARIS_NO_ACCEPT_REJECT 2u /* paris_smoother(accept_reject=False), pf.py:226-236: every child draws its Ntilde
                                            * parents from the exact backward categorical (REPLAY + paris_stream only) */
#define PFG_FLAG_PARIS_RAW_STREAM 4u       /* paris_stream is the window's WHOLE np.random stream (see pfg_problem.paris_stream) */
#define PFG_FLAG_PARIS_RAW_CARRY 8u        /* ... and its first double is the generator's cached Gaussian (has_gauss = 1) */
/* EXTENSION (not in the reference, which resamples at every timestep): ESS-triggered (ADAPTIVE) resampling with the
 * threshold tau in (0, 1], an IEEE binary32 whose BITS travel in `reserved`, the int32 right behind `flags` in pfg_problem
 * and pfg_dev_problem (tau = 0.5 is 0x3F000000; memcpy(&reserved, &tau, 4); 0 without the flag).  At timestep t, with
 * w_i = exp(logw_i - m), m = max logw and p = w / sum w (S, the shrinkage target, is sum_i p_i stats_i of the CURRENT weights
 * as always), the step resamples iff, in fp64,
 *     (sum w)^2 < ((double)tau * N) * sum w^2                      (ESS = 1 / sum p^2 < tau N)
 * as today: multinomial ancestors from the unchanged CDF, the children's log-weights are new_logw.  Otherwise child i is
 * parent i (trace_anc is the identity) and
 *     logw_i = ((logw_i - m) - log(sum w)) + log N + new_logw_i    (log domain: an underflowed weight stays finite)
 * so the log-likelihood increment log(mean(exp(logw))) and the final mean_stat use the carried weights.
 * Built for: smoother NEMETH (any lambduh), stat SCORE / SUFF / NONE, both generators, f64 and f32 state, N <= 16384 --
 * "adaptive256x4" (N <= 1024), above it "mem1024_adaptive" (REPLAY) or "big4096_adaptive" / "big16384_adaptive" (DEVICE);
 * pfg_last_variant reports these.  A step that keeps its particles builds no CDF and runs no search.
 * REPLAY: the window reads the streams of a multinomial window; u[t] of a step that does not resample is ignored.
 * DEVICE: on a step that does not resample a lane of adaptive256x4 draws its normals only (no resampling word); a lane of
 * big*_adaptive has drawn -- and drops -- the step's spacing words (they come before the decision).  Traced launches record
 * as the multinomial kernels do (rec_ud: the uniform child i searched with; rec_z, rec_z0); what rec_ud holds for a step
 * that did not resample is unspecified.
 * pfg_run / pfg_run_batch route by the flag: a batch is all-adaptive or adaptive-free (INVALID); with FILTER, PARIS,
 * POYIADJIS_N2, systematic or stratified windows, PFG_STAT_PREDICTIVE, `elementwise` or N > 16384 (whole-GPU windows):
 * UNSUPPORTED, the message says which; tau outside (0, 1] (NaN included): INVALID.  Resident launches: pfg_launch_device_adaptive. */
#define PFG_FLAG_ADAPTIVE_RESAMPLING 16u

/* One buffered PF window, host side (all pointers are HOST pointers, C-contiguous f64). */
typedef struct pfg_problem {
    int32_t model, kernel, smoother, stat, dtype, rng;
    int32_t N;               /* particles */
    int32_t T;               /* timesteps of the buffered window */
    int32_t t1, tL;          /* statistic / log-likelihood accumulate on [t1, tL) */
    uint32_t flags;
    int32_t reserved;        /* PFG_FLAG_ADAPTIVE_RESAMPLING: the bits of the binary32 threshold tau in (0, 1]; else 0 */
    double lambduh;          /* Nemeth shrinkage; 1.0 = Poyiadjis O(N) */
    double prior_mean, prior_var;
    const double *y;         /* [T] observations (m = 1) */
    const double *weights;   /* [tL-t1] importance weights or NULL (= 1) */
    const double *theta;     /* raw parameters, model layout above */
    const double *z0, *u, *z;/* REPLAY streams: [N], [T*N], [T*N]; NULL for DEVICE */
    uint64_t seed, stream;   /* DEVICE rng: key and stream id (global chain id) */
    const double *init_x, *init_logw, *init_stats; /* optional warm start: [N*n],[N],[N*h] */
    /* PaRIS only.  REPLAY pools of uniforms addressed by (timestep, j, round, particle):
     * paris_idx_u / paris_acc_u [T][Ntilde][max_accept_reject][N] (index draw, accept draw),
     * paris_man_u [T][Ntilde][N] (fallback draw); NULL with the DEVICE rng. */
    int32_t Ntilde, max_accept_reject;
    const double *paris_idx_u, *paris_acc_u, *paris_man_u;
    /* PFG_STAT_PREDICTIVE only: leads 0..num_steps_ahead; REPLAY pool of the standard normals the
     * statistic draws, pred_z [T][num_steps_ahead+1][N] (SVM, GARCH; unused for LGSSM). */
    int32_t num_steps_ahead;
    /* != 0: also compute the ELEMENTWISE sufficient statistics of the window -- the reference's
     * `elementwise_statistic=True` run (buffered_smoother.py:64-65, 201-210) behind
     * Helper.pf_latent_var_distr (svm/helper.py:249-294): one 3-column block [x', x'^2, x x'] (GARCH:
     * [x', x'^2, x'^4]) per window timestep, 3 (tL - t1) columns per particle, carried through the
     * smoother's recursion.  The filter runs once (its trajectory does not depend on the statistic) and
     * records what the recursion needs on the device; a second pass streams the [N][3 (tL-t1)]
     * statistic matrix through HBM step by step.  NEMETH (any lambduh) and PARIS. */
    int32_t elementwise;
    const double *pred_z;
    /* PaRIS in the REFERENCE's np.random order (REPLAY): ONE sequential stream of uniforms, consumed as
     * accept_reject_based_backward_sampling does (pf.py:260-341): per draw j and round, len(L) doubles for
     * np.random.choice then len(L) for np.random.rand, the k-th pending child in index order taking the k-th of each;
     * once <= paris_manual_threshold children are left (or after max_accept_reject rounds) one double per child for
     * its exact draw.  Replaces the addressed pools paris_idx_u / acc_u / man_u (which must then be NULL).  The number
     * of doubles consumed is data dependent: pfg_result.paris_consumed returns it (-1: the stream was too short, run
     * again with a longer one -- the consumption of a window is bounded by (T + 1) (4 N + 2 N Ntilde max_accept_reject +
     * N Ntilde) doubles, a caller that still sees -1 beyond that has a different problem).  The filter's own draws of a timestep (u, z) precede them in np.random's order, so a
     * caller that reproduces np.random.seed() runs ONE timestep per call (warm start init_x / init_logw / init_stats),
     * as sgmcmc_ssm_amd.particle_filters does.  A window of several timesteps carries the cursor from one timestep to
     * the next (PARIS_NO_ACCEPT_REJECT: child i's draw j at timestep t reads double (t N + i) Ntilde + j): given the
     * concatenation of what the single-timestep calls consumed it repeats them in one launch (with `elementwise`).
     * PFG_FLAG_PARIS_RAW_STREAM (dtype f64; N <= 16384): z0 / u / z are NULL and paris_stream holds what RandomState.random_sample
     * delivers from the generator's current state: the kernel takes EVERYTHING from it in np.random's order -- N normals
     * for x0, then per timestep N uniforms, N normals and the backward sampling's uniforms -- so a whole window is one
     * launch.  The normals are NumPy's legacy Gaussians (Marsaglia's polar method on pairs of doubles, second variate of
     * a pair cached for the next draw): acceptance is exact fp64 arithmetic, so the consumption is the reference's to
     * the double; the values go through the device's log (<= 1 ulp from the host libm's; REPLAY tolerance).  With
     * PFG_FLAG_PARIS_RAW_CARRY paris_stream[0] is the generator's pending cached Gaussian and the doubles start at [1].
     * pfg_result.paris_consumed counts the doubles taken (incl. that slot); pfg_result.paris_carry_back != 0: a cached
     * Gaussian is pending at the end, the second variate of the pair of doubles that starts paris_carry_back doubles
     * before the end of the consumption (the caller recomputes it with its own libm and hands the generator on). */
    const double *paris_stream;
    int64_t paris_stream_len;
    int32_t paris_manual_threshold, reserved2;
    /* DEVICE rng: SGLD step the window belongs to, mixed into the generator key exactly as a resident chain's
     * device-side counter (*pfg_dev_problem.step_ctr) is: a window run through pfg_run_batch with
     * (seed, stream = global chain id, step) draws what that chain draws at that step through pfg_launch_device. */
    uint64_t step;
} pfg_problem;

/* Result of one window; optional arrays are caller-allocated HOST buffers or NULL. */
typedef struct pfg_result {
    double mean_stat[PFG_MAX_STAT]; /* sum_i stats_i softmax(logw)_i (average_statistic); FILTER: running m */
    double loglik;                  /* loglikelihood_estimate */
    double *x_T;        /* [N*n]  final particles          */
    double *logw_T;     /* [N]    final log weights        */
    double *stats_T;    /* [N*h]  final per-particle statistics (NEMETH only) */
    double *trace_x;    /* [(T+1)*N*n]  = save_all 'all_x_t'            */
    double *trace_logw; /* [(T+1)*N]    = 'all_log_weights'             */
    double *trace_stats;/* [(T+1)*N*h]  = 'all_statistics' (NEMETH)     */
    double *trace_ll;   /* [T+1]        = 'all_loglikelihood_estimate'  */
    int32_t status;
    int32_t paris_carry_back;   /* PFG_FLAG_PARIS_RAW_STREAM: see pfg_problem.paris_stream; else 0 */
    int32_t *trace_anc; /* [T*N] ancestor index of every particle at every step (with trace_x):
                           the genealogy, from which smoothed marginals are traced back */
    double pred[PFG_MAX_PRED]; /* PFG_STAT_PREDICTIVE: out['statistics'][k] of the reference */
    /* DEVICE rng + trace_x only (test instrumentation of the device-generator kernels): the random
     * inputs the kernel drew, so that a CPU oracle can replay the SAME launch deterministically.
     * rec_u [T*N]: the raw 32-bit word child i searched the resampling CDF with at step t;
     * rec_z [T*N]: its standard normal (as widened to f64);  rec_z0 [N]: the x0 normals.  Every device-generator
     * family that the launch plan picks writes rec_z and rec_z0: pf_reg_kernel, pf_big_kernel, the grid kernels and
     * pf_mem_kernel's PaRIS and O(N^2) sweeps (paris_mem1024, n2_mem1024: 1024 < N <= 16384; a twin of the production
     * instantiation that pfg_run_batch and pfg_launch_device_traced run when buffers are asked for).  pf_mem_kernel's plain
     * sweep forced onto the device generator (PFGRAD_VARIANT=mem1024) records nothing.  The backward-sampling uniforms of
     * PaRIS and the normals of the predictive statistic are recorded nowhere. */
    uint32_t *rec_u;
    double *rec_z, *rec_z0;
    double *rec_ud;     /* [T*N]: large-N device kernel (pf_big_kernel), whose resampling uniforms are not raw
                           generator words but SORTED uniforms built from exponential spacings: the uniform in
                           (0,1) child i searched the CDF with at step t (rec_u stays 0 there); the stratified,
                           adaptive and systematic instantiations record the uniform of child i the same way, and
                           so do pf_mem_kernel's PaRIS and O(N^2) sweeps on the device generator: (word + 0.5) / 2^32
                           of child i's word, searched against the f64 CDF in particle order */
    /* pfg_problem.elementwise: ew_mean [3 (tL-t1)] = average_statistic of the elementwise run (required);
     * ew_stats [N * 3 (tL-t1)] = its per-particle statistics, row-major (optional) */
    double *ew_mean, *ew_stats;
    int64_t paris_consumed;  /* doubles of pfg_problem.paris_stream the window consumed; -1 = stream too short */
    /* PARIS + trace_x only (test instrumentation, both generators; NULL = not wanted): [T][Ntilde][N] int32, the
     * backward-sampled parent of child i's draw j at step t at (t Ntilde + j) N + i -- what the accept-reject rounds or
     * the exact categorical fallback returned, in [0, N).  With the trajectories it determines the statistics.  Not with
     * `elementwise` (that pass owns the buffer as a work piece): INVALID. */
    int32_t *trace_paris_J;
} pfg_result;

/* Device-side descriptor: one per workgroup, resident in HBM.  All pointers are DEVICE
 * pointers.  Used by pfg_launch_device() for callers that keep everything resident
 * (multi-chain SGLD engine, bench).  Layout is part of the ABI (Python mirrors it). */
typedef struct pfg_dev_problem {
    const double *y;
    const double *weights;
    const double *theta;
    const double *z0, *u, *z;
    const double *init_x, *init_logw, *init_stats;
    double *out;             /* [PFG_OUT_DOUBLES]: mean_stat[0..3], loglik, sum of weights W_T,
                                max log weight m_T, min |u - cdf| tie margin (REPLAY) */
    double *final_x, *final_logw, *final_stats;
    double *trace_x, *trace_logw, *trace_stats, *trace_ll;
    const uint64_t *step_ctr;/* optional: *step_ctr is mixed into the DEVICE rng key */
    void *scratch;           /* large-N variant: per-problem state buffers, else NULL */
    double prior_mean, prior_var, lambduh;
    uint64_t seed, stream;
    int32_t T, t1, tL, N;
    int32_t smoother, stat;
    uint32_t flags;
    int32_t reserved;        /* PFG_FLAG_ADAPTIVE_RESAMPLING: the bits of the binary32 threshold tau in (0, 1]; else 0 */
    const double *paris_idx_u, *paris_acc_u, *paris_man_u;   /* PaRIS REPLAY pools (see pfg_problem) */
    int32_t Ntilde, max_accept_reject;
    int32_t *trace_anc;      /* [T*N] or NULL */
    const double *pred_z;    /* PREDICTIVE, REPLAY: [T][num_steps_ahead+1][N] */
    double *pred_out;        /* PREDICTIVE: [PFG_MAX_PRED] */
    void *pred_scratch;      /* PREDICTIVE: [N][PFG_MAX_PRED] of the state type */
    int32_t num_steps_ahead, reserved3;
    uint32_t *rec_u;         /* [T*N] or NULL: see pfg_result.rec_u (DEVICE rng, with trace_x) */
    double *rec_z, *rec_z0;  /* [T*N], [N] or NULL */
    double *rec_ud;          /* [T*N] or NULL: see pfg_result.rec_ud */
    int32_t *trace_paris_J;  /* [T][Ntilde][N] or NULL (PARIS, with trace_x): the backward-sampled parent of
                                every child and draw: the structure the elementwise statistics are carried through */
    const double *paris_stream;      /* see pfg_problem.paris_stream */
    int64_t paris_stream_len;
    int64_t *paris_consumed;         /* [2] or NULL: doubles consumed (-1: stream too short), carry-back distance */
    int32_t paris_manual_threshold, reserved4;
    uint64_t *stamps;        /* [PFG_STAMP_WORDS] or NULL (measurement): wave 0 of the workgroup writes
                                s_memtime / s_memrealtime (100 MHz) at kernel start [0],[1] and end [2],[3]
                                -> in-kernel shader clock = ([2]-[0]) / ([3]-[1]) * 100 MHz; [4..15]: per-phase
                                cycle sums, only in diagnostic builds (-DPFG_PHASE_STAMPS), else untouched */
} pfg_dev_problem;

int pfg_version(void);
/* sizeof() of an ABI struct: 0 pfg_problem, 1 pfg_result, 2 pfg_dev_problem, 3 pfg_prior_hyper, 4 pfg_csmc_problem,
 * 5 pfg_cpm_problem, 6 pfg_sqmc_problem (bindings assert their mirror has the same size) */
int pfg_struct_size(int which);
int pfg_create(pfg_ctx **out, int device_id);
void pfg_destroy(pfg_ctx *ctx);
const char *pfg_last_error(pfg_ctx *ctx);   /* ctx may be NULL: last error of pfg_create */

/* Host-buffer entry points: stage inputs to HBM, run, copy results back, synchronise.
 * pfg_run_batch requires all problems to share model/kernel/dtype/rng; N, T, windows,
 * parameters and seeds may differ per problem.  One workgroup per problem. */
int pfg_run(pfg_ctx *ctx, const pfg_problem *p, pfg_result *r);
int pfg_run_batch(pfg_ctx *ctx, int B, const pfg_problem *ps, pfg_result *rs);

/* The context's own (non-blocking) stream, as a hipStream_t. */
void *pfg_ctx_stream(pfg_ctx *ctx);

/* Resident entry point: `dev_probs` is a DEVICE array of B descriptors; launches on
 * `hip_stream` (a hipStream_t used as is: NULL is HIP's default stream; pass
 * pfg_ctx_stream(ctx) for the context's own) and returns without synchronising.
 * n_max = the largest N in the batch (selects the kernel variant).  The variant is chosen without
 * reading the descriptors: where it is the large-N kernel's N <= 4096 instantiation (REPLAY,
 * 1024 < n_max <= 4096), a PFG_STAT_PREDICTIVE descriptor gets NaNs in out[] -- that statistic is
 * served by pfg_run_batch, which plans predictive batches onto the general kernel. */
int pfg_launch_device(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max,
                      int B, const pfg_dev_problem *dev_probs, void *hip_stream);
/* pfg_launch_device / pfg_launch_device_smoother are the PRODUCTION launches: for the plain (NEMETH / FILTER)
 * LDS-resident kernels (DEVICE generator, and REPLAY) they run an instantiation with the trace instrumentation compiled
 * out, which IGNORES the trace_x / trace_logw / trace_stats / trace_ll / trace_anc / rec_* fields of the
 * descriptors (out / final_* / stamps are honoured).  pfg_launch_device_traced runs the twin that honours them
 * (save_all trajectories, recorded generator draws); same arguments as pfg_launch_device_smoother.  Both twins
 * return bitwise the same `out` record for the same descriptor (tests/test_gpu_device_replay.py).
 * pfg_last_traced: 1 if the latest launch through the context honoured trace buffers, 0 if not. */
int pfg_launch_device_traced(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother,
                             int n_max, int B, const pfg_dev_problem *dev_probs, void *hip_stream);
int pfg_last_traced(pfg_ctx *ctx);
/* as pfg_launch_device for a batch whose descriptors all have smoother = `smoother`
 * (PFG_SMOOTHER_PARIS, _NEMETH_SYSTEMATIC, _NEMETH_STRATIFIED and _POYIADJIS_N2 have their own kernel instantiations;
 * the plain entry point serves NEMETH / FILTER).  PFG_SMOOTHER_KALMAN: the exact-score kernel, one lane per
 * descriptor (kernel, rng and n_max are ignored; every descriptor brings its scratch).  PFG_SMOOTHER_KALMAN_FFBS: the
 * FFBS kernel, one workgroup per descriptor (n_max = the most paths N of a descriptor picks the workgroup size; every
 * descriptor brings its scratch).  PFG_SMOOTHER_PARIS runs an LDS-resident variant for n_max <= 1024 --
 * "paris64x2" (one wave per window, 64 threads x 2 particles: n_max <= 128, the DEVICE rng and more than 64 descriptors;
 * PFGRAD_VARIANT=paris64x2 forces it wherever it holds n_max, REPLAY included), "paris256x1" (the rest of n_max <= 256),
 * "paris256x4" (n_max <= 1024) -- and "paris_mem1024" above that (state in
 * the descriptors' scratch).  PFG_SMOOTHER_POYIADJIS_N2 likewise: "n2_64x2" (one wave per window: n_max <= 128, the
 * DEVICE rng and more than 64 descriptors; PFGRAD_VARIANT=n2_64x2 forces it wherever it holds n_max, REPLAY included),
 * "n2_256x1" (the rest of n_max <= 256), "n2_256x4" (n_max <= 1024; PFGRAD_VARIANT=n2_256x1 / n2_256x4 force those where
 * they hold n_max), "n2_mem1024" above that (state in the descriptors' scratch) */
int pfg_launch_device_smoother(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother,
                               int n_max, int B, const pfg_dev_problem *dev_probs, void *hip_stream);
/* as pfg_launch_device for a batch of ADAPTIVE windows (PFG_FLAG_ADAPTIVE_RESAMPLING; the launch does not read the
 * descriptors, so the family is stated here): NEMETH descriptors with the flag and the threshold's bits in `reserved`, n_max <= 16384.
 * traced != 0: the launch honours trace_* / rec_* (one instantiation serves both; the `out` records are bitwise the same).
 * A descriptor without the flag, with another smoother or with PFG_STAT_PREDICTIVE gets NaNs in out[0..7].  Scratch per
 * descriptor (n_max > 1024): pfg_scratch_bytes(model, dtype, PFG_RNG_REPLAY, n_max) -- the large-N kernels' state, the same
 * for both generators, and what pfg_scratch_bytes_smoother(..., PFG_SMOOTHER_NEMETH, N) answers except for the DEVICE
 * generator and 1024 < N <= 4096, where plain windows run LDS-resident (0) and adaptive ones do not.  n_max > 16384:
 * UNSUPPORTED. */
int pfg_launch_device_adaptive(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int B,
                               const pfg_dev_problem *dev_probs, void *hip_stream, int traced);
/* N above the one-workgroup kernels' maximum (16384 < N <= 4194304; the reference has no limit and its bias experiments
 * call pf_gradient_estimate with N = 1000000: gradient_error_fig_scripts/svm_grad_compare.py:68-82): every window of the
 * batch runs as a WHOLE-GPU window -- the particle axis cut into tiles of 1024 (N <= 524288) / 2048 particles, one 256-thread workgroup each, one
 * kernel launch per timestep (T_max + 2 launches on `hip_stream`; REPLAY: 5 T_max + 2, the extra four per timestep build
 * the reference's CDF -- NumPy's sequential cumsum, bit for bit -- with the particle axis spread over the GPU).  T_max = the largest T of
 * the batch (the host issues the launches, so it has to know; shorter windows leave theirs at once).  NEMETH / FILTER
 * with the score, sufficient or no statistic.  Every descriptor needs `scratch` of pfg_scratch_bytes(model, dtype, rng, N)
 * bytes (256-byte aligned; non-decreasing in N within a tile class, so the size for n_max serves every window); windows of one batch must all have N <= 524288 or all N > 524288 (the tile size differs).
 * DEVICE rng: the resampling uniforms are SORTED uniforms (exponential spacings, rec_ud), generator lane = particle
 * index mod tile; out[7] = 1.  REPLAY: u / z as for every kernel, out[7] = the smallest |u - cdf| margin of the run.
 * pfg_run / pfg_run_batch route N > 16384 here by themselves (PFGRAD_VARIANT=grid forces it for smaller N). */
int pfg_launch_device_grid(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int T_max, int B,
                           const pfg_dev_problem *dev_probs, void *hip_stream);
/* The same window, one piece per call, for callers that put events, graph nodes or their own work between the launches:
 * phase = PFG_GRID_PHASE_INIT (x0 / warm start, the partials of timestep 0), then every timestep t = 0 .. T_max - 1 in order
 * (phase = t; REPLAY: the CDF kernel + the step kernel), then PFG_GRID_PHASE_FINISH (out / final_* / trace_ll[T]).  The
 * sequence INIT, 0, 1, ..., T_max - 1, FINISH on one stream is exactly pfg_launch_device_grid. */
#define PFG_GRID_PHASE_INIT (-2)
#define PFG_GRID_PHASE_FINISH (-3)
int pfg_launch_device_grid_phase(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int n_max, int phase, int B,
                                 const pfg_dev_problem *dev_probs, void *hip_stream);
/* Both of the above with the batch's smoother stated (as pfg_launch_device_smoother does for N <= 16384): NEMETH / FILTER
 * run what the entry points above run; PFG_SMOOTHER_POYIADJIS_N -- every window is (NEMETH, lambduh = 1, score) -- runs a
 * twin of the device-generator timestep kernel specialised to that estimator (fewer registers: g1 +2.2 %, four windows of
 * 4 10^5 particles +5.7 %; same numbers to the last place or two).  A window that breaks the statement gets out[0..7] = NaN.
 * phase = PFG_GRID_PHASE_ALL: the whole window (T_max + 2 launches); otherwise one piece, T_max is ignored.
 * pfg_run_batch states POYIADJIS_N by itself when every window of a whole-GPU batch qualifies. */
#define PFG_GRID_PHASE_ALL (-1)
int pfg_launch_device_grid_smoother(pfg_ctx *ctx, int model, int kernel, int dtype, int rng, int smoother, int n_max,
                                    int T_max, int phase, int B, const pfg_dev_problem *dev_probs, void *hip_stream);

/* Buffered-subsequence sampling for resident chains, on the device: for every descriptor b draw
 * a window start as SGMCMCSampler._random_subsequence_and_buffers does (sgmcmc_sampler.py:259-288;
 * 'uniform' style: start ~ U{0..T-S}; strict != 0: start = S * U{0..T/S-1}), keyed by
 * Philox(seed; chain_offset + b, *step_ctr), and point y / T / t1 / tL / weights at
 * [start - buffer, start + S + buffer) clipped to the series.  weights_table: [T-S+1][S] row per
 * start (random_subsequence_and_weights, :1969-2017) or NULL.  With this the whole SGLD step is
 * three launches and no host work: capturable in a hipGraph.  Asynchronous on `hip_stream`. */
int pfg_sample_windows_device(pfg_ctx *ctx, int B, pfg_dev_problem *dev_probs, const double *y_dev,
                              const double *weights_table_dev, int T, int S, int buffer, int strict,
                              uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr,
                              void *hip_stream);

/* Several windows per chain and step (the reference's minibatch_size and num_sequences, sgmcmc_sampler.py:390-425,
 * 1249-1283), for C resident chains over n_seq sequences laid end to end in y_dev: sequence k is
 * y_dev[seq_bounds_dev[k], seq_bounds_dev[k+1]) (DEVICE int64 [n_seq + 1], increasing; a single series is n_seq = 1).
 * Per chain, K_eff sequences: num_sequences = -1 takes all n_seq in index order (no draw); 1 <= num_sequences = K <=
 * min(n_seq, PFG_MAX_DRAWN_SEQUENCES) draws K distinct sequences, uniformly and in random order (the law of
 * np.random.choice(n_seq, K, replace=False)).  In each, M windows: start as pfg_sample_windows_device ('uniform':
 * U{0..T_k-S}; strict != 0: S U{0..T_k/S-1}), the window [start, start + S) with `buffer` points each side clipped to
 * the SEQUENCE; a sequence with T_k <= S (or S < 1) is taken whole, weights NULL.  Writes y / T / t1 / tL / weights of
 * dev_probs[c W + w], W = K_eff M, chain-major, window w = k M + m the m-th window in the k-th chosen sequence, and
 * seq_len_dev[c W + w] = T_k (DEVICE int32 [C W]); every other descriptor field is left as it is.  weights_dev: the
 * per-sequence random_subsequence_and_weights tables, UNSCALED, sequence k's [T_k - S + 1][S] rows (one per start)
 * from weights_dev + weight_offsets_dev[k] (DEVICE int64 [n_seq]; entries of sequences with T_k <= S are not read);
 * NULL: weights NULL.  Draws: Philox4x32-10 keyed by `seed`, counter (global chain id = chain_offset + c, *step_ctr,
 * draw index): sequence draw j and the start of window w are distinct draws, so a chain's windows depend on its global
 * id and the step only.  Asynchronous on `hip_stream`.  Refuses num_sequences outside -1 / 1..n_seq (INVALID), above
 * PFG_MAX_DRAWN_SEQUENCES or W >= 2^24 (UNSUPPORTED), M < 1, buffer < 0, strict with S < 1. */
#define PFG_MAX_DRAWN_SEQUENCES 1024
int pfg_sample_windows_multi_device(pfg_ctx *ctx, int C, int n_seq, const int64_t *seq_bounds_dev,
                                    const int64_t *weight_offsets_dev, int num_sequences, int M,
                                    pfg_dev_problem *dev_probs, int32_t *seq_len_dev, const double *y_dev,
                                    const double *weights_dev, int S, int buffer, int strict, uint64_t seed,
                                    uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream);
/* The C W window records win_outs [C W][PFG_OUT_DOUBLES] (layout of pfg_sample_windows_multi_device, W = K M with
 * K = num_seq_windows, the sequences of a chain) -> one record per chain, outs [C][PFG_OUT_DOUBLES], in the reference's
 * order of operations (sgmcmc_sampler.py:411-418, 1264-1282), for out[0..3] (score columns) and out[4] (log-likelihood):
 *   part_k = 0.0; for m in 0..M-1: part_k = part_k + (g[k M + m] * 1.0) / M
 *   acc = part_0; for k in 1..K-1: acc = acc + part_k
 *   rescale != 0:  S = 0.0; S = S + T_k in the same order (seq_len_dev of window k M);  acc = (acc * T_total) / S
 * out[5..7] of the reduced record are 0 (the windows' weight sums, maximum log-weights and tie margins do not combine).
 * No atomics: the order above is the contract, a host restatement is bitwise equal.  seq_len_dev may be NULL without
 * rescale.  With Tscale = T_total, pfg_sgld / sghmc / sgrld_update_device on `outs` is noisy_gradient's step
 * (sgmcmc_sampler.py:427-464).  Asynchronous on `hip_stream`. */
int pfg_reduce_windows_device(pfg_ctx *ctx, int C, int num_seq_windows, int M, const double *win_outs,
                              const int32_t *seq_len_dev, int rescale, double T_total, double *outs, void *hip_stream);

/* bytes of per-problem HBM scratch (pfg_dev_problem.scratch, 256-byte aligned) the large-N
 * kernel (N <= 16384) or the whole-GPU window (N <= 4194304) needs for (model, dtype, rng, N); 0 when an LDS-resident
 * variant serves this size, -1 when N is above the supported maximum */
int64_t pfg_scratch_bytes(int model, int dtype, int rng, int N);
/* the same for a resident batch of `smoother` windows (PFG_SMOOTHER_NEMETH .. PFG_SMOOTHER_POYIADJIS_N, or
 * PFG_SMOOTHER_NEMETH_STRATIFIED: the large-N kernels' state for 1024 < N <= 16384) launched
 * through pfg_launch_device_smoother: what that launch's plan sizes per descriptor -- PFG_SMOOTHER_PARIS: the
 * paris_mem1024 state for 1024 < N <= 16384, 0 where an LDS-resident variant serves; PFG_SMOOTHER_POYIADJIS_N2: the
 * n2_mem1024 state for 1024 < N <= 16384, 0 for N <= 1024 -- and -1 above the one-workgroup
 * kernels' maximum (16384), for another smoother id, or for a combination that launch refuses */
int64_t pfg_scratch_bytes_smoother(int model, int dtype, int rng, int smoother, int N);
/* name of the kernel variant pfg_launch_device would pick (for profiles / logs) */
const char *pfg_variant_name(int model, int kernel, int dtype, int rng, int n_max);
/* tag of the kernel variant the latest launch through this context ran ("wg256x4s", "wg1024x1",
 * "wg1024x4s", "wg64x2", "big4096", "big16384", "mem1024", ...): the batch size takes part in the
 * choice, so tests and profiles read it back instead of predicting it */
const char *pfg_last_variant(pfg_ctx *ctx);
int pfg_synchronize(pfg_ctx *ctx);

/* SGLD parameter update for B resident chains (sgmcmc_sampler.py:427-464, 529-566, 650-656):
 *   theta_v += eps*(grad_logprior_v(theta) + ghat_v)/Tscale + sqrt(2 eps) N(0, 1/Tscale)
 * followed by project_parameters.  `outs` is the [B][PFG_OUT_DOUBLES] result array the
 * PF kernel wrote (score column order), `theta` [B][PFG_MAX_THETA] is updated in place.
 * hyper: model-specific prior hyper-parameters, see pfg_prior_hyper.  The noise of chain b is
 * keyed by (seed, chain_offset + b, *step_ctr): a chain's trajectory depends on its GLOBAL
 * index only, not on how chains are spread over GPUs.  *step_ctr is incremented afterwards. */
typedef struct pfg_prior_hyper {
    double df_Qinv, scale_Qinv, df_Rinv, scale_Rinv;  /* Wishart on Qinv/Rinv (covariance.py:252-284) */
    double mean_A, var_col_A, mean_C, var_col_C;      /* matrix normal (matrices.py:597-607) */
    double scale_mu, shape_mu, alpha_phi, beta_phi, alpha_lambduh, beta_lambduh; /* garch_var.py:152-165 */
} pfg_prior_hyper;
int pfg_sgld_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                           const pfg_prior_hyper *hyper, double epsilon, double Tscale,
                           uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr,
                           void *hip_stream);

/* EXTENSION (not in the reference: its samplers are SGD / ADAGRAD / SGLD / SGRLD / Gibbs,
 * sgmcmc_sampler.py:467-648): SGHMC update with friction alpha in (0, 1] for resident chains,
 *   v <- (1 - alpha) v + eps (grad_logprior + ghat)/Tscale + N(0, 2 alpha eps / Tscale),  theta <- theta + v,
 * then project_parameters.  momentum [B][PFG_MAX_THETA] is updated in place; alpha = 1 is exactly
 * pfg_sgld_update_device (same noise stream).  Parity-unpinned. */
int pfg_sghmc_update_device(pfg_ctx *ctx, int model, int B, double *theta, double *momentum,
                            const double *outs, const pfg_prior_hyper *hyper, double epsilon, double alpha,
                            double Tscale, uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr,
                            void *hip_stream);

/* SGRLD parameter update for B resident LGSSM chains: sample_sgrld with the LGSSM preconditioner
 * (sgmcmc_sampler.py:613-640, lgssm/parameters.py:58-67), then project_parameters.  With theta = (A, C, LQinv,
 * LRinv), Qinv = LQinv^2 + 1e-16, Q = 1 / Qinv and g_v = grad_logprior_v + ghat_v, all at the pre-step theta:
 *   A     += eps Q g_A / Tscale                           + sqrt(2 eps / Tscale) z_A / LQinv
 *   LQinv += eps (0.5 Qinv g_LQinv + LQinv) / Tscale      + sqrt(2 eps / Tscale) sqrt(0.5) LQinv z_Q
 * (C and LRinv likewise with R); the projection then sets C = 1.  The four normals of chain b are those of
 * pfg_sgld_update_device: keyed by (seed, chain_offset + b, *step_ctr).  *step_ctr is incremented afterwards.
 * LGSSM only: SVM and GARCH return PFG_ERR_UNSUPPORTED (the reference defines no preconditioner for them). */
int pfg_sgrld_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                            const pfg_prior_hyper *hyper, double epsilon, double Tscale,
                            uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream);

/* SGD and ADAGRAD steps for B resident chains (sgmcmc_sampler.py:467-484, 504-527), every model, on the `outs` and
 * `hyper` of pfg_sgld_update_device, followed by project_parameters.  With g_v = (grad_logprior_v(theta) + ghat_v) / Tscale:
 *   pfg_sgd_update_device      theta_v += eps g_v
 *   pfg_adagrad_update_device  G_v += g_v g_v;  theta_v += eps g_v / sqrt(G_v + 1e-9)      (NOISE_NUGGET)
 * moment [B][PFG_MAX_THETA] holds G and is updated in place; it covers every variable, LGSSM's C included although the
 * projection pins C; SVM's fourth slot is untouched.  Neither draws anything.  *step_ctr (may be NULL) is incremented
 * afterwards, so that the filters of the next step draw afresh. */
int pfg_sgd_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs, const pfg_prior_hyper *hyper,
                          double epsilon, double Tscale, uint64_t *step_ctr, void *hip_stream);
int pfg_adagrad_update_device(pfg_ctx *ctx, int model, int B, double *theta, double *moment, const double *outs,
                              const pfg_prior_hyper *hyper, double epsilon, double Tscale, uint64_t *step_ctr,
                              void *hip_stream);

/* EXTENSION: SGLD with control variates (Baker, Fearnhead, Fox and Nemeth 2019) for B resident chains.  outs and
 * outs_centre [B][PFG_OUT_DOUBLES]: the records of the chain's window at theta and of the SAME window at the centre
 * (ChainEnsemble runs both in one launch on the same draws); centre_grad [B][4]: the whole-data score at the centre in
 * score-column order, raw and unscaled, without the prior.  The step is pfg_sgld_update_device's -- the same device code,
 * normals and key -- on
 *   ghat_k = centre_grad_k + (outs_k - outs_centre_k),   k = 0..3, in that operand order,
 * so with outs == outs_centre it is pfg_sgld_update_device on a record holding centre_grad, and with centre_grad = 0,
 * outs_centre = 0 it is pfg_sgld_update_device on outs, both bit for bit.  *step_ctr is incremented afterwards.
 *
 * pfg_cv_accumulate_device: the mean over num_repeats launches behind centre_grad.  Call `repeat` (0 .. num_repeats - 1, in
 * order) adds columns 0..4 of outs [B][PFG_OUT_DOUBLES] into acc [B][PFG_OUT_DOUBLES] (repeat 0 stores), and the last one
 * divides once by num_repeats: a fixed order of IEEE operations, no atomics.  Columns 5..7 of acc are not touched.
 * *step_ctr (may be NULL: the counter of the centring launches) is incremented afterwards. */
int pfg_sgld_cv_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs, const double *outs_centre,
                              const double *centre_grad, const pfg_prior_hyper *hyper, double epsilon, double Tscale,
                              uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream);
int pfg_cv_accumulate_device(pfg_ctx *ctx, int B, const double *outs, double *acc, int repeat, int num_repeats,
                             uint64_t *step_ctr, void *hip_stream);

/* Gibbs parameter draw for B resident LGSSM chains: LGSSMPrior.sample_posterior (base_parameters.py:354-377,
 * 437-450) from the PFG_STAT_GIBBS statistics an FFBS launch with one path per chain left in `outs`
 * [B][PFG_OUT_DOUBLES] -- Qinv, Rinv from their 1 x 1 Wishart (scale * chi2(df)) posteriors, A given Q from its
 * normal posterior -- then project_parameters (C = 1, so C is not drawn).  The chi2 variates come from a bounded
 * rejection sampler, every attempt keyed by (seed, chain_offset + b, *step_ctr, attempt); a chain whose 64 attempts
 * are all rejected gets NaN.  *step_ctr is incremented afterwards.  LGSSM only (PFG_ERR_UNSUPPORTED otherwise). */
int pfg_gibbs_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                            const pfg_prior_hyper *hyper, uint64_t seed, uint64_t chain_offset,
                            uint64_t *step_ctr, void *hip_stream);

/* EXTENSION (not in the reference): particle marginal Metropolis-Hastings (Andrieu, Doucet and Holenstein 2010) for B
 * resident chains -- a random-walk proposal, a launch that leaves a log-likelihood estimate of the WHOLE data set at the
 * proposal in out[4] (a particle filter, whatever its N, or the Kalman launch), and an accept / reject step.  All
 * arrays are DEVICE memory; the draws of chain b are Philox4x32-10 keyed by (seed, chain_offset + b, *step_ctr) with
 * tags of their own (csrc/pfg_chains.hip), so a chain depends on its GLOBAL index only.
 *
 * pfg_logprior_device: logprior[b] = Prior.logprior of the raw row theta[b] (SVM (A, LQinv, LRinv), LGSSM (A, C, LQinv,
 * LRinv), GARCH (log_mu, logit_phi, logit_lambduh, LRinv)), without Jacobian terms and up to a constant of the
 * hyper-parameters: differences of it are differences of the host's log-prior.
 *
 * pfg_pmmh_propose_device: theta_prop[b] = theta[b] + scale (.) z, scale [PFG_MAX_THETA] doubles, z standard normals
 * (LGSSM: C stays 1 whatever scale[1] is).  The support is what project_parameters leaves unchanged: |A| <= 0.9999 and
 * every Cholesky factor > 0.  valid[b] = 1 inside it; outside, valid[b] = 0 and theta_prop[b] = theta[b], so the launch
 * that follows runs on a legal parameter vector.  *step_ctr is read, not incremented.
 *
 * pfg_pmmh_accept_device: outs [B][PFG_OUT_DOUBLES], out[4] the estimate at theta_prop.  init != 0: ll_cur[b] = out[4],
 * nothing else changes, *step_ctr is left as it is.  Otherwise
 *   log alpha = (out[4] + logprior(theta_prop)) - (ll_cur + logprior(theta)),  u uniform in (0, 1),
 * and chain b accepts iff valid[b], out[4] is finite and log(u) < log alpha (a NaN log alpha rejects): theta[b] =
 * theta_prop[b], ll_cur[b] = out[4], n_accept[b] += 1.  A chain that rejects keeps theta AND ll_cur -- the estimate is
 * never refreshed, which is what makes the chain exact for every N.  *step_ctr is incremented afterwards.
 * A bad model id, B < 0 or a NULL array: PFG_ERR_INVALID (step_ctr may be NULL: counter 0, no increment). */
int pfg_logprior_device(pfg_ctx *ctx, int model, int B, const double *theta, const pfg_prior_hyper *hyper,
                        double *logprior, void *hip_stream);
int pfg_pmmh_propose_device(pfg_ctx *ctx, int model, int B, const double *theta, double *theta_prop, int32_t *valid,
                            const double *scale, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr,
                            void *hip_stream);
int pfg_pmmh_accept_device(pfg_ctx *ctx, int model, int B, double *theta, const double *theta_prop,
                           const int32_t *valid, const double *outs, double *ll_cur, uint64_t *n_accept,
                           const pfg_prior_hyper *hyper, int init, uint64_t seed, uint64_t chain_offset,
                           uint64_t *step_ctr, void *hip_stream);

/* EXTENSION (not in the reference): the particle Metropolis-adjusted Langevin algorithm (Nemeth, Sherlock and Fearnhead
 * 2016) for B resident chains -- PMMH with a Langevin proposal driven by the filter's own score estimate.  The launch
 * between the two calls is the SCORE launch on theta_prop: it leaves the score in out[0..3] (score-column order: SVM
 * [LRinv, LQinv, A], LGSSM [LRinv, LQinv, C, A], GARCH [LRinv, log_mu, logit_phi, logit_lambduh]) and the
 * log-likelihood estimate of the WHOLE data set in out[4].  Coordinates, support, arrays and the keying of the draws
 * are those of the PMMH calls above (tags of their own, csrc/pfg_chains.hip).  With s = scale [PFG_MAX_THETA] and
 *   d_j(theta, g) = grad_logprior_j(theta) + g_j      (the prior gradient pfg_sgld_update_device adds, g mapped from
 *                                                      score columns to theta coordinates as that call maps it)
 *
 * pfg_pmala_propose_device: theta_prop[b]_j = theta[b]_j + (s_j^2 / 2) d_j(theta[b], grad_cur[b]) + s_j z_j, grad_cur
 * [B][PFG_MAX_THETA] the score the chain's current state was accepted with (LGSSM: C stays 1 and takes no normal).
 * With s_j^2 / 2 = epsilon / Tscale for every j this is the law of pfg_sgld_update_device's step before
 * project_parameters.  valid and the treatment of a proposal outside the support: as pfg_pmmh_propose_device.
 * *step_ctr is read, not incremented.
 *
 * pfg_pmala_accept_device: init != 0: ll_cur[b] = out[4], grad_cur[b] = out[0..3], nothing else changes, *step_ctr is
 * left as it is.  Otherwise, with log q(b | a, g) = -sum_j (b_j - a_j - (s_j^2 / 2) d_j(a, g))^2 / (2 s_j^2) over the
 * coordinates that move,
 *   log alpha = (out[4] + logprior(theta_prop)) - (ll_cur + logprior(theta))
 *               + log q(theta | theta_prop, out[0..3]) - log q(theta_prop | theta, grad_cur),
 * and chain b accepts iff valid[b], out[4] and every score component the drift uses are finite and log(u) < log alpha
 * (a NaN rejects): theta[b] = theta_prop[b], ll_cur[b] = out[4], grad_cur[b] = out[0..3] verbatim, n_accept[b] += 1.
 * A chain that rejects keeps theta, ll_cur AND grad_cur: neither estimate is ever refreshed, which is what makes the
 * chain exact for every N.  The target is PMMH's, exp(logprior(theta)) p(y | theta) on the raw row: the drift uses
 * grad_logprior, which is not the gradient of logprior in every coordinate, and need not be -- q is evaluated with the
 * same drift in both directions.  *step_ctr is incremented afterwards.
 * A bad model id, B < 0 or a NULL array: PFG_ERR_INVALID (step_ctr may be NULL: counter 0, no increment). */
int pfg_pmala_propose_device(pfg_ctx *ctx, int model, int B, const double *theta, const double *grad_cur,
                             double *theta_prop, int32_t *valid, const double *scale, const pfg_prior_hyper *hyper,
                             uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream);
int pfg_pmala_accept_device(pfg_ctx *ctx, int model, int B, double *theta, const double *theta_prop,
                            const int32_t *valid, const double *outs, double *ll_cur, double *grad_cur,
                            uint64_t *n_accept, const pfg_prior_hyper *hyper, const double *scale, int init,
                            uint64_t seed, uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream);

/* EXTENSION (not in the reference, whose SVM sample_x / sample_gibbs raise): particle Gibbs (Andrieu, Doucet and Holenstein
 * 2010) for B resident SVM or LGSSM chains -- a conditional SMC sweep with ancestor sampling (Lindsten, Jordan and Schon
 * 2014) that moves each chain's latent path, then the conjugate parameter draw from that path's statistics.
 *
 * pfg_csmc_problem: one chain's sweep.  Every pointer is DEVICE memory.  theta: the raw row (PFG_MAX_THETA doubles); y [T];
 * path [T]: the reference path x*, replaced by the new path (has_ref = 0: written only -- all N particles are free, a
 * bootstrap filter with stored genealogy); scratch: pfg_csmc_scratch_bytes(T, N) bytes, 256-byte aligned -- the states
 * [T][N] f64, then the parents [T][N] uint16 (row 0 unused); out: PFG_OUT_DOUBLES doubles, the statistics of the NEW path
 * -- LGSSM the PFG_STAT_GIBBS record, SVM [sum_{t>=1} x_{t-1}^2, sum_{t>=1} x_t x_{t-1}, sum_{t>=1} x_t^2,
 * sum_t y_t^2 exp(-x_t), 0, 0, T, 0]; n_degenerate: one counter.  The target is the law the filters and FFBS target:
 * x_{-1} ~ N(prior_mean, prior_var), x_t | x_{t-1} ~ f_theta, weights g_theta(y_t | x_t), prior proposal, multinomial
 * resampling at every step; particle N-1 carries the reference path and draws its parent from W_{t-1}^i f(x*_t | x_{t-1}^i).
 * A chain whose weight sum or ancestor-weight sum is zero or not finite at some step keeps its path, gets the statistics
 * of that path and *n_degenerate += 1 (has_ref = 0: a NaN record); NaN is never written to a path.  A descriptor with a
 * NULL array, T < 1, N < 2 or above the launch's n_max, or a prior variance that is not positive: a NaN record and the
 * count.  The trace pointers are read by a traced launch only and may be NULL: trace_anc [T][N] every particle's parent
 * (row 0 not written), trace_ref_anc [T] the reference particle's sampled ancestor (entry 0 not written), trace_w [T][N]
 * the normalised weights, trace_k [1] the final index.
 *
 * pfg_csmc_device: one workgroup per problem, 64 x 2 (one wave) for n_max <= 128, 256 x 4 up to 1024; `problems` is a
 * DEVICE array of B records, n_max >= every record's N.  Draws: Philox4x32-10 keyed by (seed, chain_offset + b,
 * *step_ctr, t, particle) under tags of their own (csrc/pfg_csmc.hip); *step_ctr is read, not incremented.  traced != 0
 * runs the twin that honours the trace pointers; both write the same path, bit for bit.  PFG_ERR_UNSUPPORTED: GARCH, a
 * dtype other than PFG_F64, n_max > 1024 or < 2; PFG_ERR_INVALID: a bad model id, B < 0, problems == NULL.
 *
 * pfg_pgibbs_update_device: the parameter draw from `outs` [B][PFG_OUT_DOUBLES], one lane per chain, keyed as
 * pfg_gibbs_update_device.  LGSSM: that call's arithmetic, expression for expression.  SVM: Qinv and A | Q from
 * out[0..2] as there (T - 1 transitions), Rinv = scale chi2(df) with df = df_Rinv + T, scale = 1 / (1 / scale_Rinv +
 * out[3]) -- the emission law is y_t ~ N(0, R exp(x_t)) --, then project_parameters.  The transition sums run over
 * t >= 1: the dependence of x_0's law on theta is left out of the conditional, as in the reference's LGSSM Gibbs.
 * *step_ctr is incremented afterwards.  GARCH: PFG_ERR_UNSUPPORTED (its prior has no conjugate draw). */
typedef struct pfg_csmc_problem {
    const double *theta;
    const double *y;
    double *path;
    void *scratch;
    double *out;
    uint64_t *n_degenerate;
    int32_t *trace_anc;
    int32_t *trace_ref_anc;
    double *trace_w;
    int32_t *trace_k;
    double prior_mean, prior_var;
    int32_t T, N, has_ref, reserved;
} pfg_csmc_problem;
int64_t pfg_csmc_scratch_bytes(int T, int N);   /* -1: T < 1, N < 2 or N > 1024 */
int pfg_csmc_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_csmc_problem *problems, uint64_t seed,
                    uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced);
int pfg_pgibbs_update_device(pfg_ctx *ctx, int model, int B, double *theta, const double *outs,
                             const pfg_prior_hyper *hyper, uint64_t seed, uint64_t chain_offset,
                             uint64_t *step_ctr, void *hip_stream);

/* EXTENSION (not in the reference): the filter of correlated pseudo-marginal PMMH (Deligiannidis, Doucet and Pitt 2018) for
 * B resident SVM or LGSSM chains.  The log-likelihood estimate out[4] is a deterministic function of theta and of an array
 * U [T+1][N+1] of standard normals that the chain carries; a step proposes U' = rho U + sqrt(1 - rho^2) eps beside theta'
 * and accepts both with pfg_pmmh_accept_device, unchanged.  Particles are sorted by state before each resampling and
 * resampled systematically on one uniform taken from U', which makes the estimate a smooth function of U; the chain is
 * exact for every N and every rho in [0, 1).
 *
 * pfg_cpm_problem: one chain's filter.  Every pointer is DEVICE memory.  theta: the raw row (PFG_MAX_THETA doubles); y [T];
 * u0, u1: the chain's two buffers, pfg_cpm_aux_bytes(T, N) bytes each -- row 0, columns 0 .. N-1: the normals of x_{-1};
 * row t+1, columns 0 .. N-1: the state normals of step t, column N: its resampling normal (column N of rows 0 and 1 is
 * carried and not read); which: the selector, the kernel reads u[*which & 1], writes U' to the other buffer and filters
 * on U' (rho == 0 reads no buffer: the init pass); out: PFG_OUT_DOUBLES doubles, out[4] = sum_t log((1 / N) sum_i w_t^i)
 * with the Gaussian constants of the emission density, every other slot 0.  The target is the law the filters target:
 * x_{-1} ~ N(prior_mean, prior_var), x_t | x_{t-1} ~ f_theta, weights g_theta(y_t | x_t), prior proposal, resampling at
 * every step t >= 1.  A weight sum that is zero or not finite: out[4] = -inf (pfg_pmmh_accept_device rejects it), U' is
 * written in full and stays finite.  A descriptor with a NULL array (the trace pointers may be NULL), T < 1, N < 2 or above
 * the launch's n_max, or a prior variance that is not positive: a NaN record and no other store.  The trace pointers are
 * read by a traced launch only: trace_anc [T][N] each child's parent in sorted coordinates (row 0 not written),
 * trace_ll [T] the per-step increments of out[4].
 *
 * pfg_cpm_device: one workgroup per problem, 64 x 2 (one wave) for n_max <= 128, 256 x 4 up to 1024; `problems` is a DEVICE
 * array of B records, n_max >= every record's N.  eps: Philox4x32-10 keyed by (seed, chain_offset + b, *step_ctr, row,
 * column) under tags of their own (csrc/pfg_cpm.hip); *step_ctr is read, not incremented.  traced != 0 runs the twin that
 * honours the trace pointers; both write the same out[4] and the same U', bit for bit.  PFG_ERR_UNSUPPORTED: GARCH, a dtype
 * other than PFG_F64, n_max > 1024 or < 2; PFG_ERR_INVALID: a bad model id, B < 0, problems == NULL, rho outside [0, 1).
 *
 * pfg_cpm_commit_device: one lane per chain, after pfg_pmmh_accept_device: if (init || n_accept[b] != seen[b])
 * { which[b] ^= 1; seen[b] = n_accept[b]; } -- a chain that accepted now reads the buffer the filter wrote. */
typedef struct pfg_cpm_problem {
    const double *theta;
    const double *y;
    double *u0;
    double *u1;
    const int32_t *which;
    double *out;
    int32_t *trace_anc;
    double *trace_ll;
    double prior_mean, prior_var;
    int32_t T, N;
} pfg_cpm_problem;
int64_t pfg_cpm_aux_bytes(int T, int N);        /* one buffer, rounded up to 256; -1: T < 1, N < 2 or N > 1024 */
int pfg_cpm_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_cpm_problem *problems, double rho,
                   uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced);
int pfg_cpm_commit_device(pfg_ctx *ctx, int B, const uint64_t *n_accept, uint64_t *seen, int32_t *which, int init,
                          void *hip_stream);

/* EXTENSION (not in the reference): the filter of sequential quasi-Monte Carlo (Gerber and Chopin 2015) for B resident SVM or
 * LGSSM chains, as the estimate of PMMH.  The particles are sorted by state before each resampling, and the N (resampling,
 * move) pairs of a timestep are one randomised Sobol' point set in [0, 1)^2: with a_i = bitreverse32(i) and b_i the second
 * Sobol' coordinate of index i (the XOR over the set bits k of i of V_k, V_0 = 0x80000000, V_{k+1} = V_k ^ (V_k >> 1)), row
 * r = 0 .. T (row 0 serves x_{-1}, row t+1 step t) draws four words (s_a, s_b, l_a, l_b) once and point i of the row is
 * u = ((((a_i ^ s_a) << 20) | (l_a >> 12)) + 0.5) 2^-52, v likewise from b_i, s_b, l_b -- a random digital shift, which keeps
 * the net and makes every point uniform, so the estimate is unbiased and PMMH on it exact for every N.  x_{-1}^i = prior_mean
 * + sqrt(prior_var) Phi^-1(v_i) of row 0.  Step 0: the particles in ascending order of (x_{-1}, index), the child at position
 * k moves from the parent at position k.  Step t >= 1: the particles in ascending order of (state, index), the CDF of their
 * weights W in that order, and the child at position k takes the smallest j with cdf[j] > u_(k) W (at most N-1), u_(k) =
 * (k + delta) / N the k-th smallest u of row t+1.  Every child moves by the prior kernel with z = Phi^-1(v) of the point whose
 * u has rank k, i(k) = bitreverse_m(k ^ (s_a >> (32 - m))), N = 2^m.
 *
 * pfg_sqmc_problem: one chain's filter.  Every pointer is DEVICE memory.  theta: the raw row (PFG_MAX_THETA doubles); y [T];
 * out: PFG_OUT_DOUBLES doubles, out[4] = sum_t log((1 / N) sum_i w_t^i) with the Gaussian constants of the emission density,
 * every other slot 0.  A weight sum that is zero or not finite: out[4] = -inf (pfg_pmmh_accept_device rejects it).  A
 * descriptor with a NULL array (the trace pointers may be NULL), T < 1, N not a power of two, N < 2 or above the launch's
 * n_max, or a prior variance that is not positive: a NaN record and no other store.  The trace pointers are read by a
 * traced launch only: trace_anc [T][N] each child's parent in sorted coordinates (row 0: -1), trace_ll [T] the per-step
 * increments of out[4], trace_z [T+1][N] the normals as used (row 0 by particle, the later rows by child).
 *
 * pfg_sqmc_device: one workgroup per problem, 64 x 2 (one wave) for n_max <= 128, 256 x 4 up to 1024; `problems` is a DEVICE
 * array of B records, n_max >= every record's N.  The shifts: Philox4x32-10 keyed by (seed, chain_offset + b, *step_ctr,
 * row) under a tag of their own (csrc/pfg_sqmc.hip); *step_ctr is read, not incremented.  traced != 0 runs the twin that
 * honours the trace pointers; both write the same out, bit for bit.  PFG_ERR_UNSUPPORTED: GARCH, a dtype other than PFG_F64,
 * n_max > 1024 or < 2; PFG_ERR_INVALID: a bad model id, B < 0, problems == NULL. */
typedef struct pfg_sqmc_problem {
    const double *theta;
    const double *y;
    double *out;
    int32_t *trace_anc;
    double *trace_ll;
    double *trace_z;
    double prior_mean, prior_var;
    int32_t T, N;
} pfg_sqmc_problem;
int pfg_sqmc_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_sqmc_problem *problems, uint64_t seed,
                    uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced);

/* EXTENSION (not in the reference): the two sorted filters with a score beside out[4] -- the drift of particle MALA on
 * correlated or quasi-Monte Carlo chains (Nemeth, Sherlock and Fearnhead 2016, on the filters above).  The same kernels,
 * instantiated with the score statistic: the same descriptors, keys, draws, sort, resampling, U' (pfg_cpm_score_device) and
 * trace arrays, and out[4] is bit for bit what pfg_cpm_device / pfg_sqmc_device write for the same arguments.  Every particle
 * carries alpha [H] (H = 3 SVM: [LRinv, LQinv, A]; 4 LGSSM: [LRinv, LQinv, C, A]) through the sort and the gather:
 *   t = 0    alpha_i = add(x_{-1}^i -> x_0^i, y_0), the complete-data score increment of the move from x_{-1} (under
 *            pfg_sqmc_score_device the parent at sorted position k)
 *   t >= 1   alpha_r = lambduh alpha_parent(r) + (1 - lambduh) S_{t-1} + add(x_parent -> x_r, y_t), S_{t-1} = sum_i w_i alpha_i /
 *            sum_i w_i under the weights the CDF of step t is built from.  lambduh == 1 is Poyiadjis' O(N) recursion and does
 *            not read S; lambduh < 1 is the fixed-lag shrinkage of Nemeth, Sherlock and Fearnhead.
 *   out      out[h] = S_{T-1}[h] for h < H, 0 for H <= h < 4 and for slots 5 .. 7; a degenerate chain: out[4] = -inf and every
 *            other slot 0; a refused descriptor: a NaN record and no other store, as above.
 * Shapes as above; the 256 x 4 units keep H * 1024 more doubles in LDS (alpha by particle).  Errors as pfg_cpm_device /
 * pfg_sqmc_device, and PFG_ERR_INVALID for lambduh outside (0, 1]. */
int pfg_cpm_score_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_cpm_problem *problems, double rho,
                         double lambduh, uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream,
                         int traced);
int pfg_sqmc_score_device(pfg_ctx *ctx, int model, int dtype, int n_max, int B, const pfg_sqmc_problem *problems, double lambduh,
                          uint64_t seed, uint64_t chain_offset, const uint64_t *step_ctr, void *hip_stream, int traced);

/* EXTENSION (not in the reference): density-tempered SMC over B resident PMMH chains (Del Moral, Doucet and Jasra 2006; Duan
 * and Fulop 2015).  The chains are one interacting population that is carried from a Gaussian q0 -- the product over the
 * slots a PMMH proposal moves of N(q0_mean[j], q0_sd[j]^2), two DEVICE arrays of PFG_MAX_THETA doubles -- to the posterior
 * through temperatures phi in [0, 1], the target at phi being q0(theta)^(1 - phi) (exp(logprior(theta)) p-hat(y | theta))^phi on
 * PMMH's support.  A stage is: pfg_smc_logtarget_device, pfg_smc_temper_device, pfg_smc_gather_device,
 * pfg_smc_scale_device, then PMMH steps (pfg_pmmh_propose_device, the launch, pfg_smc_accept_device).  Everything is f64 and
 * a pure function of the inputs and (seed, stage); all arrays are DEVICE memory.
 *
 * pfg_smc_logtarget_device: h[b] = (ll_cur[b] + logprior(theta[b])) - log q0(theta[b]), log q0(theta) = sum over the slots
 * that move of -(theta_j - m_j)^2 / (2 s_j^2) - log(s_j sqrt(2 pi)).
 *
 * pfg_smc_temper_device: one workgroup of 1024 threads over h [B], 2 <= B <= 2^20 (anything else: PFG_ERR_INVALID, no
 * launch).  With w_i(d) = exp(d (h_i - h_max)) (0 for h_i = -inf) and ESS(d) = (sum w_i)^2 / sum w_i^2: delta = 1 - *phi if
 * ESS(1 - *phi) >= ess_target B, otherwise the lower end of 60 rounds of bisection on [0, 1 - *phi].  result
 * [PFG_SMC_RESULT_DOUBLES] = {phi' = *phi + delta (1 exactly in the first case), delta, the evidence increment
 * delta h_max + log(W / B), ESS(delta), the uniform u, W = cdf[B - 1], h_max, 0}; *phi = phi'; cdf (scratch,
 * pfg_smc_scratch_bytes(B) bytes) the running sum of w(delta) in chain order; parent[r] the smallest j with
 * cdf[j] > ((r + u) / B) W, B - 1 when there is none: systematic resampling of the chains on one uniform per stage,
 * u = uniform53 of Philox4x32-10 with counter {stage_lo, stage_hi, 0, 0x534D0001} under seed ^ 0x534D4353.  *status = 0, or
 * 1: no h is finite, 2: some h is NaN or +inf, 4: delta ended at exactly 0, 8: *phi is not in [0, 1) -- and then NOTHING
 * but *status is stored.
 *
 * pfg_smc_gather_device: theta[b] = theta[parent[b]], ll[b] = ll[parent[b]] through theta_tmp [B][PFG_MAX_THETA] and ll_tmp
 * [B] (out of place, then copied back: two launches).  A parent outside [0, B) leaves the chain as it is.
 *
 * pfg_smc_scale_device: one workgroup of 1024 threads; for every slot j whose bit is set in `slots`, scale[j] = factor sd_j,
 * sd_j = sqrt(sum_b (theta[b][j] - mean_j)^2 / B) by two passes summed in a fixed order, unless sd_j is 0 or not finite:
 * then, as for every other slot, scale[j] stays.
 *
 * pfg_smc_accept_device: pfg_pmmh_accept_device's step (never init) at the temperature *phi,
 *   log alpha = *phi ((out[4] + logprior(theta_prop)) - (ll_cur + logprior(theta)))
 *               + (1 - *phi) (log q0(theta_prop) - log q0(theta)),
 * on PMMH's uniform and with PMMH's commit; log_alpha (may be NULL) receives every chain's log alpha.  At *phi = 1 the
 * decision, theta, ll_cur and n_accept are pfg_pmmh_accept_device's bit for bit.  *step_ctr is incremented afterwards. */
#define PFG_SMC_RESULT_DOUBLES 8
int64_t pfg_smc_scratch_bytes(int B);           /* the CDF, rounded up to 256; -1: B < 2 or B > 2^20 */
int pfg_smc_logtarget_device(pfg_ctx *ctx, int model, int B, const double *theta, const double *ll_cur,
                             const pfg_prior_hyper *hyper, const double *q0_mean, const double *q0_sd, double *h,
                             void *hip_stream);
int pfg_smc_temper_device(pfg_ctx *ctx, int B, const double *h, double *phi, double ess_target, uint64_t seed,
                          uint64_t stage, double *result, int32_t *status, int32_t *parent, void *scratch,
                          void *hip_stream);
int pfg_smc_gather_device(pfg_ctx *ctx, int B, const int32_t *parent, double *theta, double *ll, double *theta_tmp,
                          double *ll_tmp, void *hip_stream);
int pfg_smc_scale_device(pfg_ctx *ctx, int B, const double *theta, uint32_t slots, double factor, double *scale,
                         void *hip_stream);
int pfg_smc_accept_device(pfg_ctx *ctx, int model, int B, double *theta, const double *theta_prop, const int32_t *valid,
                          const double *outs, double *ll_cur, uint64_t *n_accept, const pfg_prior_hyper *hyper,
                          const double *q0_mean, const double *q0_sd, const double *phi, double *log_alpha, uint64_t seed,
                          uint64_t chain_offset, uint64_t *step_ctr, void *hip_stream);

/* EXTENSION (not in the reference): SMC^2 over B resident PMMH chains (Chopin, Jacob and Papaspiliopoulos 2013; Fulop and Li
 * 2013) -- the sequential form of the population above.  The chains take the observations chunk by chunk; every chain keeps
 * its filter's particle system as one row of row_doubles = N (NS + 1) doubles, x [N][NS] then logw [N] (what final_x /
 * final_logw of a pfg_dev_problem write and init_x / init_logw read), a running log-weight and the sum of its chunks'
 * estimates.  A stage is: the warm-started launch on the chunk, pfg_seq_reweight_device, and where that resampled
 * pfg_seq_gather_device, pfg_smc_scale_device and PMMH steps on the prefix (pfg_pmmh_propose_device, a launch from scratch,
 * pfg_pmmh_accept_device, pfg_seq_adopt_device).  Everything is f64 and a pure function of the inputs and (seed, stage); all
 * arrays are DEVICE memory.
 *
 * pfg_seq_reweight_device: one workgroup of 1024 threads over logw [B] (in and out) and incr[b * incr_stride] (the chunk's
 * estimates: column 4 of the records with stride PFG_OUT_DOUBLES, or any array with stride 1).  v_b = (logw_b - max logw) +
 * incr_b, a logw or incr of -inf being a zero weight; record [PFG_SEQ_RECORD_DOUBLES] = {the evidence increment v_max +
 * log(sum e^(v_b - v_max) / sum e^(logw_b - max logw)), ESS = (sum e^(v - v_max))^2 / sum e^(2 (v - v_max)), resampled (0 | 1),
 * the uniform u, v_max, W = sum e^(v - v_max), max logw, 0}.  ESS < ess_target B: parent[r] the smallest j with cdf[j] >
 * ((r + u) / B) W, B - 1 when there is none (cdf, pfg_smc_scratch_bytes(B) bytes of scratch: the running sum of e^(v - v_max) in
 * chain order; u keyed as pfg_smc_temper_device keys its own) and logw = 0.  Otherwise parent = identity and logw = v - v_max.
 * *status = 0, or 1: no v is finite, 2: some logw or incr is NaN or +inf, 4: B is not in 2 .. 2^20 -- and then NOTHING but
 * *status is stored (the call itself returns PFG_OK: the status word is the population's channel).  PFG_ERR_INVALID: a NULL
 * argument, incr_stride < 0, ess_target outside (0, 1] (1 resamples whenever the weights are not all equal).
 *
 * pfg_seq_gather_device: row b of dst = row parent[b] of src (src != dst, [B][row_doubles] each), one workgroup per row, 16
 * bytes per lane and access; theta[b] = theta[parent[b]] and ll[b] = ll[parent[b]] through theta_tmp [B][PFG_MAX_THETA] and
 * ll_tmp [B] as pfg_smc_gather_device moves them.  A parent outside [0, B) leaves the chain as it is (its own row is copied).
 *
 * pfg_seq_adopt_device: one workgroup per chain, after pfg_pmmh_accept_device: if (n_accept[b] != seen[b]) { row b of cur =
 * row b of fresh; seen[b] = n_accept[b]; } -- pfg_cpm_commit_device's rule with a copy in place of the selector flip; every
 * other row of cur is untouched.
 *
 * gather and adopt: PFG_ERR_INVALID for B outside 2 .. 2^20, row_doubles < 1 or B row_doubles > 2^40, a NULL argument, or the
 * two row arrays being the same. */
#define PFG_SEQ_RECORD_DOUBLES 8
int pfg_seq_reweight_device(pfg_ctx *ctx, int B, double *logw, const double *incr, int64_t incr_stride, double ess_target,
                            uint64_t seed, uint64_t stage, double *record, int32_t *status, int32_t *parent, void *scratch,
                            void *hip_stream);
int pfg_seq_gather_device(pfg_ctx *ctx, int B, const int32_t *parent, int64_t row_doubles, const double *src, double *dst,
                          double *theta, double *theta_tmp, double *ll, double *ll_tmp, void *hip_stream);
int pfg_seq_adopt_device(pfg_ctx *ctx, int B, const uint64_t *n_accept, uint64_t *seen, int64_t row_doubles, double *cur,
                         const double *fresh, void *hip_stream);

/* Inverse-multiquadric kernel Stein discrepancy of K points x[K][d] with score estimates
 * g[K][d] (HOST pointers, d <= 8): sqrt(sum_{i,j} k0(x_i,x_j)) / K for
 * k(x,y) = (c^2 + |x-y|^2)^(-beta) -- IMQ_KSD of sgmcmc_ssm/trace_metric_functions.py:20-81
 * (the O(K^2) pass of the KSD evaluation, nonlinear_ssm_pf_experiment_scripts/svm/driver.py:906-1090). */
int pfg_imq_ksd(pfg_ctx *ctx, int K, int d, const double *x, const double *g, double c, double beta,
                double *ksd_out);

/* Host helper of the REPLAY path (no GPU involved): NumPy's legacy RandomState stream of one particle-filter
 * window, bit-identical to
 *     z0 = rs.normal(size=N);  for t in range(T): u[t] = rs.random_sample(N); z[t] = rs.normal(size=N)
 * -- the order in which the reference's filter consumes the global np.random state
 * (particle_filters/pf.py:26-38, kernels.py:83-100) -- generated natively (MT19937 + polar method in one tight
 * loop, the sqrt/log of the accepted pairs on `threads` worker threads; 0 = the default, 2).
 * The state is RandomState.get_state()'s (key[624], pos, has_gauss, cached_gaussian), advanced in place. */
int pfg_legacy_streams(uint32_t *key, int32_t *pos, int32_t *has_gauss, double *gauss, int N, int T,
                       double *z0, double *u, double *z, int threads);

/* Page-lock a caller-owned host buffer (hipHostRegister) so that pfg_run_batch stages it with a DMA straight
 * from where it lies: an input array of a pfg_problem that falls inside a registered range skips the pack copy
 * into the library's own pinned arena (the 2 x 8 MB replay streams of a T = N = 1000 window: 1.2 ms of a 5.6 ms
 * step).  The buffer must stay allocated and registered until pfg_host_unregister; registering a range twice
 * is an error.  Returns PFG_OK or a negative code (no message channel: there is no context here). */
int pfg_host_register(void *ptr, size_t bytes);
int pfg_host_unregister(void *ptr);

#ifdef __cplusplus
}
#endif
#endif /* PFGRAD_H */
