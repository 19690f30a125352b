// libpfgrad device code: what pf_reg_kernel is at compile time.  Its build switches, every switch derived from the template arguments
// (RegTraits) and the ONE description of its LDS block (RegTraits::layout): the host's sizing and the kernel's pointers both come from it.
#pragma once
#include "pfg_models.hpp"

namespace pfg {

// ---- Build switches.  Each -DPFG_OPT_x=0 / -DPFG_OCCx=n rebuilds without one measure for A/B timing; the defaults are
// production.  What was measured and NOT kept: DESIGN.md, section 4.1, "Measured and not kept".
// PFG_OPT_PADSTATE: state arrays x[NS][.], stats[H][.] of a FAST layout are NL + pad elements apart (pad = 8 bytes).  With a stride of
// exactly NL = NT * PPT elements (a multiple of 512 bytes) the compiler fuses the gathers / stores of one particle's
// entries in two arrays into ds_read2st64_b64 / ds_write2st64_b64, which the LDS serves at HALF the rate of two
// ds_read_b64 (MI355X_MICROARCH.md, LDS table: 8 cycles per wave-instruction against 2 + 2; with the random
// addresses of a gather about 24 against 14).  A stride that is no multiple of 512 bytes keeps them apart.
// Device-generator kernels only: they are bound by LDS-array cycles (c2: 51.4 -> 47.0 ms with the pad).  The REPLAY
// kernels wait on their HBM streams instead and run 17 % SLOWER with twice the LDS instructions (768 windows of
// T = N = 1000: 6.8 ms fused, 8.0 ms padded), so they keep the fused form.  -DPFG_OPT_PADSTATE=0 restores it everywhere (A/B).
#ifndef PFG_OPT_PADSTATE
#define PFG_OPT_PADSTATE 1
#endif
// PFG_OCC64: one-wave workgroups (NT = 64): LDS admits many windows per CU, the register budget decides how many waves
// a SIMD holds (-DPFG_OCC64=n for A/B builds)
#ifndef PFG_OCC64
#define PFG_OCC64 4
#endif
// PFG_OCC4: the device-generator SVM single-buffer workgroup needs 39.5 KB of LDS with the 32-bit CDF:
// FOUR workgroups fit a CU if the kernel stays within 128 VGPRs (34 spilled registers; measured
// +3.6 % workgroups per ms over occupancy 3).  -DPFG_OCC4=0 restores occupancy 3.
#ifndef PFG_OCC4
#define PFG_OCC4 1
#endif
// PFG_OPT_SORTED1024 (SORTED: the 1024-thread device-generator variant, N <= 4096): the N resampling uniforms of a timestep are drawn
// as the ORDER STATISTICS of N i.i.d. uniforms -- exponential spacings e_r = -log u_r, U_(r) = sum_{q<=r} e_q /
// sum_{q<=N+1} e_q, by a second prefix scan that rides on the weight scan's barriers -- and child r takes U_(r)
// (multinomial resampling does not care which child gets which uniform; children are exchangeable).  CDF and
// ranks both run in thread-major order, so neighbouring lanes search neighbouring keys (coherent probes: LDS
// broadcasts instead of bank conflicts) and gather neighbouring parents.  One such workgroup fills a CU's LDS, so
// nothing else hides its LDS stalls: the knock-out with evenly spaced words was worth 15 % there (4 % on the
// 256-thread SVM kernel, where the second scan costs more than that).  -DPFG_OPT_SORTED1024=0 restores i.i.d. words.
#ifndef PFG_OPT_SORTED1024
#define PFG_OPT_SORTED1024 1
#endif
// PFG_OPT_PRIO (PRIO): wave issue priority (s_setprio) by phase.  A timestep alternates between phases that are mostly LDS round
// trips (E search, F gather) and phases that are mostly VALU work (A-D, G, H); the arbiter of a SIMD otherwise picks by age.  256 x
// 4, four workgroups per CU in different phases: the VALU phases at priority 2 and E, F at 0 -- a wave that is about to wait for the
// LDS anyway gives way -- 45.6 -> 44.8 ms per bench launch (-1.9 %; the same with 3 instead of 2; nothing if only G, H are raised).
// 1024 x 4, ONE workgroup per CU whose 16 waves are in the same phase: the other way round (E, F at 2: the waves that reach the
// search first get their probes out) 11.26 -> 11.03 ms (-2.0 %), and +0.4 % with the 256 x 4 setting.  512 x 2 (GARCH) and the
// one-wave kernels: 0 ... +4 % with either, so none (profiles/r03_ab_wave_priority.txt).  The REPLAY instantiation of 256 x 4 (768
// windows, three per CU): 5.85 -> 5.26 ms with the 256 x 4 setting (5.52 with the opposite one).  -DPFG_OPT_PRIO=0 builds without.
#ifndef PFG_OPT_PRIO
#define PFG_OPT_PRIO 1
#endif
// PFG_OPT_PAIRSTATE (PAIRED; round 4; the device-generator production kernels in fp64 with an even record length: SVM, GARCH): the state
// is stored as (NS + H) / 2 arrays of 16-byte PAIRS {component 2p, component 2p + 1} instead of NS + H arrays of
// doubles.  The parent gathers -- 16 random ds_read_b64 per lane-timestep of the SVM kernel, 56 % of its LDS
// bank-conflict cycles (profiles/r04_lds_conflict_split.txt) -- become 8 ds_read_b128, which use the full width of
// the LDS; the children's stores stay lane-contiguous (ds_write_b128).  -DPFG_OPT_PAIRSTATE=0 restores the arrays.
#ifndef PFG_OPT_PAIRSTATE
#define PFG_OPT_PAIRSTATE 1
#endif
//  PFG_OPT_STALESHIFT  (SVM prior kernel, 256 x 4 on one buffer, fp64: STALE) the shift s of exp(lw - s) is the exact
//                  maximum of the PREVIOUS step instead of this step's: the max reduction needs no barrier of its own (three
//                  s_barrier per timestep instead of four).  Any shift gives the same normalised weights and the same
//                  s + log(W/N) up to rounding; it only has to keep exp in range: a wave-uniform guard |m_t - s| <= 512
//                  sends a gross outlier (NaN, +-inf too) to a cold path that recomputes the log-weights from the
//                  published states and redoes exp, sums and scan with s = m_t (for the bounds).
//                  Hazards: the maxima of step t are written to red_maxf before barrier 2 of step t and read between
//                  its barriers 2 and 3; those of step t + 1 are written behind barriers 3 and 4 of step t, when every
//                  wave is done with that read.  The retry's own two barriers order its rewrite of red_scan / red_S
//                  behind every wave's first read of them.  The state, red_scan and the CDF keep the barriers they have.
//  PFG_OPT_GATHERADDR  (the same kernel: GADDR) the search's final byte offset becomes the gather's byte address in eight
//                  instructions per particle instead of ten.
//  Both: c2 kernel 42.75 -> 41.84 ms (-2.1 %; profiles/r05_ab_stale_shift.txt).
#ifndef PFG_OPT_STALESHIFT
#define PFG_OPT_STALESHIFT 1
#endif
#ifndef PFG_OPT_GATHERADDR
#define PFG_OPT_GATHERADDR 1
#endif
//  The same two STALE instantiations (TRACE twins), three instruction-count measures that move no barrier:
//  PFG_OPT_SUMSHIFT    (SUMSHIFT) no max reduction in the T-loop..  The shift of the next step comes from the scan total W_t
//                  = sum exp(lw_t - s_t) that the CDF needs anyway: s_{t+1} = (float)(s_t + ln2 * e) with W_t = f 2^e, f in
//                  [0.5, 1) (the binary exponent, read from W's high word with scalar integer instructions).  s_t + ln W_t
//                  is the step's log-sum-exp, in [max, max + ln 1024], and absolute: it does not drift with s_t.  The
//                  range guard sits on W: accepted iff 2^-728 <= W_t < 2^728 (one unsigned compare of the high word; NaN,
//                  +-inf, 0, denormals and negatives fail it), so the true maximum of an accepted step lies in
//                  [s_t - 728 ln2 - ln 1024, s_t + 728 ln2) = [s_t - 511.6, s_t + 504.7): stricter than |m_t - s_t| <= 512.
//                  The t = 0 prologue keeps its exact maximum; the cold retry now forms the exact block maximum itself
//                  (wave_max, red_maxf, one more barrier).  Phase A, the red_maxf write before barrier 2 and its read-back
//                  behind it are gone.
//  PFG_OPT_SHIFTFOLD   (SHIFTFOLD) the next shift is known behind barrier 2, before phase G: the children's log-weights are
//                  born as lw - s_next (k0 - s_next in svm_logw, one wave-uniform add per timestep) and cross the loop
//                  edge that way; phase B exponentiates them without its four v_add_f64.  Traces and final_logw add the
//                  shift back; the retry recomputes unshifted log-weights as before.
//  PFG_OPT_SCOREDZ     (SCOREDZ) particle_step, SVM score: dx = x1 - A xp IS iLQinv z, so x1 = fma(A, xp, dz), add[1] =
//                  fma(-dz, z, iLQinv), add[2] = ((Qinv iLQinv) z) xp: two fp64 instructions per particle less.
//  A/B (profiles/r06_ab_sum_shift.txt; c2 kernel ms per 12288 chains, medians of five interleaved processes per library, the
//  parent's own max - min 0.13): parent 41.68; SCOREDZ alone 41.17 (-1.2 %, 3.8 x the spread): ON -- its outputs are the
//  parent's to rounding (120 bench steps, 12288 chains: every chain within 5e-11).  SUMSHIFT alone 40.28 (-3.4 %), with
//  SCOREDZ 39.75 (-4.8 %): measured and NOT kept, OFF -- another shift moves every argument of the table exp, whose cubic's
//  error (2e-12, a function of the reduced argument) then differs per particle: the normalised weights move at 1e-12, an
//  ancestor flips about once in ten launches of 12288 chains, and after 120 bench steps 14 of the 12288 chains had left
//  the parent's trajectory (same distribution, not the same numbers).  SHIFTFOLD alone 41.80 (+0.3 %), on top of the other
//  two +0.5 %: NOT kept, OFF.  Default build (SCOREDZ): 128 VGPRs, no spill, occupancy 4; the traced twin 1 spilled VGPR (the
//  GADDR trace index is stored behind the search instead of being held across phases F-H).
#ifndef PFG_OPT_SUMSHIFT
#define PFG_OPT_SUMSHIFT 0
#endif
#ifndef PFG_OPT_SHIFTFOLD
#define PFG_OPT_SHIFTFOLD 0
#endif
#ifndef PFG_OPT_SCOREDZ
#define PFG_OPT_SCOREDZ 1
#endif
//  PFG_OPT_RAWSCORE    (RAWSCORE; the same two STALE instantiations) the Poyiadjis O(N) score of a `raw` window -- plain (no filter,
//                  lambda = 1) with stat = score, both window-uniform and fixed for the whole T-loop -- is carried along the
//                  genealogy as RAW SUMS and scaled where a statistic leaves the kernel.  With normalised weights sum_i W_i (a +
//                  b r_i) = a + b sum_i W_i r_i, and of the score's terms  w_t (iLRinv - y^2 LRinv e),  w_t iLQinv (1 - z^2),
//                  w_t (Qinv iLQinv) z xp  the constants iLRinv, iLQinv, the factors LRinv, iLQinv, Qinv iLQinv and w_t are the
//                  same for every particle of the window.  The three statistic slots of a raw window's LDS records hold
//                    r0 += (w_t y^2) e,   r1 += (w_t z) z,   r2 += (w_t z) xp       (w_t y^2 wave-uniform; zw = w_t z)
//                  and Cw += w_t (uniform; on the steps that add a statistic) rides in scalar registers:
//                    s0 = iLRinv Cw - LRinv r0,   s1 = iLQinv (Cw - r1),   s2 = (Qinv iLQinv) r2          (raw_score_out)
//                  on P.trace_stats (per step, with that step's Cw), P.final_stats and the three uniform sums S[h] before P.out;
//                  P.init_stats enters as r0 = -s0 / LRinv, r1 = -s1 / iLQinv, r2 = s2 / (Qinv iLQinv) with Cw = 0 (raw_score_in:
//                  converted, not sent down the general path -- a fallback would keep one more children block in the loop body).
//                  One multiply and three fma per particle instead of seven fp64 instructions; x', the log-weight and everything on
//                  the weight path are instruction for instruction what they were.  Record layout, pairs, gathers and stores do not
//                  change; every other window (lambda != 1, filter, stat suff / none) keeps the general path in the original scale.
//                  Accuracy: s1 = iLQinv (Cw - r1) cancels -- r1 is about Cw +- sqrt(2 Cw) -- so it loses about log10(sqrt(Cw / 2))
//                  digits (1.3 at Cw = 1000); Cw grows with the window length, the window weights and every warm start that
//                  carries statistics on.  Harmless at T = 1000; a caller with windows orders of magnitude longer builds with
//                  -DPFG_OPT_RAWSCORE=0.
//                  Measured and not kept (no longer in the source): a children block of its own for steps with w_t == 1, without the
//                  multiply zw = w_t z: -0.1 ... -0.3 % against the general form, under its gate.
//  A/B: profiles/r07_ab_raw_score.txt.
#ifndef PFG_OPT_RAWSCORE
#define PFG_OPT_RAWSCORE 1
#endif
//  The eight hot exp of a lane-timestep (the same two STALE instantiations: four in phase B, four in the particle step of phase G), each
//  one ds_read_b64 of e2[k & 127] at a per-lane random index -- 128 entries fold onto 32 bank pairs, so the 32 lanes the LDS serves at
//  a time collide like 32 balls in 32 bins.  What they cost is measured with PFG_EXP_TABLANE (profiles/r08_lds_table_split.txt).
//  PFG_OPT_EXPTABMEM   (TABMEM_B = bit 0, TABMEM_G = bit 1; 3 = both) those lookups read a copy of the table in global memory
//                  (pfg::ExpTabMem: 1 KB that lives in the CU's vector L1) with global_load_dwordx2, scalar base + 32-bit lane offset:
//                  they leave the LDS array and the lgkmcnt queue for the idle vector-memory pipe and wait on vmcnt.  The same 128
//                  doubles and the same instructions on them: outputs are bitwise the LDS form's.  The LDS copy stays for the cold
//                  paths (prologue, stale-shift retry, log-likelihood flush).
//  PFG_OPT_EXPMAGIC    (EXPMAGIC) the same lookups reduce their argument with the magic-number form (exp_tab_hot, PFG_HOT_MAGIC): two
//                  fp64-class instructions instead of three per exp, and the table address one instruction earlier.
//  A/B, gates and verdicts: profiles/r08_ab_exp_table.txt.
#ifndef PFG_OPT_EXPTABMEM
#define PFG_OPT_EXPTABMEM 0
#endif
#ifndef PFG_OPT_EXPMAGIC
#define PFG_OPT_EXPMAGIC 1
#endif
// PFG_OPT_N2SKIP (the O(N^2) instantiations, MODE_N2): the backward sweep over all parents is skipped on the steps before t1 of a
// window that starts without init_stats -- its result there is +0.0 exactly, see n2_slots.  -DPFG_OPT_N2SKIP=0 runs every sweep (A/B).
#ifndef PFG_OPT_N2SKIP
#define PFG_OPT_N2SKIP 1
#endif
// TRACE (template parameter of pf_reg_kernel): the instantiation honours the trace_* / rec_* buffers of its
// descriptors (save_all trajectories, recorded generator draws: tests, elementwise statistics).  TRACE = false is
// the production twin of the plain device-generator kernels: the same code with every trace / record test compiled
// out of the T-loop -- each was a scalar load of a descriptor field plus a wait on the critical path of every
// timestep, and their address registers cost spills (measured: -5 % kernel time on BASELINE configs[1], -12 % on
// config 3, -6 % on config 1, -2 % on config 4).  tests/test_gpu_device_replay.py replays the TRACE = true twin from its
// recorded draws and asserts that the TRACE = false twin returns bitwise the same statistics for the same key.
#define PFG_TR(p) (TRACE && (p))
// A/B experiment switches (diagnostic builds only; default = production):
//  PFG_EXP_PLAIN      compile the filter / lambda != 1 / no-statistic cases out (Poyiadjis O(N) score only)
//  PFG_EXP_OWNGATHER  knock-out: every child gathers its own slot (pf_reg_kernel, phase E); no GADDR then
//  PFG_EXP_TABLANE    knock-out: the eight hot exp of the STALE kernels read table entry (tid & 127) -- conflict-free -- instead of
//                     (k & 127); the real index is kept alive, the VALU work is unchanged (NOT a valid sampler; PFG_BENCH_KNOCKOUT)
#ifndef PFG_EXP_PLAIN
#define PFG_EXP_PLAIN 0
#endif
#ifdef PFG_EXP_TABLANE
#define PFG_TABLANE_ON 1
#else
#define PFG_TABLANE_ON 0
#endif
#ifdef PFG_EXP_OWNGATHER
#define PFG_GATHERADDR_ON 0
#else
#define PFG_GATHERADDR_ON PFG_OPT_GATHERADDR
#endif
// Device-generator units only (-DPFG_FAST_ALGEBRA; the REPLAY units keep the reference's operation
// order and phase structure).  Each can be switched off for A/B timing (-DPFG_OPT_x=0):
//  PFG_OPT_LAZYLL  the log-likelihood increment  w (m + log(W/N))  used to cost wave 0 an fp64 log and
//                  a division per timestep while the other waves waited at the next barrier; now wave 0
//                  parks (W, m, w) of step t in lane t % 64 and evaluates 64 steps at once (one table log
//                  per lane + one wave sum);
//  PFG_OPT_RCPW    1/W by v_rcp_f64 + two Newton steps instead of the IEEE division sequence;
//  PFG_OPT_SEL32   the 32-bit search's compare + select in the VOP2 forms (NT >= 512: see the search, phase E);
//  PFG_OPT_PIVOTS  (A/B, off; 1024 slots) the three entries the first two levels of every search compare with
//                  (positions 511, 255, 767) are read ONCE per wave and timestep (broadcast reads) and held in
//                  scalar registers: two dependent LDS round trips and eight ds_read per lane-timestep less.
#ifdef PFG_FAST_ALGEBRA
#ifndef PFG_OPT_LAZYLL
#define PFG_OPT_LAZYLL 1
#endif
#ifndef PFG_OPT_RCPW
#define PFG_OPT_RCPW 1
#endif
#ifndef PFG_OPT_SEL32
#define PFG_OPT_SEL32 1
#endif
#ifndef PFG_OPT_PIVOTS
#define PFG_OPT_PIVOTS 0
#endif
#else
#undef PFG_OPT_LAZYLL
#undef PFG_OPT_RCPW
#define PFG_OPT_LAZYLL 0
#define PFG_OPT_RCPW 0
#undef PFG_OPT_SEL32
#define PFG_OPT_SEL32 0
#undef PFG_OPT_PIVOTS
#define PFG_OPT_PIVOTS 0
#endif

// the cdf of a FAST layout is stored at physical index i + (i >> 5): the binary search's power-of-two strides would otherwise
// all hit one LDS bank (measured: 720 conflict cycles per wave-timestep, i.e. all of SQ_LDS_BANK_CONFLICT)
__host__ __device__ __forceinline__ constexpr int cdf_phys(int i) { return i + (i >> 5); }

// Byte offsets of pf_reg_kernel's regions in its dynamic LDS block, in carving order (RegTraits::layout), and what aliases what.
struct RegLdsLayout {
    int NL, NLS;            // particle slots; stride of the state arrays in elements (NL + pad, see PFG_OPT_PADSTATE)
    size_t cdf;             // [NL, padded 33/32 if FAST] f64, or u32 fixed point (BLK); rounded up to 16 bytes
    size_t buf0, buf1;      // state buffers {x[NS][NLS], stats[H][NLS]} of REAL; buf1 == buf0 unless PP
    size_t red_scan;        // [PPT * NW] f64 wave totals of the scan(s).  Alias: [PPT][NW] int counts of the raw-stream reader
    size_t red_max;         // [NW] f64; its first NW floats are red_maxf.  Alias: PaRIS's queue count, one int BEHIND those floats
    size_t red_S;           // [PFG_MAX_STAT * NW] f64 partial statistic sums
    size_t red_W0;          // [8] spare f64: [0] systematic offset, [1] the raw stream's cached Gaussian, [2..3] as two int64 (raw_slots)
    size_t tab;             // LDS math tables (tab_bytes)
    // PaRIS / O(N^2) only (LWL); nothing behind `tab` exists otherwise
    size_t lwL;             // [NL] REAL parents' log-weights, in NL * 8 bytes whatever REAL is
    size_t queue;           // [NL] int children left to the exact fallback.  Alias: queue + wq0 as [N] f64 = one raw-stream call's normals
    size_t wq0, wq1;        // [NL] int each: wave-local work queues.  Alias: wq0 as [PPT][NW] int = pending counts of the ordered rounds
    size_t Jres;            // [NL] int accepted parent of every child of the current backward draw
    size_t total;           // = the end of the last region carved
};

// Every compile-time switch of pf_reg_kernel<MODEL, KERNEL, REAL, NT, PPT, RNG, PP, MODE, ...>, defined once, and its LDS layout.
template <int MODEL, int KERNEL, typename REAL, int NT, int PPT, int RNG, bool PP, int MODE = MODE_PLAIN>
struct RegTraits {
    static constexpr int NS = ModelDims<MODEL>::NS, H = ModelDims<MODEL>::H;
    static constexpr int NW = NT / WAVE, SLOTS = NT * PPT;
    static constexpr bool PARIS = MODE == MODE_PARIS, N2 = MODE == MODE_N2, SYSTEMATIC = MODE == MODE_SYSTEMATIC;
    static constexpr bool STRATIFIED = MODE == MODE_STRATIFIED;     // one uniform per child, (r + U_r) / N: see phase E
    // ESS-triggered resampling (PFG_FLAG_ADAPTIVE_RESAMPLING): a step whose effective sample size is at least tau N keeps
    // every particle where it is -- no CDF, no search, no gather -- and carries its normalised log-weight on
    static constexpr bool ADAPTIVE = MODE == MODE_ADAPTIVE;
    static_assert(!ADAPTIVE || NT / WAVE <= 4, "the per-wave sums of w^2 sit in red_W0[4 .. 4 + NW)");
    static constexpr bool LWL = PARIS || N2;            // the parents' log-weights (and the PaRIS queues) in LDS
    // FAST layout = LDS math tables + sentinel-padded, bank-conflict-free cdf with an unrolled search, NT * PPT particle
    // slots whatever N is (the array stride is a compile-time constant and folds into the ds_read / ds_write immediates).
    // Every variant built today; a layout that is not FAST sizes its arrays by N and spends all LDS on particles.
    static constexpr bool FAST = PP || NT <= 512 || NT == 1024;
    static constexpr bool TAB = FAST;
    // Device RNG only: the CDF is built in THREAD-major order (position tid*PPT + k <-> particle k*NT + tid)..  Multinomial
    // resampling does not care how particles are labelled, and in this order a thread's PPT weights are contiguous: one in-register
    // prefix + ONE wave scan per thread instead of PPT wave scans..  REPLAY keeps the reference's index order (parity). The uniforms
    // carry 32 random bits, so the CDF is kept as 32-bit fixed point (floor(cdf * 2^32)) and searched with the raw generator word:
    // integer compares, half the LDS bytes per probe, no u32 -> f64 conversion of the uniform.
    static constexpr bool BLK = FAST && RNG == PFG_RNG_DEVICE && MODE == MODE_PLAIN && (PPT & (PPT - 1)) == 0;
    static constexpr int LOG_PPT = PPT == 1 ? 0 : (PPT == 2 ? 1 : (PPT == 4 ? 2 : (PPT == 8 ? 3 : 4)));
    static_assert(PPT <= 16, "LOG_PPT covers 1, 2, 4, 8, 16 particles per thread");
    static constexpr bool SORTED = PFG_OPT_SORTED1024 && BLK && NT == 1024 && PPT == 4 && !SYSTEMATIC && NW > 1;   // see PFG_OPT_SORTED1024
    static constexpr int PRIO = !(PFG_OPT_PRIO && (BLK || (RNG == PFG_RNG_REPLAY && MODE == MODE_PLAIN)) && !PP && PPT == 4) ? 0
                                : (NT == 1024 ? 1 : (NT == 256 ? 2 : 0));                                           // see PFG_OPT_PRIO
    static constexpr bool PAIRED = PFG_OPT_PAIRSTATE && BLK && sizeof(REAL) == 8 && ((NS + H) % 2 == 0);            // see PFG_OPT_PAIRSTATE
    // STALE: the previous step's maximum as this step's shift, see PFG_OPT_STALESHIFT
    static constexpr bool STALE = PFG_OPT_STALESHIFT && BLK && MODEL == PFG_MODEL_SVM && KERNEL == PFG_KERNEL_PRIOR && NT == 256 && PPT == 4 &&
                                  !PP && sizeof(REAL) == 8;
    // the three instruction-count measures of the STALE kernels, see PFG_OPT_SUMSHIFT; STEP_TUNE selects particle_step_svm_tuned
    static constexpr bool SUMSHIFT = PFG_OPT_SUMSHIFT && STALE, SHIFTFOLD = PFG_OPT_SHIFTFOLD && STALE, SCOREDZ = PFG_OPT_SCOREDZ && STALE;
    // RAWSCORE: the score of a raw window as raw sums, see PFG_OPT_RAWSCORE
    static constexpr bool RAWSCORE = PFG_OPT_RAWSCORE && STALE;
    // the hot table lookups of phase B / of the particle step (phase G), see PFG_OPT_EXPTABMEM, PFG_OPT_EXPMAGIC, PFG_EXP_TABLANE: HOT_x = exp_tab_hot's bits
#ifdef PFG_HAS_EXP_HOT
    static constexpr bool TABMEM_B = (PFG_OPT_EXPTABMEM & 1) && STALE, TABMEM_G = (PFG_OPT_EXPTABMEM & 2) && STALE, EXPMAGIC = PFG_OPT_EXPMAGIC && STALE;
    static constexpr int HOT_COMMON = (EXPMAGIC ? PFG_HOT_MAGIC : 0) | ((PFG_TABLANE_ON && STALE) ? PFG_HOT_LANE : 0);
    static constexpr int HOT_B = HOT_COMMON | (TABMEM_B ? PFG_HOT_MEM : 0), HOT_G = HOT_COMMON | (TABMEM_G ? PFG_HOT_MEM : 0);
#else
    static constexpr bool TABMEM_B = false, TABMEM_G = false, EXPMAGIC = false;
    static constexpr int HOT_B = 0, HOT_G = 0;
#endif
    static constexpr bool TABMEM = TABMEM_B || TABMEM_G;        // the instantiation reads pfg::ExpTabMem<EXPTAB_TAG>: its launcher fills it first
    static constexpr int EXPTAB_TAG = MODEL * 16 + KERNEL;
    static constexpr int STEP_TUNE = (SHIFTFOLD ? PFG_STEP_SHIFTFOLD : 0) | (SCOREDZ ? PFG_STEP_SCOREDZ : 0) | (RAWSCORE ? PFG_STEP_RAWSCORE : 0) |
                                     (HOT_G << PFG_STEP_HOT_SHIFT);
    // GADDR (256 x 4): search offset -> gather byte address..  rel = 4 x physical CDF position (one pad slot per 32 entries), p4 =
    // rel - 4 (rel * 993 >> 17) = 4 x CDF position p (exact: rel * 993 < 2^23), and (p4 * 1025) & 0x3ff0 = 16 x the particle index
    // ((p & 3) << 8) | (p >> 2): p4 < 2^12, so the copies p4 << 10 and p4 do not overlap -- bits 4..11 of p4 are p >> 2 and bits
    // 12, 13 of p4 << 10 are p & 3..  Clamped to 16 x last it is the byte offset of the parent's first 16-byte pair..  Ancestors
    // are those of the general form, bit for bit (tests/test_gather_address_host.py). (the arithmetic holds for every BLK && PAIRED
    // 256 x 4 kernel; it is switched on where it was timed: the SVM kernel on one buffer, bench config c2, and its TRACE twin)
    static constexpr bool GADDR = PFG_GATHERADDR_ON && BLK && PAIRED && NT == 256 && PPT == 4 && MODEL == PFG_MODEL_SVM && !PP;
    static_assert(!GADDR || 4 * (SLOTS + SLOTS / 32) * 993 < (1 << 23), "GADDR: rel * 993 must fit the 24-bit multiply");
    static constexpr bool LAZYLL = PFG_OPT_LAZYLL && TAB && sizeof(REAL) == 8;
    // LAZYLL in an instantiation without a production twin (systematic included: its one TRACE = true instantiation serves
    // production launches too): tracing the running log-likelihood must not move the flushes
    static constexpr bool TWINLESS_LL = STRATIFIED || N2 || ADAPTIVE || PARIS || SYSTEMATIC;
    static constexpr bool PIVOTS = PFG_OPT_PIVOTS && SLOTS == 1024;
    static constexpr bool RAWCAP = MODE == MODE_PARIS && RNG == PFG_RNG_REPLAY;     // PaRIS on the window's raw np.random stream

    // waves per SIMD the register allocator should aim for: what LDS lets a CU hold anyway.
    // 256x4 fp64: ping-pong state is 80 KB/workgroup -> 2 workgroups (2 waves/SIMD); the single
    // buffer is 50 KB -> 3, which is worth a few spilled registers (measured +15 %).
    // 4096 slots in 512 / 256 threads (A/B of round 3, no longer built: see the variant table in pfg_plan.hip): ONE workgroup per CU
    static constexpr bool OCC_LDS4096 = SLOTS == 4096 && NT < 1024;
    // GARCH fp64 single buffer: six state arrays = 56.8 KB of LDS -> two workgroups per CU; give the allocator the 256 VGPRs (168 -> 32 spills)
    static constexpr bool OCC_TWO = MODEL == PFG_MODEL_GARCH && sizeof(REAL) == 8 && NT == 256 && PPT == 4 && !PP;
    static constexpr bool OCC_DEV4 = PFG_OCC4 && MODEL == PFG_MODEL_SVM && NT == 256 && PPT == 4 && !PP && RNG == PFG_RNG_DEVICE && MODE == MODE_PLAIN;  // see PFG_OCC4
    static constexpr int OCC_MAX = OCC_TWO ? 2 : OCC_LDS4096 ? (NT == 512 ? 2 : 1) : NT == 64 ? PFG_OCC64
                                   : (NT >= 512 || PPT == 1 || OCC_DEV4) ? 4 : ((PP && sizeof(REAL) == 8) ? 2 : 3);
    static constexpr int OCC_MIN = OCC_TWO ? 2 : OCC_LDS4096 ? (NT == 512 ? 2 : 1)
                                   : NT == 512 ? 4        // two 8-wave workgroups per CU
                                   : OCC_DEV4 ? 4 : ((NT == 256 && PPT == 4 && !PP) ? 3 : 1);

    // element index of component d of particle i in a state buffer of stride NLS
    __device__ __forceinline__ static size_t sidx(int NLS, int d, int i) {
        return PAIRED ? (size_t)(d >> 1) * (2 * (size_t)NLS) + 2 * (size_t)i + (size_t)(d & 1) : (size_t)d * NLS + (size_t)i;
    }

    // The LDS block; KERNEL does not enter and N only where the layout is not FAST.  The host evaluates this in a unit built
    // without PFG_FAST_ALGEBRA (the largest math tables any build of the kernel units carries): see reg_lds in pfg_plan.hip.
    static constexpr int RED_SCAN = PPT * NW, RED_MAX = NW, RED_S = PFG_MAX_STAT * NW, RED_W0 = 8;   // doubles of reduction scratch
    static_assert(sizeof(int) * (NW + 1) <= sizeof(double) * RED_MAX, "the queue count fits behind red_maxf");
    __host__ __device__ static constexpr RegLdsLayout layout(int N) {
        RegLdsLayout L = {};
        L.NL = FAST ? SLOTS : (N + WAVE - 1) / WAVE * WAVE;
        L.NLS = L.NL + ((PFG_OPT_PADSTATE && FAST && RNG == PFG_RNG_DEVICE) ? (int)(8 / sizeof(REAL)) : 0);
        const size_t NL = (size_t)L.NL, NC = FAST ? NL + NL / 32 : NL;
        const size_t bufsz = (size_t)L.NLS * (NS + H) * sizeof(REAL);
        size_t at = 0;
        auto carve = [&at](size_t bytes) { const size_t o = at; at += bytes; return o; };
        L.cdf = carve((NC * (BLK ? 4 : 8) + 15) / 16 * 16);
        L.buf0 = carve(bufsz);
        L.buf1 = PP ? carve(bufsz) : L.buf0;
        L.red_scan = carve(8 * (size_t)RED_SCAN);
        L.red_max = carve(8 * (size_t)RED_MAX);
        L.red_S = carve(8 * (size_t)RED_S);
        L.red_W0 = carve(8 * (size_t)RED_W0);
        L.tab = carve(tab_bytes<REAL, RNG, TAB>());
        L.lwL = carve(LWL ? NL * 8 : 0);
        L.queue = carve(LWL ? NL * 4 : 0);
        L.wq0 = carve(LWL ? NL * 4 : 0);
        L.wq1 = carve(LWL ? NL * 4 : 0);
        L.Jres = carve(LWL ? NL * 4 : 0);
        L.total = at;
        return L;
    }
};

// the kernel's pointer to one region; the offsets of a FAST layout are compile-time constants (N does not enter)
template <typename T, class TR, size_t RegLdsLayout::*REGION>
__device__ __forceinline__ T *reg_lds_ptr(unsigned char *smem, int N) {
    constexpr RegLdsLayout F = TR::layout(0);
    return reinterpret_cast<T *>(smem + (TR::FAST ? F.*REGION : TR::layout(N).*REGION));
}

template <int MODEL, typename REAL, int NT, int PPT, int RNG, bool PP, int MODE = 0>
__host__ __device__ inline size_t reg_kernel_lds_bytes(int N) {
    return RegTraits<MODEL, PFG_KERNEL_PRIOR, REAL, NT, PPT, RNG, PP, MODE>::layout(N).total;
}

}  // namespace pfg
