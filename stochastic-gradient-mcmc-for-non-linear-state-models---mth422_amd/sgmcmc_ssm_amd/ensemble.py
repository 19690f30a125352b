"""ChainEnsemble: many independent SGLD / SGHMC / SGRLD / Gibbs / PMMH / pMALA / particle Gibbs chains resident on one MI355X.

The reference runs one chain in one Python thread; its experiment grid fans chains / settings
out over processes (driver_utils.py:69-111).  On an MI355X one chain keeps one workgroup (one
of 256 CUs) busy, so the native unit of work is an *ensemble*: C chains advance in lock-step,
each SGLD step = ONE particle-filter launch (one workgroup per chain x window) + ONE tiny
update kernel (prior gradient, 1/T scaling, Langevin noise, projection).  Everything --
observations, parameters, descriptors, RNG counters, results -- stays in HBM between steps;
the host only enqueues launches.  PyTorch is used for device memory, streams and
`torch.distributed` (RCCL) only.

Multi-GPU: chains are independent, so rank r owns chains [r*C, (r+1)*C) (weak scaling) and
the only collective is the gather of the parameter samples (`gather_samples`).

Per-step semantics follow `SGMCMCSampler.sample_sgld` + `project_parameters`
(sgmcmc_sampler.py:549-567, 650-656) with `noisy_gradient(kind='pf')` (:427-464); the RNG is
the device Philox generator, so trajectories are statistically, not bitwise, equivalent to
the reference (bitwise parity is what the REPLAY mode of the Sampler classes is for).
"""
import numpy as np
import torch

from . import _capi
from .ensemble_settings import ACCESSORS, FILTERS, SAMPLERS, filter_family, resolve_settings, window_counts

_MODELS = {}
# the score columns pMALA's drift reads (LGSSM: not C's, column 2: C stays 1)
_PMALA_SCORE_COLUMNS = {"svm": (0, 1, 2), "lgssm": (0, 1, 3), "garch": (0, 1, 2, 3)}


def _model_info(model):
    if not _MODELS:
        from .models import svm, garch, lgssm
        _MODELS.update(svm=(svm.SVMParameters, svm.SVMPrior, svm.SVMHelper),
                       garch=(garch.GARCHParameters, garch.GARCHPrior, garch.GARCHHelper),
                       lgssm=(lgssm.LGSSMParameters, lgssm.LGSSMPrior, lgssm.LGSSMHelper))
    return _MODELS[model]


def prior_hyper(model, prior):
    """Flatten a (1-D) Prior's hyper-parameters into the pfg_prior_hyper struct."""
    h = _capi.PriorHyper()
    hp = prior.hyperparams
    first = lambda v: float(np.asarray(v).reshape(-1)[0])
    h.df_Rinv, h.scale_Rinv = first(hp['df_Rinv']), first(hp['scale_Rinv'])
    h.df_Qinv = h.scale_Qinv = h.var_col_A = h.var_col_C = 1.0
    if model in ("svm", "lgssm"):
        h.df_Qinv, h.scale_Qinv = first(hp['df_Qinv']), first(hp['scale_Qinv'])
        h.mean_A, h.var_col_A = first(hp['mean_A']), first(hp['var_col_A'])
    if model == "lgssm":
        h.mean_C, h.var_col_C = first(hp['mean_C']), first(hp['var_col_C'])
    if model == "garch":
        for k in ('scale_mu', 'shape_mu', 'alpha_phi', 'beta_phi', 'alpha_lambduh', 'beta_lambduh'):
            setattr(h, k, first(hp[k]))
    return h


class ChainEnsemble(object):
    """C independent SGLD chains of one model on one series, resident on `device`.

    Args:
      model: 'svm' | 'garch' | 'lgssm';  observations: (T,) or (T,1), or a LIST of such arrays =
             independent sequences (the Seq*Sampler setting, e.g. the gap-split EURUS segments):
             every chain and step draws ONE sequence uniformly (num_sequences = 1) and a buffered
             window inside it, its gradient rescaled by T_total / T_sequence
             (sgmcmc_sampler.py:1249-1283)
      parameters: a Parameters object (all chains start there) or an array [C, P] of raw thetas
      num_chains: C (ignored when `parameters` is an array)
      N, pf ('poyiadjis_N' | 'nemeth' | 'paris' | 'poyiadjis_N2'), lambduh, kernel: particle-filter settings
               pf='poyiadjis_N2' (N <= 1024; the multi-window path up to 16384): the Poyiadjis O(N^2) smoother, the score
               with lambduh = 1, multinomial resampling, kind 'pf'; N <= 128 runs one wave per window (n2_64x2) once a
               launch has more than 64 windows.  GARCH: the reference's backward kernel scores only the x component of the
               state, so the O(N^2) (and PaRIS) phi / lambda scores differ systematically from the O(N) ones; this backend
               reproduces the reference
      Ntilde, max_accept_reject, accept_reject: pf='paris' (N <= 1024): the backward draws per particle, the
               accept-reject rounds before the exact draw (default 64; accept_reject=False: none, every draw exact),
               as the Helper's device-generator path (particle_filters.make_problem)
      epsilon: SGLD step size;  prior: Prior (default: the model's default prior, var=100 / 1)
      subsequence_length S / buffer_length B: -1 = full sequence (no window sampling)
      dtype: 'f64' | 'f32' particle-state arithmetic;  seed: Philox key
      chain_offset: global index of this rank's first chain (keeps streams distinct across GPUs)
      resampling: 'multinomial' (the reference's) | 'systematic' (extension, N <= 1024: no REPLAY stream -- the reference has no
               such resampler --, the kernel is replayed on the CPU from the draws a traced launch records) |
               'stratified' (extension: child r of a step resamples with (r + U_r) / N, one uniform per child -- the
               score's variance falls to 0.2-0.5 of the multinomial one at the same N; pf 'poyiadjis_N' | 'nemeth',
               kind 'pf', N <= 16384, every path those serve: single- and multi-window, host and device windows, graphs)
      ess_threshold: None | tau in (0, 1] (extension: ESS-triggered, "adaptive" resampling -- a timestep resamples only
               when the effective sample size 1 / sum p_i^2 is below tau N; otherwise every particle stays where it is and
               carries its normalised weight on, so the genealogy is thinned less often: at tau = 0.5 the score's variance
               falls to about 0.5-0.7 of the always-resampling one and some 70-80 % of the steps run no CDF, search or
               gather; pf 'poyiadjis_N' | 'nemeth', kind 'pf', resampling 'multinomial', N <= 16384, every path those
               serve: single- and multi-window, host and device windows, graphs, every sampler; None or 0 = resample at
               every step, today's kernels and numbers; include/pfgrad.h: PFG_FLAG_ADAPTIVE_RESAMPLING)
      sampler: 'sgld' (sample_sgld + project_parameters) | 'sghmc' (extension: momentum with
               friction `friction` in (0,1]; friction = 1 is SGLD) | 'sgrld' (model 'lgssm': sample_sgrld with the
               LGSSM preconditioner + project_parameters, pfg_sgrld_update_device; every kind, pf and dtype) |
               'gibbs' (model 'lgssm', dtype 'f64', subsequence_length = buffer_length = -1: the blocked Gibbs sampler
               of sample_gibbs -- one FFBS path of the whole series with the PFG_STAT_GIBBS statistics, then the
               conjugate draw of pfg_gibbs_update_device; kind, N, pf, num_samples and epsilon are ignored, sequence
               lists are refused, and last_gradient_statistics() returns the sufficient statistics) |
               'pmmh' (extension: particle marginal Metropolis-Hastings, Andrieu, Doucet and Holenstein 2010 -- a step
               proposes theta' = theta + proposal_scale (.) z in the raw parameterisation (pfg_pmmh_propose_device; outside
               the support of project_parameters the proposal is rejected unseen), runs the launch of the resolved kind
               on theta' and accepts on its log-likelihood estimate out[4] plus the log-prior (pfg_pmmh_accept_device).
               The chain keeps the estimate it was accepted with, so it samples the posterior exactly for every N.  It
               needs the whole data set in every step: a single series with subsequence_length = buffer_length = -1, or
               a list on the multi-window path with num_sequences = -1 and whole sequences (subsequence_length = -1), the
               reduced out[4] being the sum over the sequences.  kind 'pf' with pf 'poyiadjis_N' | 'nemeth', any
               resampling and ess_threshold (the statistic is not computed: stat 'none'), or kind 'marginal' (LGSSM, f64:
               Metropolis-Hastings on the Kalman likelihood).  The target is prior.logprior(theta) in the raw coordinates
               WITHOUT Jacobian terms -- the density whose gradient SGLD uses.  epsilon, friction and lambduh are
               ignored; loglik() and acceptance_rate() read the chains' estimates and acceptance; the constructor runs
               one launch at the initial parameters (the init pass: it consumes counter value 0, step s draws with
               counter s + 1) and refuses a chain whose initial log-likelihood is not finite) |
               'pmala' (extension: the particle Metropolis-adjusted Langevin algorithm, Nemeth, Sherlock and Fearnhead
               2016 -- PMMH whose proposal drifts along the filter's own score estimate.  With s = proposal_scale, g the
               score and ll the log-likelihood estimate the chain's current state was accepted with, and
               d(theta, g) = grad_logprior(theta) + g (the drift of the SGLD update, score columns mapped as there), a step
               proposes theta'_j = theta_j + (s_j^2 / 2) d_j(theta, g) + s_j z_j (pfg_pmala_propose_device; LGSSM's C
               stays 1; PMMH's support), runs the SCORE launch of the resolved kind on theta' -- the launch of a
               full-series SGLD step -- and accepts on (pfg_pmala_accept_device)
                   log alpha = (ll' + logprior(theta')) - (ll + logprior(theta)) + log q(theta | theta', g') - log q(theta' | theta, g),
                   log q(b | a, g) = -sum_j (b_j - a_j - (s_j^2 / 2) d_j(a, g))^2 / (2 s_j^2).
               With s_j^2 / 2 = epsilon / T for every j the proposal is the law of the SGLD step before
               project_parameters, so this is SGLD with the Metropolis correction it lacks.  A chain that rejects keeps
               theta, ll AND g -- neither estimate is refreshed -- so it samples PMMH's target exactly for every N: exp(
               prior.logprior(theta)) p(y | theta) on the raw row.  (grad_logprior is not the gradient of logprior on
               every coordinate; exactness does not need it to be, q uses the same drift both ways.)
               Settings as 'pmmh' -- the whole data set in every step, kind 'pf' with pf 'poyiadjis_N' | 'nemeth', any
               resampling and ess_threshold, N <= 16384, or kind 'marginal' (LGSSM, f64: the Kalman score and likelihood
               are exact, plain MALA); pmmh_stat is refused.  loglik(), score() and acceptance_rate() read the chains'
               estimates and acceptance, last_gradient_statistics() the estimates at the latest proposals; the init
               pass is PMMH's and refuses a chain whose initial log-likelihood or score is not finite) |
               'pmala_sorted' (extension: 'pmala' on one of the two sorted filters, whose estimate is usable at N = 64 .. 128.
               It takes exactly one of correlation=rho and sqmc=True (below); the launch is pfg_cpm_score_device or
               pfg_sqmc_score_device -- the filter of sampler='pmmh' with that option, draw for draw and with the same
               out[4], carrying Poyiadjis' O(N) score through the sort (pf='poyiadjis_N', the default) or its fixed-lag
               shrinkage (pf='nemeth', lambduh in (0, 1], default 0.95).  The drift g-hat(theta, U) is a deterministic
               function of theta and of the filter's draws U, and U -> U' is reversible with respect to their law, so with
               q(theta' | theta, U) one way and q(theta | theta', U') the other the chain is exact on the extended target
               for every N, rho and lambduh; no smoothness of the score in U is needed.  State: 'pmala's, and under
               correlation the correlated chain's buffers and selector; propose, accept, commit, checkpoints and graphs
               are theirs.  Refusals: the filter family's (SVM | LGSSM, f64, one whole series, kind 'pf', the prior kernel,
               its own resampling, N <= 1024, a power of two under sqmc), pf = 'paris' | 'poyiadjis_N2', pmmh_stat)
               'pgibbs' (extension: particle Gibbs, Andrieu, Doucet and Holenstein 2010, model 'svm' | 'lgssm', dtype 'f64',
               2 <= N <= 1024, the whole series: a step is one conditional SMC sweep with ancestor sampling (Lindsten,
               Jordan and Schon 2014; pfg_csmc_device) that replaces each chain's latent path [T] -- the path is part of
               the chain's state --, then the conjugate draw of the parameters from that path's statistics
               (pfg_pgibbs_update_device).  The only sampler here that gives latent paths for the nonlinear model.
               Prior proposal, multinomial resampling at every step; pf, resampling, ess_threshold, kernel='optimal',
               windows, sequence lists and W > 1 are refused by name, epsilon is ignored.  The constructor runs one
               unconditional sweep at the initial parameters for the first path (the init pass: counter value 0, step s
               draws with s + 1).  path(), suff_stats() and n_degenerate() read the chains' paths, the statistics of the
               latest paths and how often a chain's sweep kept its path because its weights degenerated.  The scratch is
               C * pfg_csmc_scratch_bytes(T, N) bytes: 10 T N per chain)
               'sgd' | 'adagrad' (step_sgd and step_adagrad + project_parameters, pfg_sgd_update_device /
               pfg_adagrad_update_device: optimisers towards the MAP, another update on the launch of an 'sgld' step, so
               they take whatever 'sgld' takes; they draw nothing; moment() reads ADAGRAD's G, which travels in state_dict)
               'sgld_cv' (extension: SGLD with control variates, Baker, Fearnhead, Fox and Nemeth 2019 -- the step's gradient
               is centre_gradient + (window score at theta - window score at the centre), pfg_sgld_cv_update_device.  Every
               descriptor has a TWIN that differs in theta (the centre's row), out and scratch alone, launched with it in
               ONE launch of 2 * _nd descriptors: same window, same seed, stream and counter, hence the same normals and
               uniforms -- common random numbers -- and at theta = centre the two records are bitwise equal, the step a
               Langevin step on centre_gradient.  On buffered windows the variance of a plain step's gradient is dominated
               by which window was drawn; the control variate removes that term down to O(|theta - centre|^2).  With
               kind='marginal' (LGSSM) the window scores are exact and the classic result holds without qualification;
               with kind='pf' the particle noise cancels as far as resampling, which is discontinuous in theta, lets it
               (measured, DESIGN section 7: a large gain in A at every N; in LQinv / LRinv a gain at N = 1000 that fades by
               one posterior sd from the centre, and a LOSS at N = 100 from a quarter sd on -- re-centre, or use
               minibatch_size = 2, which costs the same).
               A single series; kind 'pf' with pf 'poyiadjis_N' | 'nemeth', every resampling, ess_threshold, both dtypes,
               N <= 16384, single- and multi-window, host and device windows, graphs -- or kind 'marginal'.  Lists of
               sequences, pf 'paris' | 'poyiadjis_N2', kind 'complete' and N > 16384 are refused by name.  centre(),
               centre_gradient() and cv_statistics() read the centres, their gradients and the two records of the latest
               step; set_centre() moves the centre, e.g. to the end of an 'adagrad' run, or re-centres mid-run.  A step
               costs the launch of twice the descriptors.  NOT the drop-in sampler's sample_sgld_cv, by design: there both
               filters run at the current parameters on independent draws)
      centre, centre_repeats, centre_N: sampler='sgld_cv' (refused elsewhere): the constructor's last act is
               set_centre(centre, centre_repeats) -- centre [P], [C, P], a Parameters object or None = the start parameters;
               centre_repeats whole-series launches (default 1) with centre_N particles (default N, at most 16384; refused
               with kind='marginal', which centres on one exact Kalman launch) are averaged into the centre gradient.  An
               error in that gradient is a bias that does not average out over steps: see set_centre
      proposal_scale: sampler='pmmh' | 'pmala' (required there, refused elsewhere): the random walk's (the Langevin
               proposal's) standard deviations in raw-theta units, a positive scalar or a length-P vector (LGSSM: C stays 1
               whatever its entry)
      pmmh_stat: sampler='pmmh', kind='pf': None | 'none' (the launch computes no statistic, the default) | 'score' (the
               score launch of the same shape, its score ignored: tools/pmmh_time.py measures one against the other)
      correlation: sampler='pmmh': None (the default: plain PMMH, today's launches, numbers and state_dict keys) | rho in [0, 1)
               (extension: the correlated pseudo-marginal method, Deligiannidis, Doucet and Pitt 2018.  The chain keeps the
               standard normals U [T+1, N+1] its estimate was computed from as part of its state; a step proposes
               U' = rho U + sqrt(1 - rho^2) eps beside theta' and runs pfg_cpm_device, a filter that is a smooth function of
               U' -- the particles are sorted by state before each resampling, and resampling is systematic on one uniform
               taken from U' -- so the two estimates in the accept ratio share most of their noise: at T = 1000, N = 100 the
               acceptance rises from 0.06 to 0.51 at rho = 0.99.  The accept step is PMMH's, unchanged; a chain that rejects
               keeps theta, its estimate AND its normals.  U -> U' is reversible with respect to N(0, I) and the estimate is
               unbiased under it, so the chain is exact for every N and rho; rho = 0 draws fresh normals at every step.
               Model 'svm' | 'lgssm', dtype 'f64', 2 <= N <= 1024, the whole series, kind 'pf'; pf, resampling,
               ess_threshold, kernel='optimal', pmmh_stat, windows, sequence lists, W > 1 and every other sampler are
               refused by name.  aux() reads the normals the chains hold; state_dict carries them ('aux', the current
               buffer only) with 'correlation' and 'T', and load_state_dict refuses another rho, T or N.  The ensemble keeps
               two buffers per chain: 2 * C * pfg_cpm_aux_bytes(T, N) bytes, 19.9 GB at T = 1000, N = 100, 12288 chains)
      sqmc: sampler='pmmh': False (the default: today's PMMH, bit for bit) | True (extension: sequential quasi-Monte Carlo,
               Gerber and Chopin 2015.  launch_pf is pfg_sqmc_device: the particles are sorted by state before each resampling
               and the N (resampling, move) pairs of a timestep are one Sobol' point set in [0, 1)^2 under a fresh random
               digital shift, so the estimate itself is less noisy at a given N; it stays unbiased, so the chain is exact for
               every N.  The chain carries nothing beyond PMMH's state; state_dict records 'sqmc' = True and load_state_dict
               refuses a checkpoint of the other kind.  Model 'svm' | 'lgssm', dtype 'f64', N a power of two in 2 .. 1024,
               the whole series, kind 'pf'; correlation, pf, resampling, ess_threshold, kernel='optimal', pmmh_stat, windows,
               sequence lists, W > 1 and every other sampler are refused by name)
      kind: 'pf' (the particle-filter score) | 'marginal' (LGSSM, dtype 'f64': the exact Kalman score of
               every window, PFG_SMOOTHER_KALMAN -- the reference's kind='marginal', the KF baseline of its
               LGSSM experiment; N, pf and resampling are ignored) | 'complete' (LGSSM, dtype 'f64': the
               complete-data score averaged over num_samples FFBS paths of every window's buffer,
               PFG_SMOOTHER_KALMAN_FFBS with the device generator -- the reference's kind='complete', the
               MC row of its LGSSM experiment; N, pf and resampling are ignored)
      num_samples: kind='complete': the paths per window
      window_sampling: 'host' (one window start per chain and step drawn on the host, keyed by
               (seed, global chain id, step) so that a chain's windows do not depend on the rank
               partition; descriptors are re-uploaded) | 'device' (a Philox-keyed kernel rewrites the descriptors in HBM: the
               step is three launches with no host work, and `run(..., graph_steps=K)` replays K
               steps per hipGraph launch)
      minibatch_size, num_sequences: SEVERAL windows per chain and step, the reference's _noisy_grad_loglikelihood
               (sgmcmc_sampler.py:390-425, 1249-1283): minibatch_size = M windows in each of K_eff sequences -- a single
               series: K_eff = 1 (num_sequences = 1 only); a list: num_sequences = K in 1..len(list) distinct
               sequences drawn per chain and step, or -1 = every sequence in order (the reference's default; here the
               default stays 1, one sequence per step, as above).  W = K_eff * M windows per chain run in ONE
               particle-filter launch of C * W descriptors (window w of global chain g: stream g * W + w), then a
               reduction in the reference's order of operations (within a sequence, across sequences, times
               T_total / sum of the chosen T_k when num_sequences != -1: pfg_reduce_windows_device) and the update.
               Passing either argument (1 included) selects this multi-window path; it samples windows on the device
               (window_sampling='device', needed whenever there is anything to draw), so it replays in hipGraphs for
               sequence lists too, and it runs pf='paris' and pf='poyiadjis_N2' up to N = 16384 (paris_mem1024 /
               n2_mem1024 above N = 1024).  Leaving
               both out keeps the single-window launches described above.  Refused: sampler='gibbs' or kind != 'pf'
               with W > 1, window_sampling='host' when windows are drawn, N > 16384.

    How it is put together (each decision is made in one place):
      ensemble_settings.SAMPLERS: one record per sampler -- the update rule launch_update runs, the propose / accept pair of
               a step that has one (PMMH's or pMALA's) and whether the proposal drifts along the filter's score, whether every
               descriptor has a twin ('sgld_cv'), what a chain carries beyond theta, the momentum and the counter as ordered
               (checkpoint key, attribute) pairs, the keys that name the sampler in a checkpoint, what
               last_gradient_statistics returns, the accessors that are its own, and the methods that allocate for it
               (_mh_alloc, _adagrad_alloc) and run its init pass (_mh_init, _pgibbs_init, _cv_init).
      ensemble_settings.FILTERS: one record per family of filter launch -- 'descriptors' (the pfg_dev_problem records of
               `_desc` / desc_dev: launch_descriptors), 'csmc' (launch_csmc on csmc_desc_dev), 'cpm' (launch_cpm on
               cpm_desc_dev) and 'sqmc' (launch_sqmc on sqmc_desc_dev): the library call and its score twin, the record
               dtype, the salt of its key (seed ^ salt), the method that allocates what it carries and its static records
               (_csmc_alloc, _cpm_alloc, _sqmc_alloc), what it carries and what it writes into a checkpoint, and the wording
               of its refusals.  The constructor resolves (sampler, correlation, sqmc) to one family once (filter_family);
               `_rule` and `_family` are the two records, and no other line asks which sampler this is.
      _resolve_settings (ensemble_settings.resolve_settings): the arguments above -> kind, pf, N, lambduh, the descriptor
               smoother `_smoother` and the launch smoother `_launch_smoother`, the stat, the PaRIS fields, M / K / W, the
               path (`_multi`: W descriptors per chain, records in win_out_dev, a reduction before the update), S, B,
               `strict`, the sequence bounds, and every refusal that needs no device.  Nothing is allocated before it returns.
               pf='poyiadjis_N2' is resolved there to the descriptor and launch smoother 'poyiadjis_n2' (lambduh = 1, the
               score); from then on it takes the paths of the other smoothers unchanged.
      _capi.device_descriptors: the static fields of the `_nd` = C (single-window) or C * W (multi-window, chain-major)
               records of `_desc`; stream ids chain_offset + c, or (chain_offset + c) * W + w.
      _weights_blocks: weights_dev, one row per window start of every sequence longer than S, with the offsets of the
               sequences' blocks (_seg_weight_offsets; woffs_dev on the multi-window path); _weights_table is the 2-D
               view of a single series' block.
      _set_windows: the host draw of (sequence, start) per chain and the one derivation of
               y, T, t1, tL, weights from it -- a single series is a list of one sequence; a full single series has a
               null weights pointer, a whole short sequence of a list points at its row of T_total / T_k.
      _scratch_bytes: the scratch per descriptor of the resolved smoother.
      launch_windows / launch_propose / launch_pf / launch_reduce / launch_update: the launches of a step on one stream
               (_stream); _enqueue_step is the one sequence of them -- the windows where `_window_draws` says who draws them,
               then `_step`, the list the constructor builds once: the proposal if the sampler has one, the family's launch,
               the reduction on the multi-window path, the update -- and step / run / _graph drive it; _update_key keys
               every update rule.  launch_pf is the family's launch; a family with records of its own launches through
               _launch_chain_filter, its score twin with lambduh where the sampler drifts along the score.  launch_update is
               the record's rule, or launch_accept where the step has a pair; launch_accept ends in the commit that flips the
               selector of a chain that accepted where the family keeps two buffers of normals ('cpm').  _init_launch is the
               launch of every init pass: the family's launch with its init keywords (cpm: rho = 0; csmc: has_ref = 0), the
               reduction, the accept step, counter 1.
               sampler='sgld_cv': _desc / desc_dev hold _nl = 2 * _nd records, the chains' and behind them their twins'
               (_cv_alloc); launch_windows and launch_reduce serve both halves, launch_pf launches them together, set_centre is
               the centring pass on centre_desc_dev.
      _chain_state: the sampler's carried pairs, then the family's, and the scratch of a step: the one list state_dict,
               load_state_dict and _graph's snapshot follow.  _need: the one guard of the accessors.
    """

    def __init__(self, model, observations, parameters, num_chains=None, N=1000, pf="poyiadjis_N",
                 lambduh=None, kernel=None, epsilon=0.1, prior=None, subsequence_length=-1,
                 buffer_length=-1, dtype="f64", seed=0, chain_offset=0, device=None,
                 forward_message=None, partition_style=None, resampling="multinomial",
                 sampler="sgld", friction=0.1, window_sampling="host", kind="pf", num_samples=None,
                 Ntilde=2, max_accept_reject=None, accept_reject=True, minibatch_size=None, num_sequences=None,
                 ess_threshold=None, proposal_scale=None, pmmh_stat=None, correlation=None, sqmc=False, centre=None,
                 centre_repeats=1, centre_N=None):
        s = self._resolve_settings(
            model, observations, parameters, num_chains=num_chains, N=N, pf=pf, lambduh=lambduh,
            subsequence_length=subsequence_length, buffer_length=buffer_length, dtype=dtype, partition_style=partition_style,
            resampling=resampling, sampler=sampler, window_sampling=window_sampling, kind=kind, num_samples=num_samples,
            Ntilde=Ntilde, max_accept_reject=max_accept_reject, accept_reject=accept_reject, minibatch_size=minibatch_size,
            num_sequences=num_sequences, ess_threshold=ess_threshold, proposal_scale=proposal_scale, pmmh_stat=pmmh_stat,
            kernel=kernel, correlation=correlation, centre=centre, centre_repeats=centre_repeats, centre_N=centre_N,
            sqmc=sqmc)
        if not torch.cuda.is_available():
            raise RuntimeError("ChainEnsemble needs an MI355X (no CPU fallback)")
        Parameters, Prior, Helper = _model_info(model)
        self.model, self.dtype, self.epsilon, self._Parameters = model, dtype, float(epsilon), Parameters
        self.kind, self.pf, self.N, self.lambduh = s.kind, s.pf, s.N, s.lambduh
        self._smoother, self._launch_smoother = s.smoother, s.launch_smoother
        self.Ntilde, self.max_accept_reject = s.Ntilde, s.max_accept_reject
        self.resampling, self.sampler, self.friction = resampling, sampler, float(friction)
        self.ess_threshold = s.ess_threshold        # None: resample at every step
        self.correlation = s.correlation            # None: plain PMMH, a fresh estimate per proposal
        self.sqmc = getattr(s, "sqmc", False)       # True: PMMH on the sequential quasi-Monte Carlo filter's estimate
        # what the sampler is and which family of filter its step launches: the two records every later decision reads
        rule = self._rule = SAMPLERS[sampler]
        self._filter = filter_family(sampler, self.correlation, self.sqmc)
        family = self._family = FILTERS[self._filter]
        self._twins = rule.twins                    # every descriptor has a twin at the centre, in the same launch
        self._accessors = frozenset(rule.accessors + family.accessors)
        # ordered (checkpoint key, attribute) pairs: the sampler's, then the family's (_chain_state)
        self._carries = rule.carries + family.carries
        self.window_sampling, self.partition_style, self.strict = window_sampling, partition_style, s.strict
        self._multi, self.W, self.segments, self.T, self.S, self.B = s.multi, s.W, s.segments, s.T, s.S, s.B
        self.P, self.C = s.theta0.shape[1], s.theta0.shape[0]
        self.seed, self.chain_offset = int(seed), int(chain_offset)
        self._graphs = {}
        self.steps_done = 0
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.ctx = _capi.default_context(self.device.index)
        self.helper = Helper(n=1, m=1, forward_message=forward_message)
        self.kernel = self.helper._get_kernel(kernel)
        if prior is None:
            prior = Prior.generate_default_prior(var=1.0 if model == "garch" else 100.0, n=1, m=1)
        self.prior = prior
        self.hyper = prior_hyper(model, prior)
        if s.kind in ("marginal", "complete"):
            # (a refusal that needs no device either, but it reads the Helper's message, so it is stated here, before
            # anything is allocated, and not in _resolve_settings)
            # the message of x_{-1} itself: mean mean_precision / precision, variance 1 / precision
            fm = self.helper.default_forward_message
            prec = float(np.reshape(fm['precision'], -1)[0])
            if not (0.0 < prec < np.inf):
                raise ValueError("the forward message needs a finite precision > 0, got {0}".format(prec))
            pm, pv = float(np.reshape(fm['mean_precision'], -1)[0]) / prec, 1.0 / prec
        else:
            pm, pv, _ = self._prior_x(s.proto, s.theta0[0])

        dev, C, W = self.device, self.C, self.W
        th = np.zeros((C, _capi.MAX_THETA))
        th[:, :self.P] = s.theta0
        self.y_dev = torch.from_numpy(s.y).to(dev)
        self.theta_dev = torch.from_numpy(th).to(dev)
        self.out_dev = torch.zeros((C, _capi.OUT_DOUBLES), dtype=torch.float64, device=dev)
        self.step_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self.momentum_dev = torch.zeros((C, _capi.MAX_THETA), dtype=torch.float64, device=dev)
        self.proposal_scale = s.proposal_scale
        if rule.alloc is not None:
            getattr(self, rule.alloc)(s)
        # one weights row per window start of every sequence longer than S.  Single-window lists: every row times
        # T_total / T_sequence, the Seq sampler's rescaling of a one-sequence gradient, whole short sequences a row of it;
        # the multi-window path leaves that rescaling to the reduction
        bounds = self._bounds = s.bounds
        scale = self.T / np.diff(bounds).astype(np.float64) if self.segments is not None and not self._multi else None
        flat, self._seg_weight_offsets = self._weights_blocks(bounds, self.S, scale)
        self._weights_table = None
        if flat is not None and self.segments is None and not self._multi:
            flat = self._weights_table = flat.reshape(-1, self.S)       # a single series: resident as the [starts, S] table
        self.weights_dev = torch.from_numpy(flat).to(dev) if flat is not None else None
        self._nd = C * W if self._multi else C
        records = self.out_dev
        chain = np.repeat(np.arange(C, dtype=np.uint64), W if self._multi else 1)
        stream = chain + np.uint64(self.chain_offset)
        if self._multi:
            # W = K_eff * M descriptors per chain (chain-major, window w = k * M + m), their records win_out_dev [C * W, 8],
            # each window's sequence length seq_len_dev [C * W]; out_dev [C, 8] holds the reduced records the update reads
            self.M, self.num_sequences, self.K_eff = s.M, s.K, W // s.M
            self._draws, self._rescale = s.draws, s.rescale       # rescale: T_total / S (sgmcmc_sampler.py:1278-1282)
            self.bounds_dev = torch.from_numpy(np.ascontiguousarray(bounds, dtype=np.int64)).to(dev)
            self.woffs_dev = torch.from_numpy(self._seg_weight_offsets).to(dev)
            self.seq_len_dev = torch.zeros(self._nd, dtype=torch.int32, device=dev)
            records = self.win_out_dev = torch.zeros((self._nd, _capi.OUT_DOUBLES), dtype=torch.float64, device=dev)
            stream = stream * np.uint64(W) + np.tile(np.arange(W, dtype=np.uint64), C)
        sb = self._scratch_bytes()
        if self._multi:
            self.scratch_bytes_per_window = sb
        # the descriptors of one launch: the chains', and under 'sgld_cv' their twins' behind them
        self._nl = 2 * self._nd if self._twins else self._nd
        self.scratch_dev = None
        if sb > 0:       # state in HBM (L2-resident), one slab per descriptor: the large-N kernel, paris_mem1024, Kalman messages
            self.scratch_dev = torch.empty(self._nl * sb, dtype=torch.uint8, device=dev)
        garch_stationary = model == "garch" and self.helper.default_forward_message is None
        # sampler='pgibbs' launches none of these records (its sweep reads csmc_desc_dev) and N <= 1024 gives them no scratch;
        # they are kept, C * 376 bytes, because the step, the graph snapshot and enable_stamps address _desc / desc_dev
        # without asking the sampler
        self._desc = _capi.device_descriptors(
            self._nd, theta=self.theta_dev if rule.propose is None else self.theta_prop_dev, row=chain, out=records,
            step_ctr=self.step_ctr, scratch=self.scratch_dev, scratch_bytes=sb, stream=stream, prior_mean=pm, prior_var=pv,
            lambduh=self.lambduh, seed=self.seed, N=self.N, smoother=s.smoother, stat=s.stat,
            flags=_capi.FLAG_GARCH_STATIONARY_PRIOR if garch_stationary else 0, ess_threshold=s.ess_threshold, **s.paris)
        if self._twins:
            self._cv_alloc(s, records, sb)
        if not self._multi:
            self._set_windows(first=True)
        self.desc_dev = torch.from_numpy(self._desc.view(np.uint8).reshape(self._nl, -1)).to(dev)
        if self._multi and not self._draws:
            self.launch_windows()           # static windows: written once, no draw
        # who draws a step's windows: nobody when they are static (a proposal is judged on the whole data set on either path)
        if self._multi:
            self._window_draws = "device" if self._draws else None
        else:
            self._window_draws = window_sampling if rule.propose is None else None
        # the family's launch: launch_descriptors | launch_csmc | launch_cpm | launch_sqmc, with the score twin of a sorted
        # filter where the sampler drifts along the score, under the family's key; then the launches of a step, in order
        # (the class's functions, called with the ensemble: a bound method kept on the instance would be a reference cycle,
        # and the buffers in HBM would wait for the garbage collector)
        cls = type(self)
        self._launch_filter = getattr(cls, "launch_" + self._filter)
        if family.launch is not None:
            self._filter_call = family.score if rule.score else family.launch
            self._filter_score = (self.lambduh,) if rule.score else ()
            self._filter_key = (self.seed ^ family.salt, self.chain_offset, self.step_ctr.data_ptr())
        self._step = [launch for launch, has in ((cls.launch_propose, rule.propose is not None), (self._launch_filter, True),
                                                 (cls.launch_reduce, self._multi), (cls.launch_update, True)) if has]
        # what the family carries and its records, then the sampler's init pass
        if family.alloc is not None:
            getattr(self, family.alloc)(pm, pv)
        if rule.init is not None:
            s.centre = centre
            getattr(self, rule.init)(s)

    def _mh_alloc(self, s):
        """What a step with a propose / accept pair needs beside theta: the proposal the launch reads, its validity, each
        chain's current estimate and acceptance count; where the proposal drifts along the score, the score estimate each
        chain's current state was accepted with (out[0..3], verbatim)."""
        C, dev = self.C, self.device
        self.theta_prop_dev = self.theta_dev.clone()
        self.valid_dev = torch.ones(C, dtype=torch.int32, device=dev)
        self.ll_dev = torch.zeros(C, dtype=torch.float64, device=dev)
        self.accept_dev = torch.zeros(C, dtype=torch.int64, device=dev)       # (the library's uint64 counts)
        self.scale_dev = torch.from_numpy(s.proposal_scale).to(dev)
        if self._rule.score:
            self.grad_cur_dev = torch.zeros((C, _capi.MAX_THETA), dtype=torch.float64, device=dev)

    def _adagrad_alloc(self, s):
        """G, the running sum of squared scaled gradients, per variable."""
        self.moment_dev = torch.zeros((self.C, _capi.MAX_THETA), dtype=torch.float64, device=self.device)

    # -- sampler='sgld_cv': the twins, the centre and its gradient -----------------------------------------------------
    _CENTRE_SEED = 0x43454E5452453031       # "CENTRE01": the centring launches draw under seed ^ this

    def _cv_alloc(self, s, records, sb):
        """The state of a control-variate chain beyond SGLD's: the centre theta_centre_dev [C, MAX_THETA], its whole-series
        score centre_grad_dev [C, 4] (score-column order, raw) and the counter of the centring launches centre_ctr_dev; the
        twins' records (single-window: out_centre_dev [C, 8] itself; multi-window: twin_out_dev [C * W, 8] and their sequence
        lengths, reduced into out_centre_dev); the twin descriptors, appended to _desc -- a twin is its chain's record but for
        theta (the centre's row), out and scratch, so it filters the same window on the same draws; and the C descriptors of
        the centring pass (centre_desc_dev: the whole series at the centre, centre_N particles, keys of their own)."""
        C, dev, nd = self.C, self.device, self._nd
        self.theta_centre_dev = self.theta_dev.clone()
        self.centre_grad_dev = torch.zeros((C, 4), dtype=torch.float64, device=dev)
        self.centre_ctr_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.centre_repeats, self.centre_N = s.centre_repeats, s.centre_N
        self.out_centre_dev = torch.zeros((C, _capi.OUT_DOUBLES), dtype=torch.float64, device=dev)
        twin_records = self.out_centre_dev
        if self._multi:
            twin_records = self.twin_out_dev = torch.zeros((nd, _capi.OUT_DOUBLES), dtype=torch.float64, device=dev)
            self.twin_seq_len_dev = torch.zeros(nd, dtype=torch.int32, device=dev)
        idx = np.arange(nd, dtype=np.uint64)
        chain = idx // np.uint64(self.W if self._multi else 1)
        twins = self._desc.copy()
        twins["theta"] = self.theta_centre_dev.data_ptr() + chain * np.uint64(8 * _capi.MAX_THETA)
        twins["out"] = twin_records.data_ptr() + idx * np.uint64(8 * _capi.OUT_DOUBLES)
        if self.scratch_dev is not None:
            twins["scratch"] = self.scratch_dev.data_ptr() + (idx + np.uint64(nd)) * np.uint64(sb)
        self._desc = np.concatenate([self._desc, twins])
        # the centring pass: one whole-series window per chain
        self._centre_sb = csb = self._scratch_bytes(N=self.centre_N, whole=True)
        self.centre_scratch_dev = torch.empty(C * csb, dtype=torch.uint8, device=dev) if csb > 0 else None
        self.centre_out_dev = torch.zeros((C, _capi.OUT_DOUBLES), dtype=torch.float64, device=dev)
        self.centre_acc_dev = torch.zeros((C, _capi.OUT_DOUBLES), dtype=torch.float64, device=dev)
        c = np.arange(C, dtype=np.uint64)
        d = self._desc[:nd:self.W if self._multi else 1].copy()       # chain c's static fields (its first window's)
        d["theta"] = self.theta_centre_dev.data_ptr() + c * np.uint64(8 * _capi.MAX_THETA)
        d["out"] = self.centre_out_dev.data_ptr() + c * np.uint64(8 * _capi.OUT_DOUBLES)
        d["scratch"] = 0 if self.centre_scratch_dev is None else self.centre_scratch_dev.data_ptr() + c * np.uint64(csb)
        d["step_ctr"] = self.centre_ctr_dev.data_ptr()
        d["seed"] = np.uint64((self.seed ^ self._CENTRE_SEED) & 0xFFFFFFFFFFFFFFFF)
        d["stream"] = c + np.uint64(self.chain_offset)
        d["N"] = self.centre_N
        d["y"], d["weights"], d["T"], d["t1"], d["tL"] = self.y_dev.data_ptr(), 0, self.T, 0, self.T
        self._centre_desc = d
        self.centre_desc_dev = self._upload_records(d)

    def set_centre(self, theta=None, repeats=None):
        """sampler='sgld_cv': move the centre and recompute its gradient.  theta: [P], [C, P], a Parameters object, or None =
        each chain's current parameters (periodic re-centring).  theta_centre_dev takes the projection of it
        (project_parameters).  Then `repeats` (default: the constructor's centre_repeats) whole-series launches at the centre --
        y whole, t1 = 0, tL = T, no weights, the ensemble's filter settings with centre_N particles -- keyed by (seed ^ a
        constant of its own, the global chain id, centre_ctr), centre_ctr advancing by one per launch in device memory: the
        centre gradient depends on (seed, global chain id, the calls made so far) only, never on the rank partition.
        pfg_cv_accumulate_device leaves their mean in centre_grad_dev [C, 4].  kind='marginal': one exact Kalman launch
        whatever `repeats` says.  The launches are enqueued on torch's current stream; the call then waits for them, to
        refuse a centre whose gradient is not finite.

        An error in centre_gradient() enters every step of every chain with the same sign: a BIAS that does not average out
        over steps, unlike the window noise the control variate removes.  repeats and centre_N are the knobs (the error's
        variance falls as 1 / (repeats * centre_N)); with kind='marginal' there is no such error."""
        self._need("set_centre")
        R = self.centre_repeats if repeats is None else int(repeats)
        if self.kind == "marginal":
            R = 1
        if R < 1:
            raise ValueError("set_centre needs repeats >= 1, got {0}".format(repeats))
        if theta is None:
            self.theta_centre_dev.copy_(self.theta_dev)
        else:
            th = np.asarray(theta.theta() if hasattr(theta, "theta") else theta, dtype=np.float64)
            if th.shape not in ((self.P,), (self.C, self.P)):
                raise ValueError("set_centre takes theta of shape [{0}] or [{1}, {0}], got {2}".format(self.P, self.C, th.shape))
            rows = np.zeros((self.C, _capi.MAX_THETA))
            rows[:, :self.P] = th
            self.theta_centre_dev.copy_(torch.from_numpy(rows))
        self._project_rows(self.theta_centre_dev)
        stream = self._stream(None)
        for r in range(R):
            if self.ess_threshold:
                self.ctx.launch_device_adaptive(self.model, self.kernel, self.dtype, "device", self.centre_N, self.C,
                                                self.centre_desc_dev.data_ptr(), stream)
            else:
                self.ctx.launch_device_smoother(self.model, self.kernel, self.dtype, "device", self._launch_smoother,
                                                1 if self._smoother == "kalman" else self.centre_N, self.C,
                                                self.centre_desc_dev.data_ptr(), stream)
            self.ctx.cv_accumulate_device(self.C, self.centre_out_dev.data_ptr(), self.centre_acc_dev.data_ptr(), r, R,
                                          self.centre_ctr_dev.data_ptr(), stream)
        self.centre_grad_dev.copy_(self.centre_acc_dev[:, :4])
        self.synchronize()
        used = self.centre_grad_dev.cpu().numpy()[:, list(_PMALA_SCORE_COLUMNS[self.model])]
        bad = np.flatnonzero(~np.all(np.isfinite(used), axis=1))
        if bad.size:
            raise ValueError("sgld_cv: the centre gradient of chain {0} is not finite".format(int(bad[0]) + self.chain_offset))

    def _cv_init(self, s):
        """The init pass of sampler='sgld_cv', the constructor's last act: the centring launches at the centre it was given."""
        self.set_centre(s.centre, s.centre_repeats)

    def _project_rows(self, t):
        """project_parameters on the rows of the device tensor t [*, MAX_THETA], in place (the rule of pfg_chains.hip's
        project_store: |A| <= 0.9999, a negative Cholesky factor reflected, LGSSM's C = 1; GARCH: its LRinv alone)."""
        def reflect(j):
            L = t[:, j]
            t[:, j] = torch.where(L < 0.0, torch.sqrt(L * L + 1e-16), L)
        if self.model != "garch":
            A = t[:, 0]
            t[:, 0] = torch.where(A.abs() > 0.9999, A * (0.9999 / A.abs()), A)
        if self.model == "lgssm":
            t[:, 1] = 1.0
        for j in ((3,) if self.model == "garch" else (self.P - 2, self.P - 1)):
            reflect(j)

    def centre(self):
        """sampler='sgld_cv': [C, P] the centres the chains' control variates are taken at."""
        self._need("centre")
        return self.theta_centre_dev[:, :self.P].cpu().numpy()

    def centre_gradient(self):
        """sampler='sgld_cv': [C, h] the whole-series score estimate at each chain's centre (score-column order, raw, without
        the prior), as last_gradient_statistics()[0]."""
        self._need("centre_gradient")
        return self.centre_grad_dev[:, :_capi.STAT_DIM[self.model]].cpu().numpy()

    def cv_statistics(self):
        """sampler='sgld_cv': (cur, centre), the [C, 8] records of the latest step's window at each chain's parameters and at
        its centre (multi-window path: the reduced records).  The step's gradient is centre_gradient() + (cur - centre)."""
        self._need("cv_statistics")
        return self.out_dev.cpu().numpy(), self.out_centre_dev.cpu().numpy()

    def moment(self):
        """sampler='adagrad': [C, P] the running sums of squared scaled gradients G."""
        self._need("moment")
        return self.moment_dev[:, :self.P].cpu().numpy()

    def _need(self, what):
        """Refuse the accessor `what` unless it is the sampler's or the filter family's own (the records' accessors)."""
        if what not in self._accessors:
            raise ValueError("{0}() belongs to {1}".format(what, ACCESSORS[what].format(self.sampler)))

    # the arguments -> the resolved settings or the refusal, without a device: ensemble_settings.py
    _resolve_settings = staticmethod(resolve_settings)
    _window_counts = staticmethod(window_counts)

    def _scratch_bytes(self, N=None, whole=False):
        """pfg_dev_problem.scratch bytes per descriptor of the resolved smoother; refuses what the library refuses.
        N, whole: of a launch with another particle count on whole-series windows (the centring pass of 'sgld_cv')."""
        N, S = self.N if N is None else int(N), -1 if whole else self.S
        if self._smoother == "kalman":
            # the backward messages of the longest window: S (segments: no window is longer), or the whole series
            return _capi.kalman_scratch_bytes(S if S > 0 else self.T)
        if self._smoother == "kalman_ffbs":
            # the forward messages of the longest buffer: a window and its two buffers, or the whole series
            return _capi.kalman_scratch_bytes(min(self.T, S + 2 * self.B) if S > 0 else self.T)
        if self.ess_threshold or self._multi or self._smoother in ("paris", "poyiadjis_n2", "nemeth_stratified"):
            # PaRIS, N <= 1024: 0, the LDS-resident variants keep their state in LDS; above: paris_mem1024's slab.  The
            # single-window PaRIS path (N <= 1024 only) relies on that answer of 0 where it once wrote the literal.
            # The O(N^2) smoother likewise: 0 for N <= 1024, n2_mem1024's slab above it (multi-window path only).
            # Stratified and adaptive windows: 0 for N <= 1024, the large-N twins' slab up to 16384 (adaptive: also where
            # plain device-generator windows would run LDS-resident, 1024 < N <= 4096)
            if self.ess_threshold:
                sb = self.ctx.scratch_bytes_adaptive(self.model, self.dtype, N)
            else:
                sb = self.ctx.scratch_bytes_smoother(self.model, self.dtype, "device", self._smoother, N)
            if sb < 0:
                raise NotImplementedError("N = {0} is above the one-workgroup kernels' maximum (16384)".format(N))
            return sb
        # pfg_scratch_bytes answers above N = 16384 too (the whole-GPU plan's slab) where pfg_scratch_bytes_smoother says -1,
        # and 'nemeth_systematic' says -1 above N = 1024; the single-window path keeps the query it has always made
        sb = self.ctx.scratch_bytes(self.model, self.dtype, "device", N)
        if sb < 0:
            raise ValueError("N = {0} is above the supported maximum".format(N))
        return sb

    def _weights_blocks(self, bounds, S, scale=None):
        """(flat array or None, [n_seq] offsets into it): for every sequence longer than S one row of
        random_subsequence_and_weights per window start; scale [n_seq]: every row times scale[k], and a sequence no longer
        than S gets the one row of its whole window (without a scale it needs none: its weights are 1)."""
        blocks, offs, off = [], np.zeros(len(bounds) - 1, dtype=np.int64), 0
        for k, Tk in enumerate(np.diff(bounds).tolist()):
            if S > 0 and Tk > S:
                blk = np.stack([self._weights_for(st, T=Tk) for st in range(Tk - S + 1)])
            elif scale is not None:
                blk = np.ones((1, Tk))
            else:
                continue
            if scale is not None:
                blk = blk * scale[k]
            offs[k], off = off, off + blk.size
            blocks.append(blk.reshape(-1))
        return (np.concatenate(blocks) if blocks else None), offs

    # ------------------------------------------------------------------------------------
    def _weights_for(self, start, T=None):
        """weights of random_subsequence_and_weights for a given start ('uniform' style)."""
        S, T = self.S, (self.T if T is None else T)
        style = self.partition_style or 'uniform'
        if style in ('strict', 'naive'):
            return np.ones(S) * T / S
        t = np.arange(start, start + S)
        cap = np.ones_like(t) * min(S, T - S + 1)
        if start + S <= 2 * S:
            covering = np.min(np.array([t + 1, cap]), axis=0)
        elif start >= T - 2 * S - 1:
            covering = np.min(np.array([T - t, cap]), axis=0)
        else:
            covering = np.ones(S) * S
        return np.ones(S, dtype=float) * (T - S + 1) / covering

    def _prior_x(self, proto, theta_row):
        if proto is None:
            proto = self._params_from_theta(theta_row)
        return self.helper._prior_x(None, proto)

    def _params_from_theta(self, th):
        if self.model == "svm":
            return self._Parameters(A=np.eye(1) * th[0], LQinv=np.eye(1) * th[1], LRinv=np.eye(1) * th[2])
        if self.model == "lgssm":
            return self._Parameters(A=np.eye(1) * th[0], C=np.eye(1) * th[1], LQinv=np.eye(1) * th[2],
                                    LRinv=np.eye(1) * th[3])
        return self._Parameters(log_mu=th[0], logit_phi=th[1], logit_lambduh=th[2], LRinv=np.eye(1) * th[3])

    def _host_uniforms(self, salt):
        """[C] uniforms in [0,1) for the step `steps_done`, one per chain, keyed by (seed, GLOBAL chain id,
        step, salt) with a splitmix64 finaliser: a chain's window sequence does not depend on how chains
        are partitioned over ranks (chain_offset / C), nor on what other chains do."""
        M = np.uint64(0xFFFFFFFFFFFFFFFF)
        with np.errstate(over="ignore"):
            x = (np.arange(self.C, dtype=np.uint64) + np.uint64(self.chain_offset)) * np.uint64(0x9E3779B97F4A7C15)
            x ^= np.uint64(self.seed & 0xFFFFFFFFFFFFFFFF) * np.uint64(0xD1B54A32D192ED03)
            x ^= (np.uint64(self.steps_done) * np.uint64(0xBF58476D1CE4E5B9)) ^ (np.uint64(salt) * np.uint64(0x94D049BB133111EB))
            for _ in range(2):
                x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9) & M
                x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB) & M
                x = x ^ (x >> np.uint64(31))
        return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)

    def _set_windows(self, first=False):
        """Full series: static descriptors (placed once, `first`).  Otherwise draw, per chain, the sequence (lists:
        np.random.choice(K, 1)) and a window start inside it on the host (sgmcmc_sampler.py:259-288).  Either way
        y / T / t1 / tL / weights follow from (sequence, start) below, a single series being a list of one sequence: the
        window is S long, or the whole sequence when that is no longer than S; weights is the start's row of the sequence's
        block, null without a table (a full single series).  Returns whether the descriptors changed.  sampler='sgld_cv': the
        twins (the records behind the chains') take their chains' windows."""
        changed = self._set_chain_windows(self._desc[:self.C], first)
        if self._twins and (changed or first):
            for f in ("y", "T", "t1", "tL", "weights"):
                self._desc[f][self.C:] = self._desc[f][:self.C]
        return changed

    def _set_chain_windows(self, d, first):
        S, B, C, bounds = self.S, self.B, self.C, self._bounds
        static = self.segments is None and S == -1
        if static and not first:
            return False
        K = len(bounds) - 1
        seg = np.zeros(C, dtype=np.int64) if K == 1 else np.minimum((self._host_uniforms(1) * K).astype(np.int64), K - 1)
        base, Tk = bounds[seg], bounds[seg + 1] - bounds[seg]
        whole = Tk - S <= 0 if S > 0 else np.ones(C, dtype=bool)
        if static:
            start = np.zeros(C, dtype=np.int64)
        else:
            # starts to choose from: one in a whole sequence, else the S-blocks ('strict') or every offset
            span = np.where(whole, 1, Tk // S if self.strict else Tk - S + 1)
            start = np.minimum((self._host_uniforms(2) * span).astype(np.int64), span - 1)
            if self.strict:
                start = start * S
        length = np.where(whole, Tk, S)
        left = np.maximum(0, start - B)
        right = np.minimum(Tk, start + length + B)
        d["y"] = self.y_dev.data_ptr() + (base + left).astype(np.uint64) * 8
        d["T"] = right - left
        d["t1"] = start - left
        d["tL"] = start + length - left
        if self.weights_dev is not None:
            d["weights"] = self.weights_dev.data_ptr() + (self._seg_weight_offsets[seg] + start * length).astype(np.uint64) * 8
        return not static

    # ------------------------------------------------------------------------------------
    def _stream(self, stream):
        """The hipStream_t handle of `stream` (default: torch's current stream on the ensemble's device)."""
        return (stream or torch.cuda.current_stream(self.device)).cuda_stream

    def launch_pf(self, stream=None, traced=False):
        """Enqueue one particle-filter launch for all chains on `stream` (default: torch's
        current stream; kind='marginal': the exact Kalman score; kind='complete': the FFBS score).  Results land in self.out_dev[C, 8]
        (score columns, loglik).
        traced=True runs the twin instantiation that honours trace_* / rec_* buffers a caller put into
        the descriptors (tests, diagnostics); the production launch ignores them.
        The launch is the resolved family's (ensemble_settings.FILTERS): launch_descriptors, or the conditional sweep
        (launch_csmc), the sorted, correlated filter (launch_cpm) or the sequential quasi-Monte Carlo filter (launch_sqmc) on
        records of their own."""
        if traced and self.kind != "pf":
            raise ValueError("kind='{0}' has no particles to trace".format(self.kind))
        return self._launch_filter(self, stream, traced=traced)

    def launch_descriptors(self, stream=None, traced=False):
        """The launch on the window descriptors: the launch smoother (_resolve_settings), at most N particles (the Kalman
        score has none: 1) in each of _nl descriptors (_nd, and under 'sgld_cv' the twins behind them: ONE launch, so a chain
        and its twin run the same kernel instantiation)."""
        if self.ess_threshold:      # adaptive resampling: its own kernels, the family stated at launch level
            return self.ctx.launch_device_adaptive(self.model, self.kernel, self.dtype, "device", self.N, self._nl,
                                                   self.desc_dev.data_ptr(), self._stream(stream), traced=traced)
        launch, smoother = self.ctx.launch_device_smoother, self._launch_smoother
        if traced and self.pf != "paris":       # the PaRIS kernels always honour trace buffers: traced or not, the same launch
            launch, smoother = self.ctx.launch_device_traced, self._smoother
        launch(self.model, self.kernel, self.dtype, "device", smoother, 1 if self._smoother == "kalman" else self.N, self._nl,
               self.desc_dev.data_ptr(), self._stream(stream))

    def launch_update(self, stream=None):
        """The sampler's update rule (ensemble_settings.SAMPLERS); where the step has a propose / accept pair, the accept step."""
        if self._rule.update is None:
            return self.launch_accept(stream)
        self._rule.update(self, (self.model, self.C, self.theta_dev.data_ptr()), (self.out_dev.data_ptr(), self.hyper),
                          self._update_key(stream))

    def _update_key(self, stream):
        """What keys the draws of every update rule and says where it runs: seed, first chain id, the counter, the stream."""
        return (self.seed ^ 0x5DEECE66D, self.chain_offset, self.step_ctr.data_ptr(), self._stream(stream))

    def launch_propose(self, stream=None):
        """sampler='pmmh': theta_prop_dev = theta_dev + proposal_scale (.) z, valid_dev (pfg_pmmh_propose_device).
        sampler='pmala' | 'pmala_sorted': the Langevin proposal along grad_cur_dev (pfg_pmala_propose_device)."""
        self._rule.propose(self, self._update_key(stream))

    def launch_accept(self, stream=None, init=False):
        """sampler='pmmh': accept / reject on out_dev[:, 4] and the log-prior; bumps the counter (pfg_pmmh_accept_device).
        sampler='pmala' | 'pmala_sorted': the same with the two proposal densities, on out_dev[:, :5] (pfg_pmala_accept_device).
        With correlation set, either ends in the commit."""
        self._rule.accept(self, init, self._update_key(stream))
        if self._family.aux:            # a chain that accepted (init: every chain) now reads the buffer the filter wrote
            self.ctx.cpm_commit_device(self.C, self.accept_dev.data_ptr(), self.seen_dev.data_ptr(), self.which_dev.data_ptr(),
                                       init, self._stream(stream))

    def _init_launch(self):
        """The launch of an init pass at the initial parameters.  It consumes counter value 0 -- the counter is 1 afterwards,
        step s (from 0) draws with s + 1 -- so that no step's filter repeats the draws the initial state was made with."""
        self._launch_filter(self, **self._family.init)
        if self._multi:
            self.launch_reduce()
        if self._rule.accept is not None:
            self.launch_accept(init=True)
        self.step_ctr.fill_(1)
        self.synchronize()

    def _mh_init(self, s):
        """The init pass of sampler='pmmh' | 'pmala' | 'pmala_sorted', the constructor's last act: the launch at the initial
        parameters (the correlated filter: at rho = 0, fresh normals, no buffer is read), ll_dev = its out[4] (along a score:
        grad_cur_dev = its out[0..3] as well)."""
        self.theta_prop_dev.copy_(self.theta_dev)
        self._init_launch()
        finite, what = np.isfinite(self.ll_dev.cpu().numpy()), "log-likelihood"
        if self._rule.score:        # ... and the score columns the drift reads
            used = self.grad_cur_dev.cpu().numpy()[:, list(_PMALA_SCORE_COLUMNS[self.model])]
            finite, what = finite & np.all(np.isfinite(used), axis=1), "log-likelihood or score"
        bad = np.flatnonzero(~finite)
        if bad.size:
            raise ValueError("{0}: the initial {1} of chain {2} is not finite".format(self.sampler, what,
                                                                                   int(bad[0]) + self.chain_offset))

    def _launch_chain_filter(self, desc, stream, traced, *before_key):
        """One launch of the family that runs one workgroup per chain on its own records `desc`: the filter, or its score
        twin with lambduh (sampler='pmala_sorted'), under the family's key (seed ^ its salt)."""
        getattr(self.ctx, self._filter_call)(self.model, self.dtype, self.N, self.C, desc.data_ptr(), *before_key,
                                             *self._filter_score, *self._filter_key, self._stream(stream), traced=traced)

    def launch_cpm(self, stream=None, traced=False, init=False):
        """sampler='pmmh' with correlation: one sorted, correlated filter per chain on theta_prop_dev (pfg_cpm_device): U' = rho U +
        sqrt(1 - rho^2) eps goes to the chain's other buffer, the estimate on U' to out_dev[:, 4].  init: rho = 0.
        sampler='pmala_sorted': the same filter with the score beside it, out_dev[:, :H] (pfg_cpm_score_device, lambduh)."""
        self._launch_chain_filter(self.cpm_desc_dev, stream, traced, 0.0 if init else self.correlation)

    def launch_sqmc(self, stream=None, traced=False):
        """sampler='pmmh' with sqmc: one sequential quasi-Monte Carlo filter per chain on theta_prop_dev (pfg_sqmc_device), the
        estimate to out_dev[:, 4].  The init pass is the same launch at counter 0.
        sampler='pmala_sorted': the same filter with the score beside it, out_dev[:, :H] (pfg_sqmc_score_device, lambduh)."""
        self._launch_chain_filter(self.sqmc_desc_dev, stream, traced)

    def launch_csmc(self, stream=None, traced=False, init=False):
        """sampler='pgibbs': one conditional SMC sweep with ancestor sampling per chain (pfg_csmc_device): path_dev is replaced,
        the new paths' statistics land in out_dev.  init: the descriptors with has_ref = 0, an unconditional sweep."""
        self._launch_chain_filter(self._csmc_init_desc_dev if init else self.csmc_desc_dev, stream, traced)

    def _alloc_per_chain(self, make, kept, per_chain, sb, copies=1):
        """`copies` * C slabs of sb bytes in one uint8 tensor (make: torch.zeros | torch.empty); a refusal names what is kept,
        the size formula and the byte count."""
        n = copies * self.C * sb
        try:
            return make(n, dtype=torch.uint8, device=self.device)
        except RuntimeError as e:       # (torch.cuda.OutOfMemoryError is one)
            times = "{0} * ".format(copies) if copies != 1 else ""
            raise MemoryError("{0}: {1}C * {2} = {1}{3} * {4} = {5} bytes ({6:.2f} GB) could not be allocated ({7})".format(
                kept, times, per_chain, self.C, sb, n, n / 1e9, str(e).splitlines()[0])) from e

    def _chain_filter_records(self, theta, prior_mean, prior_var):
        """(d, idx): C records of the family's descriptor (pfg_csmc_problem | pfg_cpm_problem | pfg_sqmc_problem) with what all
        have filled in -- chain b reads row b of `theta` and the whole series, writes row b of out_dev -- and the chain indices as uint64."""
        idx = np.arange(self.C, dtype=np.uint64)
        d = np.zeros(self.C, dtype=self._family.dtype)
        d["theta"] = theta.data_ptr() + idx * np.uint64(8 * _capi.MAX_THETA)
        d["y"] = self.y_dev.data_ptr()
        d["out"] = self.out_dev.data_ptr() + idx * np.uint64(8 * _capi.OUT_DOUBLES)
        d["prior_mean"], d["prior_var"], d["T"], d["N"] = prior_mean, prior_var, self.T, self.N
        return d, idx

    def _upload_records(self, d):
        return torch.from_numpy(d.view(np.uint8).reshape(len(d), -1)).to(self.device)

    def _sqmc_alloc(self, prior_mean, prior_var):
        """The pfg_sqmc_problem records (static: the step replays in hipGraphs).  An SQMC chain carries nothing beyond PMMH's
        state."""
        self._sqmc_desc, _ = self._chain_filter_records(self.theta_prop_dev, prior_mean, prior_var)
        self.sqmc_desc_dev = self._upload_records(self._sqmc_desc)

    def _cpm_alloc(self, prior_mean, prior_var):
        """The state of a correlated chain beyond PMMH's: two buffers of normals per chain (aux_dev, [2][C] slabs of
        pfg_cpm_aux_bytes(T, N) bytes), the selector which_dev, the acceptance count seen_dev the selector was last moved at, and
        the pfg_cpm_problem records (static: the step replays in hipGraphs).  The init pass fills the first buffer."""
        C, T, N, dev = self.C, self.T, self.N, self.device
        sb = self._aux_bytes = _capi.cpm_aux_bytes(T, N)
        self.aux_dev = self._alloc_per_chain(torch.zeros, "correlation keeps two buffers of normals per chain in HBM",
                                             "pfg_cpm_aux_bytes(T, N)", sb, 2)
        self.which_dev = torch.zeros(C, dtype=torch.int32, device=dev)
        self.which_dev.fill_(1)          # the init pass writes buffer 0 and commits: every chain then reads buffer 0
        self.seen_dev = torch.zeros(C, dtype=torch.int64, device=dev)        # (the library's uint64 counts)
        d, idx = self._chain_filter_records(self.theta_prop_dev, prior_mean, prior_var)
        d["u0"] = self.aux_dev.data_ptr() + idx * np.uint64(sb)
        d["u1"] = self.aux_dev.data_ptr() + (idx + np.uint64(C)) * np.uint64(sb)
        d["which"] = self.which_dev.data_ptr() + idx * np.uint64(4)
        self._cpm_desc = d
        self.cpm_desc_dev = self._upload_records(d)

    def _aux_view(self):
        """aux_dev as [2, C, doubles per slab]."""
        return self.aux_dev.view(torch.float64).view(2, self.C, self._aux_bytes // 8)

    def aux(self):
        """sampler='pmmh' with correlation: [C, T+1, N+1] the normals each chain holds, those its estimate loglik() was
        computed from."""
        self._need("aux")
        rows = torch.arange(self.C, device=self.device)
        cur = self._aux_view()[self.which_dev.long() & 1, rows]
        return cur[:, :(self.T + 1) * (self.N + 1)].reshape(self.C, self.T + 1, self.N + 1).cpu().numpy()

    def _csmc_alloc(self, prior_mean, prior_var):
        """The state of sampler='pgibbs': path_dev [C, T], the counters, the scratch and the pfg_csmc_problem records (static:
        the step replays in hipGraphs), with a copy at has_ref = 0 for the init pass."""
        C, T, N, dev = self.C, self.T, self.N, self.device
        self.path_dev = torch.zeros((C, T), dtype=torch.float64, device=dev)
        self.ndeg_dev = torch.zeros(C, dtype=torch.int64, device=dev)       # (the library's uint64 counts)
        sb = _capi.csmc_scratch_bytes(T, N)
        self.csmc_scratch_dev = self._alloc_per_chain(torch.empty, "sampler='pgibbs' keeps every chain's particle history in HBM",
                                                      "pfg_csmc_scratch_bytes(T, N)", sb)
        d, idx = self._chain_filter_records(self.theta_dev, prior_mean, prior_var)
        d["path"] = self.path_dev.data_ptr() + idx * np.uint64(8 * T)
        d["scratch"] = self.csmc_scratch_dev.data_ptr() + idx * np.uint64(sb)
        d["n_degenerate"] = self.ndeg_dev.data_ptr() + idx * np.uint64(8)
        d["has_ref"] = 1
        self._csmc_desc = d
        self.csmc_desc_dev = self._upload_records(d)
        d0 = d.copy()
        d0["has_ref"] = 0
        self._csmc_init_desc_dev = self._upload_records(d0)

    def _pgibbs_init(self, s):
        """The init pass of sampler='pgibbs', the constructor's last act: one sweep with has_ref = 0 at the initial parameters
        for the first paths."""
        self._init_launch()
        bad = np.flatnonzero(self.ndeg_dev.cpu().numpy() != 0)
        if bad.size:
            raise ValueError("pgibbs: the particle weights of chain {0} degenerated in the init pass (no first path)".format(
                int(bad[0]) + self.chain_offset))

    def launch_windows(self, stream=None):
        """Device-side window sampling (window_sampling='device'): rewrite y / T / t1 / tL / weights of
        every descriptor for the step *step_ctr is at.  No-op for full-sequence chains.  Multi-window path: all
        C * W descriptors and their sequence lengths (pfg_sample_windows_multi_device)."""
        weights = self.weights_dev.data_ptr() if self.weights_dev is not None else 0
        # sampler='sgld_cv': the twins' records are sampled again under the chains' key, so they hold the chains' windows
        halves = [(self.desc_dev.data_ptr(), self.seq_len_dev.data_ptr() if self._multi else 0)]
        if self._twins:
            halves.append((self.desc_dev.data_ptr() + self._nd * self.desc_dev.shape[1],
                           self.twin_seq_len_dev.data_ptr() if self._multi else 0))
        for desc, seq_len in halves:
            if self._multi:
                self.ctx.sample_windows_multi_device(
                    self.C, self.bounds_dev.numel() - 1, self.bounds_dev.data_ptr(), self.woffs_dev.data_ptr(),
                    self.num_sequences if self.segments is not None else -1, self.M, desc, seq_len, self.y_dev.data_ptr(),
                    weights, self.S, self.B, self.strict, self.seed ^ 0x4D554C5449574E44, self.chain_offset,
                    self.step_ctr.data_ptr(), self._stream(stream))
            elif self.S != -1:
                self.ctx.sample_windows_device(
                    self.C, desc, self.y_dev.data_ptr(), weights, self.T, self.S, self.B, self.strict,
                    self.seed ^ 0x2545F4914F6CDD1D, self.chain_offset, self.step_ctr.data_ptr(), self._stream(stream))

    def launch_reduce(self, stream=None):
        """Multi-window path: the C * W window records -> the C records the update reads (pfg_reduce_windows_device)."""
        self.ctx.reduce_windows_device(self.C, self.K_eff, self.M, self.win_out_dev.data_ptr(), self.seq_len_dev.data_ptr(),
                                       self._rescale, float(self.T), self.out_dev.data_ptr(), self._stream(stream))
        if self._twins:        # the twins' window records -> out_centre_dev
            self.ctx.reduce_windows_device(self.C, self.K_eff, self.M, self.twin_out_dev.data_ptr(),
                                           self.twin_seq_len_dev.data_ptr(), self._rescale, float(self.T),
                                           self.out_centre_dev.data_ptr(), self._stream(stream))

    def _enqueue_step(self):
        """One step: the windows if there are any to draw, then `_step`: the proposal if the sampler has one, the filter,
        the reduction on the multi-window path, the update."""
        if self._window_draws == "device":
            self.launch_windows()
        elif self._window_draws == "host" and self.steps_done > 0 and self._set_windows():
            self.desc_dev.copy_(torch.from_numpy(self._desc.view(np.uint8).reshape(self._nl, -1)),
                                non_blocking=True)
        for launch in self._step:
            launch(self)

    def step(self, num_steps=1):
        """num_steps x (the sampler's step + project_parameters) for every chain.  Asynchronous."""
        for _ in range(num_steps):
            self._enqueue_step()
            self.steps_done += 1

    def _graph(self, K):
        """A hipGraph of K whole steps (window sampling, particle filter, update -- 3K kernel nodes).
        Every input that changes between steps (parameters, descriptors, RNG step counter) lives
        in HBM and is advanced by the kernels themselves, so replaying the graph IS running K
        more steps; it is bitwise the same computation as K eager steps."""
        if not self._multi and self.S != -1 and self.window_sampling != "device":
            raise ValueError("graph capture needs window_sampling='device' (or full-sequence chains): "
                             "host-side window sampling cannot be replayed")
        g = self._graphs.get(K)
        if g is None:
            # one eager step first (code-object load, LDS-size attributes), undone afterwards so
            # that building the graph does not advance the chains
            carried, scratch = self._chain_state()
            state = [self.theta_dev, self.momentum_dev, self.step_ctr] + scratch + [t for _, t in carried]
            snap = [t.clone() for t in state]
            self._enqueue_step()
            self.synchronize()
            for t, c in zip(state, snap):
                t.copy_(c)
            self.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(K):
                    self._enqueue_step()
            self._graphs[K] = g
        return g

    def run(self, num_steps, thin=1, graph_steps=0):
        """num_steps steps, keeping every `thin`-th state: returns ndarray [num_steps // thin, C, P].
        Samples are staged in HBM and copied to the host once at the end.  graph_steps = K > 0
        replays a captured hipGraph of K steps per launch (K must divide `thin`); worth it when a
        step is launch-bound (short buffered windows, few chains)."""
        keep = num_steps // thin
        buf = torch.empty((max(keep, 1), self.C, self.P), dtype=torch.float64, device=self.device)
        K = int(graph_steps)
        if K > 0 and thin % K != 0:
            raise ValueError("graph_steps must divide thin")
        g = self._graph(K) if K > 0 else None
        it = k = 0
        while it < num_steps:
            if g is not None and num_steps - it >= K:
                g.replay()
                self.steps_done += K
                it += K
            else:
                self.step(1)
                it += 1
            if it % thin == 0 and k < keep:
                buf[k].copy_(self.theta_dev[:, :self.P])
                k += 1
        return buf[:keep].cpu().numpy()

    # -- checkpoint / resume (the reference checkpoints parameters with joblib around its fit loop,
    #    svm/driver.py:362-408; here the whole ensemble state is a few small arrays) -------------
    def state_dict(self):
        self.synchronize()
        state = dict(theta=self.theta_dev.cpu().numpy(), momentum=self.momentum_dev.cpu().numpy(),
                     step_ctr=int(self.step_ctr.item()), steps_done=int(self.steps_done),
                     seed=self.seed, chain_offset=self.chain_offset,
                     model=self.model, N=self.N, C=self.C, ess_threshold=self.ess_threshold)
        # what names the sampler and the filter family (load_state_dict), then what a chain carries
        state.update((key, getattr(self, key)) for key in self._rule.names)
        state.update((key, getattr(self, attr)) for key, attr in self._family.checkpoint)
        state.update((key, t.cpu().numpy()) for key, t in self._chain_state()[0])
        if self._family.aux:        # the current buffer only (the other one is a step's scratch)
            state["aux"] = self.aux()
        return state

    def _chain_state(self):
        """(carried, scratch).  carried: what a chain carries beyond theta, the momentum and the counter, as ordered
        (checkpoint key, tensor) pairs: the sampler's record's, then the filter family's (ensemble_settings: `carries`).
        state_dict and load_state_dict follow it.  scratch: what a step overwrites besides; _graph restores both after its
        eager step."""
        carried = [(key, getattr(self, attr)) for key, attr in self._carries]
        scratch = [self.desc_dev] + ([self.theta_prop_dev, self.valid_dev] if self._rule.propose is not None else [])
        return carried, scratch

    def load_state_dict(self, state):
        # a checkpoint that names its sampler is taken by that sampler alone ('pgibbs': another would drop the path silently),
        # and a sampler that names itself wants its names; correlation and sqmc are compared whoever wrote the checkpoint
        # (either side may be a plain PMMH chain: None, False), ess_threshold likewise (checkpoints from before the option: None)
        def same(key, got):
            if got != getattr(self, key):
                raise ValueError("checkpoint {0} = {1} does not match the ensemble ({2})".format(key, got, getattr(self, key)))
        for key in self._rule.names or (("sampler",) if state.get("sampler", None) is not None else ()):
            same(key, state.get(key, None))
        for key in ("model", "N", "C", "seed", "chain_offset"):
            same(key, state[key])
        same("correlation", state.get("correlation", None))
        same("sqmc", bool(state.get("sqmc", False)))
        if self._family.aux:
            shape = (self.C, self.T + 1, self.N + 1)
            if state.get("T", None) != self.T or tuple(np.shape(state["aux"])) != shape:
                raise ValueError("checkpoint T = {0}, aux {1} does not match the ensemble (T = {2}, aux {3})".format(
                    state.get("T", None), tuple(np.shape(state["aux"])), self.T, shape))
        same("ess_threshold", state.get("ess_threshold", None))
        self.theta_dev.copy_(torch.from_numpy(np.ascontiguousarray(state["theta"])))
        self.momentum_dev.copy_(torch.from_numpy(np.ascontiguousarray(state["momentum"])))
        self.step_ctr.fill_(int(state["step_ctr"]))
        for key, t in self._chain_state()[0]:
            dtype = {torch.int64: np.int64, torch.int32: np.int32}.get(t.dtype, np.float64)
            t.copy_(torch.from_numpy(np.ascontiguousarray(state[key], dtype=dtype)))
        if self._family.aux:        # into the buffer each chain's selector (just loaded) names
            flat = torch.from_numpy(np.ascontiguousarray(state["aux"], dtype=np.float64).reshape(self.C, -1)).to(self.device)
            view, rows = self._aux_view(), torch.arange(self.C, device=self.device)
            view[self.which_dev.long() & 1, rows, :flat.shape[1]] = flat
        self.steps_done = int(state["steps_done"])       # host window draws are keyed by (seed, chain, steps_done)
        self.synchronize()

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    # -- measurement hooks ---------------------------------------------------------------------
    def enable_stamps(self):
        """Point every descriptor at a [C, 16] uint64 stamp record (pfg_dev_problem.stamps): the PF
        kernel's wave 0 then writes s_memtime / s_memrealtime at its start and end (two scalar
        instructions outside the T-loop).  Multi-window path: one record per window, [C * W, 16]."""
        if self._multi:         # the device wrote the windows: start from its copy
            self._desc = self.desc_dev.cpu().numpy().reshape(-1).view(_capi.DEV_PROBLEM_DTYPE).copy()
        self.stamps_dev = torch.zeros((self._nl, _capi.STAMP_WORDS), dtype=torch.int64, device=self.device)
        self._desc["stamps"] = self.stamps_dev.data_ptr() + np.arange(self._nl, dtype=np.uint64) * np.uint64(8 * _capi.STAMP_WORDS)
        self.desc_dev.copy_(torch.from_numpy(self._desc.view(np.uint8).reshape(self._nl, -1)))
        self.synchronize()

    def kernel_clock(self):
        """From the stamps of the latest PF launch: (median in-kernel shader clock in GHz, median
        workgroup lifetime in shader cycles, per-phase cycle sums [10] or None).  The phase sums are
        filled by diagnostic builds only (-DPFG_PHASE_STAMPS)."""
        st = self.stamps_dev.cpu().numpy().astype(np.uint64)
        cyc = (st[:, 2] - st[:, 0]).astype(np.float64)
        real = (st[:, 3] - st[:, 1]).astype(np.float64)          # 100 MHz ticks
        ok = real > 0
        ghz = float(np.median(cyc[ok] / real[ok] * 0.1)) if ok.any() else float("nan")
        phases = st[:, 4:14].sum(axis=0).astype(np.float64)
        return ghz, float(np.median(cyc[ok])) if ok.any() else float("nan"), (phases if phases.sum() > 0 else None)

    # ------------------------------------------------------------------------------------
    def theta(self):
        """Current raw parameters of all chains, ndarray [C, P] (synchronises)."""
        return self.theta_dev[:, :self.P].cpu().numpy()

    def last_gradient_statistics(self):
        """[C, h] score estimates and [C] log-likelihood estimates of the latest PF launch (kind='marginal':
        the exact window scores and forward log-likelihoods).  sampler='gibbs': the [C, 7] sufficient statistics of
        the latest FFBS paths (PFG_STAT_GIBBS: sum_{t>=1} x_{t-1}^2, x_t x_{t-1}, x_t^2; sum_t x_t^2, y_t x_t, y_t^2;
        T) and None: a sampled path has no log-likelihood estimate.  Multi-window path: the REDUCED records
        (pfg_reduce_windows_device); window_statistics() has the windows'."""
        return self._rule.statistics(self.out_dev.cpu().numpy(), _capi.STAT_DIM[self.model])

    def loglik(self):
        """sampler='pmmh' | 'pmala': [C] log-likelihood estimates the chains hold, each the one its current state was
        accepted with."""
        self._need("loglik")
        return self.ll_dev.cpu().numpy()

    def score(self):
        """sampler='pmala': [C, h] score estimates the chains hold (score-column order, as last_gradient_statistics), each
        the one its current state was accepted with and its next proposal drifts along."""
        self._need("score")
        return self.grad_cur_dev[:, :_capi.STAT_DIM[self.model]].cpu().numpy()

    def path(self):
        """sampler='pgibbs': [C, T] latent paths the chains hold."""
        self._need("path")
        return self.path_dev.cpu().numpy()

    def suff_stats(self):
        """sampler='pgibbs': [C, 7] statistics of the latest paths, as last_gradient_statistics()[0] (SVM: the three transition
        sums, sum_t y_t^2 exp(-x_t), 0, 0, T)."""
        self._need("suff_stats")
        return self.out_dev[:, :7].cpu().numpy()

    def n_degenerate(self):
        """sampler='pgibbs': [C] sweeps in which a chain kept its path because its weights degenerated."""
        self._need("n_degenerate")
        return self.ndeg_dev.cpu().numpy()

    def acceptance_rate(self):
        """sampler='pmmh' | 'pmala': [C] accepted proposals / steps done (nan before the first step)."""
        self._need("acceptance_rate")
        n = self.accept_dev.cpu().numpy().astype(np.float64)
        return n / self.steps_done if self.steps_done else np.full(self.C, np.nan)

    def window_statistics(self):
        """Multi-window path: the latest launch's [C, W, 8] window records and [C, W] sequence lengths."""
        return (self.win_out_dev.cpu().numpy().reshape(self.C, self.W, _capi.OUT_DOUBLES),
                self.seq_len_dev.cpu().numpy().reshape(self.C, self.W))

    def parameters_list(self):
        return [self._params_from_theta(th) for th in self.theta()]

    def gather_samples(self):
        """All ranks' current samples [world*C, P] on every rank, in global chain order: the one
        collective of the multi-GPU path (RCCL all_gather over xGMI; a few KB, latency-bound)."""
        from . import distributed
        return distributed.gather_samples(self.theta_dev[:, :self.P].contiguous())
