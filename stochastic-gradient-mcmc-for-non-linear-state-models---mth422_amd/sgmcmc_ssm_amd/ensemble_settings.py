"""What a ChainEnsemble is made of, stated once and without a device: the sampler table, the filter-family table, the
resolution of the constructor's arguments and every refusal that needs no GPU.  Imports neither torch nor a device; ensemble.py
walks the two tables, the host tests call resolve_settings and window_counts through ChainEnsemble's static names.

SAMPLERS: one record per sampler name -- what its step runs and what its chains carry.
FILTERS:  one record per family of filter launch -- the window descriptors (pfg_dev_problem, every smoother of
          pfg_launch_device*), and the three kernel families that run one workgroup per chain on records of their own:
          'csmc' (conditional SMC, sampler='pgibbs'), 'cpm' (the sorted, correlated filter: correlation=rho) and 'sqmc' (the
          sorted filter on Sobol' points: sqmc=True).  filter_family resolves (sampler, correlation, sqmc) to one of them.
A new sampler is one record of SAMPLERS (and its update rule, if it has one of its own); a new kernel family one of FILTERS,
its launch_<family> and _<family>_alloc in ensemble.py.
"""
import collections
import types

import numpy as np

from . import _capi
from .particle_filters import resolve_resampling


# -- the update rules: (ensemble, (model, C, theta), (out, hyper), _update_key(stream)) -----------------------------------------
def _sgld(e, theta, out, key):
    e.ctx.sgld_update_device(*theta, *out, e.epsilon, float(e.T), *key)


def _sghmc(e, theta, out, key):
    e.ctx.sghmc_update_device(*theta, e.momentum_dev.data_ptr(), *out, e.epsilon, e.friction, float(e.T), *key)


def _sgrld(e, theta, out, key):
    e.ctx.sgrld_update_device(*theta, *out, e.epsilon, float(e.T), *key)


def _gibbs(e, theta, out, key):
    e.ctx.gibbs_update_device(*theta, *out, *key)


def _pgibbs(e, theta, out, key):
    e.ctx.pgibbs_update_device(*theta, *out, *key)


def _sgd(e, theta, out, key):       # (the optimisers draw nothing: the counter and the stream alone)
    e.ctx.sgd_update_device(*theta, *out, e.epsilon, float(e.T), *key[2:])


def _adagrad(e, theta, out, key):
    e.ctx.adagrad_update_device(*theta, e.moment_dev.data_ptr(), *out, e.epsilon, float(e.T), *key[2:])


def _sgld_cv(e, theta, out, key):
    e.ctx.sgld_cv_update_device(*theta, out[0], e.out_centre_dev.data_ptr(), e.centre_grad_dev.data_ptr(), out[1], e.epsilon,
                                float(e.T), *key)


# -- the propose / accept pairs: (ensemble, _update_key(stream)) and (ensemble, init, _update_key(stream)) -----------------------
def _pmmh_propose(e, key):
    e.ctx.pmmh_propose_device(e.model, e.C, e.theta_dev.data_ptr(), e.theta_prop_dev.data_ptr(), e.valid_dev.data_ptr(),
                              e.scale_dev.data_ptr(), *key)


def _pmmh_accept(e, init, key):
    e.ctx.pmmh_accept_device(e.model, e.C, e.theta_dev.data_ptr(), e.theta_prop_dev.data_ptr(), e.valid_dev.data_ptr(),
                             e.out_dev.data_ptr(), e.ll_dev.data_ptr(), e.accept_dev.data_ptr(), e.hyper, init, *key)


def _pmala_propose(e, key):
    e.ctx.pmala_propose_device(e.model, e.C, e.theta_dev.data_ptr(), e.grad_cur_dev.data_ptr(), e.theta_prop_dev.data_ptr(),
                               e.valid_dev.data_ptr(), e.scale_dev.data_ptr(), e.hyper, *key)


def _pmala_accept(e, init, key):
    e.ctx.pmala_accept_device(e.model, e.C, e.theta_dev.data_ptr(), e.theta_prop_dev.data_ptr(), e.valid_dev.data_ptr(),
                              e.out_dev.data_ptr(), e.ll_dev.data_ptr(), e.grad_cur_dev.data_ptr(), e.accept_dev.data_ptr(),
                              e.hyper, e.scale_dev.data_ptr(), init, *key)


# -- what last_gradient_statistics returns of out [C, 8]; h: the model's score columns ------------------------------------------
def _score_and_loglik(out, h):
    return out[:, :h], out[:, 4]


def _loglik_alone(out, h):          # no score is computed: the log-likelihood estimates at the latest PROPOSALS
    return None, out[:, 4]


def _suff_stats(out, h):            # the statistics of the latest paths; a sampled path has no log-likelihood estimate
    return out[:, :7], None


# update:     the rule launch_update runs (None: the accept step is the update)
# propose, accept: the pair of a Metropolis-Hastings step (None: the step has none) -- a proposal in theta_prop_dev, the
#             filter on it, the accept step; `score`: the proposal drifts along the filter's score (grad_cur_dev), so a sorted
#             filter runs its score twin and the init pass wants a finite score too
# twins:      every descriptor has a twin at the centre, in the same launch
# filter:     the kernel family the sampler's step runs whatever else is set (None: filter_family decides)
# alloc, init: ChainEnsemble's methods that allocate what the sampler's step needs before the descriptors are built, and that
#             run its init pass as the constructor's last act
# carries:    what a chain carries beyond theta, the momentum and the counter: ordered (checkpoint key, attribute) pairs
# names:      the keys that name the sampler in a checkpoint: state_dict writes them, load_state_dict wants them equal
# statistics: what last_gradient_statistics returns
# accessors:  the methods that are the sampler's own (ACCESSORS has their refusals)
_Sampler = collections.namedtuple(
    "_Sampler", "update propose accept score twins filter alloc init carries names statistics accessors",
    defaults=(None, None, None, False, False, None, None, None, (), (), _score_and_loglik, ()))
_MH = dict(alloc="_mh_alloc", init="_mh_init", accessors=("loglik", "acceptance_rate"))
_PMALA = dict(_MH, propose=_pmala_propose, accept=_pmala_accept, score=True,
              carries=(("ll", "ll_dev"), ("grad", "grad_cur_dev"), ("n_accept", "accept_dev")),
              accessors=_MH["accessors"] + ("score",))
SAMPLERS = {
    "sgld": _Sampler(_sgld),
    "sghmc": _Sampler(_sghmc),
    "sgrld": _Sampler(_sgrld),
    "gibbs": _Sampler(_gibbs, statistics=_suff_stats),
    "pmmh": _Sampler(propose=_pmmh_propose, accept=_pmmh_accept, carries=(("ll", "ll_dev"), ("n_accept", "accept_dev")),
                     statistics=_loglik_alone, **_MH),
    "pmala": _Sampler(**_PMALA),
    # (named in its checkpoints, so that no other sampler takes one; the smoother's lambduh)
    "pmala_sorted": _Sampler(names=("sampler", "lambduh"), **_PMALA),
    # (the path and the count travel with the csmc family; named with T, so that no other sampler drops the path silently)
    "pgibbs": _Sampler(_pgibbs, filter="csmc", init="_pgibbs_init", names=("sampler", "T"), statistics=_suff_stats,
                       accessors=("path", "suff_stats", "n_degenerate")),
    "sgd": _Sampler(_sgd),
    "adagrad": _Sampler(_adagrad, alloc="_adagrad_alloc", carries=(("moment", "moment_dev"),), accessors=("moment",)),
    # (a step moves none of the three; they travel with the checkpoint)
    "sgld_cv": _Sampler(_sgld_cv, twins=True, init="_cv_init",
                        carries=(("centre", "theta_centre_dev"), ("centre_gradient", "centre_grad_dev"),
                                 ("centre_ctr", "centre_ctr_dev")),
                        accessors=("centre", "centre_gradient", "cv_statistics", "set_centre")),
}

# accessor -> whom its refusal says it belongs to ({0}: the sampler the ensemble runs)
_RUNS = ", this ensemble runs '{0}'"
ACCESSORS = dict(
    [(a, "sampler='sgld_cv'" + _RUNS) for a in SAMPLERS["sgld_cv"].accessors] +
    [(a, "sampler='pgibbs'" + _RUNS) for a in SAMPLERS["pgibbs"].accessors] +
    [(a, "sampler='pmmh' (and 'pmala')" + _RUNS) for a in _MH["accessors"]],
    moment="sampler='adagrad'" + _RUNS, score="sampler='pmala'" + _RUNS,
    aux="sampler='pmmh' with correlation set (and sampler='pmala_sorted' with it)")


def _refuse_rho(a):
    try:
        rho = float(a.correlation)
    except (TypeError, ValueError):
        rho = float("nan")
    if not 0.0 <= rho < 1.0:        # (false for a NaN as well)
        raise ValueError("correlation must lie in [0, 1) (rho of U' = rho U + sqrt(1 - rho^2) eps; 0: fresh normals at every "
                         "step), got {0}".format(a.correlation))


def _refuse_no_power_of_two(a):
    N = int(a.N)
    if N & (N - 1):
        raise NotImplementedError(FILTERS["sqmc"].refusal["what"] + "takes the first 2^m points of the Sobol' sequence, a "
                                  "(0, m, 2)-net: N must be a power of two, got N = {0}".format(N))


# launch, score: the library call of the family's filter and of its twin that carries the O(N) score beside the estimate
#             (None: the descriptors' launch is the resolved smoother's, ChainEnsemble.launch_descriptors; no twin)
# dtype:      the numpy mirror of the family's records
# salt:       the family's filter draws under seed ^ salt
# alloc:      ChainEnsemble's method that allocates what the family carries and its records (static: the step replays in
#             hipGraphs); init: the keywords of the family's launch in an init pass
# carries:    as a sampler's, and behind them in a chain's state
# checkpoint: what state_dict adds to name the family, as (key, attribute) pairs; accessors: as a sampler's
# aux:        the family keeps two buffers of normals per chain (aux_dev) and a selector: a commit behind the accept step moves
#             the selector of a chain that accepted, and the current buffer travels in the checkpoint as 'aux'
# refusal:    the wording of refuse_chain_filter -- the prefix, the reason clause of each shared check, the largest N, why
#             pMALA cannot have the option -- and `last`, the family's own check behind the shared ones
_Filter = collections.namedtuple("_Filter", "launch score dtype salt alloc init carries checkpoint accessors aux refusal last",
                                 defaults=(None, None, {}, (), (), (), False, None, None))
FILTERS = {
    "descriptors": _Filter(None, None, _capi.DEV_PROBLEM_DTYPE),
    "csmc": _Filter(
        "csmc_device", None, _capi.CSMC_PROBLEM_DTYPE, 0x43534D43, "_csmc_alloc", dict(init=True),
        carries=(("path", "path_dev"), ("n_degenerate", "ndeg_dev")),
        refusal=dict(
            what="sampler='pgibbs' (conditional SMC with ancestor sampling, then the conjugate draw) ",
            garch="GARCH's prior has no conjugate draw", lists="samples the path of one series",
            whole="samples the path of the whole series", window="draws one path per chain and step", own="sweep",
            resampling="resamples multinomially inside the conditional sweep", inside="the conditional sweep",
            particles=" and needs a free particle beside the reference", max_n=_capi.CSMC_MAX_N)),
    "cpm": _Filter(
        "cpm_device", "cpm_score_device", _capi.CPM_PROBLEM_DTYPE, 0x43504D4D, "_cpm_alloc", dict(init=True),
        # the selector names the chain's current buffer and a step writes the other one only, so restoring the selector
        # restores the buffer; the normals themselves travel as 'aux', the current buffer only
        carries=(("which", "which_dev"), ("seen", "seen_dev")), checkpoint=(("correlation", "correlation"), ("T", "T")),
        accessors=("aux",), aux=True, last=_refuse_rho,
        refusal=dict(
            what="correlation (correlated pseudo-marginal PMMH: the sorted filter on normals the chain carries) ",
            garch="the sort orders a scalar state, GARCH's has two components", lists="carries the normals of one series",
            whole="filters the whole series", window="runs one filter per chain and step", own="filter",
            resampling="resamples systematically in the order of the states, on a uniform it carries: resampling stays at its "
                       "default", inside="the sorted filter", particles="", max_n=_capi.CPM_MAX_N,
            pmala=" (pMALA would need a score that is smooth in the normals as well)")),
    "sqmc": _Filter(
        "sqmc_device", "sqmc_score_device", _capi.SQMC_PROBLEM_DTYPE, 0x53514D43, "_sqmc_alloc",
        # (no state of its own: the setting alone, so that a plain PMMH checkpoint is what it was)
        checkpoint=(("sqmc", "sqmc"),), last=_refuse_no_power_of_two,
        refusal=dict(
            what="sqmc (PMMH on sequential quasi-Monte Carlo: the sorted filter on one randomised Sobol' point set per step) ",
            garch="the sort orders a scalar state, GARCH's has two components", lists="filters one series",
            whole="filters the whole series", window="runs one filter per chain and step", own="filter",
            resampling="resamples in the order of the states on the first coordinate of its point set: resampling stays at its "
                       "default", inside="the sorted filter", particles="", max_n=_capi.SQMC_MAX_N,
            pmala=" (pMALA would need the score on the point set: not built)")),
}


def filter_family(sampler, correlation, sqmc):
    """The key of FILTERS a step of (sampler, correlation, sqmc) launches."""
    return SAMPLERS[sampler].filter or ("cpm" if correlation is not None else "sqmc" if sqmc else "descriptors")


def resolve_settings(model, observations, parameters=None, num_chains=None, N=1000, pf="poyiadjis_N", lambduh=None,
                     subsequence_length=-1, buffer_length=-1, dtype="f64", partition_style=None,
                     resampling="multinomial", sampler="sgld", window_sampling="host", kind="pf", num_samples=None,
                     Ntilde=2, max_accept_reject=None, accept_reject=True, minibatch_size=None, num_sequences=None,
                     ess_threshold=None, proposal_scale=None, pmmh_stat=None, kernel=None, correlation=None, sqmc=False,
                     centre=None, centre_repeats=1, centre_N=None):
    """The constructor's arguments -> the resolved settings (a namespace), or the refusal: every decision that needs no
    device is made here and nowhere else, so it runs (and is tested) without a GPU.

    kind, pf, N (kind='complete': num_samples), lambduh; smoother (what the descriptors say) and launch_smoother (what the
    launch states: 'poyiadjis_n' for 'nemeth' with lambduh = 1); stat; paris (the descriptors' PaRIS fields, {} otherwise),
    Ntilde, max_accept_reject; M, K, W, multi; S, B, strict; y (the concatenated series), T, segments ([K+1] offsets
    into y, None for a single series), bounds (segments, or [0, T]); multi: draws, rescale; theta0 [C, P], proto;
    ess_threshold (None unless adaptive resampling is on); proposal_scale ([MAX_THETA] doubles, None unless sampler =
    'pmmh' | 'pmala'); correlation (rho as a float, None unless the correlated pseudo-marginal filter is on); sampler =
    'sgld_cv' alone: centre_repeats, centre_N (the particles of the centring launches: N unless given); sqmc set alone:
    sqmc = True (a namespace without it is today's)."""
    a = types.SimpleNamespace(**locals())       # the arguments by name, as the refusals read them
    tau = None
    if sampler == "sgld_cv":
        _refuse_cv(a)
    elif centre is not None or centre_N is not None or centre_repeats != 1:
        raise ValueError("centre, centre_repeats and centre_N belong to sampler='sgld_cv' (SGLD with control variates), got "
                         "sampler = '{0}'".format(sampler))
    if sampler == "pmala_sorted":
        _refuse_pmala_sorted(a)
        correlation = None if sqmc else float(correlation)
    elif correlation is not None:
        _refuse_pmmh_filter("cpm", a)
        correlation = a.correlation = float(correlation)
    if sqmc and sampler != "pmala_sorted":
        _refuse_pmmh_filter("sqmc", a)
    if sampler == "pgibbs":
        refuse_chain_filter("csmc", a)
    if ess_threshold is not None and ess_threshold != 0 and (kind != "pf" or sampler == "gibbs"):
        # (what else adaptive resampling is not built for: resolve_resampling, below)
        raise NotImplementedError("adaptive resampling (ess_threshold) needs a particle filter: kind='pf'")
    if sampler not in SAMPLERS:     # (the wording and its order are older than the table's)
        raise ValueError("sampler must be 'sgld', 'sghmc', 'sgrld', 'sgd', 'adagrad', 'sgld_cv', 'pgibbs', 'pmala_sorted', "
                         "'pmala', 'gibbs' or 'pmmh'")
    mh = SAMPLERS[sampler].propose is not None
    scale = None
    if not mh:
        if proposal_scale is not None:
            raise ValueError("proposal_scale is the random walk of sampler='pmmh', got sampler = '{0}'".format(sampler))
        if pmmh_stat is not None:
            raise ValueError("pmmh_stat belongs to sampler='pmmh', got sampler = '{0}'".format(sampler))
    else:
        # particle marginal Metropolis-Hastings and particle MALA (extensions): what they are not built for is refused
        # by name
        if sampler == "pmala":
            _refuse_pmmh_stat(a)
        if proposal_scale is None:
            raise ValueError("sampler='{0}' needs proposal_scale: a positive scalar or a length-P vector in raw-theta "
                             "units".format(sampler))
        P = _capi.THETA_DIM[model]
        ps = np.asarray(proposal_scale, dtype=np.float64).reshape(-1)
        if ps.size not in (1, P) or not np.all(np.isfinite(ps)) or not np.all(ps > 0.0):
            raise ValueError("proposal_scale must be a positive scalar or a positive vector of length {0}, got {1}".format(
                P, proposal_scale))
        scale = np.zeros(_capi.MAX_THETA)
        scale[:P] = ps
        if kind == "complete":
            raise NotImplementedError("sampler='{0}' accepts on a log-likelihood estimate: kind='pf' or kind='marginal' "
                                      "(kind='complete' samples paths and has none)".format(sampler))
        if kind == "pf" and pf not in ("poyiadjis_N", "nemeth"):
            if sampler == "pmmh":
                raise NotImplementedError("sampler='pmmh' reads the filter's log-likelihood only: pf = 'poyiadjis_N' | "
                                          "'nemeth' (the smoothing of pf = '{0}' would be thrown away)".format(pf))
            raise NotImplementedError("sampler='pmala' drifts along the O(N) filter's score: pf = 'poyiadjis_N' | 'nemeth' "
                                      "(the score of pf = '{0}' as the drift is not built)".format(pf))
        if kind == "pf" and int(N) > 16384:
            raise NotImplementedError("sampler='{0}' is built for N <= 16384 (no whole-GPU windows), got N = {1}".format(
                sampler, int(N)))
        if pmmh_stat not in (None, "none", "score"):
            raise ValueError("pmmh_stat must be None, 'none' or 'score'")
    M, K, W = window_counts(observations, minibatch_size, num_sequences)
    if W > 1 and sampler == "gibbs":
        raise NotImplementedError("sampler='gibbs' draws one FFBS path per chain and step: W = 1 window "
                                  "(minibatch_size = num_sequences = 1), got W = {0}".format(W))
    if W > 1 and kind != "pf":
        raise NotImplementedError("kind='{0}' with W = {1} windows per chain and step is not built: "
                                  "the multi-window path is kind='pf' only".format(kind, W))
    explicit = minibatch_size is not None or num_sequences is not None
    multi = W > 1 or (explicit and kind == "pf" and sampler not in ("gibbs", "pgibbs"))
    if sampler == "sgrld" and model != "lgssm":           # sgmcmc_sampler.py:643-646: LGSSM alone has one
        raise NotImplementedError("No Default Preconditioner for {0}: sampler='sgrld' is built for model 'lgssm'".format(
            dict(svm="SVMSampler", garch="GARCHSampler").get(model, model)))
    stat = "score"
    if sampler == "pmmh" and kind == "pf":
        stat = pmmh_stat or "none"      # the launch computes no statistic: PMMH reads out[4] alone
    if sampler == "gibbs":
        if model != "lgssm" or dtype != "f64":
            raise NotImplementedError("sampler='gibbs' (FFBS paths, conjugate draws) is built for model 'lgssm', dtype 'f64'")
        if isinstance(observations, (list, tuple)):
            raise NotImplementedError("Gibbs over lists of sequences is not built")
        if int(subsequence_length) != -1 or int(buffer_length) != -1:
            raise NotImplementedError("sampler='gibbs' samples the path of the whole series: "
                                      "subsequence_length = buffer_length = -1")
        kind, num_samples, pf, stat = "complete", 1, "poyiadjis_N", "gibbs"      # one FFBS path per chain and step
    if kind not in ("pf", "marginal", "complete"):
        raise ValueError("kind must be 'pf', 'marginal' or 'complete'")
    if kind == "marginal" and (model != "lgssm" or dtype != "f64"):
        raise NotImplementedError("kind='marginal' (the exact Kalman score) is built for model 'lgssm', dtype 'f64'")
    if kind == "complete":
        if model != "lgssm" or dtype != "f64":
            raise NotImplementedError("kind='complete' (FFBS paths) is built for model 'lgssm', dtype 'f64'")
        if num_samples is None or int(num_samples) < 1:
            raise ValueError("kind='complete' needs num_samples >= 1 paths per window")
        N = int(num_samples)        # the paths of a window take the particles' place in the descriptors
    N, Ntilde = int(N), int(Ntilde)
    max_accept_reject = 0 if not accept_reject else (64 if max_accept_reject is None else max(0, int(max_accept_reject)))
    # which smoother runs: the one decision the descriptors, the launch and the scratch sizing follow
    lam, paris = 1.0, {}
    if kind == "pf":
        # the resampling scheme of a NEMETH window (particle_filters.SCHEMES); the other smoothers say below what they
        # make of `resampling`, and only the threshold is judged for them
        own = pf in ("poyiadjis_N", "nemeth")
        nemeth, _, tau = resolve_resampling("nemeth" if own else pf, pf, resampling if own else "multinomial",
                                            ess_threshold, N)
    if kind != "pf":
        if pf == "paris":
            raise ValueError("pf='paris' needs kind='pf'")
        if pf == "poyiadjis_N2":
            raise ValueError("pf='poyiadjis_N2' needs kind='pf'")
        if resampling == "stratified":
            raise ValueError("resampling='stratified' needs kind='pf', got kind = '{0}'".format(kind))
        smoother = {"marginal": "kalman", "complete": "kalman_ffbs"}[kind]
    elif pf == "paris":
        # PaRIS on the LDS-resident kernels (paris64x2 / paris256x1 / paris256x4): no per-chain scratch; the
        # multi-window path also runs paris_mem1024 (1024 < N <= 16384, its state in the descriptors' scratch)
        if N > 1024 and not multi:
            raise NotImplementedError("ChainEnsemble(pf='paris') is built for N <= 1024 on the single-window path, "
                                      "got N = {0}: pass minibatch_size / num_sequences for the multi-window path "
                                      "(paris_mem1024, N <= 16384)".format(N))
        if resampling != "multinomial":
            raise ValueError("pf='paris' resamples multinomially, got resampling = {0}".format(resampling))
        if Ntilde < 1:
            raise ValueError("pf='paris' needs Ntilde >= 1")
        smoother, paris = "paris", dict(Ntilde=Ntilde, max_accept_reject=max_accept_reject)
    elif pf == "poyiadjis_N2":
        # the Poyiadjis O(N^2) smoother on the LDS-resident kernels (n2_64x2 / n2_256x1 / n2_256x4): no per-chain
        # scratch; the multi-window path also runs n2_mem1024 (1024 < N <= 16384, its state in the descriptors' scratch)
        if N > 1024 and not multi:
            raise NotImplementedError("ChainEnsemble(pf='poyiadjis_N2') is built for N <= 1024 on the single-window path, "
                                      "got N = {0}: pass minibatch_size / num_sequences for the multi-window path "
                                      "(n2_mem1024, N <= 16384)".format(N))
        if resampling != "multinomial":
            raise ValueError("pf='poyiadjis_N2' resamples multinomially, got resampling = {0}".format(resampling))
        smoother = "poyiadjis_n2"
    elif pf in ("poyiadjis_N", "nemeth"):
        if pf == "nemeth":
            lam = 0.95 if lambduh is None else float(lambduh)
        smoother = nemeth           # 'nemeth', or what its resampling scheme makes of it
    else:
        raise ValueError("ChainEnsemble supports pf = 'poyiadjis_N' | 'nemeth' | 'paris' | 'poyiadjis_N2', got {0}".format(pf))
    # every chain the Poyiadjis O(N) score (NEMETH, lambduh = 1, score): units with a twin specialised to it run that
    # (their kernels answer NaN to a window that asks for another statistic: stat 'none' launches the general unit)
    launch_smoother = "poyiadjis_n" if smoother == "nemeth" and lam == 1.0 and stat == "score" else smoother
    if window_sampling not in ("host", "device"):
        raise ValueError("window_sampling must be 'host' or 'device'")

    segments = None
    if isinstance(observations, (list, tuple)):
        segs = [np.ascontiguousarray(o, dtype=np.float64).reshape(-1) for o in observations]
        if len(segs) == 0 or min(len(o) for o in segs) == 0:
            raise ValueError("every sequence needs at least one observation")
        segments = np.concatenate([[0], np.cumsum([len(o) for o in segs])]).astype(np.int64)
        y = np.concatenate(segs)
    else:
        y = np.ascontiguousarray(observations, dtype=np.float64).reshape(-1)
    T = y.shape[0]
    bounds = segments if segments is not None else np.array([0, T], dtype=np.int64)
    proto = None
    if isinstance(parameters, np.ndarray):
        theta0 = np.ascontiguousarray(parameters, dtype=np.float64).reshape(-1, _capi.THETA_DIM[model])
    else:
        if num_chains is None:
            raise ValueError("num_chains is required when `parameters` is a Parameters object")
        theta0, proto = np.tile(parameters.theta(), (int(num_chains), 1)), parameters

    S, B = int(subsequence_length), int(buffer_length)
    if segments is not None and not multi:
        if window_sampling != "host":
            raise NotImplementedError("sequence lists use host-side window sampling (device-side: pass num_sequences, "
                                      "the multi-window path)")
        if S == -1:
            S = int(np.max(np.diff(segments)))      # whole sequences
    elif S == -1 or T - S <= 0:
        S = -1
    B = T if B == -1 else B
    Tk = np.diff(bounds)
    longer = (Tk > S) if S > 0 else np.zeros(len(Tk), dtype=bool)
    strict = (partition_style or 'uniform') == 'strict'
    # (single-window lists draw their strict starts from Tk // S blocks without asking for divisibility)
    if strict and (multi or segments is None) and np.any(Tk[longer] % S != 0):
        k = int(np.flatnonzero(longer & (Tk % max(S, 1) != 0))[0])
        raise ValueError("S {0} does not evenly divide T {1}".format(S, int(Tk[k])))   # sgmcmc_sampler.py:1991-1993
    draws = rescale = None
    if multi:
        rescale = segments is not None and K != -1
        draws = rescale or bool(np.any(longer))
        if draws and window_sampling != "device":
            raise NotImplementedError("the W = {0} windows per chain and step are drawn on the device: "
                                      "window_sampling='device'".format(W))
        if N > 16384:
            raise NotImplementedError("the multi-window path is built for N <= 16384 (one workgroup per window), "
                                      "got N = {0}".format(N))
    if mh:
        # every step needs the likelihood of the whole data set: no window is drawn, nothing is rescaled
        whole = sampler + " needs the whole series in every step: "
        if segments is None and (S != -1 or int(buffer_length) != -1):
            raise NotImplementedError(whole + "subsequence_length = buffer_length = -1, got {0} / {1}".format(
                int(subsequence_length), int(buffer_length)))
        if segments is not None and (not multi or K != -1 or int(subsequence_length) != -1 or M != 1 or draws or rescale):
            raise NotImplementedError(whole + "a list of sequences takes num_sequences = -1, subsequence_length = -1, "
                                      "buffer_length = 0 and minibatch_size 1 (every sequence whole, out[4] summed{0})".format(
                                          ", the score columns too" if sampler == "pmala" else ""))
        if multi and (M != 1 or draws or rescale):
            raise NotImplementedError(whole + "minibatch_size = 1 (an average of log-likelihoods is no estimate of one)")
    s = types.SimpleNamespace(
        proposal_scale=scale, kind=kind, pf=pf, N=N, lambduh=lam, smoother=smoother, launch_smoother=launch_smoother, stat=stat,
        paris=paris, Ntilde=Ntilde, max_accept_reject=max_accept_reject, M=M, K=K, W=W, multi=multi, S=S, B=B, strict=strict,
        y=y, T=T, segments=segments, bounds=bounds, draws=draws, rescale=rescale, theta0=theta0, proto=proto, ess_threshold=tau,
        correlation=correlation)
    if sampler == "sgld_cv":        # (the other samplers' namespaces keep their fields)
        s.centre_repeats = 1 if kind == "marginal" else int(centre_repeats)
        s.centre_N = N if centre_N is None else int(centre_N)
    if sqmc:
        s.sqmc = True
    if sampler == "pmala_sorted":       # which sorted filter carries the score: 'cpm' (correlation) | 'sqmc'
        s.sorted_score = "sqmc" if sqmc else "cpm"
    return s


def _refuse_cv(a):
    """What sampler='sgld_cv' is not built for, each refusal naming its reason: the chain and its twin at the centre filter
    one window of one series on the same draws, in one launch of one-workgroup kernels."""
    what = "sampler='sgld_cv' (SGLD with control variates: every window is filtered at theta and at the centre) "
    if isinstance(a.observations, (list, tuple)):
        raise NotImplementedError(what + "centres on the whole-data gradient of one series: lists of sequences are not built")
    if a.kind == "complete":
        raise NotImplementedError(what + "needs a score that is a function of (theta, draws): kind='pf' or kind='marginal', "
                                  "got kind = 'complete' (sampled FFBS paths as a control variate are not built)")
    if a.kind == "pf" and a.pf in ("paris", "poyiadjis_N2"):
        raise NotImplementedError(what + "runs the O(N) filters: pf = 'poyiadjis_N' | 'nemeth', got pf = '{0}' (a paired "
                                  "PaRIS / O(N^2) launch is not built)".format(a.pf))
    if a.kind == "pf" and int(a.N) > 16384:
        raise NotImplementedError(what + "is built for N <= 16384 (no whole-GPU windows), got N = {0}".format(int(a.N)))
    if a.kind == "marginal" and a.centre_N is not None:
        raise ValueError(what + "with kind='marginal' centres on the exact Kalman gradient: centre_N has no particles to "
                         "count, got centre_N = {0}".format(a.centre_N))
    if a.centre_N is not None and not 1 <= int(a.centre_N) <= 16384:
        raise NotImplementedError(what + "centres with one-workgroup launches: 1 <= centre_N <= 16384, got centre_N = {0}".format(
            int(a.centre_N)))
    try:
        ok = int(a.centre_repeats) == a.centre_repeats and int(a.centre_repeats) >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(what + "needs centre_repeats >= 1 whole-series launches at the centre, got {0}".format(a.centre_repeats))


def refuse_chain_filter(family, a, also=(), score=False):
    """What the kernel families with one workgroup per chain are not built for, each refusal naming its reason: SVM and
    LGSSM, f64, the prior proposal, its own resampling at every step, the whole series, N <= 1024.  family: 'csmc' | 'cpm' |
    'sqmc', whose FILTERS record has the wording; a: the constructor's arguments by name.  also: (refused, reason) pairs of
    the caller's own, checked ahead of N.  score: the family's kernel carries the O(N) score (sampler='pmala_sorted'), so pf
    may be 'nemeth' as well."""
    f = FILTERS[family].refusal
    what = f["what"]
    if a.model == "garch":
        raise NotImplementedError(what + "is built for model 'svm' | 'lgssm': " + f["garch"])
    if a.dtype != "f64":
        raise NotImplementedError(what + "is built for dtype 'f64', got '{0}'".format(a.dtype))
    if isinstance(a.observations, (list, tuple)):
        raise NotImplementedError(what + f["lists"] + ": lists of sequences are not built")
    if int(a.subsequence_length) != -1 or int(a.buffer_length) != -1:
        raise NotImplementedError(what + f["whole"] + ": subsequence_length = buffer_length = -1, got {0} / {1}".format(
            int(a.subsequence_length), int(a.buffer_length)))
    M = 1 if a.minibatch_size is None else int(a.minibatch_size)
    K = 1 if a.num_sequences is None else int(a.num_sequences)
    if M != 1 or K != 1:
        raise NotImplementedError(what + f["window"] + ": W = 1 window (minibatch_size = num_sequences = 1), got "
                                  "minibatch_size = {0}, num_sequences = {1}".format(M, K))
    if a.kind != "pf":
        raise NotImplementedError(what + "is a particle method: kind='pf', got kind = '{0}'".format(a.kind))
    if score and a.pf not in ("poyiadjis_N", "nemeth"):
        raise NotImplementedError(what + "carries the O(N) score through its own {0}: pf = 'poyiadjis_N' | 'nemeth', got pf = "
                                  "'{1}' (a PaRIS / O(N^2) score on the sorted filters is not built)".format(f["own"], a.pf))
    if not score and a.pf != "poyiadjis_N":
        raise NotImplementedError(what + "runs its own {0}, no smoother: pf stays at its default, got pf = '{1}'".format(
            f["own"], a.pf))
    if a.resampling != "multinomial":
        raise NotImplementedError(what + f["resampling"] + ", got resampling = '{0}'".format(a.resampling))
    if a.ess_threshold is not None and a.ess_threshold != 0:
        raise NotImplementedError(what + "resamples at every step: adaptive resampling (ess_threshold) is not built inside " +
                                  f["inside"])
    if a.kernel not in (None, "prior"):
        raise NotImplementedError(what + "proposes from the prior kernel, got kernel = '{0}'".format(a.kernel))
    for refused, reason in also:
        if refused:
            raise NotImplementedError(what + reason)
    if not 2 <= int(a.N) <= f["max_n"]:
        raise NotImplementedError(what + "keeps one chain's particles in one workgroup{0}: 2 <= N <= {1}, got N = {2}".format(
            f["particles"], f["max_n"], int(a.N)))


def _refuse_pmmh_stat(a):
    if a.pmmh_stat is not None:
        raise ValueError("pmmh_stat belongs to sampler='pmmh' (sampler='{0}' needs the score launch), got sampler = "
                         "'{0}'".format(a.sampler))


def _refuse_pmmh_filter(family, a):
    """`correlation` ('cpm') and `sqmc` beside sampler='pmmh': sqmc not beside correlation, the sampler the option belongs to,
    then the shared refusals (with pmmh_stat's ahead of N), then the family's own last check (rho's range, the power of two)."""
    f = FILTERS[family]
    what = f.refusal["what"]
    if family == "sqmc" and a.correlation is not None:
        raise NotImplementedError(what + "draws a fresh point set at every step and carries no normals: correlation stays "
                                  "None, got correlation = {0}".format(a.correlation))
    if a.sampler != "pmmh":
        raise NotImplementedError(what + "belongs to sampler='pmmh', got sampler = '{0}'{1}".format(
            a.sampler, f.refusal["pmala"] if a.sampler == "pmala" else ""))
    refuse_chain_filter(family, a, also=[(
        a.pmmh_stat not in (None, "none"), "computes the log-likelihood estimate alone: pmmh_stat stays at its default, got "
                                           "pmmh_stat = '{0}'".format(a.pmmh_stat))])
    f.last(a)


def _refuse_pmala_sorted(a):
    """sampler='pmala_sorted': exactly one of `correlation` and `sqmc`, then the refusals of that filter's family
    (refuse_chain_filter, with pf = 'nemeth' admitted: the kernel carries the score), then the family's own last check,
    then lambduh's range."""
    what = "sampler='pmala_sorted' (particle MALA along the score of a sorted filter) "
    if (a.correlation is not None) == bool(a.sqmc):
        raise ValueError(what + "takes exactly one of correlation=rho (the correlated filter) and sqmc=True (the sequential "
                         "quasi-Monte Carlo filter), got {0}".format("both" if a.sqmc else "neither"))
    _refuse_pmmh_stat(a)
    if a.kind in ("marginal", "complete"):
        raise NotImplementedError(what + "drifts along a particle filter's score: kind='pf', got kind = '{0}' (sampler='pmala' "
                                  "serves the exact Kalman score)".format(a.kind))
    family = "sqmc" if a.sqmc else "cpm"
    refuse_chain_filter(family, a, score=True)
    FILTERS[family].last(a)
    if a.pf == "nemeth" and a.lambduh is not None:
        try:
            lam = float(a.lambduh)
        except (TypeError, ValueError):
            lam = float("nan")
        if not 0.0 < lam <= 1.0:
            raise ValueError(what + "shrinks the score with lambduh in (0, 1] (1: the plain O(N) recursion), got {0}".format(
                a.lambduh))


def window_counts(observations, minibatch_size, num_sequences):
    """(M, K, W): windows per sequence, sequences per step (-1 = all), windows per chain and step."""
    M = 1 if minibatch_size is None else int(minibatch_size)
    K = 1 if num_sequences is None else int(num_sequences)
    if M < 1:
        raise ValueError("minibatch_size must be >= 1, got {0}".format(M))
    if not isinstance(observations, (list, tuple)):
        if K != 1:
            raise ValueError("a single series takes num_sequences = 1, got {0}".format(K))
        return M, K, M
    n_seq = len(observations)
    if K != -1 and not 1 <= K <= n_seq:
        raise ValueError("num_sequences must be -1 or in 1..{0} (the number of sequences), got {1}".format(n_seq, K))
    if K > _capi.MAX_DRAWN_SEQUENCES:
        raise NotImplementedError("num_sequences = {0}: at most {1} sequences are drawn per chain and step "
                                  "(num_sequences = -1 takes them all)".format(K, _capi.MAX_DRAWN_SEQUENCES))
    return M, K, M * (n_seq if K == -1 else K)
