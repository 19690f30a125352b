"""TemperedPopulation: density-tempered SMC over the resident PMMH chains of a ChainEnsemble, with a log-evidence estimate.

The exact samplers of ChainEnsemble run thousands of INDEPENDENT chains from one start.  Here the chains are one interacting
population (Del Moral, Doucet and Jasra 2006; Duan and Fulop 2015, pseudo-marginal moves): it starts from a Gaussian q0 and is
carried to the posterior through temperatures phi in [0, 1] chosen on the way.  The extended target at phi is

    pi_phi(theta, u)  ~  q0(theta)^(1 - phi)  (exp(logprior(theta)) p-hat(y | theta, u))^phi  psi(u)      on PMMH's support,

q0 the product over the slots a PMMH proposal moves of N(m_j, s_j^2) (raw coordinates; LGSSM's C stays 1, SVM has three slots).
With h_i = (ll_i + logprior(theta_i)) - log q0(theta_i), ll_i the estimate chain i's state was accepted with, a stage is

  1. temperature   delta = the largest value in (0, 1 - phi] with ESS(delta) >= tau C, ESS(d) = (sum_i e^(d (h_i - h_max)))^2 /
                   sum_i e^(2 d (h_i - h_max)): 1 - phi if that passes (the last stage), otherwise the lower end of 60 rounds of
                   bisection on [0, 1 - phi]; h_i = -inf is a zero weight
  2. evidence      log Z-hat += delta h_max + log((1 / C) sum_i e^(delta (h_i - h_max)))
  3. resample      the chains systematically on w_i = e^(delta (h_i - h_max)), every stage, one uniform per stage: child r takes
                   the smallest j with cdf[j] > ((r + u) / C) W; the weights are uniform afterwards
  4. gather        theta rows and estimates by parent
  5. scale         s_j = c sd_j of the resampled population per moving slot, c = 2.38 / sqrt(d) by default (d moving slots); a
                   slot whose sd is 0 or not finite keeps its scale
  6. move          `moves` PMMH steps at phi' = phi + delta: the ensemble's own propose and filter launches, then the tempered
                   accept  log alpha = phi' ((ll' + logprior(theta')) - (ll + logprior(theta))) + (1 - phi') (log q0(theta') -
                   log q0(theta)); a chain that rejects keeps theta AND ll, as in PMMH.

Steps 1-5 and the accept are HIP kernels (csrc/pfg_smc.hip, csrc/pfg_chains.hip); the expensive part, the filter or Kalman
launch, is the ensemble's, unchanged -- so every PMMH configuration the ensemble accepts runs here (GARCH, kind='marginal',
stratified / systematic / adaptive resampling, N up to 16384, sequence lists), except `correlation` and `sqmc`.  At phi = 1 the tempered
accept is PMMH's bit for bit and `ensemble` is a plain PMMH ChainEnsemble whose chains are posterior-distributed and whose
proposal scale is the population's.

log_evidence() estimates log of the integral over the support of exp(logprior(theta)) p(y | theta) d theta, logprior being the
UNNORMALISED density the PMMH chains target (Prior.logprior of the raw row, no Jacobian terms, less its terms in the
hyper-parameters alone).  A Bayes factor between two models needs, besides, the mass of each model's exp(logprior) -- that is
not computed here, so the difference of two log_evidence() values is NOT a ready Bayes factor.
"""
import math
import os
import types

import numpy as np

from . import _capi

_RNG_SALT = 0x534D43         # the initial population: np.random.default_rng([seed, _RNG_SALT])
_SEED_MASK = 0xFFFFFFFFFFFFFFFF
A_MAX = 0.9999


def moving_slots(model):
    """The theta slots a PMMH proposal moves (LGSSM: not C)."""
    mask = _capi.PMMH_MOVING_SLOTS[model]
    return [j for j in range(_capi.THETA_DIM[model]) if (mask >> j) & 1]


def in_support(model, theta):
    """[C] bool: the rows project_parameters leaves unchanged -- |A| <= 0.9999, every Cholesky factor > 0 (GARCH: LRinv)."""
    th = np.asarray(theta, dtype=np.float64)
    ok = np.all(np.isfinite(th), axis=1)
    if model == "garch":
        return ok & (th[:, 3] > 0.0)
    P = _capi.THETA_DIM[model]
    return ok & (np.abs(th[:, 0]) <= A_MAX) & (th[:, P - 2] > 0.0) & (th[:, P - 1] > 0.0)


def log_q0_mass(model, mean, sd):
    """log of the mass the untruncated normals of q0 put on the support, in closed form: A in [-0.9999, 0.9999], Cholesky
    factors > 0, GARCH's first three slots unrestricted."""
    Phi = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
    P = _capi.THETA_DIM[model]
    out = 0.0
    for j in ((3,) if model == "garch" else (P - 2, P - 1)):
        out += math.log(Phi(mean[j] / sd[j]))
    if model != "garch":
        out += math.log(Phi((A_MAX - mean[0]) / sd[0]) - Phi((-A_MAX - mean[0]) / sd[0]))
    return out


def _world_size():
    world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            world = max(world, dist.get_world_size())
    except ImportError:
        pass
    return world


class TemperedPopulation(object):
    """C resident PMMH chains as one tempered population.

        pop = TemperedPopulation("svm", y, params, num_chains=4096, N=256, seed=1)
        info = pop.temper()                     # to phi = 1
        pop.log_evidence(), pop.schedule()
        ens = pop.ensemble                      # a plain PMMH ChainEnsemble from here on
        ens.run(100, thin=10, graph_steps=10)

    Args:
      model, observations: as ChainEnsemble;  parameters: a Parameters object, the default centre of q0
      num_chains: C, 2 <= C <= 2^20 (one workgroup reweights and resamples the population)
      init_mean, init_sd: q0 in raw coordinates, length P (default: the row of `parameters`, 0.3 per slot); entries of slots that
               do not move are ignored
      ess_target: tau in (0, 1);  moves: PMMH steps per stage, >= 1
      scale_factor: c of s_j = c sd_j (default 2.38 / sqrt(d))
      **ensemble_kwargs: forwarded to ChainEnsemble(sampler='pmmh', ...) untouched -- every refusal of a PMMH configuration is
               the ensemble's own.  proposal_scale, if given, is the scale of a slot until the population gives it one.
    Refused here, by name: correlation (the normals would have to be gathered too: not built), sqmc (its move is not routed
    through the sequential quasi-Monte Carlo filter: not built), a sampler other than 'pmmh',
    C outside 2 .. 2^20, tau outside (0, 1), moves < 1, an init_sd <= 0, and a process that is one rank of several (the
    population interacts; a rank partition of it is not built).

    The initial population is drawn on the host from q0 by rejection to the support, a pure function of the seed; the
    ensemble's init pass then supplies every chain's estimate at counter 0 and refuses a non-finite one, as for any PMMH
    ensemble.  A degenerate estimate later is a zero weight.  The stage loop is eager with one host read per stage (phi and the
    status flag, right after the temperature kernel).  The ensemble's accept counts and steps_done stay 0 through tempering --
    the wrapper counts its own -- so ensemble.acceptance_rate() afterwards counts the steps run afterwards; step_ctr advances
    once per move, so no key repeats.
    """

    def __init__(self, model, observations, parameters, num_chains=None, seed=0, init_mean=None, init_sd=None, ess_target=0.5,
                 moves=2, scale_factor=None, **ensemble_kwargs):
        s = self.resolve_settings(model, parameters, num_chains=num_chains, seed=seed, init_mean=init_mean, init_sd=init_sd,
                                  ess_target=ess_target, moves=moves, scale_factor=scale_factor, **ensemble_kwargs)
        import torch
        from .ensemble import ChainEnsemble
        kw = dict(ensemble_kwargs)
        kw.pop("sampler", None)
        kw.setdefault("proposal_scale", s.scale0[:_capi.THETA_DIM[model]])
        self.ensemble = ens = ChainEnsemble(model, observations, s.theta0, sampler="pmmh", seed=seed, **kw)
        self.model, self.C, self.seed = model, ens.C, int(seed)
        self.ess_target, self.moves, self.scale_factor = s.ess_target, s.moves, s.scale_factor
        self.q0_mean, self.q0_sd = s.q0_mean, s.q0_sd
        self._slots = _capi.PMMH_MOVING_SLOTS[model]
        dev, C = ens.device, ens.C
        self._torch = torch
        self.q0_mean_dev = torch.from_numpy(s.q0_mean).to(dev)
        self.q0_sd_dev = torch.from_numpy(s.q0_sd).to(dev)
        self.phi_dev = torch.zeros(1, dtype=torch.float64, device=dev)
        self.h_dev = torch.zeros(C, dtype=torch.float64, device=dev)
        self.parent_dev = torch.zeros(C, dtype=torch.int32, device=dev)
        # the stage's record and its status flag in one buffer: one host read per stage
        self._record_dev = torch.zeros(_capi.SMC_RESULT_DOUBLES + 1, dtype=torch.float64, device=dev)
        self.cdf_dev = torch.empty(_capi.smc_scratch_bytes(C), dtype=torch.uint8, device=dev)
        self.ll_tmp_dev = torch.zeros(C, dtype=torch.float64, device=dev)
        self.accept_dev = torch.zeros(C, dtype=torch.int64, device=dev)      # the wrapper's own counts (the library's uint64)
        self.phi, self.stage_index, self._log_z = 0.0, 0, 0.0
        self._stages = dict(phi=[], delta=[], ess=[], increment=[], u=[])
        self._accepted, self._scales = [], []           # per stage, on the device until somebody asks

    # -- what needs no device ------------------------------------------------------------------------------------------------
    @staticmethod
    def resolve_settings(model, parameters, num_chains=None, seed=0, init_mean=None, init_sd=None, ess_target=0.5, moves=2,
                         scale_factor=None, **ensemble_kwargs):
        """The wrapper's own arguments -> a namespace (q0_mean, q0_sd [MAX_THETA], theta0 [C, P] the initial population,
        scale0 [MAX_THETA], ess_target, moves, scale_factor), or the refusal.  Needs no device."""
        what = "TemperedPopulation (density-tempered SMC over resident PMMH chains) "
        if ensemble_kwargs.get("sampler", "pmmh") == "pmala_sorted":
            raise NotImplementedError(what + "moves the population by PMMH steps; tempering the Langevin proposal of "
                                      "sampler='pmala_sorted' (its score, and under correlation its normals, would have to be "
                                      "gathered and tempered too) is not built: sampler stays 'pmmh'")
        if ensemble_kwargs.get("correlation", None) is not None:
            raise NotImplementedError(what + "resamples theta and the estimate across chains; with correlation the chains' "
                                      "normals would have to be gathered too, and that is not built: correlation stays None")
        if ensemble_kwargs.get("sqmc", False):
            raise NotImplementedError(what + "moves the population through its own accept step (pfg_smc_accept_device around the "
                                      "ensemble's launch); routing that move through the sequential quasi-Monte Carlo filter is "
                                      "not built: sqmc stays False")
        if ensemble_kwargs.get("sampler", "pmmh") != "pmmh":
            raise NotImplementedError(what + "moves the population by PMMH steps: sampler stays 'pmmh', got sampler = '{0}'".format(
                ensemble_kwargs["sampler"]))
        if model not in _capi.THETA_DIM:
            raise ValueError("model must be 'svm', 'garch' or 'lgssm'")
        if num_chains is None:
            raise ValueError("num_chains is required")
        C = int(num_chains)
        if not _capi.SMC_MIN_CHAINS <= C <= _capi.SMC_MAX_CHAINS:
            raise NotImplementedError(what + "reweights and resamples the population in one workgroup: 2 <= num_chains <= 2^20, "
                                      "got {0}".format(C))
        tau = float(ess_target)
        if not 0.0 < tau < 1.0:         # (false for a NaN as well)
            raise ValueError("ess_target must lie in (0, 1) (the next temperature keeps ESS >= ess_target * C), got {0}".format(
                ess_target))
        if int(moves) < 1:
            raise ValueError("moves must be >= 1 PMMH steps per stage, got {0}".format(moves))
        if _world_size() > 1 or int(ensemble_kwargs.get("chain_offset", 0) or 0) != 0:
            raise NotImplementedError(what + "is one interacting population: a process that is one rank of several (WORLD_SIZE > 1 "
                                      "or a chain_offset) would hold a part of it, and a rank partition is not built")
        P = _capi.THETA_DIM[model]
        slots = moving_slots(model)
        mean = np.zeros(_capi.MAX_THETA)
        if init_mean is None:
            if not hasattr(parameters, "theta"):
                raise ValueError("parameters must be a Parameters object (the default centre of q0; the population's rows are "
                                 "drawn from q0)")
            init_mean = parameters.theta()
        given = np.asarray(init_mean, dtype=np.float64).reshape(-1)
        if given.size != P:
            raise ValueError("init_mean must have length {0}".format(P))
        mean[:P] = given
        sd = np.ones(_capi.MAX_THETA)
        given = np.full(P, 0.3) if init_sd is None else np.asarray(init_sd, dtype=np.float64).reshape(-1)
        if given.size not in (1, P):
            raise ValueError("init_sd must be a scalar or a vector of length {0}".format(P))
        sd[:P] = given
        if not np.all(np.isfinite(sd[slots])) or not np.all(sd[slots] > 0.0):
            raise ValueError("init_sd must be > 0 for every slot that moves, got {0}".format(init_sd))
        if not np.all(np.isfinite(mean[slots])):
            raise ValueError("init_mean must be finite, got {0}".format(init_mean))
        d = len(slots)
        c = 2.38 / math.sqrt(d) if scale_factor is None else float(scale_factor)
        if not 0.0 < c < np.inf:
            raise ValueError("scale_factor must be > 0, got {0}".format(scale_factor))
        # the initial population: q0 by rejection to the support, a pure function of the seed
        rng = np.random.default_rng([int(seed) & _SEED_MASK, _RNG_SALT])
        theta0 = np.zeros((C, P))
        if model == "lgssm":
            theta0[:, 1] = 1.0
        todo = np.arange(C)
        for _ in range(10000):
            draw = mean[slots] + sd[slots] * rng.standard_normal((todo.size, d))
            theta0[np.ix_(todo, slots)] = draw
            todo = todo[~in_support(model, theta0[todo])]
            if todo.size == 0:
                break
        else:
            raise ValueError("q0 puts (almost) no mass on the support: init_mean = {0}, init_sd = {1}".format(init_mean, init_sd))
        scale0 = np.ones(_capi.MAX_THETA)
        scale0[slots] = c * sd[slots]
        return types.SimpleNamespace(q0_mean=mean, q0_sd=sd, theta0=theta0, scale0=scale0, ess_target=tau, moves=int(moves),
                                     scale_factor=c)

    # -- the launches of a stage ---------------------------------------------------------------------------------------------
    def _record_ptrs(self):
        base = self._record_dev.data_ptr()
        return base, base + 8 * _capi.SMC_RESULT_DOUBLES         # the record, the status word behind it

    def launch_logtarget(self, stream=None):
        e = self.ensemble
        e.ctx.smc_logtarget_device(e.model, e.C, e.theta_dev.data_ptr(), e.ll_dev.data_ptr(), e.hyper, self.q0_mean_dev.data_ptr(),
                                   self.q0_sd_dev.data_ptr(), self.h_dev.data_ptr(), e._stream(stream))

    def launch_temper(self, stream=None):
        e = self.ensemble
        record, status = self._record_ptrs()
        e.ctx.smc_temper_device(e.C, self.h_dev.data_ptr(), self.phi_dev.data_ptr(), self.ess_target, self.seed, self.stage_index,
                                record, status, self.parent_dev.data_ptr(), self.cdf_dev.data_ptr(), e._stream(stream))

    def launch_gather(self, stream=None):
        """theta and ll by parent, through theta_prop_dev (free between steps) and ll_tmp_dev."""
        e = self.ensemble
        e.ctx.smc_gather_device(e.C, self.parent_dev.data_ptr(), e.theta_dev.data_ptr(), e.ll_dev.data_ptr(),
                                e.theta_prop_dev.data_ptr(), self.ll_tmp_dev.data_ptr(), e._stream(stream))

    def launch_scale(self, stream=None):
        e = self.ensemble
        e.ctx.smc_scale_device(e.C, e.theta_dev.data_ptr(), self._slots, self.scale_factor, e.scale_dev.data_ptr(),
                               e._stream(stream))

    def launch_accept(self, stream=None, log_alpha_ptr=0):
        e = self.ensemble
        e.ctx.smc_accept_device(e.model, e.C, e.theta_dev.data_ptr(), e.theta_prop_dev.data_ptr(), e.valid_dev.data_ptr(),
                                e.out_dev.data_ptr(), e.ll_dev.data_ptr(), self.accept_dev.data_ptr(), e.hyper,
                                self.q0_mean_dev.data_ptr(), self.q0_sd_dev.data_ptr(), self.phi_dev.data_ptr(), log_alpha_ptr,
                                *e._update_key(stream))

    def launch_move(self, stream=None):
        """One PMMH step at the current temperature: the ensemble's proposal and filter launches, the tempered accept."""
        e = self.ensemble
        e.launch_propose(stream)
        e.launch_pf(stream)
        if e._multi:
            e.launch_reduce(stream)
        self.launch_accept(stream)

    _STATUS = {1: "no chain has a finite h = ll + logprior - log q0", 2: "a chain's h is NaN or +inf",
               4: "the temperature step ended at exactly 0 (ESS >= ess_target * C holds for no step)",
               8: "phi is not in [0, 1)"}

    def stage(self, n=1):
        """n stages (fewer if phi reaches 1).  Returns the number run."""
        done = 0
        while done < n and self.phi < 1.0:
            self.launch_logtarget()
            self.launch_temper()
            rec = self._record_dev.cpu().numpy()            # the stage's one host read (synchronises)
            status = int(rec[_capi.SMC_RESULT_DOUBLES:].view(np.int32)[0])
            if status:
                raise RuntimeError("tempering stage {0} at phi = {1}: {2} (the population is as it was)".format(
                    self.stage_index, self.phi, "; ".join(t for bit, t in self._STATUS.items() if status & bit)))
            self.launch_gather()
            self.launch_scale()
            for _ in range(self.moves):
                self.launch_move()
            self._accepted.append(self.accept_dev.sum())
            self._scales.append(self.ensemble.scale_dev.clone())
            self.phi = float(rec[0])
            for key, v in zip(("phi", "delta", "increment", "ess", "u"), rec[:5]):
                self._stages[key].append(float(v))
            self._log_z += float(rec[2])
            self.stage_index += 1
            done += 1
        if self.phi >= 1.0 and done:
            self.ensemble.synchronize()
            self.ensemble.proposal_scale = self.ensemble.scale_dev.cpu().numpy()        # the host's copy of the adapted scale
        return done

    def temper(self, max_stages=1000):
        """Run to phi = 1 (RuntimeError if max_stages do not get there).  Returns schedule()."""
        self.stage(int(max_stages))
        if self.phi < 1.0:
            raise RuntimeError("phi = {0} after {1} stages: max_stages is too small".format(self.phi, self.stage_index))
        return self.schedule()

    # -- results -------------------------------------------------------------------------------------------------------------
    def schedule(self):
        """Per stage: phi (after the stage), delta, ess (at delta, before resampling), increment (of the log-evidence), u (the
        resampling uniform), acceptance (accepted proposals / (C * moves)) and scale [stages, P] the moves ran with."""
        torch = self._torch
        out = {k: np.array(v, dtype=np.float64) for k, v in self._stages.items()}
        S = self.stage_index
        P = _capi.THETA_DIM[self.model]
        cum = torch.stack(self._accepted).cpu().numpy().astype(np.float64) if S else np.zeros(0)
        out["acceptance"] = np.diff(np.concatenate([[0.0], cum])) / (self.C * self.moves)
        out["scale"] = torch.stack(self._scales).cpu().numpy()[:, :P] if S else np.zeros((0, P))
        return out

    def log_evidence(self):
        """sum of the stages' increments + log m(q0), m(q0) the mass of the untruncated q0 on the support: an estimate of
        log of the integral over the support of exp(logprior(theta)) p(y | theta) d theta for the UNNORMALISED prior density
        the PMMH chains target (module docstring).  Not a ready Bayes factor between models: that needs the prior's mass too."""
        if self.phi < 1.0:
            raise ValueError("log_evidence() needs phi = 1, the population is at phi = {0}".format(self.phi))
        return self._log_z + log_q0_mass(self.model, self.q0_mean, self.q0_sd)

    # -- checkpoint ----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """The ensemble's dict plus, under 'tempering', phi, the sum of the increments, the stage, the schedule, q0, the scale,
        the wrapper's accept counts and what load_state_dict compares (tau, moves, C)."""
        state = self.ensemble.state_dict()
        sched = self.schedule()
        state["tempering"] = dict(
            phi=self.phi, log_evidence=self._log_z, stage=self.stage_index, schedule=sched, q0_mean=self.q0_mean.copy(),
            q0_sd=self.q0_sd.copy(), scale=self.ensemble.scale_dev.cpu().numpy(), n_accept=self.accept_dev.cpu().numpy(),
            ess_target=self.ess_target, moves=self.moves, C=self.C, scale_factor=self.scale_factor)
        return state

    def load_state_dict(self, state):
        torch = self._torch
        t = state["tempering"]
        for key, mine in (("C", self.C), ("ess_target", self.ess_target), ("moves", self.moves), ("scale_factor", self.scale_factor)):
            if t[key] != mine:
                raise ValueError("checkpoint {0} = {1} does not match the population ({2})".format(key, t[key], mine))
        for key, mine in (("q0_mean", self.q0_mean), ("q0_sd", self.q0_sd)):
            if not np.array_equal(np.asarray(t[key]), mine):
                raise ValueError("checkpoint {0} = {1} does not match the population ({2})".format(key, t[key], mine))
        self.ensemble.load_state_dict({k: v for k, v in state.items() if k != "tempering"})
        dev = self.ensemble.device
        self.phi, self._log_z, self.stage_index = float(t["phi"]), float(t["log_evidence"]), int(t["stage"])
        self.phi_dev.fill_(self.phi)
        self.ensemble.scale_dev.copy_(torch.from_numpy(np.ascontiguousarray(t["scale"], dtype=np.float64)))
        self.ensemble.proposal_scale = np.array(t["scale"], dtype=np.float64)
        self.accept_dev.copy_(torch.from_numpy(np.ascontiguousarray(t["n_accept"], dtype=np.int64)))
        sched = t["schedule"]
        self._stages = {k: [float(v) for v in sched[k]] for k in self._stages}
        cum = np.rint(np.cumsum(np.asarray(sched["acceptance"], dtype=np.float64) * (self.C * self.moves))).astype(np.int64)
        self._accepted = [torch.tensor(int(v), dtype=torch.int64, device=dev) for v in cum]
        full = np.ones((self.stage_index, _capi.MAX_THETA))
        full[:, :np.shape(sched["scale"])[1]] = sched["scale"]
        self._scales = [torch.from_numpy(row.copy()).to(dev) for row in full]
        self.ensemble.synchronize()
