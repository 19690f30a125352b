"""SequentialPopulation: SMC^2 over the resident PMMH chains of a ChainEnsemble (Chopin, Jacob and Papaspiliopoulos 2013; Fulop
and Li 2013) -- the sequential form of TemperedPopulation.

TemperedPopulation needs the whole series up front and refilters all of it at every temperature.  Here the chains take the
observations chunk by chunk: after every chunk the weighted population targets the posterior given the observations so far,
the stage's evidence increment is the prequential score of the chunk, and extend() appends observations without starting over.

Every chain keeps, beside theta, the particle system of its own filter -- one row x [N][NS], logw [N] of a state buffer in HBM
--, the sum ll of its chunks' log-likelihood estimates and a running log-weight.  With q0 as in TemperedPopulation:

  stage 0          logw = 0; h0_i = logprior(theta_i) - log q0(theta_i) (pfg_smc_logtarget_device at ll = 0) is the first
                   increment: log((1 / C) sum_i e^(h0_i)).  It never resamples: there is nothing to move on yet
  stage on y[t : t + k)
  1. extend        ONE launch of the ensemble's filter kernel on y[t : t + k), warm-started from every chain's row
                   (pfg_dev_problem.init_x / init_logw) and leaving the new particle system in the other buffer (final_x /
                   final_logw); the buffers then swap roles.  incr_i = out[4], the chunk's estimate of p(y[t : t + k) | y[0 : t),
                   theta_i), and ll_i += incr_i: the sum over the chunks is the estimate of one filter over the series
  2. account       v_i = logw_i + incr_i; the evidence increment log(sum_i e^(v_i) / sum_i e^(logw_i)) and ESS =
                   (sum e^v)^2 / sum e^(2 v) (pfg_seq_reweight_device).  ESS >= tau C: logw = v, the stage ends
  3. resample      otherwise: the chains systematically on e^v, one uniform per stage, logw = 0; rows, theta and ll by parent
                   (pfg_seq_gather_device); the scale as TemperedPopulation's (pfg_smc_scale_device); then `moves` PMMH steps
                   on the PREFIX y[0 : t + k): the ensemble's proposal, a filter launch from scratch at the proposal that leaves
                   its particle system in the other buffer, PMMH's accept step, and pfg_seq_adopt_device, which hands a chain
                   that accepted its new row.

A chain's ll is always the estimate its particle system was built with -- the sum of its chunks, or the move's one launch --
so the move is exact PMMH on the prefix, the extension is the next steps of that very filter, and the weighted population is
exact for every N (the argument of Chopin et al., section 3: the extended target carries the filter's particle system).

The filter launches draw under (seed ^ a salt of their own, the global chain id, a counter of their own that advances once per
launch): no draw repeats between extensions and moves, nor with the ensemble's.  The stage loop is eager, one host read per
stage.  The cost: a move refilters the prefix, so a run costs about T^2 / chunk filter steps times the share of stages that
resample -- dearer than tempering when the whole series is there from the start; its case is the evidence per chunk and
extend().

log_evidence() has TemperedPopulation.log_evidence's meaning and caveats, word for word (tempering.py).
"""
import numpy as np

from . import _capi
from .tempering import TemperedPopulation, _world_size, log_q0_mass

_FILTER_SALT = 0x534551324649          # the filter launches draw under seed ^ this ("SEQ2FI")
_SEED_MASK = 0xFFFFFFFFFFFFFFFF
_MAX_N = 16384
_NEVER = 2.0 ** -1000                  # an ESS target no population falls below (ESS >= 1): stage 0 carries its weights


class SequentialPopulation(object):
    """C resident PMMH chains as one population that takes the observations chunk by chunk.

        pop = SequentialPopulation("svm", y[:500], params, num_chains=4096, N=256, chunk=50, seed=1)
        pop.run()                               # to the end of y[:500]
        pop.evidence_increments(), pop.posterior_mean(), pop.log_evidence()
        pop.extend(y[500:]); pop.run()
        ens = pop.finish()                      # a plain PMMH ChainEnsemble on the whole series from here on

    Args:
      model, observations: as ChainEnsemble, a single series;  parameters: a Parameters object, the default centre of q0
      num_chains: C, 2 <= C <= 2^20;  N: particles per chain, N <= 16384;  chunk: k >= 1 observations per stage
      init_mean, init_sd, ess_target, moves, scale_factor: as TemperedPopulation (q0, tau, PMMH steps per resampling stage, c)
      **ensemble_kwargs: forwarded to ChainEnsemble(sampler='pmmh', ...): prior, kernel ('optimal' included), forward_message,
               device, proposal_scale
    Refused here, by name and before anything is allocated: correlation, sqmc, a sampler other than 'pmmh', kind != 'pf', lists
    of sequences, windows (subsequence_length, buffer_length other than -1), minibatch_size / num_sequences other than 1, pf
    other than 'poyiadjis_N', resampling other than 'multinomial', ess_threshold, pmmh_stat, dtype other than 'f64', N > 16384,
    chunk < 1, C outside 2 .. 2^20, tau outside (0, 1), moves < 1, and a process that is one rank of several.

    The ensemble's accept counts and steps_done stay 0 until finish() -- the wrapper counts its own; the ensemble's counter
    advances once per move, the wrapper's once per filter launch.  Before finish(), `ensemble` is NOT a ready posterior ensemble:
    its chains carry weights, and its descriptors still name the series it was constructed on.
    """

    def __init__(self, model, observations, parameters, num_chains=None, N=1000, chunk=1, seed=0, init_mean=None, init_sd=None,
                 ess_target=0.5, moves=2, scale_factor=None, **ensemble_kwargs):
        s = self.resolve_settings(model, parameters, observations=observations, num_chains=num_chains, N=N, chunk=chunk, seed=seed,
                                  init_mean=init_mean, init_sd=init_sd, ess_target=ess_target, moves=moves,
                                  scale_factor=scale_factor, **ensemble_kwargs)
        import torch
        from .ensemble import ChainEnsemble
        kw = {k: v for k, v in ensemble_kwargs.items() if k not in ("sampler", "minibatch_size", "num_sequences")}
        kw.setdefault("proposal_scale", s.scale0[:_capi.THETA_DIM[model]])
        self.ensemble = ens = ChainEnsemble(model, s.y, s.theta0, sampler="pmmh", seed=seed, N=s.N, **kw)
        self.model, self.C, self.N, self.seed, self.chunk = model, ens.C, s.N, int(seed), s.chunk
        self.ess_target, self.moves, self.scale_factor = s.ess_target, s.moves, s.scale_factor
        self.q0_mean, self.q0_sd = s.q0_mean, s.q0_sd
        self._slots = _capi.PMMH_MOVING_SLOTS[model]
        self._torch = torch
        dev, C = ens.device, ens.C
        self.row_doubles = s.N * (_capi.STATE_DIM[model] + 1)
        self.y_dev = ens.y_dev                   # every observation so far; extend() replaces it
        self.T, self.t = int(s.y.shape[0]), 0
        self.q0_mean_dev = torch.from_numpy(s.q0_mean).to(dev)
        self.q0_sd_dev = torch.from_numpy(s.q0_sd).to(dev)
        self.logw_dev = torch.zeros(C, dtype=torch.float64, device=dev)
        self.h_dev = torch.zeros(C, dtype=torch.float64, device=dev)
        self.parent_dev = torch.zeros(C, dtype=torch.int32, device=dev)
        # the stage's record and its status flag in one buffer: one host read per stage
        self._record_dev = torch.zeros(_capi.SEQ_RECORD_DOUBLES + 1, dtype=torch.float64, device=dev)
        self.cdf_dev = torch.empty(_capi.smc_scratch_bytes(C), dtype=torch.uint8, device=dev)
        self.ll_tmp_dev = torch.zeros(C, dtype=torch.float64, device=dev)
        self.accept_dev = torch.zeros(C, dtype=torch.int64, device=dev)       # the wrapper's own counts (the library's uint64)
        self.seen_dev = torch.zeros(C, dtype=torch.int64, device=dev)         # ... as of the latest adopt
        # the chains' particle systems: two buffers [C, N (NS + 1)], `_cur` names the one every chain's row is in
        self.state_dev = ens._alloc_per_chain(torch.zeros, "SMC^2 keeps two particle systems per chain in HBM", "8 N (NS + 1)",
                                              8 * self.row_doubles, 2).view(torch.float64).view(2, C, self.row_doubles)
        self._cur = 0
        self.ctr_dev = torch.zeros(1, dtype=torch.int64, device=dev)          # the filter launches' own counter
        self.launches = 0                                                     # ... its host mirror
        # the from-scratch launch each chain's row descends from: its counter, the chain whose key it drew under, its length
        self.origin_dev = torch.full((C, 3), -1, dtype=torch.int64, device=dev)
        self._chain_ids = torch.arange(C, dtype=torch.int64, device=dev)
        # descriptor records of its own: the ensemble's static fields under the wrapper's seed and counter; re-uploaded per launch
        d = self._desc = ens._desc[:C].copy()
        d["seed"] = np.uint64((self.seed ^ _FILTER_SALT) & _SEED_MASK)
        d["step_ctr"] = self.ctr_dev.data_ptr()
        d["weights"], d["t1"] = 0, 0
        self.desc_dev = ens._upload_records(d)
        self.stage_index, self._log_z = 0, 0.0
        self._stages = dict(t=[], ess=[], increment=[], resampled=[], u=[])
        self._accepted, self._scales = [], []           # per stage, on the device until somebody asks
        self.finished = False
        ens.ll_dev.zero_()              # (the init pass's estimate of the whole series is not this population's)
        self._stage0()

    # -- what needs no device ------------------------------------------------------------------------------------------------
    @staticmethod
    def resolve_settings(model, parameters, observations=None, num_chains=None, N=1000, chunk=1, seed=0, init_mean=None,
                         init_sd=None, ess_target=0.5, moves=2, scale_factor=None, **ensemble_kwargs):
        """The wrapper's own arguments -> TemperedPopulation.resolve_settings's namespace (q0, the initial population, the
        scale) with N, chunk and y (the series, [T] f64) beside it, or the refusal.  Needs no device."""
        what = "SequentialPopulation (SMC^2 over resident PMMH chains) "
        kw = ensemble_kwargs
        if kw.get("correlation", None) is not None:
            raise NotImplementedError(what + "resamples theta, the estimate and the particle system across chains; with "
                                      "correlation the chains' normals would have to be carried through the chunks and gathered "
                                      "too, and that is not built: correlation stays None")
        if kw.get("sqmc", False):
            raise NotImplementedError(what + "extends every chain's filter by a warm-started launch; the sequential quasi-Monte "
                                      "Carlo filter has no warm start: sqmc stays False")
        if kw.get("sampler", "pmmh") != "pmmh":
            raise NotImplementedError(what + "moves the population by PMMH steps on the prefix: sampler stays 'pmmh', got "
                                      "sampler = '{0}'".format(kw["sampler"]))
        if kw.get("kind", "pf") != "pf":
            raise NotImplementedError(what + "carries every chain's particle system from chunk to chunk: kind='pf', got kind = "
                                      "'{0}' (the Kalman launch has no particle state to carry)".format(kw["kind"]))
        if isinstance(observations, (list, tuple)):
            raise NotImplementedError(what + "takes one series in time order: lists of sequences are not built")
        S, Bf = int(kw.get("subsequence_length", -1)), int(kw.get("buffer_length", -1))
        if S != -1 or Bf != -1:
            raise NotImplementedError(what + "chooses its own windows, the chunks and the prefixes: subsequence_length = "
                                      "buffer_length = -1, got {0} / {1}".format(S, Bf))
        M, K = kw.get("minibatch_size", None), kw.get("num_sequences", None)
        if (M is not None and int(M) != 1) or (K is not None and int(K) != 1):
            raise NotImplementedError(what + "runs one filter per chain: minibatch_size = num_sequences = 1, got minibatch_size "
                                      "= {0}, num_sequences = {1}".format(M, K))
        if kw.get("pf", "poyiadjis_N") != "poyiadjis_N":
            raise NotImplementedError(what + "reads the filter's log-likelihood and final particles only: pf stays "
                                      "'poyiadjis_N', got pf = '{0}'".format(kw["pf"]))
        if kw.get("resampling", "multinomial") != "multinomial":
            raise NotImplementedError(what + "warm-starts the multinomial filter kernels; the warm start of resampling = '{0}' is "
                                      "not established: resampling stays 'multinomial'".format(kw["resampling"]))
        if kw.get("ess_threshold", None) not in (None, 0):
            raise NotImplementedError(what + "warm-starts filters that resample at every step; the warm start of adaptive "
                                      "resampling (ess_threshold) is not established: ess_threshold stays None")
        if kw.get("pmmh_stat", None) not in (None, "none"):
            raise NotImplementedError(what + "launches the filter without a statistic: pmmh_stat stays None, got '{0}'".format(
                kw["pmmh_stat"]))
        if kw.get("dtype", "f64") != "f64":
            raise NotImplementedError(what + "keeps the particle systems and the weights in f64: dtype stays 'f64', got "
                                      "'{0}'".format(kw["dtype"]))
        if model not in _capi.THETA_DIM:
            raise ValueError("model must be 'svm', 'garch' or 'lgssm'")
        N = int(N)
        if not 1 <= N <= _MAX_N:
            raise NotImplementedError(what + "extends one-workgroup filters: 1 <= N <= 16384 (a whole-GPU window has no state to "
                                      "hand on), got N = {0}".format(N))
        if int(chunk) < 1:
            raise ValueError("chunk must be >= 1 observations per stage, got {0}".format(chunk))
        if num_chains is None:
            raise ValueError("num_chains is required")
        C = int(num_chains)
        if not _capi.SMC_MIN_CHAINS <= C <= _capi.SMC_MAX_CHAINS:
            raise NotImplementedError(what + "reweights and resamples the population in one workgroup: 2 <= num_chains <= 2^20, "
                                      "got {0}".format(C))
        if not 0.0 < float(ess_target) < 1.0:         # (false for a NaN as well)
            raise ValueError("ess_target must lie in (0, 1) (a stage resamples when ESS < ess_target * C), got {0}".format(
                ess_target))
        if int(moves) < 1:
            raise ValueError("moves must be >= 1 PMMH steps per resampling stage, got {0}".format(moves))
        if _world_size() > 1 or int(kw.get("chain_offset", 0) or 0) != 0:
            raise NotImplementedError(what + "is one interacting population: a process that is one rank of several (WORLD_SIZE > 1 "
                                      "or a chain_offset) would hold a part of it, and a rank partition is not built")
        # q0, the initial population by rejection to the support and the scale: TemperedPopulation's, stated there
        s = TemperedPopulation.resolve_settings(model, parameters, num_chains=C, seed=seed, init_mean=init_mean, init_sd=init_sd,
                                                ess_target=ess_target, moves=moves, scale_factor=scale_factor)
        s.N, s.chunk = N, int(chunk)
        s.y = None
        if observations is not None:
            s.y = np.ascontiguousarray(observations, dtype=np.float64).reshape(-1)
            if s.y.shape[0] < 1:
                raise ValueError("observations must hold at least one observation")
        return s

    # -- the launches --------------------------------------------------------------------------------------------------------
    def _record_ptrs(self):
        base = self._record_dev.data_ptr()
        return base, base + 8 * _capi.SEQ_RECORD_DOUBLES         # the record, the status word behind it

    def launch_filter(self, theta_dev, t0, length, warm, final, stream=None):
        """One filter launch for every chain on y[t0 : t0 + length) at the rows of theta_dev [C, MAX_THETA]: warm-started from
        the rows of buffer `warm` (None: from the prior), the final particle systems into the rows of buffer `final`, the
        records into the ensemble's out_dev.  Draws under (seed ^ the salt, chain id, the wrapper's counter); the counter
        advances afterwards."""
        e, d, C = self.ensemble, self._desc, self.C
        idx = np.arange(C, dtype=np.uint64)
        row, xs = np.uint64(8 * self.row_doubles), np.uint64(8 * self.N * _capi.STATE_DIM[self.model])
        d["theta"] = theta_dev.data_ptr() + idx * np.uint64(8 * _capi.MAX_THETA)
        d["y"], d["T"], d["tL"] = self.y_dev.data_ptr() + 8 * int(t0), int(length), int(length)
        if warm is None:
            d["init_x"] = d["init_logw"] = 0
        else:
            d["init_x"] = self.state_dev[warm].data_ptr() + idx * row
            d["init_logw"] = d["init_x"] + xs
        d["final_x"] = self.state_dev[final].data_ptr() + idx * row
        d["final_logw"] = d["final_x"] + xs
        self.desc_dev.copy_(self._torch.from_numpy(d.view(np.uint8).reshape(C, -1)))
        e.ctx.launch_device_smoother(e.model, e.kernel, e.dtype, "device", e._launch_smoother, self.N, C, self.desc_dev.data_ptr(),
                                     e._stream(stream))
        self.ctr_dev += 1
        self.launches += 1

    def launch_reweight(self, incr_ptr, stride, ess_target, stream=None):
        e = self.ensemble
        record, status = self._record_ptrs()
        e.ctx.seq_reweight_device(self.C, self.logw_dev.data_ptr(), incr_ptr, stride, ess_target, self.seed, self.stage_index,
                                  record, status, self.parent_dev.data_ptr(), self.cdf_dev.data_ptr(), e._stream(stream))

    def launch_gather(self, stream=None):
        """Rows, theta and ll by parent: the rows into the other buffer, theta and ll through theta_prop_dev (free between
        steps) and ll_tmp_dev; the buffers then swap roles."""
        e = self.ensemble
        e.ctx.seq_gather_device(self.C, self.parent_dev.data_ptr(), self.row_doubles, self.state_dev[self._cur].data_ptr(),
                                self.state_dev[1 - self._cur].data_ptr(), e.theta_dev.data_ptr(), e.theta_prop_dev.data_ptr(),
                                e.ll_dev.data_ptr(), self.ll_tmp_dev.data_ptr(), e._stream(stream))
        self._cur = 1 - self._cur
        self.origin_dev = self.origin_dev[self.parent_dev.long()]

    def launch_scale(self, stream=None):
        e = self.ensemble
        e.ctx.smc_scale_device(e.C, e.theta_dev.data_ptr(), self._slots, self.scale_factor, e.scale_dev.data_ptr(),
                               e._stream(stream))

    def launch_move(self, length, stream=None):
        """One PMMH step on the prefix y[0 : length): the ensemble's proposal, a filter from scratch at it into the other buffer,
        PMMH's accept step (never init) on the wrapper's counts, and the adopt."""
        e = self.ensemble
        e.launch_propose(stream)
        ctr = self.launches
        self.launch_filter(e.theta_prop_dev, 0, length, None, 1 - self._cur, stream)
        e.ctx.pmmh_accept_device(e.model, e.C, e.theta_dev.data_ptr(), e.theta_prop_dev.data_ptr(), e.valid_dev.data_ptr(),
                                 e.out_dev.data_ptr(), e.ll_dev.data_ptr(), self.accept_dev.data_ptr(), e.hyper, False,
                                 *e._update_key(stream))
        moved = (self.accept_dev != self.seen_dev).unsqueeze(1)
        fresh = self._torch.stack([self._torch.full_like(self._chain_ids, ctr), self._chain_ids,
                                   self._torch.full_like(self._chain_ids, int(length))], dim=1)
        self.origin_dev = self._torch.where(moved, fresh, self.origin_dev)
        e.ctx.seq_adopt_device(self.C, self.accept_dev.data_ptr(), self.seen_dev.data_ptr(), self.row_doubles,
                               self.state_dev[self._cur].data_ptr(), self.state_dev[1 - self._cur].data_ptr(), e._stream(stream))

    _STATUS = {1: "no chain has a finite weight", 2: "a chain's weight or estimate is NaN or +inf",
               4: "the population is not 2 .. 2^20 chains"}

    def _read_record(self, where):
        rec = self._record_dev.cpu().numpy()            # the stage's one host read (synchronises)
        status = int(rec[_capi.SEQ_RECORD_DOUBLES:].view(np.int32)[0])
        if status:
            raise RuntimeError("SMC^2 stage {0} ({1}): {2} (the population is as it was)".format(
                self.stage_index, where, "; ".join(t for bit, t in self._STATUS.items() if status & bit)))
        return rec

    def _book(self, rec, t):
        for key, v in zip(("increment", "ess", "resampled", "u"), rec[:4]):
            self._stages[key].append(float(v))
        self._stages["t"].append(int(t))
        self._accepted.append(self.accept_dev.sum())
        self._scales.append(self.ensemble.scale_dev.clone())
        self.stage_index += 1

    def _stage0(self):
        e = self.ensemble
        e.ctx.smc_logtarget_device(e.model, e.C, e.theta_dev.data_ptr(), e.ll_dev.data_ptr(), e.hyper, self.q0_mean_dev.data_ptr(),
                                   self.q0_sd_dev.data_ptr(), self.h_dev.data_ptr(), e._stream(None))
        self.launch_reweight(self.h_dev.data_ptr(), 1, _NEVER)
        rec = self._read_record("the q0 term")
        self._log_z += float(rec[0])
        self._book(rec, 0)

    def _resample_move(self, length):
        self.launch_gather()
        self.launch_scale()
        for _ in range(self.moves):
            self.launch_move(length)

    def _stage(self, k):
        e, t = self.ensemble, self.t
        first = t == 0
        self.launch_filter(e.theta_dev, t, k, None if first else self._cur, 1 - self._cur)
        self.launch_reweight(e.out_dev.data_ptr() + 8 * 4, _capi.OUT_DOUBLES, self.ess_target)
        try:
            rec = self._read_record("y[{0} : {1})".format(t, t + k))
        except RuntimeError:
            self.ctr_dev -= 1           # the launch is forgotten: its buffer is scratch, the weights were not touched
            self.launches -= 1
            raise
        e.ll_dev += e.out_dev[:, 4]
        self._cur = 1 - self._cur
        if first:                       # the rows come from this launch, each under its own chain's key
            self.origin_dev[:, 0], self.origin_dev[:, 1], self.origin_dev[:, 2] = self.launches - 1, self._chain_ids, k
        self.t = t + k
        if rec[2] != 0.0:
            self._resample_move(self.t)
        self._log_z += float(rec[0])
        self._book(rec, self.t)

    # -- the public loop -----------------------------------------------------------------------------------------------------
    def step(self, n=1):
        """n stages of `chunk` observations each (the last one of a series: what is left).  Returns the number run."""
        if self.finished:
            raise ValueError("the population was finished: its ensemble is a plain PMMH ensemble now")
        done = 0
        while done < n and self.t < self.T:
            self._stage(min(self.chunk, self.T - self.t))
            done += 1
        return done

    def run(self):
        """To the end of the series.  Returns schedule()."""
        self.step(self.T)
        return self.schedule()

    def extend(self, new_observations):
        """Append observations; the chunking continues from t."""
        if self.finished:
            raise ValueError("the population was finished: its ensemble is a plain PMMH ensemble now")
        torch = self._torch
        new = np.ascontiguousarray(new_observations, dtype=np.float64).reshape(-1)
        if new.shape[0]:
            self.y_dev = torch.cat([self.y_dev, torch.from_numpy(new).to(self.y_dev.device)])
            self.T = int(self.y_dev.shape[0])

    def finish(self):
        """The end of the sequential run: if the weights are not all equal, one forced resample-move on the series so far (its
        evidence increment is 0: it is not a stage); then `ensemble` is a plain PMMH ChainEnsemble on y[0 : t) whose chains are
        posterior-distributed and whose proposal scale is the population's.  Returns it."""
        e, torch = self.ensemble, self._torch
        if self.t < 1:
            raise ValueError("finish() needs at least one stage of observations")
        if not self.finished:
            if bool((self.logw_dev != self.logw_dev[0]).any().item()):
                self.h_dev.zero_()
                self.launch_reweight(self.h_dev.data_ptr(), 1, 1.0)
                rec = self._read_record("finish")
                if rec[2] != 0.0:
                    self._resample_move(self.t)
                self._book(rec, self.t)
            e.y_dev, e.T = self.y_dev[:self.t].contiguous(), self.t
            e._desc["y"], e._desc["T"], e._desc["tL"] = e.y_dev.data_ptr(), self.t, self.t
            e.desc_dev.copy_(torch.from_numpy(e._desc.view(np.uint8).reshape(e._nl, -1)))
            e.synchronize()
            e.proposal_scale = e.scale_dev.cpu().numpy()
            self.finished = True
        return e

    # -- results -------------------------------------------------------------------------------------------------------------
    def weights(self):
        """[C] the chains' normalised weights."""
        return self._torch.softmax(self.logw_dev, 0).cpu().numpy()

    def ess(self):
        w = self.weights()
        return float(1.0 / np.sum(w * w))

    def posterior_mean(self):
        """[P] the weighted mean of theta given y[0 : t)."""
        w = self._torch.softmax(self.logw_dev, 0)
        P = _capi.THETA_DIM[self.model]
        return (w.unsqueeze(1) * self.ensemble.theta_dev[:, :P]).sum(0).cpu().numpy()

    def evidence_increments(self):
        """One entry per stage: stage 0 is the q0 term, stage s >= 1 the estimate of log p(y[t_{s-1} : t_s) | y[0 : t_{s-1})), the
        chunk's prequential score; a forced resampling of finish() adds a 0."""
        return np.array(self._stages["increment"], dtype=np.float64)

    def log_evidence(self):
        """sum of the stages' increments + log m(q0), m(q0) the mass of the untruncated q0 on the support: an estimate of
        log of the integral over the support of exp(logprior(theta)) p(y[0 : t) | theta) d theta for the UNNORMALISED prior
        density the PMMH chains target (tempering.py's module docstring).  Not a ready Bayes factor between models: that needs
        the prior's mass too."""
        return self._log_z + log_q0_mass(self.model, self.q0_mean, self.q0_sd)

    def schedule(self):
        """Per stage: t (observations taken after it), ess (before resampling), resampled, increment, u (the resampling
        uniform), acceptance (accepted proposals / (C * moves); 0 where the stage did not move) and scale [stages, P]."""
        torch = self._torch
        out = {k: np.array(v, dtype=np.int64 if k == "t" else np.float64) for k, v in self._stages.items()}
        S, P = self.stage_index, _capi.THETA_DIM[self.model]
        cum = torch.stack(self._accepted).cpu().numpy().astype(np.float64) if S else np.zeros(0)
        out["acceptance"] = np.diff(np.concatenate([[0.0], cum])) / (self.C * self.moves)
        out["scale"] = torch.stack(self._scales).cpu().numpy()[:, :P] if S else np.zeros((0, P))
        return out

    def row_origin(self):
        """[C, 3] int64 per chain: the counter of the launch FROM SCRATCH its particle system descends from, the chain under
        whose key that launch drew, and its length.  Right after a move (or the first chunk) that launch alone reproduces the
        row; later extensions continue it."""
        return self.origin_dev.cpu().numpy()

    def state_rows(self):
        """[C, N (NS + 1)] the chains' particle systems: x [N][NS], then logw [N]."""
        return self.state_dev[self._cur].cpu().numpy()

    # -- checkpoint ----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """The ensemble's dict plus, under 'sequential': t, the weights, the chains' rows, the counters, the schedule, q0, the
        scale and what load_state_dict compares."""
        state = self.ensemble.state_dict()
        state["sequential"] = dict(
            t=self.t, logw=self.logw_dev.cpu().numpy(), rows=self.state_rows(), launches=self.launches, log_evidence=self._log_z,
            stage=self.stage_index, schedule=self.schedule(), cumulative_accepts=[int(a.item()) for a in self._accepted],
            q0_mean=self.q0_mean.copy(), q0_sd=self.q0_sd.copy(), scale=self.ensemble.scale_dev.cpu().numpy(),
            n_accept=self.accept_dev.cpu().numpy(), seen=self.seen_dev.cpu().numpy(), origin=self.row_origin(),
            ess_target=self.ess_target, moves=self.moves, C=self.C, N=self.N, chunk=self.chunk, scale_factor=self.scale_factor,
            finished=self.finished)
        return state

    def load_state_dict(self, state):
        torch = self._torch
        q = state["sequential"]
        for key in ("C", "N", "chunk", "ess_target", "moves", "scale_factor"):
            if q[key] != getattr(self, key):
                raise ValueError("checkpoint {0} = {1} does not match the population ({2})".format(key, q[key], getattr(self, key)))
        for key, mine in (("q0_mean", self.q0_mean), ("q0_sd", self.q0_sd)):
            if not np.array_equal(np.asarray(q[key]), mine):
                raise ValueError("checkpoint {0} = {1} does not match the population ({2})".format(key, q[key], mine))
        if int(q["t"]) > self.T:
            raise ValueError("checkpoint t = {0} is past the population's series (T = {1})".format(q["t"], self.T))
        if q["finished"] or self.finished:
            raise ValueError("a finished population is a plain ensemble: checkpoint its ensemble")
        e = self.ensemble
        e.load_state_dict({k: v for k, v in state.items() if k != "sequential"})
        dev = e.device
        put = lambda t, a, dt: t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=dt)))
        self.t, self.launches, self.stage_index, self._log_z = int(q["t"]), int(q["launches"]), int(q["stage"]), float(q["log_evidence"])
        self.ctr_dev.fill_(self.launches)
        put(self.logw_dev, q["logw"], np.float64)
        put(self.state_dev[self._cur], q["rows"], np.float64)
        put(e.scale_dev, q["scale"], np.float64)
        e.proposal_scale = np.array(q["scale"], dtype=np.float64)
        put(self.accept_dev, q["n_accept"], np.int64)
        put(self.seen_dev, q["seen"], np.int64)
        self.origin_dev = torch.from_numpy(np.ascontiguousarray(q["origin"], dtype=np.int64)).to(dev)
        sched = q["schedule"]
        self._stages = {k: [int(v) if k == "t" else float(v) for v in sched[k]] for k in self._stages}
        self._accepted = [torch.tensor(int(v), dtype=torch.int64, device=dev) for v in q["cumulative_accepts"]]
        full = np.ones((self.stage_index, _capi.MAX_THETA))
        full[:, :np.shape(sched["scale"])[1]] = sched["scale"]
        self._scales = [torch.from_numpy(row.copy()).to(dev) for row in full]
        e.synchronize()
