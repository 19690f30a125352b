"""Record what the device code of a resident ensemble receives: tests/golden/ensemble_desc.npz.

    python tests/golden/make_ensemble_golden.py [path]   (on an MI355X, with the library built)

What a kernel sees of a ChainEnsemble / ResidentWindows is its descriptor array, its resident buffers and the arguments of
every call into the library.  For each case of CASES this records

  * the descriptor records after construction and after each of STEPS steps -- host-drawn windows from `_desc`, device-drawn
    ones read back from `desc_dev` -- as one int64 matrix [STEPS + 1, n, len(COLUMNS)]: every pointer field becomes the pair
    (index into BUFFERS of the tensor it points into, byte offset from that tensor's data_ptr()), null = (-1, 0); the three
    double fields are stored as their bit patterns;
  * weights_dev / bounds_dev / woffs_dev / seq_len_dev after the steps, and S, B, lambduh, W and the three flags;
  * the log of the library calls of the steps (method name, scalar arguments, pointers named as above, the hyper struct as
    bytes), taken by a forwarding recorder put in place of `ctx`.  `launch_device(...)` is logged as the
    `launch_device_smoother(..., "nemeth", ...)` it is: both reach the same dispatch of csrc/pfg_plan.hip.

tests/test_gpu_ensemble_golden.py replays record_case() and compares everything for equality.  The fixture was written at
the commit before ensemble.py resolved its settings, descriptors and windows once each; it only uses names both trees have.

A second fixture, tests/golden/ensemble_samplers.npz (`python tests/golden/make_ensemble_golden.py samplers [path]`), does the
same for SAMPLER_CASES: the samplers and chain filters that came after the first one -- 'pmmh' (plain, correlated, SQMC),
'pmala', 'pmala_sorted', 'pgibbs', 'sgd', 'adagrad', 'sgld_cv', the resampling schemes and the O(N^2) smoother.  Beside what the
first fixture holds, a case of it records

  * the library calls of the CONSTRUCTOR (the init pass, the rho = 0 launch, the commit, the centring launches): the recorder
    stands in for `_capi.default_context` while the ensemble is built, keeps the raw arguments and names the pointers once the
    buffers exist; `constructor_calls` says how many of the logged calls those are;
  * the chain-filter records `_cpm_desc` / `_sqmc_desc` / `_csmc_desc` / `_centre_desc`, pointers named as above;
  * state_dict() after the steps as a sorted list of (key, dtype, shape), plain scalars by value; that load_state_dict() of
    it into a fresh ensemble of the case leaves an equal state_dict(); and what that fresh ensemble answers to the same
    checkpoint under another sampler, correlation, sqmc, T or lambduh: the exception's type and full text, or null where it
    takes it;
  * GRAPH cases: run(4, thin=2, graph_steps=2) in place of the three steps, so the log holds the eager step and the captured ones.

It was written at the commit before ensemble.py stated its samplers and chain filters in two tables.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(HERE, "ensemble_desc.npz")
STEPS = 3
BUFFERS = ("y_dev", "theta_dev", "out_dev", "win_out_dev", "step_ctr", "scratch_dev", "weights_dev", "stamps_dev",
           "seq_len_dev", "bounds_dev", "woffs_dev", "desc_dev", "momentum_dev")
NOT_POINTERS = ("seed", "stream", "paris_consumed")           # the other "u8" fields of pfg_dev_problem are addresses
SAMPLER_FIXTURE = os.path.join(HERE, "ensemble_samplers.npz")
SAMPLER_BUFFERS = BUFFERS + (
    "theta_prop_dev", "valid_dev", "ll_dev", "accept_dev", "scale_dev", "grad_cur_dev",
    "aux_dev", "which_dev", "seen_dev", "cpm_desc_dev", "sqmc_desc_dev",
    "csmc_desc_dev", "_csmc_init_desc_dev", "path_dev", "ndeg_dev", "csmc_scratch_dev",
    "moment_dev",
    "theta_centre_dev", "centre_grad_dev", "centre_ctr_dev", "out_centre_dev", "twin_out_dev", "twin_seq_len_dev",
    "centre_out_dev", "centre_acc_dev", "centre_scratch_dev", "centre_desc_dev")
# the chain-filter records of a case that has them: attribute -> the numpy mirror in _capi
RECORDS = (("_cpm_desc", "CPM_PROBLEM_DTYPE"), ("_sqmc_desc", "SQMC_PROBLEM_DTYPE"), ("_csmc_desc", "CSMC_PROBLEM_DTYPE"),
           ("_centre_desc", "DEV_PROBLEM_DTYPE"))


def _columns(dtype=None):
    from sgmcmc_ssm_amd import _capi
    dtype = _capi.DEV_PROBLEM_DTYPE if dtype is None else dtype
    cols = []
    for name in dtype.names:
        kind = dtype.fields[name][0]
        if kind == np.dtype("u8") and name not in NOT_POINTERS:
            cols += [name + ".buffer", name + ".offset"]
        else:
            cols.append(name)
    return cols


def _series(model, T, seed):
    from sgmcmc_ssm_amd.models.svm import generate_svm_data
    from sgmcmc_ssm_amd.models.garch import generate_garch_data
    from sgmcmc_ssm_amd.models.lgssm import generate_lgssm_data
    np.random.seed(seed)
    gen = dict(svm=generate_svm_data, garch=generate_garch_data, lgssm=generate_lgssm_data)[model]
    return gen(T=T, parameters=_params(model))["observations"].reshape(-1)


def _params(model):
    from sgmcmc_ssm_amd.models.svm import SVMParameters
    from sgmcmc_ssm_amd.models.garch import GARCHParameters
    from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters
    if model == "svm":
        return SVMParameters(A=np.eye(1) * 0.95, Q=np.eye(1) * 0.5, R=np.eye(1) * 0.5)
    if model == "lgssm":
        return LGSSMParameters(A=np.eye(1) * 0.9, C=np.eye(1) * 1.0, Q=np.eye(1) * 0.7, R=np.eye(1) * 1.0)
    lm, lp, ll = GARCHParameters.convert_alpha_beta_gamma(0.1, 0.8, 0.05)
    return GARCHParameters(log_mu=lm, logit_phi=lp, logit_lambduh=ll, LRinv=np.eye(1) * 0.3 ** -0.5)


def _list(model, lengths, seed):
    y = _series(model, int(sum(lengths)), seed)
    cuts = np.concatenate([[0], np.cumsum(lengths)])
    return [y[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


WIN = dict(subsequence_length=8, buffer_length=2)
LIST = [20, 7, 13]
# name -> (model, observations: T or a list of lengths, constructor keywords); "stamps": enable_stamps() after construction;
# "theta": start from a [C, P] array instead of a Parameters object
CASES = [
    ("svm_full", "svm", 40, dict(num_chains=3, N=64)),
    ("svm_host", "svm", 40, dict(num_chains=3, N=64, **WIN)),
    ("svm_host_strict", "svm", 40, dict(num_chains=3, N=64, partition_style="strict", **WIN)),
    ("svm_device", "svm", 40, dict(num_chains=3, N=64, window_sampling="device", **WIN)),
    ("garch_nemeth", "garch", 40, dict(num_chains=3, N=64, pf="nemeth")),
    ("lgssm_marginal", "lgssm", 40, dict(num_chains=3, kind="marginal", **WIN)),
    ("lgssm_complete", "lgssm", 40, dict(num_chains=3, kind="complete", num_samples=3, **WIN)),
    ("lgssm_gibbs", "lgssm", 40, dict(num_chains=3, sampler="gibbs")),
    ("lgssm_sgrld", "lgssm", 40, dict(num_chains=3, N=64, sampler="sgrld")),
    ("svm_sghmc", "svm", 40, dict(num_chains=3, N=64, sampler="sghmc", friction=0.3)),
    ("svm_paris", "svm", 40, dict(num_chains=3, N=64, pf="paris", Ntilde=3, accept_reject=False)),
    ("svm_systematic", "svm", 40, dict(num_chains=3, N=64, resampling="systematic")),
    ("svm_f32", "svm", 40, dict(num_chains=3, N=64, dtype="f32")),
    ("svm_n2000", "svm", 20, dict(num_chains=2, N=2000)),
    ("svm_theta_offset", "svm", 40, dict(theta=4, N=64, chain_offset=5, **WIN)),
    ("list_host", "svm", LIST, dict(num_chains=4, N=64, **WIN)),
    ("list_whole", "svm", LIST, dict(num_chains=4, N=64, subsequence_length=-1, buffer_length=2)),
    ("multi_series", "svm", 40, dict(num_chains=3, N=64, minibatch_size=3, window_sampling="device", **WIN)),
    ("multi_list", "svm", LIST, dict(num_chains=3, N=64, num_sequences=2, minibatch_size=2, window_sampling="device", **WIN)),
    ("multi_list_static", "svm", LIST, dict(num_chains=3, N=64, num_sequences=-1, subsequence_length=-1, buffer_length=2)),
    ("multi_paris_n1500", "svm", 20, dict(num_chains=2, N=1500, pf="paris", minibatch_size=2, window_sampling="device", **WIN)),
    ("stamps_single", "svm", 40, dict(num_chains=3, N=64, stamps=True, **WIN)),
    ("stamps_multi", "svm", 40, dict(num_chains=3, N=64, minibatch_size=2, window_sampling="device", stamps=True, **WIN)),
    ("resident_windows", "svm", 6, dict(resident=True)),
]

MH = dict(num_chains=3, N=64, proposal_scale=0.05)
WHOLE_LIST = dict(num_sequences=-1, subsequence_length=-1, buffer_length=0, window_sampling="device")
CV = dict(num_chains=3, N=64, sampler="sgld_cv")
# as CASES; "graph": run(4, thin=2, graph_steps=2) in place of the STEPS steps
SAMPLER_CASES = [
    ("pmmh_svm", "svm", 40, dict(sampler="pmmh", **MH)),
    ("pmmh_score", "svm", 40, dict(sampler="pmmh", pmmh_stat="score", **MH)),
    ("pmmh_lgssm_marginal", "lgssm", 40, dict(sampler="pmmh", kind="marginal", **MH)),
    ("pmmh_list", "svm", LIST, dict(sampler="pmmh", **MH, **WHOLE_LIST)),
    ("pmmh_correlated", "svm", 40, dict(sampler="pmmh", correlation=0.9, **MH)),
    ("pmmh_sqmc", "svm", 40, dict(sampler="pmmh", sqmc=True, **MH)),
    ("pmala_svm", "svm", 40, dict(sampler="pmala", **MH)),
    ("pmala_lgssm_marginal", "lgssm", 40, dict(sampler="pmala", kind="marginal", **MH)),
    ("pmala_sorted_correlated", "svm", 40, dict(sampler="pmala_sorted", correlation=0.9, pf="nemeth", **MH)),
    ("pmala_sorted_sqmc", "svm", 40, dict(sampler="pmala_sorted", sqmc=True, **MH)),
    ("pgibbs_svm", "svm", 40, dict(num_chains=3, N=64, sampler="pgibbs")),
    ("pgibbs_lgssm", "lgssm", 40, dict(num_chains=3, N=64, sampler="pgibbs")),
    ("sgd", "svm", 40, dict(num_chains=3, N=64, sampler="sgd")),
    ("adagrad", "svm", 40, dict(num_chains=3, N=64, sampler="adagrad")),
    ("cv_host", "svm", 40, dict(CV, **WIN)),
    ("cv_device", "svm", 40, dict(CV, window_sampling="device", **WIN)),
    ("cv_multi", "svm", 40, dict(CV, minibatch_size=2, window_sampling="device", **WIN)),
    ("cv_lgssm_marginal", "lgssm", 40, dict(num_chains=3, sampler="sgld_cv", kind="marginal", **WIN)),
    ("sgld_adaptive", "svm", 40, dict(num_chains=3, N=64, ess_threshold=0.5)),
    ("sgld_stratified", "svm", 40, dict(num_chains=3, N=64, resampling="stratified")),
    ("sgld_n2", "svm", 40, dict(num_chains=3, N=64, pf="poyiadjis_N2")),
    ("graph_pmmh_correlated", "svm", 40, dict(sampler="pmmh", correlation=0.9, graph=True, **MH)),
    ("graph_cv_device", "svm", 40, dict(CV, window_sampling="device", graph=True, **WIN)),
]


def _seed(name):
    for base, cases in ((100, CASES), (200, SAMPLER_CASES)):
        names = [c[0] for c in cases]
        if name in names:
            return base + names.index(name)
    raise KeyError(name)


def build(case):
    name, model, obs, kw = case
    kw = dict(kw)
    kw.pop("graph", None)
    seed = _seed(name)
    y = _list(model, obs, seed) if isinstance(obs, list) else _series(model, obs, seed)
    if kw.pop("resident", False):
        from sgmcmc_ssm_amd.grid import ResidentWindows
        th = np.tile(_params(model).theta(), (2, 1)) * np.array([[1.0], [0.98]])
        return ResidentWindows(model, y, th, N=20000, t1=1, tL=5, weights=np.linspace(2.0, 3.0, 4), prior_var=2.0, seed=9,
                               stream0=3)
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    stamps = kw.pop("stamps", False)
    C = kw.pop("theta", None)
    if C is not None:
        p0 = np.tile(_params(model).theta(), (C, 1)) * np.linspace(1.0, 0.97, C)[:, None]
    else:
        p0 = _params(model)
    ens = ChainEnsemble(model, y, p0, epsilon=0.01, seed=seed, **kw)
    if stamps:
        ens.enable_stamps()
    return ens


def _buffers(ens, names=BUFFERS):
    """[(index into `names`, first byte, one past the last byte)] of the tensors `ens` holds."""
    out = []
    for i, name in enumerate(names):
        t = getattr(ens, name, None)
        if t is not None and t.numel() > 0:
            out.append((i, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))
    return out


def _name_pointer(bufs, addr):
    addr = int(addr)
    if addr == 0:
        return -1, 0
    for i, lo, hi in bufs:
        if lo <= addr < hi:
            return i, addr - lo
    raise AssertionError("address {0:#x} lies in none of the ensemble's buffers".format(addr))


def _desc_matrix(ens, d, names=BUFFERS):
    """The records d (of any of the descriptor dtypes) as an int64 matrix [len(d), len(_columns(d.dtype))]."""
    bufs = _buffers(ens, names)
    cols = []
    for name in d.dtype.names:
        v = np.ascontiguousarray(d[name])
        if v.dtype == np.dtype("u8") and name not in NOT_POINTERS:
            named = np.array([_name_pointer(bufs, a) for a in v], dtype=np.int64).reshape(-1, 2)
            cols += [named[:, 0], named[:, 1]]
        elif v.dtype == np.dtype("f8"):
            cols.append(v.view(np.int64))
        else:
            cols.append(v.astype(np.uint64).view(np.int64) if v.dtype == np.dtype("u8") else v.astype(np.int64))
    return np.stack(cols, axis=1)


def _descriptors(ens, names=BUFFERS):
    from sgmcmc_ssm_amd import _capi
    on_device = getattr(ens, "_multi", False) or getattr(ens, "window_sampling", "host") == "device"
    if on_device:
        d = ens.desc_dev.cpu().numpy().reshape(-1).view(_capi.DEV_PROBLEM_DTYPE)
    else:
        d = ens._desc
    return _desc_matrix(ens, d, names)


class CallRecorder(object):
    """Forwards every method of a _capi.Context and logs (name, arguments).  The arguments are kept raw and encoded when
    `log` is read, so it may record before the ensemble's buffers exist (`ens` is then set once they do)."""

    def __init__(self, ctx, ens, names=BUFFERS):
        self._ctx, self._ens, self._names, self._raw = ctx, ens, names, []

    def _encode(self, x, bufs):
        if isinstance(x, (bool, np.bool_)):
            return bool(x)
        if isinstance(x, (int, np.integer)):
            x = int(x)
            if x >= 1 << 32:            # no scalar argument is that large but the salted seeds, which fit no buffer
                for i, lo, hi in bufs:
                    if lo <= x < hi:
                        return "{0}+{1}".format(self._names[i], x - lo)
            return x
        if isinstance(x, float):
            return x.hex()
        if x is None or isinstance(x, str):
            return x
        raise TypeError("unexpected argument {0!r}".format(x))

    @property
    def log(self):
        bufs = _buffers(self._ens, self._names)
        return [[name, [self._encode(v, bufs) for v in a], {k: self._encode(v, bufs) for k, v in sorted(kw.items())}]
                for name, a, kw in self._raw]

    def __getattr__(self, name):
        attr = getattr(self._ctx, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            from sgmcmc_ssm_amd import _capi
            a = ["hyper:" + bytes(v).hex() if isinstance(v, _capi.PriorHyper) else v for v in args]
            logged = name
            if not name.startswith("scratch_bytes"):        # (those are questions about sizes: no stream)
                # every other logged method takes the stream handle last: the steps run on the default stream, 0; any other
                # handle is a per-process address and is logged as such
                a[-1] = a[-1] and "stream"
            if name == "launch_device":         # = launch_device_smoother(..., "nemeth", ...): the same dispatch
                logged, a = "launch_device_smoother", a[:4] + ["nemeth"] + a[4:]
            self._raw.append((logged, a, dict(kw)))
            return attr(*args, **kw)
        return call


def _build_recorded(case):
    """(ens, rec): the case's ensemble, built with the recorder in place of _capi.default_context."""
    from sgmcmc_ssm_amd import _capi
    real, rec = _capi.default_context, CallRecorder(None, None, SAMPLER_BUFFERS)

    def recording(device_id=None):
        rec._ctx = real(device_id)
        return rec
    _capi.default_context = recording
    try:
        ens = build(case)
    finally:
        _capi.default_context = real
    rec._ens = ens
    return ens, rec


def _settings(ens, rec):
    lam = getattr(ens, "lambduh", None)
    info = dict(S=getattr(ens, "S", None), B=getattr(ens, "B", None), lambduh=None if lam is None else float(lam).hex(),
                W=getattr(ens, "W", None))
    for flag in ("_multi", "_draws", "_rescale"):
        v = getattr(ens, flag, None)
        info[flag] = None if v is None else bool(v)
    info = {k: (int(v) if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else v) for k, v in info.items()}
    info["calls"] = rec.log
    return info


def _results(ens, arrays, resident=False):
    if resident:
        stat, ll = ens.results()
        arrays["ab_theta"] = ens.theta_dev.cpu().numpy()
    else:
        stat, ll = ens.last_gradient_statistics()
        arrays["ab_theta"] = ens.theta()
    if stat is not None:
        arrays["ab_stat"] = np.asarray(stat)
    if ll is not None:
        arrays["ab_loglik"] = np.asarray(ll)


def record_case(case, with_results=False):
    """{key: ndarray} and the JSON-able settings / call log of one case.  with_results adds theta and the latest gradient
    statistics after the steps (bytes of what the kernels computed: for A/B runs, not for the fixture)."""
    import torch
    ens = build(case)
    resident = case[3].get("resident", False)
    snaps = [_descriptors(ens)]
    rec = CallRecorder(ens.ctx, ens)
    ens.ctx = rec
    for _ in range(STEPS):
        if resident:
            ens.launch()
        else:
            ens.step(1)
        torch.cuda.synchronize(ens.device)
        snaps.append(_descriptors(ens))
    ens.ctx = rec._ctx
    arrays = {"desc": np.stack(snaps)}
    for name in ("weights_dev", "bounds_dev", "woffs_dev", "seq_len_dev"):
        t = getattr(ens, name, None)
        if t is not None:
            arrays[name] = t.cpu().numpy()
    info = _settings(ens, rec)
    if with_results:
        _results(ens, arrays, resident)
    return arrays, json.loads(json.dumps(info))


def _checkpoint(state):
    """state_dict() as a sorted list: [key, dtype, shape] of an array, [key, value] of a plain scalar."""
    out = []
    for key in sorted(state):
        v = state[key]
        if isinstance(v, np.ndarray):
            out.append([key, str(v.dtype), list(v.shape)])
        else:
            assert v is None or isinstance(v, (bool, int, float, str)), (key, type(v))
            out.append([key, v])
    return out


def _same_state(a, b):
    return sorted(a) == sorted(b) and all(
        (isinstance(b[k], np.ndarray) and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
         np.array_equal(a[k], b[k], equal_nan=True)) if isinstance(a[k], np.ndarray) else
        (type(a[k]) is type(b[k]) and a[k] == b[k]) for k in a)


def _other_checkpoints(ens, state):
    """name -> the checkpoint `state` with that one entry made another's."""
    return dict(sampler=dict(state, sampler="pmala_sorted" if ens.sampler == "pgibbs" else "pgibbs"),
                correlation=dict(state, correlation=0.5),
                sqmc=dict(state, sqmc=not bool(state.get("sqmc", False))),
                T=dict(state, T=ens.T + 1),
                lambduh=dict(state, lambduh=0.5))


def record_sampler_case(case, with_results=False):
    """record_case() for a case of SAMPLER_CASES: the constructor's calls, the chain-filter records and the checkpoint too."""
    import torch
    from sgmcmc_ssm_amd import _capi
    names = SAMPLER_BUFFERS
    ens, rec = _build_recorded(case)
    constructor_calls = len(rec._raw)
    snaps = [_descriptors(ens, names)]
    if case[3].get("graph", False):
        ens.run(4, thin=2, graph_steps=2)
        torch.cuda.synchronize(ens.device)
        snaps.append(_descriptors(ens, names))
    else:
        for _ in range(STEPS):
            ens.step(1)
            torch.cuda.synchronize(ens.device)
            snaps.append(_descriptors(ens, names))
    ens.ctx = rec._ctx
    arrays = {"desc": np.stack(snaps)}
    for name in ("weights_dev", "bounds_dev", "woffs_dev", "seq_len_dev", "twin_seq_len_dev"):
        t = getattr(ens, name, None)
        if t is not None:
            arrays[name] = t.cpu().numpy()
    for attr, dtype in RECORDS:
        d = getattr(ens, attr, None)
        if d is not None:
            assert d.dtype == getattr(_capi, dtype), attr
            arrays[attr.lstrip("_")] = _desc_matrix(ens, d, names)
    info = _settings(ens, rec)
    info["constructor_calls"] = constructor_calls
    state = ens.state_dict()
    info["state_dict"] = _checkpoint(state)
    fresh = build(case)
    info["refused"] = {}
    for what, other in sorted(_other_checkpoints(ens, state).items()):
        try:
            fresh.load_state_dict(other)
            info["refused"][what] = None            # (taken: recorded as it is)
        except Exception as e:
            info["refused"][what] = [type(e).__name__, str(e)]
    fresh.load_state_dict(state)
    info["round_trip"] = _same_state(fresh.state_dict(), state)
    if with_results:
        _results(ens, arrays)
    return arrays, json.loads(json.dumps(info))


def record_all(with_results=False, samplers=False):
    cases, record, buffers = (SAMPLER_CASES, record_sampler_case, SAMPLER_BUFFERS) if samplers else (CASES, record_case, BUFFERS)
    arrays, meta = {}, {"columns": _columns(), "buffers": list(buffers), "cases": {}}
    if samplers:
        from sgmcmc_ssm_amd import _capi
        meta["record_columns"] = {attr.lstrip("_"): _columns(getattr(_capi, dtype)) for attr, dtype in RECORDS}
    for case in cases:
        a, info = record(case, with_results)
        meta["cases"][case[0]] = info
        for k, v in a.items():
            arrays["{0}/{1}".format(case[0], k)] = v
    return arrays, meta


def main(path=None, samplers=False):
    path = path or (SAMPLER_FIXTURE if samplers else FIXTURE)
    arrays, meta = record_all(samplers=samplers)
    np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,",
          sum(v.shape[1] for k, v in arrays.items() if k.endswith("/desc")), "descriptors")


if __name__ == "__main__":
    args = sys.argv[1:]
    main(*[a for a in args if a != "samplers"][:1], samplers="samplers" in args)
