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


def _columns():
    from sgmcmc_ssm_amd import _capi
    cols = []
    for name in _capi.DEV_PROBLEM_DTYPE.names:
        kind = _capi.DEV_PROBLEM_DTYPE.fields[name][0]
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


def build(case):
    name, model, obs, kw = case
    kw = dict(kw)
    seed = 100 + [c[0] for c in CASES].index(name)
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


def _buffers(ens):
    """[(index into BUFFERS, first byte, one past the last byte)] of the tensors `ens` holds."""
    out = []
    for i, name in enumerate(BUFFERS):
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


def _desc_matrix(ens, d):
    from sgmcmc_ssm_amd import _capi
    bufs = _buffers(ens)
    cols = []
    for name in _capi.DEV_PROBLEM_DTYPE.names:
        v = np.ascontiguousarray(d[name])
        if v.dtype == np.dtype("u8") and name not in NOT_POINTERS:
            named = np.array([_name_pointer(bufs, a) for a in v], dtype=np.int64).reshape(-1, 2)
            cols += [named[:, 0], named[:, 1]]
        elif v.dtype == np.dtype("f8"):
            cols.append(v.view(np.int64))
        else:
            cols.append(v.astype(np.uint64).view(np.int64) if v.dtype == np.dtype("u8") else v.astype(np.int64))
    return np.stack(cols, axis=1)


def _descriptors(ens):
    from sgmcmc_ssm_amd import _capi
    on_device = getattr(ens, "_multi", False) or getattr(ens, "window_sampling", "host") == "device"
    if on_device:
        d = ens.desc_dev.cpu().numpy().reshape(-1).view(_capi.DEV_PROBLEM_DTYPE)
    else:
        d = ens._desc
    return _desc_matrix(ens, d)


class CallRecorder(object):
    """Forwards every method of a _capi.Context and logs (name, arguments)."""

    def __init__(self, ctx, ens):
        self._ctx, self._ens, self.log = ctx, ens, []

    def _encode(self, x):
        from sgmcmc_ssm_amd import _capi
        if isinstance(x, _capi.PriorHyper):
            return "hyper:" + bytes(x).hex()
        if isinstance(x, (bool, np.bool_)):
            return bool(x)
        if isinstance(x, (int, np.integer)):
            x = int(x)
            if x >= 1 << 32:            # no scalar argument is that large but the two salted seeds, which fit no buffer
                for i, lo, hi in _buffers(self._ens):
                    if lo <= x < hi:
                        return "{0}+{1}".format(BUFFERS[i], x - lo)
            return x
        if isinstance(x, float):
            return x.hex()
        if x is None or isinstance(x, str):
            return x
        raise TypeError("unexpected argument {0!r}".format(x))

    def __getattr__(self, name):
        attr = getattr(self._ctx, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            # every logged method takes the stream handle last: the steps run on the default stream, 0; any other handle is
            # a per-process address and is logged as such
            logged, a = name, [self._encode(v) for v in args[:-1]] + [args[-1] and "stream"]
            if name == "launch_device":         # = launch_device_smoother(..., "nemeth", ...): the same dispatch
                logged, a = "launch_device_smoother", a[:4] + ["nemeth"] + a[4:]
            self.log.append([logged, a, {k: self._encode(v) for k, v in sorted(kw.items())}])
            return attr(*args, **kw)
        return call


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
    lam = getattr(ens, "lambduh", None)
    info = dict(S=getattr(ens, "S", None), B=getattr(ens, "B", None), lambduh=None if lam is None else float(lam).hex(),
                W=getattr(ens, "W", None))
    for flag in ("_multi", "_draws", "_rescale"):
        v = getattr(ens, flag, None)
        info[flag] = None if v is None else bool(v)
    info = {k: (int(v) if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else v) for k, v in info.items()}
    info["calls"] = rec.log
    if with_results:
        if resident:
            stat, ll = ens.results()
            arrays["ab_theta"] = ens.theta_dev.cpu().numpy()
        else:
            stat, ll = ens.last_gradient_statistics()
            arrays["ab_theta"] = ens.theta()
        arrays["ab_stat"] = np.asarray(stat)
        if ll is not None:
            arrays["ab_loglik"] = np.asarray(ll)
    return arrays, json.loads(json.dumps(info))


def record_all(with_results=False):
    arrays, meta = {}, {"columns": _columns(), "buffers": list(BUFFERS), "cases": {}}
    for case in CASES:
        a, info = record_case(case, with_results)
        meta["cases"][case[0]] = info
        for k, v in a.items():
            arrays["{0}/{1}".format(case[0], k)] = v
    return arrays, meta


def main(path=FIXTURE):
    arrays, meta = record_all()
    np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,",
          sum(v.shape[1] for k, v in arrays.items() if k.endswith("/desc")), "descriptors")


if __name__ == "__main__":
    main(*sys.argv[1:2])
