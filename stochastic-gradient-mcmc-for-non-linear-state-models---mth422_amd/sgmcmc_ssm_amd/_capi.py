"""ctypes binding of libpfgrad.so (include/pfgrad.h).

This is the only door from Python to the particle-filter kernels.  There is no CPU
fallback: if the library is missing or no MI355X is visible the calls raise."""
import collections
import ctypes as C
import gc
import os
import time

import numpy as np

from . import _build

# ---- enums (include/pfgrad.h) ---------------------------------------------------------
MODEL = {"svm": 0, "garch": 1, "lgssm": 2}
KERNEL = {"prior": 0, "optimal": 1}
SMOOTHER = {"nemeth": 0, "filter": 1, "paris": 2, "nemeth_systematic": 3, "poyiadjis_n2": 4,
            "poyiadjis_n": 5,       # launch-level id only (never in a descriptor): see include/pfgrad.h
            "kalman": 6,            # the exact LGSSM score (kind='marginal'), no particles: see include/pfgrad.h
            "kalman_ffbs": 7,       # FFBS latent paths of LGSSM and their complete-data score (kind='complete')
            "nemeth_stratified": 8}  # NEMETH with stratified resampling (resampling='stratified'), N <= 16384
STAT = {"score": 0, "suff": 1, "none": 2, "predictive": 3,
        "gibbs": 4}         # FFBS, one path: the Gibbs sufficient statistics of the buffer (include/pfgrad.h)
DTYPE = {"f64": 0, "f32": 1}
RNG = {"replay": 0, "device": 1, "philox": 1}     # "philox" = alias of "device" (Philox-keyed lanes)
FLAG_GARCH_STATIONARY_PRIOR = 1
FLAG_PARIS_NO_ACCEPT_REJECT = 2
FLAG_PARIS_RAW_STREAM = 4        # paris_stream = the window's whole np.random stream of doubles (pfgrad.h)
FLAG_PARIS_RAW_CARRY = 8         # ... whose first entry is the generator's pending cached Gaussian
FLAG_ADAPTIVE_RESAMPLING = 16    # resample only when ESS < ess_threshold * N (extension; include/pfgrad.h)
MAX_STAT, MAX_THETA, OUT_DOUBLES, MAX_PRED, STAMP_WORDS = 4, 4, 8, 16, 16
MAX_DRAWN_SEQUENCES = 1024       # PFG_MAX_DRAWN_SEQUENCES: sequences a chain draws per step (num_sequences != -1)
STATE_DIM = {"svm": 1, "garch": 2, "lgssm": 1}
STAT_DIM = {"svm": 3, "garch": 4, "lgssm": 4}
THETA_DIM = {"svm": 3, "garch": 4, "lgssm": 4}


def ess_threshold_bits(tau):
    """The `reserved` word of a PFG_FLAG_ADAPTIVE_RESAMPLING descriptor: the bits of tau as an IEEE binary32 (0: off)."""
    return int(np.array(tau or 0.0, dtype=np.float32).view(np.int32))


def ess_threshold_from_bits(bits):
    return float(np.array(bits, dtype=np.int32).view(np.float32))


def kalman_scratch_bytes(L):
    """pfg_dev_problem.scratch a PFG_SMOOTHER_KALMAN window of L = tL - t1 steps needs (include/pfgrad.h)."""
    return (16 * (int(L) + 1) + 255) // 256 * 256


PFG_OK, PFG_ERR_INVALID, PFG_ERR_UNSUPPORTED, PFG_ERR_DEVICE, PFG_ERR_NOMEM, PFG_ERR_NUMERIC = 0, -1, -2, -3, -4, -5

_dp = C.POINTER(C.c_double)
_SCALAR = {"i4": C.c_int32, "u4": C.c_uint32, "i8": C.c_int64, "u8": C.c_uint64, "f8": C.c_double}


def _mirrors(name, fields):
    """The two forms of one host struct of include/pfgrad.h, from its fields stated as the header declares them --
    (scalar kind, names[, array length]), '*kind' a pointer to that scalar: the ctypes structure, and the aligned numpy
    dtype (a pointer is a 'u8' address there) of the vectorised marshalling of large batches (Context._run_batch_plain)."""
    c_fields, np_fields = [], []
    for kind, names, *length in fields:
        for n in names.split():
            if kind[0] == "*":
                c_fields.append((n, C.POINTER(_SCALAR[kind[1:]])))
                np_fields.append((n, "u8"))
            elif length:
                c_fields.append((n, _SCALAR[kind] * length[0]))
                np_fields.append((n, kind, (length[0],)))
            else:
                c_fields.append((n, _SCALAR[kind]))
                np_fields.append((n, kind))
    return type(name, (C.Structure,), {"_fields_": c_fields}), np.dtype(np_fields, align=True)


Problem, PROBLEM_DTYPE = _mirrors("Problem", (             # pfg_problem
    ("i4", "model kernel smoother stat dtype rng N T t1 tL"), ("u4", "flags"), ("i4", "reserved"),
    ("f8", "lambduh prior_mean prior_var"),
    ("*f8", "y weights theta z0 u z"),
    ("u8", "seed stream"),
    ("*f8", "init_x init_logw init_stats"),
    ("i4", "Ntilde max_accept_reject"),
    ("*f8", "paris_idx_u paris_acc_u paris_man_u"),
    ("i4", "num_steps_ahead elementwise"),
    ("*f8", "pred_z paris_stream"), ("i8", "paris_stream_len"),
    ("i4", "paris_manual_threshold reserved2"),
    ("u8", "step")))
Result, RESULT_DTYPE = _mirrors("Result", (                # pfg_result
    ("f8", "mean_stat", MAX_STAT), ("f8", "loglik"),
    ("*f8", "x_T logw_T stats_T trace_x trace_logw trace_stats trace_ll"),
    ("i4", "status paris_carry_back"),
    ("*i4", "trace_anc"),
    ("f8", "pred", MAX_PRED),
    ("*u4", "rec_u"), ("*f8", "rec_z rec_z0 rec_ud ew_mean ew_stats"),
    ("i8", "paris_consumed"),
    ("*i4", "trace_paris_J")))
assert PROBLEM_DTYPE.itemsize == C.sizeof(Problem) and RESULT_DTYPE.itemsize == C.sizeof(Result)
assert all(PROBLEM_DTYPE.fields[n][1] == getattr(Problem, n).offset for n, _ in Problem._fields_)
assert all(RESULT_DTYPE.fields[n][1] == getattr(Result, n).offset for n, _ in Result._fields_)


class PriorHyper(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "df_Qinv", "scale_Qinv", "df_Rinv", "scale_Rinv",
        "mean_A", "var_col_A", "mean_C", "var_col_C",
        "scale_mu", "shape_mu", "alpha_phi", "beta_phi", "alpha_lambduh", "beta_lambduh")]


# numpy mirror of pfg_dev_problem (device descriptors are built on the host as a structured
# array and uploaded; all pointer fields are device addresses)
DEV_PROBLEM_DTYPE = np.dtype([
    ("y", "u8"), ("weights", "u8"), ("theta", "u8"),
    ("z0", "u8"), ("u", "u8"), ("z", "u8"),
    ("init_x", "u8"), ("init_logw", "u8"), ("init_stats", "u8"),
    ("out", "u8"),
    ("final_x", "u8"), ("final_logw", "u8"), ("final_stats", "u8"),
    ("trace_x", "u8"), ("trace_logw", "u8"), ("trace_stats", "u8"), ("trace_ll", "u8"),
    ("step_ctr", "u8"), ("scratch", "u8"),
    ("prior_mean", "f8"), ("prior_var", "f8"), ("lambduh", "f8"),
    ("seed", "u8"), ("stream", "u8"),
    ("T", "i4"), ("t1", "i4"), ("tL", "i4"), ("N", "i4"),
    ("smoother", "i4"), ("stat", "i4"), ("flags", "u4"), ("reserved", "i4"),
    ("paris_idx_u", "u8"), ("paris_acc_u", "u8"), ("paris_man_u", "u8"),
    ("Ntilde", "i4"), ("max_accept_reject", "i4"),
    ("trace_anc", "u8"),
    ("pred_z", "u8"), ("pred_out", "u8"), ("pred_scratch", "u8"),
    ("num_steps_ahead", "i4"), ("reserved3", "i4"),
    ("rec_u", "u8"), ("rec_z", "u8"), ("rec_z0", "u8"),
    ("rec_ud", "u8"), ("trace_paris_J", "u8"),
    ("paris_stream", "u8"), ("paris_stream_len", "i8"), ("paris_consumed", "u8"),
    ("paris_manual_threshold", "i4"), ("reserved4", "i4"),
    ("stamps", "u8"),
], align=True)


# numpy mirror of pfg_csmc_problem (one conditional SMC sweep; every pointer a device address)
CSMC_PROBLEM_DTYPE = np.dtype([
    ("theta", "u8"), ("y", "u8"), ("path", "u8"), ("scratch", "u8"), ("out", "u8"), ("n_degenerate", "u8"),
    ("trace_anc", "u8"), ("trace_ref_anc", "u8"), ("trace_w", "u8"), ("trace_k", "u8"),
    ("prior_mean", "f8"), ("prior_var", "f8"),
    ("T", "i4"), ("N", "i4"), ("has_ref", "i4"), ("reserved", "i4"),
], align=True)
CSMC_MAX_N = 1024

# numpy mirror of pfg_cpm_problem (one correlated pseudo-marginal filter; every pointer a device address)
CPM_PROBLEM_DTYPE = np.dtype([
    ("theta", "u8"), ("y", "u8"), ("u0", "u8"), ("u1", "u8"), ("which", "u8"), ("out", "u8"),
    ("trace_anc", "u8"), ("trace_ll", "u8"),
    ("prior_mean", "f8"), ("prior_var", "f8"),
    ("T", "i4"), ("N", "i4"),
], align=True)
CPM_MAX_N = 1024

# numpy mirror of pfg_sqmc_problem (one sequential quasi-Monte Carlo filter; every pointer a device address)
SQMC_PROBLEM_DTYPE = np.dtype([
    ("theta", "u8"), ("y", "u8"), ("out", "u8"), ("trace_anc", "u8"), ("trace_ll", "u8"), ("trace_z", "u8"),
    ("prior_mean", "f8"), ("prior_var", "f8"),
    ("T", "i4"), ("N", "i4"),
], align=True)
SQMC_MAX_N = 1024                                   # and a power of two
SMC_MIN_CHAINS, SMC_MAX_CHAINS = 2, 1 << 20        # a tempered population (pfg_smc_temper_device: one workgroup)
SMC_RESULT_DOUBLES = 8                              # PFG_SMC_RESULT_DOUBLES
SEQ_RECORD_DOUBLES = 8                              # PFG_SEQ_RECORD_DOUBLES
# the theta slots a PMMH proposal moves (pfg_chains.hip: moves), as pfg_smc_scale_device's bit mask
PMMH_MOVING_SLOTS = {"svm": 0b0111, "lgssm": 0b1101, "garch": 0b1111}


def csmc_scratch_bytes(T, N):
    """pfg_csmc_scratch_bytes: the states [T][N] f64 and the parents [T][N] uint16 of one chain, rounded up to 256 bytes
    (-1: T < 1, N < 2 or N > 1024).  The library's own answer: the formula is stated once, in pfg_csmc.hip."""
    return int(load_library().pfg_csmc_scratch_bytes(int(T), int(N)))


def cpm_aux_bytes(T, N):
    """pfg_cpm_aux_bytes: one buffer U [T+1][N+1] f64 of one chain, rounded up to 256 bytes (-1: T < 1, N < 2 or N > 1024).
    The library's own answer: the formula is stated once, in pfg_cpm.hip."""
    return int(load_library().pfg_cpm_aux_bytes(int(T), int(N)))


def smc_scratch_bytes(B):
    """pfg_smc_scratch_bytes: the CDF [B] f64 of one tempering stage, rounded up to 256 bytes (-1: B < 2 or B > 2^20)."""
    return int(load_library().pfg_smc_scratch_bytes(int(B)))


def device_descriptors(n, *, theta, row, out, step_ctr, scratch, scratch_bytes, stream, prior_mean, prior_var, lambduh, seed,
                       N, smoother, stat="score", flags=0, Ntilde=0, max_accept_reject=0, ess_threshold=None):
    """The static fields of n pfg_dev_problem records (the windows -- y, T, t1, tL, weights -- are the caller's):
    descriptor i reads row `row[i]` of the tensor theta [*, MAX_THETA], writes record i of out [n, OUT_DOUBLES], owns bytes
    [i * scratch_bytes, (i + 1) * scratch_bytes) of `scratch` (None: no scratch) and draws from the stream id `stream[i]`."""
    d = np.zeros(n, dtype=DEV_PROBLEM_DTYPE)
    idx = np.arange(n, dtype=np.uint64)
    d["theta"] = theta.data_ptr() + np.asarray(row, dtype=np.uint64) * np.uint64(8 * MAX_THETA)
    d["out"] = out.data_ptr() + idx * np.uint64(8 * OUT_DOUBLES)
    if scratch is not None:
        d["scratch"] = scratch.data_ptr() + idx * np.uint64(scratch_bytes)
    d["step_ctr"] = step_ctr.data_ptr()
    d["prior_mean"], d["prior_var"], d["lambduh"] = prior_mean, prior_var, lambduh
    d["seed"] = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    d["stream"] = stream
    d["N"], d["smoother"], d["stat"], d["flags"] = N, SMOOTHER[smoother], STAT[stat], int(flags)
    d["Ntilde"], d["max_accept_reject"] = Ntilde, max_accept_reject
    if ess_threshold:       # adaptive resampling (pfg_launch_device_adaptive): the flag and tau travel in every descriptor
        d["flags"] |= FLAG_ADAPTIVE_RESAMPLING
        d["reserved"] = ess_threshold_bits(ess_threshold)
    return d


# ---- entry points (include/pfgrad.h) -----------------------------------------------------
# A kind is how one sort of C argument or return value crosses the boundary: its ctypes type, which checks and converts
# the Python value (an int is anything with __index__ and wraps to the type's width, a double anything with __float__,
# None or 0 is a NULL pointer, a structure meets a pointer to it by reference), and for what ctypes cannot take as it is,
# the conversion Context._call applies first.  Those are few and C-level: a step of a small ensemble is bound by these calls.
_Kind = collections.namedtuple("_Kind", "ctype convert")


class _Ids(dict):
    """The ids of one enum by name; an id stands for itself (a bad one is the library's to refuse)."""

    def __missing__(self, key):
        if isinstance(key, int):
            return key
        raise KeyError(key)


_ctx = _Kind(C.c_void_p, None)                      # the handle: Context._call passes its own
_ctx_out = _Kind(C.POINTER(C.c_void_p), None)
_model, _kernel, _dtype, _rng, _smoother = (_Kind(C.c_int, _Ids(ids).__getitem__)
                                            for ids in (MODEL, KERNEL, DTYPE, RNG, SMOOTHER))
_int = _Kind(C.c_int, None)
_flag = _Kind(C.c_int, bool)                        # any truth value
_f64 = _Kind(C.c_double, None)
_u64 = _Kind(C.c_uint64, None)                      # seeds, chain ids and counters: masked to 64 bits
_u32 = _Kind(C.c_uint32, None)
_size = _Kind(C.c_size_t, None)
_i64 = _Kind(C.c_int64, None)
_addr = _Kind(C.c_void_p, None)                     # a device or host address as an int; None or 0 is NULL
_stream = _Kind(C.c_void_p, None)                   # a hipStream_t as an int; 0 is HIP's default stream
_hyper = _Kind(C.POINTER(PriorHyper), None)         # a PriorHyper; None is NULL
_problem_p, _result_p = _Kind(C.POINTER(Problem), None), _Kind(C.POINTER(Result), None)
_f64_p, _i32_p = _Kind(_dp, None), _Kind(C.POINTER(C.c_int32), None)
_status = _Kind(C.c_int, None)                      # 0 or a negative PFG_ERR_*: Context._call hands it to _check
_cstr = _Kind(C.c_char_p, None)
_void = _Kind(None, None)

# every exported function, in the header's order: name -> (return kind, argument kinds)
_ENTRY_POINTS = {
    "pfg_version": (_int, ()),
    "pfg_struct_size": (_int, (_int,)),
    "pfg_create": (_status, (_ctx_out, _int)),
    "pfg_destroy": (_void, (_ctx,)),
    "pfg_last_error": (_cstr, (_ctx,)),
    "pfg_run": (_status, (_ctx, _problem_p, _result_p)),
    "pfg_run_batch": (_status, (_ctx, _int, _problem_p, _result_p)),
    "pfg_ctx_stream": (_addr, (_ctx,)),
    "pfg_launch_device": (_status, (_ctx, _model, _kernel, _dtype, _rng, _int, _int, _addr, _stream)),
    "pfg_launch_device_traced": (_status, (_ctx, _model, _kernel, _dtype, _rng, _smoother, _int, _int, _addr, _stream)),
    "pfg_last_traced": (_int, (_ctx,)),
    "pfg_launch_device_smoother": (_status, (_ctx, _model, _kernel, _dtype, _rng, _smoother, _int, _int, _addr, _stream)),
    "pfg_launch_device_adaptive": (_status, (_ctx, _model, _kernel, _dtype, _rng, _int, _int, _addr, _stream, _flag)),
    "pfg_launch_device_grid": (_status, (_ctx, _model, _kernel, _dtype, _rng, _int, _int, _int, _addr, _stream)),
    "pfg_launch_device_grid_phase": (_status, (_ctx, _model, _kernel, _dtype, _rng, _int, _int, _int, _addr, _stream)),
    "pfg_launch_device_grid_smoother": (_status, (_ctx, _model, _kernel, _dtype, _rng, _smoother, _int, _int, _int, _int,
                                                  _addr, _stream)),
    "pfg_sample_windows_device": (_status, (_ctx, _int, _addr, _addr, _addr, _int, _int, _int, _flag, _u64, _u64, _addr,
                                            _stream)),
    "pfg_sample_windows_multi_device": (_status, (_ctx, _int, _int, _addr, _addr, _int, _int, _addr, _addr, _addr, _addr,
                                                  _int, _int, _flag, _u64, _u64, _addr, _stream)),
    "pfg_reduce_windows_device": (_status, (_ctx, _int, _int, _int, _addr, _addr, _flag, _f64, _addr, _stream)),
    "pfg_scratch_bytes": (_i64, (_model, _dtype, _rng, _int)),
    "pfg_scratch_bytes_smoother": (_i64, (_model, _dtype, _rng, _smoother, _int)),
    "pfg_variant_name": (_cstr, (_model, _kernel, _dtype, _rng, _int)),
    "pfg_last_variant": (_cstr, (_ctx,)),
    "pfg_synchronize": (_status, (_ctx,)),
    "pfg_sgld_update_device": (_status, (_ctx, _model, _int, _addr, _addr, _hyper, _f64, _f64, _u64, _u64, _addr, _stream)),
    "pfg_sghmc_update_device": (_status, (_ctx, _model, _int, _addr, _addr, _addr, _hyper, _f64, _f64, _f64, _u64, _u64,
                                          _addr, _stream)),
    "pfg_sgrld_update_device": (_status, (_ctx, _model, _int, _addr, _addr, _hyper, _f64, _f64, _u64, _u64, _addr, _stream)),
    "pfg_sgd_update_device": (_status, (_ctx, _model, _int, _addr, _addr, _hyper, _f64, _f64, _addr, _stream)),
    "pfg_adagrad_update_device": (_status, (_ctx, _model, _int, _addr, _addr, _addr, _hyper, _f64, _f64, _addr, _stream)),
    "pfg_sgld_cv_update_device": (_status, (_ctx, _model, _int, _addr, _addr, _addr, _addr, _hyper, _f64, _f64, _u64, _u64,
                                            _addr, _stream)),
    "pfg_cv_accumulate_device": (_status, (_ctx, _int, _addr, _addr, _int, _int, _addr, _stream)),
    "pfg_gibbs_update_device": (_status, (_ctx, _model, _int, _addr, _addr, _hyper, _u64, _u64, _addr, _stream)),
    "pfg_logprior_device": (_status, (_ctx, _model, _int, _addr, _hyper, _addr, _stream)),
    "pfg_pmmh_propose_device": (_status, (_ctx, _model, _int, _addr, _addr, _addr, _addr, _u64, _u64, _addr, _stream)),
    "pfg_pmmh_accept_device": (_status, (_ctx, _model, _int, _addr, _addr, _addr, _addr, _addr, _addr, _hyper, _flag,
                                         _u64, _u64, _addr, _stream)),
    "pfg_pmala_propose_device": (_status, (_ctx, _model, _int, _addr, _addr, _addr, _addr, _addr, _hyper, _u64, _u64,
                                           _addr, _stream)),
    "pfg_pmala_accept_device": (_status, (_ctx, _model, _int, _addr, _addr, _addr, _addr, _addr, _addr, _addr, _hyper,
                                          _addr, _flag, _u64, _u64, _addr, _stream)),
    "pfg_csmc_scratch_bytes": (_i64, (_int, _int)),
    "pfg_csmc_device": (_status, (_ctx, _model, _dtype, _int, _int, _addr, _u64, _u64, _addr, _stream, _flag)),
    "pfg_pgibbs_update_device": (_status, (_ctx, _model, _int, _addr, _addr, _hyper, _u64, _u64, _addr, _stream)),
    "pfg_cpm_aux_bytes": (_i64, (_int, _int)),
    "pfg_cpm_device": (_status, (_ctx, _model, _dtype, _int, _int, _addr, _f64, _u64, _u64, _addr, _stream, _flag)),
    "pfg_cpm_commit_device": (_status, (_ctx, _int, _addr, _addr, _addr, _flag, _stream)),
    "pfg_sqmc_device": (_status, (_ctx, _model, _dtype, _int, _int, _addr, _u64, _u64, _addr, _stream, _flag)),
    "pfg_cpm_score_device": (_status, (_ctx, _model, _dtype, _int, _int, _addr, _f64, _f64, _u64, _u64, _addr, _stream, _flag)),
    "pfg_sqmc_score_device": (_status, (_ctx, _model, _dtype, _int, _int, _addr, _f64, _u64, _u64, _addr, _stream, _flag)),
    "pfg_smc_scratch_bytes": (_i64, (_int,)),
    "pfg_smc_logtarget_device": (_status, (_ctx, _model, _int, _addr, _addr, _hyper, _addr, _addr, _addr, _stream)),
    "pfg_smc_temper_device": (_status, (_ctx, _int, _addr, _addr, _f64, _u64, _u64, _addr, _addr, _addr, _addr, _stream)),
    "pfg_smc_gather_device": (_status, (_ctx, _int, _addr, _addr, _addr, _addr, _addr, _stream)),
    "pfg_smc_scale_device": (_status, (_ctx, _int, _addr, _u32, _f64, _addr, _stream)),
    "pfg_smc_accept_device": (_status, (_ctx, _model, _int, _addr, _addr, _addr, _addr, _addr, _addr, _hyper, _addr, _addr,
                                        _addr, _addr, _u64, _u64, _addr, _stream)),
    "pfg_seq_reweight_device": (_status, (_ctx, _int, _addr, _addr, _i64, _f64, _u64, _u64, _addr, _addr, _addr, _addr, _stream)),
    "pfg_seq_gather_device": (_status, (_ctx, _int, _addr, _i64, _addr, _addr, _addr, _addr, _addr, _addr, _stream)),
    "pfg_seq_adopt_device": (_status, (_ctx, _int, _addr, _addr, _i64, _addr, _addr, _stream)),
    "pfg_imq_ksd": (_status, (_ctx, _int, _int, _f64_p, _f64_p, _f64, _f64, _f64_p)),
    "pfg_legacy_streams": (_status, (_addr, _i32_p, _i32_p, _f64_p, _int, _int, _addr, _addr, _addr, _int)),
    "pfg_host_register": (_status, (_addr, _size)),
    "pfg_host_unregister": (_status, (_addr,)),
}
EXPORTS = tuple(_ENTRY_POINTS)

_lib = None
_calls = {}     # name -> (function, ((position after the handle, conversion), ...), takes the handle, returns a status)


class PfgError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libpfgrad error {0}: {1}".format(code, message))
        self.code = code
        self.message = message


def library_path():
    """In-tree csrc/libpfgrad.so; PFGRAD_LIB=<path> substitutes another build (A/B timing)."""
    return os.environ.get("PFGRAD_LIB") or _build.LIB_PATH


def load_library():
    """dlopen the in-tree libpfgrad.so (never builds implicitly on a GPU box: build() does)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            "libpfgrad.so is not built ({0}). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `python -m sgmcmc_ssm_amd._build`; there is no CPU fallback.".format(path))
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64 (ROCm 7.0 here)
    # while libpfgrad.so was linked against the system one (ROCm 7.2, same SONAME).  Whichever
    # is loaded first serves both; loading the system runtime first breaks torch.cuda.  So when
    # torch is installed, let it load its runtime before we dlopen (torch is only plumbing:
    # device memory, streams, torch.distributed -- no torch type crosses the C ABI).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (ret, kinds) in _ENTRY_POINTS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ret.ctype, [k.ctype for k in kinds]
        takes_handle = bool(kinds) and kinds[0] is _ctx         # (`is`: an address is the same pair of type and conversion)
        converts = tuple((i, k.convert) for i, k in enumerate(kinds[takes_handle:]) if k.convert)
        _calls[name] = (fn, converts, takes_handle, ret is _status)
    sizes = (C.sizeof(Problem), C.sizeof(Result), DEV_PROBLEM_DTYPE.itemsize, C.sizeof(PriorHyper), CSMC_PROBLEM_DTYPE.itemsize,
             CPM_PROBLEM_DTYPE.itemsize, SQMC_PROBLEM_DTYPE.itemsize)
    for which, mine in enumerate(sizes):
        if lib.pfg_struct_size(which) != mine:
            raise RuntimeError("ABI mismatch: struct {0} is {1} bytes in libpfgrad.so, {2} in the binding"
                               .format(which, lib.pfg_struct_size(which), mine))
    _lib = lib
    return lib


def legacy_streams(random_state, N, T, z0, u, z, threads=0):
    """Fill z0 (N,), u (T,N), z (T,N) with what `random_state` (np.random or a RandomState) would return
    for  z0 = normal(size=N); for t: u[t] = random_sample(N); z[t] = normal(size=N)  -- natively, bit for
    bit -- and advance its state accordingly."""
    lib = load_library()
    rs = random_state            # np.random (module: get_state / set_state act on the global generator) or a RandomState
    name, key, pos, has_gauss, gauss = rs.get_state()
    if name != "MT19937":
        raise ValueError("legacy streams need an MT19937 RandomState")
    key = np.ascontiguousarray(key, dtype=np.uint32).copy()
    pos_c, hg_c, g_c = C.c_int32(int(pos)), C.c_int32(int(has_gauss)), C.c_double(float(gauss))
    for a in (z0, u, z):
        if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
            raise ValueError("stream buffers must be C-contiguous float64")
    rc = lib.pfg_legacy_streams(key.ctypes.data_as(C.c_void_p), C.byref(pos_c), C.byref(hg_c), C.byref(g_c), int(N), int(T),
                                z0.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p),
                                int(threads))
    if rc != 0:
        raise PfgError(rc, "pfg_legacy_streams failed")
    rs.set_state((name, key, pos_c.value, hg_c.value, g_c.value))


def host_register(a):
    """Page-lock the ndarray `a` (pfg_host_register): pfg_run_batch then stages it by DMA from where it lies.
    The caller keeps `a` alive until host_unregister(a).  Returns False when the runtime refuses (no GPU, limits)."""
    return load_library().pfg_host_register(a.ctypes.data_as(C.c_void_p), a.nbytes) == 0


def host_unregister(a):
    return load_library().pfg_host_unregister(a.ctypes.data_as(C.c_void_p)) == 0


_OPTIONAL_ARRAYS = ("weights", "z0", "u", "z", "init_x", "init_logw", "init_stats",
                    "paris_idx_u", "paris_acc_u", "paris_man_u", "pred_z", "paris_stream")
_NO_ARRAYS = dict.fromkeys(("y", "theta") + _OPTIONAL_ARRAYS)


def _as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


class Context:
    """One pfg_ctx (one per process / GPU). Not thread-safe."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.pfg_create(C.byref(h), int(device_id))
        if rc != 0:
            msg = self.lib.pfg_last_error(None).decode()
            raise PfgError(rc, msg + " (the HIP particle-filter path needs an MI355X; there is no CPU fallback)")
        self.handle = h
        self.device_id = device_id

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pfg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.pfg_last_error(self.handle).decode()
            if rc == PFG_ERR_NUMERIC:
                raise ValueError(msg)
            if rc == PFG_ERR_UNSUPPORTED:
                raise NotImplementedError(msg)
            if rc == PFG_ERR_INVALID:
                raise ValueError(msg)
            raise PfgError(rc, msg)

    def _call(self, name, *args):
        """The entry point `name` on Python values, converted by the kinds of its row in _ENTRY_POINTS (the handle is
        passed for a row that starts with one); a status goes through _check, any other result is returned."""
        fn, converts, takes_handle, is_status = _calls[name]
        if converts:
            args = list(args)
            for i, convert in converts:
                args[i] = convert(args[i])
        rc = fn(self.handle, *args) if takes_handle else fn(*args)
        if is_status:
            self._check(rc)
        return rc

    # ---- host-buffer path ----------------------------------------------------------------
    def run_batch(self, problems, want_final=False, want_trace=False, want_draws=False, want_elementwise=False):
        """problems: list of dicts with keys
             model, kernel, smoother, stat, dtype, rng (strings), N, T (implied by y), t1, tL,
             lambduh, prior_mean, prior_var, flags, y, weights, theta, z0,u,z | seed,stream,
             init_x, init_logw, init_stats
           returns list of dicts(mean_stat, loglik[, x_t, log_weights, statistics, all_*]).  stat='gibbs' (FFBS
           windows, N = 1): mean_stat = the 8-double record of the Gibbs statistics, loglik = nan."""
        B = len(problems)
        if B == 0:
            return []
        if B >= 64 and not (want_final or want_trace or want_draws or want_elementwise):
            outs = self._run_batch_plain(problems)
            if outs is not None:
                return outs
        ps = (Problem * B)()
        rs = (Result * B)()
        gc_was_on = gc.isenabled() and B >= 256
        if gc_was_on:
            gc.disable()        # thousands of small containers below: generation-2 sweeps made this loop superlinear in B
        try:
            keep, outs = self._marshal(problems, ps, rs, want_final, want_trace, want_draws, want_elementwise)
        finally:
            if gc_was_on:
                gc.enable()     # also when a problem is refused (ValueError): the collector must not stay off
        t_call = time.perf_counter()
        rc = self.lib.pfg_run_batch(self.handle, B, ps, rs)
        self.last_call_seconds = time.perf_counter() - t_call      # the C call alone (pack, H2D, launch, D2H), without this marshalling
        self._check(rc)
        for b, o in enumerate(outs):
            if problems[b].get("stat", "score") == "gibbs":
                # the Gibbs statistics of an FFBS path: the whole record, returned in pfg_result.pred; no log-likelihood
                o["mean_stat"] = np.array(rs[b].pred[:OUT_DOUBLES])
                o["loglik"] = float("nan")
                continue
            # the device record is STAT_DIM[model] wide; sufficient statistics use 3 columns
            h = 3 if problems[b].get("stat", "score") != "score" else STAT_DIM[problems[b]["model"]]
            o["mean_stat"] = np.array(rs[b].mean_stat[:h])
            o["loglik"] = float(rs[b].loglik)
            if problems[b].get("stat", "score") == "predictive":
                o["predictive"] = np.array(rs[b].pred[:int(problems[b].get("num_steps_ahead", 0)) + 1])
            if problems[b].get("paris_stream", None) is not None:
                o["paris_consumed"] = int(rs[b].paris_consumed)
                o["paris_carry_back"] = int(rs[b].paris_carry_back)
            for name in ("statistics", "all_statistics"):
                if name in o:
                    o[name] = o[name][..., :h]
        del keep
        return outs

    def _marshal(self, problems, ps, rs, want_final, want_trace, want_draws, want_elementwise):
        """Fill the ctypes problem / result arrays from the problem dicts; returns (arrays kept alive, output dicts)."""
        keep = []           # keep numpy buffers alive for the duration of the call
        outs = []
        for b, q in enumerate(problems):
            model = q["model"]
            ns, h = STATE_DIM[model], STAT_DIM[model]
            y = _as_f64(q["y"]).reshape(-1)
            T, N = y.shape[0], int(q["N"])
            p = ps[b]
            p.model, p.kernel = MODEL[model], KERNEL[q["kernel"]]
            p.smoother, p.stat = SMOOTHER[q.get("smoother", "nemeth")], STAT[q.get("stat", "score")]
            p.dtype, p.rng = DTYPE[q.get("dtype", "f64")], RNG[q.get("rng", "replay")]
            p.N, p.T = N, T
            p.t1 = int(q.get("t1", 0))
            tL = q.get("tL", None)
            p.tL = T if tL is None else int(tL)
            p.flags = int(q.get("flags", 0))
            p.reserved = ess_threshold_bits(q.get("ess_threshold", None))
            p.lambduh = float(q.get("lambduh", 1.0))
            p.prior_mean = float(q.get("prior_mean", 0.0))
            p.prior_var = float(q.get("prior_var", 1.0))
            theta = _as_f64(q["theta"]).reshape(-1)
            arrs = _NO_ARRAYS.copy()
            arrs["y"], arrs["theta"] = y, theta
            p.y, p.theta = _ptr(y), _ptr(theta)
            p.Ntilde = int(q.get("Ntilde", 2))
            p.max_accept_reject = int(q.get("max_accept_reject", 0))
            p.num_steps_ahead = int(q.get("num_steps_ahead", 0))
            for name in _OPTIONAL_ARRAYS:               # absent arrays stay NULL in the zero-initialised struct
                v = q.get(name, None)
                if v is not None:
                    a = arrs[name] = _as_f64(v).reshape(-1)
                    setattr(p, name, _ptr(a))
            if arrs["weights"] is not None and arrs["weights"].shape[0] < p.tL - p.t1:
                raise ValueError("weights shorter than tL - t1")
            ffbs = p.smoother == SMOOTHER["kalman_ffbs"]
            if ffbs and p.rng == RNG["replay"]:
                if arrs["z"] is None or arrs["z"].shape[0] != T * N:
                    raise ValueError("FFBS replay normals z must have T*N entries")
            elif p.rng == RNG["replay"] and not (p.flags & FLAG_PARIS_RAW_STREAM):
                if arrs["u"] is None or arrs["z"] is None or arrs["u"].shape[0] != T * N or arrs["z"].shape[0] != T * N:
                    raise ValueError("replay streams u, z must have T*N entries")
                if arrs["init_x"] is None and (arrs["z0"] is None or arrs["z0"].shape[0] != N):
                    raise ValueError("replay stream z0 must have N entries")
            p.seed = int(q.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
            p.stream = int(q.get("stream", 0)) & 0xFFFFFFFFFFFFFFFF
            p.step = int(q.get("step", 0)) & 0xFFFFFFFFFFFFFFFF
            keep.append(arrs)
            o = {}
            r = rs[b]
            if arrs["paris_stream"] is not None:
                p.paris_stream_len = arrs["paris_stream"].shape[0]
                p.paris_manual_threshold = int(q.get("paris_manual_threshold", 0))
            elif p.smoother == SMOOTHER["paris"] and p.rng == RNG["replay"]:
                pool = T * p.Ntilde * p.max_accept_reject * N
                for name, need in (("paris_idx_u", pool), ("paris_acc_u", pool), ("paris_man_u", T * p.Ntilde * N)):
                    if need and (arrs[name] is None or arrs[name].shape[0] != need):
                        raise ValueError("{0} must have {1} entries".format(name, need))
            if p.stat == STAT["predictive"] and p.rng == RNG["replay"] and model != "lgssm":
                need = T * (p.num_steps_ahead + 1) * N
                if need and (arrs["pred_z"] is None or arrs["pred_z"].shape[0] != need):
                    raise ValueError("pred_z must have T*(num_steps_ahead+1)*N = {0} entries".format(need))
            is_filter = p.smoother == SMOOTHER["filter"]
            if ffbs:
                # FFBS: no particles; want_trace asks for the sampled paths, [T][N] with t ascending
                if want_final or want_draws or want_elementwise:
                    raise ValueError("FFBS latent paths have no particles: only want_trace (the paths)")
                if want_trace:
                    o["paths"] = np.zeros((T, N))
                    r.trace_x = _ptr(o["paths"])
                outs.append(o)
                continue
            if want_final or want_trace:
                o["x_t"] = np.zeros((N, ns))
                o["log_weights"] = np.zeros(N)
                r.x_T, r.logw_T = _ptr(o["x_t"]), _ptr(o["log_weights"])
                if not is_filter:
                    o["statistics"] = np.zeros((N, h))
                    r.stats_T = _ptr(o["statistics"])
            if want_elementwise:
                # elementwise sufficient statistics of the window (pf_latent_var_distr): device pass
                L = min(p.tL, T) - p.t1
                p.elementwise = 1
                o["ew_mean"] = np.zeros(3 * max(L, 0))
                r.ew_mean = _ptr(o["ew_mean"])
                if want_final:
                    o["ew_stats"] = np.zeros((N, 3 * max(L, 0)))
                    r.ew_stats = _ptr(o["ew_stats"])
            if want_trace:
                o["all_x_t"] = np.zeros((T + 1, N, ns))
                o["all_log_weights"] = np.zeros((T + 1, N))
                o["all_loglikelihood_estimate"] = np.zeros(T + 1)
                o["all_ancestors"] = np.zeros((T, N), dtype=np.int32)
                r.trace_anc = o["all_ancestors"].ctypes.data_as(C.POINTER(C.c_int32))
                if p.smoother == SMOOTHER["paris"]:
                    # test instrumentation: the backward-sampled parent of every child and draw (both generators)
                    o["all_paris_J"] = np.zeros((T, p.Ntilde, N), dtype=np.int32)
                    r.trace_paris_J = o["all_paris_J"].ctypes.data_as(C.POINTER(C.c_int32))
                r.trace_x, r.trace_logw = _ptr(o["all_x_t"]), _ptr(o["all_log_weights"])
                r.trace_ll = _ptr(o["all_loglikelihood_estimate"])
                if not is_filter:
                    o["all_statistics"] = np.zeros((T + 1, N, h))
                    r.trace_stats = _ptr(o["all_statistics"])
                if want_draws:
                    # test instrumentation: the DEVICE generator's draws of this very launch
                    o["rec_u"] = np.zeros((T, N), dtype=np.uint32)
                    o["rec_z"] = np.zeros((T, N))
                    o["rec_z0"] = np.zeros(N)
                    r.rec_u = o["rec_u"].ctypes.data_as(C.POINTER(C.c_uint32))
                    r.rec_z, r.rec_z0 = _ptr(o["rec_z"]), _ptr(o["rec_z0"])
                    o["rec_ud"] = np.zeros((T, N))
                    r.rec_ud = _ptr(o["rec_ud"])
            outs.append(o)
        return keep, outs

    def _run_batch_plain(self, problems):
        """Large batches that only ask for (mean_stat, loglik) from the device generator: the descriptors are
        filled column by column into a structured array (a ctypes attribute store per field and problem cost
        19 us per problem, four times the kernel's share of a 12288-window launch).  None = not eligible."""
        B = len(problems)
        blocked = ("z0", "u", "z", "init_x", "init_logw", "init_stats", "paris_idx_u", "paris_acc_u", "paris_man_u", "pred_z", "paris_stream")
        for q in problems:
            if RNG[q.get("rng", "replay")] != RNG["device"] or q.get("stat", "score") in ("predictive", "gibbs"):
                return None
            for name in blocked:
                if q.get(name, None) is not None:
                    return None
        conv = {}                                   # id(array) -> (converted array, address, length): shared inputs convert once

        def prep(a):
            k = id(a)
            got = conv.get(k)
            if got is None:
                b = _as_f64(a).reshape(-1)
                got = conv[k] = (b, b.ctypes.data, b.shape[0], a)          # `a` kept alive: its id must stay unique
            return got
        ps = np.zeros(B, PROBLEM_DTYPE)
        ys = [prep(q["y"]) for q in problems]
        ths = [prep(q["theta"]) for q in problems]
        ws = [None if q.get("weights", None) is None else prep(q["weights"]) for q in problems]
        ps["y"] = [t[1] for t in ys]
        ps["T"] = T = np.array([t[2] for t in ys], dtype=np.int64)
        ps["theta"] = [t[1] for t in ths]
        ps["weights"] = [0 if t is None else t[1] for t in ws]
        ps["model"] = [MODEL[q["model"]] for q in problems]
        ps["kernel"] = [KERNEL[q["kernel"]] for q in problems]
        ps["smoother"] = [SMOOTHER[q.get("smoother", "nemeth")] for q in problems]
        ps["stat"] = [STAT[q.get("stat", "score")] for q in problems]
        ps["dtype"] = [DTYPE[q.get("dtype", "f64")] for q in problems]
        ps["rng"] = RNG["device"]
        ps["N"] = [q["N"] for q in problems]
        ps["t1"] = t1 = np.array([q.get("t1", 0) for q in problems], dtype=np.int64)
        tL = [q.get("tL", None) for q in problems]
        ps["tL"] = tL = np.array([t if v is None else v for v, t in zip(tL, T)], dtype=np.int64)
        ps["flags"] = [q.get("flags", 0) for q in problems]
        ps["reserved"] = [ess_threshold_bits(q.get("ess_threshold", None)) for q in problems]
        ps["lambduh"] = [q.get("lambduh", 1.0) for q in problems]
        ps["prior_mean"] = [q.get("prior_mean", 0.0) for q in problems]
        ps["prior_var"] = [q.get("prior_var", 1.0) for q in problems]
        ps["Ntilde"] = [q.get("Ntilde", 2) for q in problems]
        ps["max_accept_reject"] = [q.get("max_accept_reject", 0) for q in problems]
        ps["seed"] = np.array([int(q.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF for q in problems], dtype=np.uint64)
        ps["stream"] = np.array([int(q.get("stream", 0)) & 0xFFFFFFFFFFFFFFFF for q in problems], dtype=np.uint64)
        ps["step"] = np.array([int(q.get("step", 0)) & 0xFFFFFFFFFFFFFFFF for q in problems], dtype=np.uint64)
        wlen = np.array([1 << 62 if t is None else t[2] for t in ws], dtype=np.int64)
        if np.any(wlen < tL - t1):
            raise ValueError("weights shorter than tL - t1")
        rs = np.zeros(B, RESULT_DTYPE)
        t_call = time.perf_counter()
        rc = self.lib.pfg_run_batch(self.handle, B, C.cast(ps.ctypes.data, C.POINTER(Problem)), C.cast(rs.ctypes.data, C.POINTER(Result)))
        self.last_call_seconds = time.perf_counter() - t_call
        self._check(rc)
        mean, ll = rs["mean_stat"], rs["loglik"]
        outs = []
        for b, q in enumerate(problems):
            # the device record is STAT_DIM[model] wide; sufficient statistics use 3 columns
            h = 3 if q.get("stat", "score") != "score" else STAT_DIM[q["model"]]
            outs.append({"mean_stat": mean[b, :h], "loglik": float(ll[b])})
        return outs

    # ---- resident path ---------------------------------------------------------------------
    def stream(self):
        """The context's own hipStream_t (as an integer handle)."""
        return self._call("pfg_ctx_stream") or 0

    GRID_PHASE_INIT, GRID_PHASE_FINISH = -2, -3

    def launch_device_grid_phase(self, model, kernel, dtype, rng, n_max, phase, B, dev_probs_ptr, stream_ptr=0):
        """One piece of a whole-GPU window: phase = GRID_PHASE_INIT, a timestep t >= 0, or GRID_PHASE_FINISH."""
        self._call("pfg_launch_device_grid_phase", model, kernel, dtype, rng, n_max, phase, B, dev_probs_ptr, stream_ptr)

    GRID_PHASE_ALL = -1

    def launch_device_grid_smoother(self, model, kernel, dtype, rng, smoother, n_max, T_max, phase, B, dev_probs_ptr, stream_ptr=0):
        """The whole-GPU window (phase = GRID_PHASE_ALL) or one piece of it with the batch's smoother stated: 'nemeth' /
        'filter' as launch_device_grid[_phase]; 'poyiadjis_n' (every window NEMETH, lambduh = 1, score) runs the score-only
        twin of the device-generator timestep kernel."""
        self._call("pfg_launch_device_grid_smoother", model, kernel, dtype, rng, smoother, n_max, T_max, phase, B,
                   dev_probs_ptr, stream_ptr)

    def launch_device_smoother(self, model, kernel, dtype, rng, smoother, n_max, B, dev_probs_ptr, stream_ptr=0):
        self._call("pfg_launch_device_smoother", model, kernel, dtype, rng, smoother, n_max, B, dev_probs_ptr, stream_ptr)

    def launch_device_traced(self, model, kernel, dtype, rng, smoother, n_max, B, dev_probs_ptr, stream_ptr=0):
        """The launch that honours the trace_* / rec_* buffers of the descriptors (pfg_launch_device_traced)."""
        self._call("pfg_launch_device_traced", model, kernel, dtype, rng, smoother, n_max, B, dev_probs_ptr, stream_ptr)

    def launch_device_adaptive(self, model, kernel, dtype, rng, n_max, B, dev_probs_ptr, stream_ptr=0, traced=False):
        """A batch of adaptive-resampling windows (descriptors with FLAG_ADAPTIVE_RESAMPLING and ess_threshold):
        pfg_launch_device_adaptive; traced: honour the trace_* / rec_* buffers."""
        self._call("pfg_launch_device_adaptive", model, kernel, dtype, rng, n_max, B, dev_probs_ptr, stream_ptr, traced)

    def last_traced(self):
        return bool(self._call("pfg_last_traced"))

    def launch_device_grid(self, model, kernel, dtype, rng, n_max, T_max, B, dev_probs_ptr, stream_ptr=0):
        """Whole-GPU windows (N > 16384: one launch per timestep, pfg_launch_device_grid); T_max = the largest T."""
        self._call("pfg_launch_device_grid", model, kernel, dtype, rng, n_max, T_max, B, dev_probs_ptr, stream_ptr)

    def launch_device(self, model, kernel, dtype, rng, n_max, B, dev_probs_ptr, stream_ptr=0):
        """stream_ptr: a hipStream_t handle used as is (0 = HIP's default stream, which is also
        torch's default `torch.cuda.current_stream().cuda_stream`)."""
        self._call("pfg_launch_device", model, kernel, dtype, rng, n_max, B, dev_probs_ptr, stream_ptr)

    def sample_windows_device(self, B, dev_probs_ptr, y_ptr, weights_table_ptr, T, S, buffer, strict, seed,
                              chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        self._call("pfg_sample_windows_device", B, dev_probs_ptr, y_ptr, weights_table_ptr, T, S, buffer, strict, seed,
                   chain_offset, step_ctr_ptr, stream_ptr)

    def sample_windows_multi_device(self, num_chains, n_seq, bounds_ptr, weight_offsets_ptr, num_sequences, M, dev_probs_ptr,
                                    seq_len_ptr, y_ptr, weights_ptr, S, buffer, strict, seed, chain_offset=0,
                                    step_ctr_ptr=None, stream_ptr=0):
        """pfg_sample_windows_multi_device: W = K_eff * M window descriptors per chain, chain-major (include/pfgrad.h)."""
        self._call("pfg_sample_windows_multi_device", num_chains, n_seq, bounds_ptr, weight_offsets_ptr, num_sequences, M,
                   dev_probs_ptr, seq_len_ptr, y_ptr, weights_ptr, S, buffer, strict, seed, chain_offset, step_ctr_ptr,
                   stream_ptr)

    def reduce_windows_device(self, num_chains, K, M, win_outs_ptr, seq_len_ptr, rescale, T_total, outs_ptr, stream_ptr=0):
        """pfg_reduce_windows_device: [C*K*M][8] window records -> [C][8], in the reference's order (include/pfgrad.h)."""
        self._call("pfg_reduce_windows_device", num_chains, K, M, win_outs_ptr, seq_len_ptr, rescale, T_total, outs_ptr,
                   stream_ptr)

    def sgld_update_device(self, model, B, theta_ptr, outs_ptr, hyper, epsilon, Tscale, seed,
                           chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        self._call("pfg_sgld_update_device", model, B, theta_ptr, outs_ptr, hyper, epsilon, Tscale, seed, chain_offset,
                   step_ctr_ptr, stream_ptr)

    def sgrld_update_device(self, model, B, theta_ptr, outs_ptr, hyper, epsilon, Tscale, seed,
                            chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        self._call("pfg_sgrld_update_device", model, B, theta_ptr, outs_ptr, hyper, epsilon, Tscale, seed, chain_offset,
                   step_ctr_ptr, stream_ptr)

    def sgd_update_device(self, model, B, theta_ptr, outs_ptr, hyper, epsilon, Tscale, step_ctr_ptr=None, stream_ptr=0):
        """pfg_sgd_update_device: theta += eps (grad_logprior + ghat) / Tscale, then the projection; no draws."""
        self._call("pfg_sgd_update_device", model, B, theta_ptr, outs_ptr, hyper, epsilon, Tscale, step_ctr_ptr, stream_ptr)

    def adagrad_update_device(self, model, B, theta_ptr, moment_ptr, outs_ptr, hyper, epsilon, Tscale, step_ctr_ptr=None,
                              stream_ptr=0):
        """pfg_adagrad_update_device: the SGD step on g / sqrt(G + 1e-9), G [B][MAX_THETA] += g g in place."""
        self._call("pfg_adagrad_update_device", model, B, theta_ptr, moment_ptr, outs_ptr, hyper, epsilon, Tscale,
                   step_ctr_ptr, stream_ptr)

    def sgld_cv_update_device(self, model, B, theta_ptr, outs_ptr, outs_centre_ptr, centre_grad_ptr, hyper, epsilon, Tscale,
                              seed, chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        """pfg_sgld_cv_update_device: the SGLD step on centre_grad + (outs - outs_centre) (include/pfgrad.h)."""
        self._call("pfg_sgld_cv_update_device", model, B, theta_ptr, outs_ptr, outs_centre_ptr, centre_grad_ptr, hyper,
                   epsilon, Tscale, seed, chain_offset, step_ctr_ptr, stream_ptr)

    def cv_accumulate_device(self, B, outs_ptr, acc_ptr, repeat, num_repeats, step_ctr_ptr=None, stream_ptr=0):
        """pfg_cv_accumulate_device: repeat `repeat` of the mean over num_repeats records (include/pfgrad.h)."""
        self._call("pfg_cv_accumulate_device", B, outs_ptr, acc_ptr, repeat, num_repeats, step_ctr_ptr, stream_ptr)

    def gibbs_update_device(self, model, B, theta_ptr, outs_ptr, hyper, seed, chain_offset=0, step_ctr_ptr=None,
                            stream_ptr=0):
        self._call("pfg_gibbs_update_device", model, B, theta_ptr, outs_ptr, hyper, seed, chain_offset, step_ctr_ptr,
                   stream_ptr)

    def pgibbs_update_device(self, model, B, theta_ptr, outs_ptr, hyper, seed, chain_offset=0, step_ctr_ptr=None,
                             stream_ptr=0):
        """pfg_pgibbs_update_device: the conjugate draw from the statistics of a conditional SMC path (SVM, LGSSM)."""
        self._call("pfg_pgibbs_update_device", model, B, theta_ptr, outs_ptr, hyper, seed, chain_offset, step_ctr_ptr,
                   stream_ptr)

    def csmc_device(self, model, dtype, n_max, B, problems_ptr, seed, chain_offset=0, step_ctr_ptr=None, stream_ptr=0,
                    traced=False):
        """pfg_csmc_device: one conditional SMC sweep with ancestor sampling per pfg_csmc_problem record (a device array)."""
        self._call("pfg_csmc_device", model, dtype, n_max, B, problems_ptr, seed, chain_offset, step_ctr_ptr, stream_ptr,
                   traced)

    def cpm_device(self, model, dtype, n_max, B, problems_ptr, rho, seed, chain_offset=0, step_ctr_ptr=None, stream_ptr=0,
                   traced=False):
        """pfg_cpm_device: one sorted, correlated filter per pfg_cpm_problem record (a device array): U' = rho U + sqrt(1 -
        rho^2) eps into the chain's other buffer, out[4] the log-likelihood estimate on U'."""
        self._call("pfg_cpm_device", model, dtype, n_max, B, problems_ptr, rho, seed, chain_offset, step_ctr_ptr, stream_ptr,
                   traced)

    def cpm_commit_device(self, B, n_accept_ptr, seen_ptr, which_ptr, init, stream_ptr=0):
        """pfg_cpm_commit_device: a chain whose acceptance count moved (init: every chain) flips its buffer selector."""
        self._call("pfg_cpm_commit_device", B, n_accept_ptr, seen_ptr, which_ptr, init, stream_ptr)

    def sqmc_device(self, model, dtype, n_max, B, problems_ptr, seed, chain_offset=0, step_ctr_ptr=None, stream_ptr=0,
                    traced=False):
        """pfg_sqmc_device: one sequential quasi-Monte Carlo filter per pfg_sqmc_problem record (a device array): sorted
        particles on one randomised Sobol' point set per timestep, out[4] the log-likelihood estimate."""
        self._call("pfg_sqmc_device", model, dtype, n_max, B, problems_ptr, seed, chain_offset, step_ctr_ptr, stream_ptr,
                   traced)

    def cpm_score_device(self, model, dtype, n_max, B, problems_ptr, rho, lambduh, seed, chain_offset=0, step_ctr_ptr=None,
                         stream_ptr=0, traced=False):
        """pfg_cpm_score_device: pfg_cpm_device's filter (the same U', the same out[4], bit for bit) with the score beside it:
        out[0..H-1] the weighted mean of the particles' additive statistics, carried through the sort (lambduh = 1: Poyiadjis'
        O(N) recursion; lambduh < 1: the fixed-lag shrinkage of Nemeth, Sherlock and Fearnhead)."""
        self._call("pfg_cpm_score_device", model, dtype, n_max, B, problems_ptr, rho, lambduh, seed, chain_offset, step_ctr_ptr,
                   stream_ptr, traced)

    def sqmc_score_device(self, model, dtype, n_max, B, problems_ptr, lambduh, seed, chain_offset=0, step_ctr_ptr=None,
                          stream_ptr=0, traced=False):
        """pfg_sqmc_score_device: pfg_sqmc_device's filter (the same out[4], bit for bit) with the score beside it, as
        cpm_score_device."""
        self._call("pfg_sqmc_score_device", model, dtype, n_max, B, problems_ptr, lambduh, seed, chain_offset, step_ctr_ptr,
                   stream_ptr, traced)

    def logprior_device(self, model, B, theta_ptr, hyper, logprior_ptr, stream_ptr=0):
        """pfg_logprior_device: logprior[b] = Prior.logprior of the raw row theta[b], up to a constant of the hyper-parameters."""
        self._call("pfg_logprior_device", model, B, theta_ptr, hyper, logprior_ptr, stream_ptr)

    def pmmh_propose_device(self, model, B, theta_ptr, theta_prop_ptr, valid_ptr, scale_ptr, seed, chain_offset=0,
                            step_ctr_ptr=None, stream_ptr=0):
        """pfg_pmmh_propose_device: theta_prop = theta + scale (.) z, or theta and valid = 0 outside the support."""
        self._call("pfg_pmmh_propose_device", model, B, theta_ptr, theta_prop_ptr, valid_ptr, scale_ptr, seed, chain_offset,
                   step_ctr_ptr, stream_ptr)

    def pmmh_accept_device(self, model, B, theta_ptr, theta_prop_ptr, valid_ptr, outs_ptr, ll_ptr, n_accept_ptr, hyper, init,
                           seed, chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        """pfg_pmmh_accept_device: the accept / reject step on out[4] (init: ll = out[4] only); bumps *step_ctr unless init."""
        self._call("pfg_pmmh_accept_device", model, B, theta_ptr, theta_prop_ptr, valid_ptr, outs_ptr, ll_ptr, n_accept_ptr,
                   hyper, init, seed, chain_offset, step_ctr_ptr, stream_ptr)

    def pmala_propose_device(self, model, B, theta_ptr, grad_ptr, theta_prop_ptr, valid_ptr, scale_ptr, hyper, seed,
                             chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        """pfg_pmala_propose_device: theta_prop = theta + scale^2 / 2 (.) (grad_logprior + grad) + scale (.) z, or theta and
        valid = 0 outside the support."""
        self._call("pfg_pmala_propose_device", model, B, theta_ptr, grad_ptr, theta_prop_ptr, valid_ptr, scale_ptr, hyper,
                   seed, chain_offset, step_ctr_ptr, stream_ptr)

    def pmala_accept_device(self, model, B, theta_ptr, theta_prop_ptr, valid_ptr, outs_ptr, ll_ptr, grad_ptr, n_accept_ptr,
                            hyper, scale_ptr, init, seed, chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        """pfg_pmala_accept_device: the accept / reject step on out[4], out[0..3] and the two proposal densities (init:
        ll = out[4], grad = out[0..3] only); bumps *step_ctr unless init."""
        self._call("pfg_pmala_accept_device", model, B, theta_ptr, theta_prop_ptr, valid_ptr, outs_ptr, ll_ptr, grad_ptr,
                   n_accept_ptr, hyper, scale_ptr, init, seed, chain_offset, step_ctr_ptr, stream_ptr)

    def smc_logtarget_device(self, model, B, theta_ptr, ll_ptr, hyper, q0_mean_ptr, q0_sd_ptr, h_ptr, stream_ptr=0):
        """pfg_smc_logtarget_device: h[b] = (ll[b] + logprior(theta[b])) - log q0(theta[b])."""
        self._call("pfg_smc_logtarget_device", model, B, theta_ptr, ll_ptr, hyper, q0_mean_ptr, q0_sd_ptr, h_ptr, stream_ptr)

    def smc_temper_device(self, B, h_ptr, phi_ptr, ess_target, seed, stage, result_ptr, status_ptr, parent_ptr, scratch_ptr,
                          stream_ptr=0):
        """pfg_smc_temper_device: the next temperature, the evidence increment and the chains' parents (one workgroup)."""
        self._call("pfg_smc_temper_device", B, h_ptr, phi_ptr, ess_target, seed, stage, result_ptr, status_ptr, parent_ptr,
                   scratch_ptr, stream_ptr)

    def smc_gather_device(self, B, parent_ptr, theta_ptr, ll_ptr, theta_tmp_ptr, ll_tmp_ptr, stream_ptr=0):
        """pfg_smc_gather_device: theta[b], ll[b] = theta[parent[b]], ll[parent[b]] through the two scratch arrays."""
        self._call("pfg_smc_gather_device", B, parent_ptr, theta_ptr, ll_ptr, theta_tmp_ptr, ll_tmp_ptr, stream_ptr)

    def smc_scale_device(self, B, theta_ptr, slots, factor, scale_ptr, stream_ptr=0):
        """pfg_smc_scale_device: scale[j] = factor * sd_j of the population for every slot j in the bit mask `slots`."""
        self._call("pfg_smc_scale_device", B, theta_ptr, slots, factor, scale_ptr, stream_ptr)

    def smc_accept_device(self, model, B, theta_ptr, theta_prop_ptr, valid_ptr, outs_ptr, ll_ptr, n_accept_ptr, hyper,
                          q0_mean_ptr, q0_sd_ptr, phi_ptr, log_alpha_ptr, seed, chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        """pfg_smc_accept_device: pfg_pmmh_accept_device's step at the temperature *phi; bumps *step_ctr."""
        self._call("pfg_smc_accept_device", model, B, theta_ptr, theta_prop_ptr, valid_ptr, outs_ptr, ll_ptr, n_accept_ptr,
                   hyper, q0_mean_ptr, q0_sd_ptr, phi_ptr, log_alpha_ptr, seed, chain_offset, step_ctr_ptr, stream_ptr)

    def seq_reweight_device(self, B, logw_ptr, incr_ptr, incr_stride, ess_target, seed, stage, record_ptr, status_ptr, parent_ptr,
                            scratch_ptr, stream_ptr=0):
        """pfg_seq_reweight_device: the chains' running weights times the chunk's estimates, the evidence increment, the ESS
        and, below the target, the chains' parents (one workgroup)."""
        self._call("pfg_seq_reweight_device", B, logw_ptr, incr_ptr, incr_stride, ess_target, seed, stage, record_ptr, status_ptr,
                   parent_ptr, scratch_ptr, stream_ptr)

    def seq_gather_device(self, B, parent_ptr, row_doubles, src_ptr, dst_ptr, theta_ptr, theta_tmp_ptr, ll_ptr, ll_tmp_ptr,
                          stream_ptr=0):
        """pfg_seq_gather_device: row b of dst = row parent[b] of src; theta and ll by parent through the two scratch arrays."""
        self._call("pfg_seq_gather_device", B, parent_ptr, row_doubles, src_ptr, dst_ptr, theta_ptr, theta_tmp_ptr, ll_ptr,
                   ll_tmp_ptr, stream_ptr)

    def seq_adopt_device(self, B, n_accept_ptr, seen_ptr, row_doubles, cur_ptr, fresh_ptr, stream_ptr=0):
        """pfg_seq_adopt_device: a chain whose acceptance count moved copies its row fresh -> cur and takes the count."""
        self._call("pfg_seq_adopt_device", B, n_accept_ptr, seen_ptr, row_doubles, cur_ptr, fresh_ptr, stream_ptr)

    def scratch_bytes(self, model, dtype, rng, N):
        return self._call("pfg_scratch_bytes", model, dtype, rng, N)

    def scratch_bytes_smoother(self, model, dtype, rng, smoother, N):
        """Per-descriptor scratch of a pfg_launch_device_smoother batch of `smoother` windows (-1: above its maximum)."""
        return self._call("pfg_scratch_bytes_smoother", model, dtype, rng, smoother, N)

    def scratch_bytes_adaptive(self, model, dtype, N):
        """Per-descriptor scratch of a pfg_launch_device_adaptive batch: 0 for N <= 1024, above it the large-N kernels' state,
        the same for both generators -- pfg_scratch_bytes of the REPLAY plan (include/pfgrad.h; the DEVICE plan of plain
        windows keeps N <= 4096 in LDS and answers 0 there).  -1 above N = 16384."""
        return -1 if int(N) > 16384 else self.scratch_bytes(model, dtype, "replay", N)

    def imq_ksd(self, x, gradlogp, c=1.0, beta=0.5):
        x, g = _as_f64(x), _as_f64(gradlogp)
        if x.ndim != 2 or x.shape != g.shape:
            raise ValueError("x and gradlogp dimensions do not match")
        out = C.c_double()
        self._call("pfg_imq_ksd", x.shape[0], x.shape[1], _ptr(x), _ptr(g), c, beta, C.byref(out))
        return float(out.value)

    def sghmc_update_device(self, model, B, theta_ptr, momentum_ptr, outs_ptr, hyper, epsilon, alpha, Tscale, seed,
                            chain_offset=0, step_ctr_ptr=None, stream_ptr=0):
        self._call("pfg_sghmc_update_device", model, B, theta_ptr, momentum_ptr, outs_ptr, hyper, epsilon, alpha, Tscale,
                   seed, chain_offset, step_ctr_ptr, stream_ptr)

    def variant_name(self, model, kernel, dtype, rng, n_max):
        return self._call("pfg_variant_name", model, kernel, dtype, rng, n_max).decode()

    def last_variant(self):
        """Tag of the kernel variant the latest launch through this context ran."""
        return self._call("pfg_last_variant").decode()

    def synchronize(self):
        self._call("pfg_synchronize")


_default_ctx = {}


def default_context(device_id=None):
    """Process-wide context for `device_id` (default: LOCAL_RANK or 0)."""
    if device_id is None:
        device_id = int(os.environ.get("LOCAL_RANK", "0"))
    if device_id not in _default_ctx:
        _default_ctx[device_id] = Context(device_id)
    return _default_ctx[device_id]
