"""Trace-driven reference of the elementwise-statistics pass (csrc/pfg_elementwise.hip), NumPy longdouble.

The pass is a pure function of the filter's trace -- particles x[t], log-weights logw[t], the resampling ancestors of
every step -- so the reference takes the trace and evaluates the recursion stated at the top of pfg_elementwise.hip:
    S'[i] = lam S[anc_i] + (1 - lam) sum_k w_k S[k]        block t - t1 += weights[t - t1] h(x_t[anc_i], x_{t+1}[i])
    O(N^2):  bw_ij = softmax_j(logw_j + log q(x'_i | x_j)),  S'[i] = sum_j bw_ij S[j],  block += w_t [x', x'^2, (bw x) x']
with h = [x', x'^2, x x'] (GARCH [x', x'^2, x'^4]) on the first state component.  Vectorised, so that the shapes of
tests/test_gpu_elementwise_shapes.py cost seconds where the oracle's loops cost minutes; pinned to the oracle at small
shapes by tests/test_elementwise_model_host.py.  `dtype=np.float64` evaluates the same expressions in plain float64
(BLAS summation order): its distance from the longdouble result is the floor `float64_floors` measures."""
import numpy as np

from oracle import pf_oracle as po

LD = np.longdouble

# the shapes of tests/test_gpu_elementwise_shapes.py
_MK = [("svm", "prior"), ("garch", "optimal"), ("lgssm", "optimal")]
# (T, t1, tL): Wd = 3 (tL - t1) = 255 (one column block, one idle lane), 258 (block 1 has two live lanes, the last
# triple sits in columns 255 / 256 / 257), 513 (three blocks), 258 again (steps outside the window on both sides)
_ON_SHAPES = [(88, 1, 86), (90, 2, 88), (175, 2, 173), (90, 2, 88)]


def _on_cases():
    """(model, kernel, N, T, t1, tL, lam, salt): every shape at lam = 0.9 and 1.0 for the three models; N walks
    37..40 (the four N mod 4 tails of ews_colsum_kernel's unroll), so every model meets every tail.  Then N = 1100 once:
    the large-N kernel's trace and the softmax's second stride."""
    out = []
    for r, (T, t1, tL) in enumerate(_ON_SHAPES):
        for c, lam in enumerate((0.9, 1.0)):
            for s, mk in enumerate(_MK):
                out.append(mk + (37 + (r + c + s) % 4, T, t1, tL, lam, r))
    return out + [("svm", "prior", 1100, 90, 2, 88, 0.9, 9)]


CASES_ON = _on_cases()
# (model, kernel, N, T, t1, tL, salt): second j stride with an odd tail; odd N over two full strides; the trace of
# n2_mem1024; the whole bw[4096]; Wd = 270 (the col += 256 loop)
CASES_N2 = [mk + shape + (0,) for shape in ((257, 5, 1, 4), (515, 5, 1, 4), (1025, 4, 0, 3)) for mk in _MK] + \
           [("lgssm", "optimal", 4096, 3, 0, 3, 0), ("garch", "optimal", 70, 92, 1, 91, 0)]


def softmax(lw):
    e = np.exp(lw - np.max(lw, axis=-1, keepdims=True))
    return e / np.sum(e, axis=-1, keepdims=True)


def _h(model, xp, xn):
    """[N, 3] block of one step from the parents' and the children's first state component"""
    if model == "garch":
        return np.stack([xn, xn * xn, (xn * xn) * (xn * xn)], axis=1)
    return np.stack([xn, xn * xn, xp * xn], axis=1)


def ew_reference(model, x, logw, anc, t1, tL, weights, lam, dtype=LD):
    """nemeth (lam < 1 or lam = 1) / poyiadjis_N (lam = 1).  x [T+1, N, ns], logw [T+1, N], anc [T, N] ->
    (stats [N, 3L], mean [3L]) with L = min(tL, T) - t1."""
    x = np.asarray(x, dtype=dtype)
    logw = np.asarray(logw, dtype=dtype)
    anc = np.asarray(anc).astype(np.int64)
    T, N = anc.shape
    tL = min(tL, T)
    S = np.zeros((N, 3 * (tL - t1)), dtype=dtype)
    lam = dtype(lam)
    for t in range(T):
        a = anc[t]
        Sn = S[a]
        if lam != 1:
            Sn = lam * Sn + (1 - lam) * (softmax(logw[t]) @ S)
        if t1 <= t < tL:
            wt = dtype(1.0 if weights is None else weights[t - t1])
            Sn[:, 3 * (t - t1):3 * (t - t1) + 3] += wt * _h(model, x[t][a, 0], x[t + 1][:, 0])
        S = Sn
    return S, softmax(logw[T]) @ S


def _log_q(model, d, x_t, xn, dtype):
    """log q(x'_i | x_j) as oracle.pf_oracle.prior_log_density states it, [children, parents]"""
    c = lambda k: dtype(np.asarray(d[k]).reshape(-1)[0])
    half, log2pi = dtype(0.5), np.log(2 * dtype(np.pi))
    if model == "garch":
        s2 = c("alpha") + c("beta") * x_t[:, 0] ** 2 + c("gamma") * x_t[:, 1]
        return -half * xn[:, None] ** 2 / s2[None, :] - half * log2pi - half * np.log(s2)[None, :]
    diff = xn[:, None] - c("A") * x_t[None, :, 0]
    return -half * diff ** 2 * c("Qinv") - half * log2pi + np.log(c("LQinv"))


def ew_reference_n2(model, theta, x, logw, t1, tL, weights, dtype=LD, chunk=256):
    """poyiadjis_N2: every child averages over all parents with the backward weights.  Children go in chunks, so that
    N = 4096 never holds an N x N matrix."""
    x = np.asarray(x, dtype=dtype)
    logw = np.asarray(logw, dtype=dtype)
    d = po.derived(model, theta)
    T, N = x.shape[0] - 1, x.shape[1]
    tL = min(tL, T)
    S = np.zeros((N, 3 * (tL - t1)), dtype=dtype)
    for t in range(T):
        Sn = np.zeros_like(S)
        bx = np.zeros(N, dtype=dtype)
        carry = bool(np.any(S))
        for i0 in range(0, N, chunk):
            bw = softmax(logw[t][None, :] + _log_q(model, d, x[t], x[t + 1][i0:i0 + chunk, 0], dtype))
            if carry:
                Sn[i0:i0 + chunk] = bw @ S
            bx[i0:i0 + chunk] = bw @ x[t][:, 0]
        if t1 <= t < tL:
            wt = dtype(1.0 if weights is None else weights[t - t1])
            xn = x[t + 1][:, 0]
            third = (xn * xn) * (xn * xn) if model == "garch" else bx * xn
            Sn[:, 3 * (t - t1):3 * (t - t1) + 3] += wt * np.stack([xn, xn * xn, third], axis=1)
        S = Sn
    return S, softmax(logw[T]) @ S


def case_inputs(model, kernel, N, T, t1, tL, salt=0):
    """Observations, importance weights and replayed streams of one case (the GPU test and the floor share them)"""
    import zlib
    from test_host_logic import default_params, GEN
    rs = np.random.RandomState(zlib.crc32("{0} {1} {2} {3} {4}".format(model, N, T, t1, salt).encode()) & 0x7FFFFFFF)
    p = default_params(model)
    state = np.random.get_state()
    np.random.seed(3)
    y = GEN[model](T=T, parameters=p)["observations"].reshape(-1)
    np.random.set_state(state)
    w = rs.uniform(1.0, 3.0, size=tL - t1)
    z0, u, z = po.draw_streams(rs, N, T)
    return dict(theta=p.theta(), y=y, weights=w, z0=z0, u=u, z=z)


def normalised_error(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref)) / max(LD(1), np.max(np.abs(ref))))


def float64_floors(verbose=False):
    """The error any float64 evaluation in another summation order has: the helper in float64 against itself in
    longdouble on the oracle's filter trace of every case, normalised per case; the largest of each family."""
    floors = {}
    for fam, cases in (("on", CASES_ON), ("n2", CASES_N2)):
        worst = 0.0
        for case in cases:
            model, kernel, N, T, t1, tL = case[:6]
            q = case_inputs(model, kernel, N, T, t1, tL, case[-1])
            tr = po.pf_window(model, q["theta"], q["y"], N, q["z0"], q["u"], q["z"], kernel=kernel, pf="poyiadjis_N",
                              stat="none", t1=t1, tL=tL, prior_mean=0.0, prior_var=1.3, save_all=True)
            tx, tlw, ta = tr["all_x_t"], tr["all_log_weights"], tr["all_ancestors"]
            if fam == "on":
                ref = ew_reference(model, tx, tlw, ta, t1, tL, q["weights"], case[6])
                f64 = ew_reference(model, tx, tlw, ta, t1, tL, q["weights"], case[6], dtype=np.float64)
            else:
                ref = ew_reference_n2(model, q["theta"], tx, tlw, t1, tL, q["weights"])
                f64 = ew_reference_n2(model, q["theta"], tx, tlw, t1, tL, q["weights"], dtype=np.float64)
            err = max(normalised_error(f64[0], ref[0]), normalised_error(f64[1], ref[1]))
            if verbose:
                print(fam, case, "max|ref| = {0:.3g}".format(float(np.max(np.abs(ref[0])))), "floor = {0:.3g}".format(err), flush=True)
            worst = max(worst, err)
        floors[fam] = worst
    return floors
