"""Host restatement of the SGD, ADAGRAD and control-variate SGLD update rules of resident chains and of the centring pass's
accumulation (pfg_chains.hip: optim_update_kernel, sgld_cv_update_kernel, cv_accumulate_kernel), on the pieces of
keyed_draws.py -- the prior gradient, the score-column map, the keyed normals, the projection's two branches -- in
np.longdouble.  Test-only.

  sgd         p = theta + eps ((grad_logprior(theta) + ghat) / T), then the projection
  adagrad     g = (grad_logprior(theta) + ghat) / T;  G' = G + g g;  p = theta + eps (g / sqrt(G' + 1e-9)), then the projection
  sgld_cv     ghat_k = centre_grad_k + (outs_k - outs_centre_k) on the four score columns, IN DOUBLE and in that operand order
              (two IEEE operations: the host's are the kernel's), then keyed_draws.sgld_expected on it
  accumulate  repeat 0 stores columns 0..4, repeat r adds them, the last repeat divides by R: float64, the kernel's order, so
              the result is bitwise
"""
import numpy as np

import keyed_draws as kd

LD = kd.LD
NUGGET = 1e-9           # the reference's NOISE_NUGGET


def _project(model, pre, tol):
    """The projection of pfg_chains.hip on pre [C, P] with the other branch near a threshold: (new, other, amb)."""
    P = pre.shape[1]
    new, other, amb = pre.copy(), pre.copy(), np.zeros(pre.shape, bool)
    if model in ("svm", "lgssm"):
        new[:, 0], other[:, 0], amb[:, 0] = kd._clip_A(pre[:, 0], tol[:, 0])
        if model == "lgssm":
            new[:, 1] = other[:, 1] = 1.0
        for j in (P - 2, P - 1):
            new[:, j], other[:, j], amb[:, j] = kd._reflect(pre[:, j], tol[:, j])
    else:
        new[:, 3], other[:, 3], amb[:, 3] = kd._reflect(pre[:, 3], tol[:, 3])
    return new, other, amb


def _scaled_gradient(model, theta, ghat, hy, T):
    """(theta [C, P], g = (grad_logprior + ghat) / T, the magnitude of g's terms: the scale of its rounding), long double."""
    hy = kd._hy(hy)
    th = np.asarray(theta, dtype=float)[:, :len(kd.SLOTS[model])].astype(LD)
    g = np.asarray(ghat, dtype=float)[:, list(kd.SCORE_COL[model])].astype(LD)
    gp, gmag = kd.prior_gradient(model, th, hy)
    return th, (gp + g) / LD(T), (gmag + np.abs(g)) / LD(T)


def sgd_expected(model, theta, ghat, hy, eps, T):
    """One SGD step of C chains: theta [C, >= P] and ghat [C, 8] as the kernel reads them (double)."""
    th, g, gmag = _scaled_gradient(model, theta, ghat, hy, T)
    tol = kd.TOL_ULPS * kd.ULP * (np.abs(th) + LD(eps) * gmag)
    new, other, amb = _project(model, th + LD(eps) * g, tol)
    return kd.Expected(new, tol, other, amb)


def adagrad_expected(model, theta, ghat, hy, eps, T, moment):
    """One ADAGRAD step of C chains from the moments `moment` [C, >= P]; Expected.momentum is the new G, mom_tol its
    tolerance.  An error dg in g moves G by 2 |g| dg and the increment g / sqrt(G + nugget) by at most dg / sqrt(G + nugget)."""
    th, g, gmag = _scaled_gradient(model, theta, ghat, hy, T)
    G0 = np.asarray(moment, dtype=float)[:, :th.shape[1]].astype(LD)
    G = G0 + g * g
    root = np.sqrt(G + LD(NUGGET))
    inc = g / root
    tol = kd.TOL_ULPS * kd.ULP * (np.abs(th) + LD(eps) * (gmag / root + np.abs(inc)))
    new, other, amb = _project(model, th + LD(eps) * inc, tol)
    return kd.Expected(new, tol, other, amb, momentum=G, mom_tol=kd.TOL_ULPS * kd.ULP * (G + 2 * np.abs(g) * gmag))


def cv_gradient(outs, outs_centre, centre_grad):
    """[C, 8] with columns 0..3 = centre_grad + (outs - outs_centre) in double, in that operand order; the rest zero."""
    o, oc = np.asarray(outs, dtype=np.float64), np.asarray(outs_centre, dtype=np.float64)
    g = np.zeros((o.shape[0], 8))
    g[:, :4] = np.asarray(centre_grad, dtype=np.float64)[:, :4] + (o[:, :4] - oc[:, :4])
    return g


def sgld_cv_expected(model, theta, outs, outs_centre, centre_grad, hy, eps, T, seed, chain_offset, step):
    """One control-variate SGLD step of C chains: SGLD's step on cv_gradient."""
    return kd.sgld_expected(model, theta, cv_gradient(outs, outs_centre, centre_grad), hy, eps, T, seed, chain_offset, step)


def accumulate_expected(records):
    """The accumulator [C, 8] after the R = len(records) repeats of pfg_cv_accumulate_device on records[r] [C, 8], from a
    zeroed one: columns 0..4 the mean in the kernel's order of operations (bitwise), columns 5..7 untouched."""
    R = len(records)
    acc = np.zeros((np.shape(records[0])[0], 8))
    for r, rec in enumerate(records):
        rec = np.asarray(rec, dtype=np.float64)
        acc[:, :5] = rec[:, :5] if r == 0 else acc[:, :5] + rec[:, :5]
        if r == R - 1:
            acc[:, :5] = acc[:, :5] / np.float64(R)
    return acc
