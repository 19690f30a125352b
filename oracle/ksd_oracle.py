"""CPU oracle for the kernel Stein discrepancy (TEST INFRASTRUCTURE ONLY).

NumPy restatement of `IMQ_KSD` / `compute_KSD` of the reference
(`sgmcmc_ssm/trace_metric_functions.py:20-112`), written from its behaviour.  Pinned against
values produced by the reference itself (tests/golden/ksd.npz, tests/golden/make_golden.py)."""
import numpy as np


def imq_ksd(x, gradlogp, c=1.0, beta=0.5):
    """sqrt( sum_{i,j} k0(x_i, x_j) ) / K for the Stein kernel of the inverse multiquadric
    k(x,y) = (c^2 + |x-y|^2)^(-beta):
      k0 = g_i.g_j k  + (g_i - g_j).(x_j - x_i)... expanded as in trace_metric_functions.py:66-75."""
    x = np.asarray(x, dtype=float)
    g = np.asarray(gradlogp, dtype=float)
    if x.shape != g.shape:
        raise ValueError("x and gradlogp dimensions do not match")
    K, d = x.shape
    total = 0.0
    for i in range(K):                      # row-wise to bound memory
        diff = x[i] - x                     # x0 - x1 with x0 = x_i
        diff2 = np.sum(diff ** 2, axis=1)
        base = diff2 + c ** 2
        base_beta = base ** -beta
        base_beta1 = base_beta / base
        coeffgrad = -2.0 * beta * base_beta1
        kterm = np.sum(g[i] * g, axis=1) * base_beta
        g0 = np.sum(g[i] * -diff, axis=1) * coeffgrad
        g1 = np.sum(g * diff, axis=1) * coeffgrad
        g01 = (-d + 2 * (beta + 1) * diff2 / base) * coeffgrad
        total += np.sum(kterm + g0 + g1 + g01)
    return np.sqrt(total) / K


def imq_ksd_terms(x, gradlogp, c=1.0, beta=0.5, rows=64):
    """(tot, abs_tot) = (sum_ij term_ij, sum_ij |term_ij|) in longdouble, term_ij exactly as `imq_ksd` forms it;
    imq_ksd = sqrt(tot) / K.  abs_tot is the scale a summation-order error bound is stated on: the square root of a
    signed sum says little when terms cancel.  c and beta may be equally long sequences: one pair of sums per (c, beta),
    the distances and inner products (which depend on neither) formed once.  `rows` rows at a time bound the memory."""
    LD = np.longdouble
    x = np.asarray(x, dtype=LD)
    g = np.asarray(gradlogp, dtype=LD)
    if x.shape != g.shape:
        raise ValueError("x and gradlogp dimensions do not match")
    K, d = x.shape
    scalar = np.ndim(c) == 0 and np.ndim(beta) == 0
    pairs = [(LD(a), LD(b)) for a, b in zip(np.atleast_1d(c), np.atleast_1d(beta))]
    sums = [[LD(0), LD(0)] for _ in pairs]
    for i0 in range(0, K, rows):
        gi = g[i0:i0 + rows]
        diff = x[i0:i0 + rows, None, :] - x[None, :, :]             # x0 - x1 with x0 = x_i
        diff2 = np.einsum("ijk,ijk->ij", diff, diff)
        gg = np.einsum("ik,jk->ij", gi, g)
        g0d = np.einsum("ik,ijk->ij", gi, -diff)
        g1d = np.einsum("jk,ijk->ij", g, diff)
        for s, (cc, bb) in zip(sums, pairs):
            base = diff2 + cc ** 2
            base_beta = base ** -bb
            coeffgrad = -2 * bb * (base_beta / base)
            term = gg * base_beta + g0d * coeffgrad + g1d * coeffgrad + (-d + 2 * (bb + 1) * diff2 / base) * coeffgrad
            s[0] += np.sum(term)
            s[1] += np.sum(np.abs(term))
    out = [(s[0], s[1]) for s in sums]
    return out[0] if scalar else out
