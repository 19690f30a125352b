"""NumPy restatement of the 1-D LGSSM chain rules the resident SGRLD and Gibbs updates implement
(csrc/pfg_chains.hip): the SGRLD drift and per-variable noise scale of sample_sgrld with the LGSSM preconditioner, and
the conjugate posterior LGSSMPrior.sample_posterior draws from.  theta = (A, C, LQinv, LRinv); score columns
[LRinv, LQinv, C, A] as the kernels write them."""
import numpy as np

THETA = ("A", "C", "LQinv_vec", "LRinv_vec")
SCORE_COL = dict(LRinv_vec=0, LQinv_vec=1, C=2, A=3)


def hyper_of(prior):
    h = prior.hyperparams
    first = lambda v: float(np.asarray(v).reshape(-1)[0])
    return {k: first(h[k]) for k in ("df_Qinv", "scale_Qinv", "df_Rinv", "scale_Rinv", "mean_A", "var_col_A",
                                     "mean_C", "var_col_C")}


def grad_logprior(theta, hy):
    """[n, 4] grad log-prior at theta [n, 4] (covariance.py:272-284, matrices.py:597-607), theta order."""
    A, C, LQ, LR = (theta[:, j] for j in range(4))
    Qinv, Rinv = LQ * LQ + 1e-16, LR * LR + 1e-16
    return np.column_stack([-1.0 * (Qinv * (A - hy["mean_A"])) / hy["var_col_A"],
                            -1.0 * (Rinv * (C - hy["mean_C"])) / hy["var_col_C"],
                            (hy["df_Qinv"] - 2.0) / LQ - LQ / hy["scale_Qinv"],
                            (hy["df_Rinv"] - 2.0) / LR - LR / hy["scale_Rinv"]])


def sgrld_precondition(theta, grad, scale):
    """D(theta) grad * scale, theta order: A: Q g, C: R g, LQinv: 0.5 Qinv g, LRinv: 0.5 Rinv g."""
    LQ, LR = theta[:, 2], theta[:, 3]
    Qinv, Rinv = LQ * LQ + 1e-16, LR * LR + 1e-16
    return np.column_stack([(1.0 / Qinv) * grad[:, 0], (1.0 / Rinv) * grad[:, 1],
                            (0.5 * Qinv) * grad[:, 2], (0.5 * Rinv) * grad[:, 3]]) * scale


def sgrld_correction(theta, scale):
    """correction_term: 0 for the matrices, (n + 1) / 2 L = L for the Cholesky factors (n = 1)."""
    return np.column_stack([np.zeros(len(theta)), np.zeros(len(theta)), theta[:, 2], theta[:, 3]]) * scale


def sgrld_noise_factor(theta):
    """precondition_noise per unit normal (scale 1): z / LQinv, z / LRinv, sqrt(0.5) LQinv z, sqrt(0.5) LRinv z."""
    LQ, LR = theta[:, 2], theta[:, 3]
    return np.column_stack([1.0 / LQ, 1.0 / LR, np.sqrt(0.5) * LQ, np.sqrt(0.5) * LR])


def sgrld_drift(theta, ghat, hy, eps, T):
    """eps (D (grad_logprior + ghat) / T + correction / T), theta order; ghat in score columns."""
    g = grad_logprior(theta, hy) + ghat[:, [SCORE_COL[v] for v in THETA]]
    return eps * (sgrld_precondition(theta, g, 1.0 / T) + sgrld_correction(theta, 1.0 / T))


def sgrld_noise_sd(theta, eps, T):
    """standard deviation of the SGRLD noise of each variable: sqrt(2 eps / T) |noise factor|."""
    return np.sqrt(2.0 * eps) * np.sqrt(1.0 / T) * np.abs(sgrld_noise_factor(theta))


def gibbs_stats(x, y):
    """The 8-double record of PFG_STAT_GIBBS for one path x and series y (both [T])."""
    x, y = np.asarray(x, float).reshape(-1), np.asarray(y, float).reshape(-1)
    return np.array([x[:-1] @ x[:-1], x[1:] @ x[:-1], x[1:] @ x[1:], x @ x, y @ x, y @ y, len(x), 0.0])


def gibbs_posterior(stats, hy):
    """The conjugate posterior of (Qinv, A | Q) and (Rinv, C | R) given the statistics: Xinv ~ scale * chi2(df),
    M | X ~ N(mean, var_unit / (LXinv^2 + 1e-9))."""
    s = np.asarray(stats, float)
    T = s[6]
    out = {}
    for name, mat, spp, scp, scc, count in (("Q", "A", s[0], s[1], s[2], T - 1), ("R", "C", s[3], s[4], s[5], T)):
        mean, var_col = hy["mean_" + mat], hy["var_col_" + mat]
        Spp = 1.0 / var_col + spp
        Scp = mean / var_col + scp
        Scc = mean * mean / var_col + scc
        out["df_" + name] = hy["df_{0}inv".format(name)] + count
        out["scale_" + name] = 1.0 / (1.0 / hy["scale_{0}inv".format(name)] + Scc - Scp * Scp / Spp)
        out["mean_" + mat] = Scp / Spp
        out["var_unit_" + mat] = 1.0 / Spp
    return out
