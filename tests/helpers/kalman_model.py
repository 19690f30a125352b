"""Test-side model of the exact LGSSM score (PFG_SMOOTHER_KALMAN), written from the equations of the scalar model
    x_t = A x_{t-1} + N(0, Q),  y_t = C x_t + N(0, R),  Qinv = LQinv^2,  Rinv = LRinv^2
in the information (mean_precision m, precision P) form of the Kalman messages:

  forward  (x_{t-1} | y_{<t}) -> (x_t | y_{<=t}):  J = A Qinv / (A^2 Qinv + P),  m' = J m + C Rinv y_t,
           P' = Qinv - A Qinv J + C^2 Rinv;  log c_t = log N(y_t; C m_pred / P_pred, 1 / y_prec) with
           y_prec = Rinv - (C Rinv)^2 / (C^2 Rinv + P_pred)
  backward (y_{>t} | x_t) -> (y_{>=t} | x_{t-1}):  xi = Qinv + P + C^2 Rinv,  m' = (A Qinv / xi)(m + C Rinv y_t),
           P' = A^2 Qinv - (A Qinv)^2 / xi
  score    the expected complete-data score under the smoothed marginals of x_t and the joint of (x_{t-1}, x_t),
           d/dLRinv: 1/LRinv - E[(y - C x)^2] LRinv,  d/dC: Rinv (y E[x] - C E[x^2]),
           d/dLQinv: 1/LQinv - E[(x_t - A x_{t-1})^2] LQinv,  d/dA: Qinv (E[x_t x_{t-1}] - A E[x_{t-1}^2])

evaluated like the kernel: left buffer forward, right buffer backward, window backward (messages kept), window
forward.  `run_windows_kalman` evaluates problem dicts with it and hands particle-filter problems to the CPU oracle,
so that it can stand in for `particle_filters.run_windows` in the CPU tests."""
import math

LOG_2PI_HALF = 0.5 * math.log(2.0 * math.pi)


def _forward(th, m, P, y):
    A, C, Qinv, Rinv = th
    J = A * Qinv / (A * A * Qinv + P)
    pm, pP = J * m, Qinv - A * Qinv * J
    y_prec = Rinv - C * Rinv * (C * Rinv / (C * C * Rinv + pP))
    r = y - C * (pm / pP)
    log_c = -0.5 * r * r * y_prec + 0.5 * math.log(abs(y_prec)) - LOG_2PI_HALF
    return pm + C * Rinv * y, pP + C * C * Rinv, log_c


def _backward(th, m, P, y):
    A, C, Qinv, Rinv = th
    xi = Qinv + P + C * C * Rinv
    L = A * Qinv / xi
    return L * (m + C * Rinv * y), A * A * Qinv - A * Qinv * L


def kalman_window(theta, y, t1, tL, weights=None, prior_mean=0.0, prior_var=10.0):
    """-> (gradient [LRinv, LQinv, C, A], forward log-likelihood of [t1, tL))."""
    A, C, LQinv, LRinv = (float(v) for v in theta[:4])
    Qinv, Rinv = LQinv * LQinv, LRinv * LRinv
    th = (A, C, Qinv, Rinv)
    y = [float(v) for v in y]
    T = len(y)
    tL = min(tL, T)
    bm, bP = 0.0, 0.0
    for t in range(T - 1, tL - 1, -1):
        bm, bP = _backward(th, bm, bP, y[t])
    P = 1.0 / prior_var
    m = prior_mean * P
    for t in range(t1):
        m, P, _ = _forward(th, m, P, y[t])
    back = [None] * (tL - t1)
    for t in range(tL - t1 - 1, -1, -1):
        back[t] = (bm, bP)
        bm, bP = _backward(th, bm, bP, y[t1 + t])
    gA = gC = gLQ = gLR = ll = 0.0
    for t in range(tL - t1):
        yt = y[t1 + t]
        w = 1.0 if weights is None or len(weights) == 0 else float(weights[t])
        bm, bP = back[t]
        # (x_{t-1}, x_t): precision [[P + A^2 Qinv, -A Qinv], [-A Qinv, bP + C^2 Rinv + Qinv]]
        a, c, e = P + A * A * Qinv, -A * Qinv, bP + C * C * Rinv + Qinv
        r1, r2 = m, bm + C * Rinv * yt
        det = P * e + A * A * Qinv * (bP + C * C * Rinv)
        xp, xn = (e * r1 - c * r2) / det, (a * r2 - c * r1) / det
        xpxp, xnxp, xnxn = e / det + xp * xp, -c / det + xn * xp, a / det + xn * xn
        gA += w * Qinv * (xnxp - A * xpxp)
        gLQ += w * (1.0 / LQinv - (xnxn - 2.0 * A * xnxp + A * A * xpxp) * LQinv)
        m, P, log_c = _forward(th, m, P, yt)
        ll += w * log_c
        cP = P + bP
        x = (m + bm) / cP
        xx = 1.0 / cP + x * x
        gC += w * Rinv * (yt * x - C * xx)
        gLR += w * (1.0 / LRinv - (yt * yt - 2.0 * C * x * yt + C * C * xx) * LRinv)
    return [gLR, gLQ, gC, gA], ll


def run_windows_kalman(problems, ctx=None, want_final=False):
    """Stand-in for particle_filters.run_windows: Kalman problems by the model above, the rest by the CPU oracle."""
    import numpy as np
    from oracle_backend import run_windows_oracle
    outs = []
    for q in problems:
        if q["smoother"] != "kalman":
            outs.append(run_windows_oracle([q], ctx, want_final)[0])
            continue
        if not q["prior_var"] > 0:
            raise ValueError("prior_var must be > 0")
        g, ll = kalman_window(q["theta"], np.reshape(q["y"], -1), q["t1"], q["tL"], q.get("weights"),
                              q["prior_mean"], q["prior_var"])
        outs.append(dict(mean_statistic=np.array(g), loglikelihood_estimate=ll))
    return outs
