"""Test-side model of FFBS for the scalar LGSSM (PFG_SMOOTHER_KALMAN_FFBS), written from the equations of
    x_t = A x_{t-1} + N(0, Q),  y_t = C x_t + N(0, R),  Qinv = LQinv^2,  Rinv = LRinv^2

  forward   the Kalman messages (mean_precision m_t, precision P_t) of x_t given y_{<=t}, from the message of x_{-1}:
            J = A Qinv / (A Qinv A + P),  m' = J m + C Rinv y_t,  P' = (Qinv - A Qinv J) + C Rinv C
  backward  x_{T-1} ~ N(m / P, 1 / P) at the end, then x_t | x_{t+1} ~ N(c (m_t + A Qinv x_{t+1}), c) with
            c = 1 / (P_t + A Qinv A); a draw is mean + z sqrt(variance), written in the reference's operation order
            x_{T-1} = z sqrt(c) + c m,  x_t = c (m_t + A Qinv x_{t+1}) + (z sqrt(c) + 0.0)
  score     the complete-data score of a window [t1, tL) of the buffer, averaged over the paths: per step
            d/dA: w Qinv <(x_t - A x_{t-1}) x_{t-1}>,  d/dLQinv: w (1/LQinv - <(x_t - A x_{t-1})^2> LQinv),
            d/dC: w Rinv <(y_t - C x_t) x_t>,  d/dLRinv: w (1/LRinv - <(y_t - C x_t)^2> LRinv);
            the transition terms only where x_{t-1} is in the buffer

The normals of path s at time t are z[(T-1-t) S + s] (one np.random.standard_normal(T S) in the reference's order).
`run_windows_ffbs` evaluates problem dicts with it and hands the others to the Kalman / particle-filter stand-ins, so
that it can stand in for `particle_filters.run_windows` in the CPU tests."""
import math


def forward_messages(theta, y, prior_mean=0.0, prior_var=10.0):
    """[(m_t, P_t)] for t = 0..T-1, from the message of x_{-1} (mean prior_mean, variance prior_var)."""
    A, C, LQinv, LRinv = (float(v) for v in theta[:4])
    Qinv, Rinv = LQinv * LQinv, LRinv * LRinv
    AtQinv = A * Qinv
    AtQinvA = AtQinv * A
    CtRinv = C * Rinv
    CtRinvC = CtRinv * C
    P = 1.0 / prior_var
    m = prior_mean * P
    out = []
    for yt in y:
        J = AtQinv / (AtQinvA + P)
        pm, pP = J * m, Qinv - AtQinv * J
        m, P = pm + CtRinv * float(yt), pP + CtRinvC
        out.append((m, P))
    return out


def sample_paths(theta, y, z, S, prior_mean=0.0, prior_var=10.0):
    """S backward-sampled paths, [T][S]."""
    A, LQinv = float(theta[0]), float(theta[2])
    AtQinv = A * (LQinv * LQinv)
    AtQinvA = AtQinv * A
    msgs = forward_messages(theta, y, prior_mean, prior_var)
    T = len(msgs)
    x = [[0.0] * S for _ in range(T)]
    if T == 0:
        return x
    m, P = msgs[-1]
    c = 1.0 / P
    for s in range(S):
        x[T - 1][s] = float(z[s]) * math.sqrt(c) + c * m
    for t in range(T - 2, -1, -1):
        m, P = msgs[t]
        c = 1.0 / (P + AtQinvA)
        k = T - 1 - t
        for s in range(S):
            x[t][s] = c * (m + AtQinv * x[t + 1][s]) + (float(z[k * S + s]) * math.sqrt(c) + 0.0)
    return x


def complete_score(theta, y, x, t1, tL, weights=None, x_prev=None):
    """The score [LRinv, LQinv, C, A] of y[t1:tL] given the paths x[t1:tL] ([L][S]) and, if not None, x_prev ([S]),
    the paths at t1 - 1."""
    A, C, LQinv, LRinv = (float(v) for v in theta[:4])
    Qinv, Rinv = LQinv * LQinv, LRinv * LRinv
    gA = gC = gLQ = gLR = 0.0
    prev = x_prev
    for i, t in enumerate(range(t1, tL)):
        w = 1.0 if weights is None or len(weights) == 0 else float(weights[i])
        xt = x[i]
        S = len(xt)
        if prev is not None:
            d = [xt[s] - A * prev[s] for s in range(S)]
            gA += w * Qinv * sum(d[s] * prev[s] for s in range(S)) / S
            gLQ += w * (1.0 / LQinv - sum(v * v for v in d) * LQinv / S)
        e = [float(y[t]) - C * xt[s] for s in range(S)]
        gC += w * Rinv * sum(e[s] * xt[s] for s in range(S)) / S
        gLR += w * (1.0 / LRinv - sum(v * v for v in e) * LRinv / S)
        prev = xt
    return [gLR, gLQ, gC, gA]


def ffbs_window(q):
    """One FFBS problem dict (REPLAY normals q['z']) -> (score or zeros, paths [T][S])."""
    import numpy as np
    if not q["prior_var"] > 0:
        raise ValueError("prior_var must be > 0")
    y = np.reshape(q["y"], -1)
    T, S = y.shape[0], int(q["N"])
    if q.get("rng", "replay") != "replay":
        raise NotImplementedError("the CPU model replays host normals only")
    z = np.reshape(q["z"], -1)
    if z.shape[0] != T * S:
        raise ValueError("z must have T*N entries")
    x = sample_paths(q["theta"], y, z, S, q["prior_mean"], q["prior_var"])
    t1, tL = int(q["t1"]), min(int(q["tL"]), T)
    g = [0.0, 0.0, 0.0, 0.0]
    if q.get("stat", "score") == "score":
        g = complete_score(q["theta"], y, x[t1:tL], t1, tL, q.get("weights"), x[t1 - 1] if t1 > 0 else None)
    return g, x


def run_windows_ffbs(problems, ctx=None, want_final=False, want_paths=False):
    """Stand-in for particle_filters.run_windows: FFBS problems by the model above, the rest by the Kalman model and
    the CPU oracle."""
    import numpy as np
    from kalman_model import run_windows_kalman
    outs = []
    for q in problems:
        if q["smoother"] != "kalman_ffbs":
            outs.append(run_windows_kalman([q], ctx, want_final)[0])
            continue
        g, x = ffbs_window(q)
        o = dict(mean_statistic=np.array(g), loglikelihood_estimate=0.0)
        if want_paths:
            o["paths"] = np.array(x, dtype=float).reshape(len(x), int(q["N"]))
        outs.append(o)
    return outs
