"""One step of a Poyiadjis O(N^2) window recomputed from a launch's own trace (teacher-forced), and the law of a step's
ancestors -- for units that record no normals or no resampling words.

`forced_steps` takes the traced particles, log-weights, statistics and ancestors of a window and recomputes, for every step
t, what step t + 1 must hold given step t AS TRACED: the log-weights with po.kernel_reweight on (x_t[anc_t], x_{t+1}), and
the statistics with the reference's O(N^2) recursion (pf.py:84-136: every child averages stats_j + weight_t h(x_j, child)
over ALL parents j with the backward weights log_normalize(logw_t + prior_log_density(x_j -> child))), through
po.prior_log_density, po.log_normalize, po.score_statistic and po.sufficient_statistic.  Plain NumPy in float64, one step
at a time; nothing of one recomputed step enters the next.  The proposal itself (x_{t+1} from its normal) is NOT checked
here: that needs the recorded normals.

`ancestor_law_z` is a z-score of one resampling step against the multinomial law."""
import numpy as np

from oracle import pf_oracle as po


def forced_step(model, kernel, d, x, logw, stats, anc, x_next, y_t, stat, inside, weight_t):
    """(log-weights, statistics [N, h], log-likelihood increment) of step t + 1 from the traced step t.

    x [N, ns], logw [N], stats [N, h]: particles, log-weights and statistics before the step; anc [N]: the ancestors the
    step resampled; x_next [N, ns]: the children it proposed; y_t: the observation; stat: 'score' | 'suff' | 'none';
    inside: t1 <= t < tL; weight_t: the step's importance weight (1.0 outside the window)."""
    x, x_next = np.asarray(x, dtype=np.float64), np.asarray(x_next, dtype=np.float64)
    logw, stats = np.asarray(logw, dtype=np.float64), np.asarray(stats, dtype=np.float64)
    N, h = stats.shape
    y_t = np.asarray(y_t, dtype=np.float64).reshape(1)
    new_logw = po.kernel_reweight(model, kernel, d, x[np.asarray(anc)], x_next, y_t)
    bw = np.empty((N, N))
    for i in range(N):
        bw[i] = po.log_normalize(logw + po.prior_log_density(model, d, x, np.outer(np.ones(N), x_next[i])))
    parent = np.tile(np.arange(N), N)           # row i * N + j: child i, parent j
    child = np.repeat(np.arange(N), N)
    if inside and stat == "score":
        add = po.score_statistic(model, d, x[parent], x_next[child], y_t)
    elif inside and stat == "suff":
        add = po.sufficient_statistic(model, x[parent], x_next[child])
    else:
        add = np.zeros((N * N, h))
    add = add[:, :h] * float(weight_t)
    new_stats = np.einsum("ijk,ij->ik", np.reshape(stats[parent] + add, (N, N, h)), bw)
    dll = float(weight_t) * np.log(np.mean(np.exp(new_logw))) if inside else 0.0
    return new_logw, new_stats, dll


def forced_steps(model, kernel, theta, y, all_x, all_logw, all_stats, all_anc, stat="score", t1=0, tL=None, weights=None):
    """forced_step for t = 0 .. T - 1 on a window's trace (all_x [T+1, N, ns], all_logw [T+1, N], all_stats [T+1, N, h],
    all_anc [T, N]) -> (log-weights [T, N], statistics [T, N, h], log-likelihood increments [T]); entry t is what the
    trace must hold at t + 1."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    T = y.shape[0]
    tL = T if tL is None else tL
    d = po.derived(model, theta)
    lws, sts, dlls = [], [], []
    for t in range(T):
        inside = t1 <= t < tL
        wt = float(weights[t - t1]) if inside and weights is not None else 1.0
        lw, st, dll = forced_step(model, kernel, d, all_x[t], all_logw[t], all_stats[t], all_anc[t], all_x[t + 1], y[t],
                                  stat, inside, wt)
        lws.append(lw); sts.append(st); dlls.append(dll)
    return np.array(lws), np.array(sts), np.array(dlls)


def ancestor_law_z(logw, anc):
    """z-score of one resampling step against the multinomial law.  With w = softmax(logw) and ancestors drawn i.i.d. from
    w, w[anc_i] has mean sum(w^2) and variance sum(w^3) - sum(w^2)^2, so
        Z = (mean_i w[anc_i] - sum(w^2)) / sqrt((sum(w^3) - sum(w^2)^2) / N)
    is asymptotically standard normal.  None where the weights are all equal (the statistic is constant)."""
    w = po.log_normalize(np.asarray(logw, dtype=np.float64))
    N = w.shape[0]
    s2, s3 = np.sum(w ** 2), np.sum(w ** 3)
    var = s3 - s2 ** 2
    if not var > 1e-12 * s2 ** 2:
        return None
    return float((np.mean(w[np.asarray(anc)]) - s2) / np.sqrt(var / N))


def ancestor_law_score(all_logw, all_anc):
    """|sum_t Z_t| / sqrt(#steps) over the steps whose weights vary: below 5 for multinomial ancestors (it is |N(0, 1)|),
    and it grows like sqrt(#steps) times the per-step bias when the ancestors are shifted against the weights."""
    zs = [ancestor_law_z(all_logw[t], all_anc[t]) for t in range(len(all_anc))]
    zs = [z for z in zs if z is not None]
    assert zs, "no step with varying weights"
    return abs(float(np.sum(zs))) / np.sqrt(len(zs)), len(zs)
