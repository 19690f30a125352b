"""One step of a Poyiadjis O(N^2) window recomputed from a launch's own trace (teacher-forced), and the law of a step's
ancestors -- for units that record no normals or no resampling words.

`forced_steps` takes the traced particles, log-weights, statistics and ancestors of a window and recomputes, for every step
t, what step t + 1 must hold given step t AS TRACED: the log-weights with po.kernel_reweight on (x_t[anc_t], x_{t+1}), and
the statistics with the reference's O(N^2) recursion (pf.py:84-136: every child averages stats_j + weight_t h(x_j, child)
over ALL parents j with the backward weights log_normalize(logw_t + prior_log_density(x_j -> child))), through
po.prior_log_density, po.log_normalize, po.score_statistic and po.sufficient_statistic.  Plain NumPy in float64, one step
at a time; nothing of one recomputed step enters the next.  The proposal itself (x_{t+1} from its normal) is NOT checked
here: that needs the recorded normals.

`ancestor_law_z` is a z-score of one resampling step against the multinomial law.  `ancestors_against_restatement` derives the
ancestors of a unit that does record its resampling uniforms (pf_mem_kernel on the device generator) and counts the
children that differ, inside and outside the exemption for uniforms that sit on a CDF entry.

`forced_paris_steps` is the same for a PaRIS window (pf.py:183-258): the statistics of step t + 1 are the reference's rewiring
mean_j(stats_t[J_ij] + weight_t h(x_t[J_ij], x_{t+1}[i])) over the Ntilde backward-sampled parents J the launch traced.
The parents themselves cannot be recomputed without the launch's uniforms; `backward_law_scores` tests their LAW: given the
traced particles and log-weights every J_ij is an independent draw from the exact backward law of child i, whether it left
an accept-reject round or the categorical fallback."""
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


def ancestors_against_restatement(all_logw, ud, all_anc, gap_tol=1e-10):
    """The traced ancestors of pf_mem_kernel's device-generator units against po.particle_order_ancestors on the traced
    log-weights of step t and the uniforms the launch recorded (ud [T, N]) -> (wrong, exempt, flips).

    exempt: children whose uniform lies within gap_tol of a CDF entry -- the device's weights go through its fast exp (below
    3e-12 relative) and its sum is a wave scan plus offsets, so such a child may take either neighbour.  wrong: children
    outside the exemption whose traced ancestor is not the restatement's, plus exempt ones further than one neighbour away.
    flips: all children whose traced ancestor differs, exempt or not."""
    wrong = exempt = flips = 0
    for t in range(len(all_anc)):
        ref, gap = po.particle_order_ancestors(all_logw[t], ud[t])
        got = np.asarray(all_anc[t])
        ex = gap < gap_tol
        exempt += int(np.sum(ex))
        wrong += int(np.sum((got != ref) & ~ex)) + int(np.sum(np.abs(got - ref)[ex] > 1))
        flips += int(np.sum(got != ref))
    return wrong, exempt, flips


def recorded_draws_are_sound(o, T, N):
    """What every traced device-generator launch of pf_mem_kernel must have recorded: finite normals, no row of them all
    zero; uniforms in (0, 1) that are (word + 0.5) / 2^32 of a 32-bit word."""
    z, z0, ud = o["rec_z"], o["rec_z0"], o["rec_ud"]
    assert z.shape == (T, N) and z0.shape == (N,) and ud.shape == (T, N)
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(z0))
    assert np.all(np.any(z != 0.0, axis=1)) and np.any(z0 != 0.0)
    assert np.all(ud > 0.0) and np.all(ud < 1.0)
    words = ud * 4294967296.0 - 0.5
    assert np.all(words == np.round(words))
    return True


def forced_paris_step(model, kernel, d, x, logw, stats, anc, J, x_next, y_t, stat, inside, weight_t):
    """(log-weights, statistics [N, h], log-likelihood increment) of step t + 1 of a PaRIS window from the traced step t.

    As forced_step, with J [N, Ntilde]: the backward-sampled parents of every child (row i: child i).  The rewiring reads
    the parents' particles and statistics, not their log-weights: logw is taken for symmetry with forced_step only."""
    x, x_next = np.asarray(x, dtype=np.float64), np.asarray(x_next, dtype=np.float64)
    stats = np.asarray(stats, dtype=np.float64)
    N, h = stats.shape
    J = np.asarray(J).reshape(N, -1)
    Ntilde = J.shape[1]
    y_t = np.asarray(y_t, dtype=np.float64).reshape(1)
    new_logw = po.kernel_reweight(model, kernel, d, x[np.asarray(anc)], x_next, y_t)
    flat = J.reshape(-1)                        # row i * Ntilde + j: child i, draw j
    child = np.repeat(np.arange(N), Ntilde)
    if inside and stat == "score":
        add = po.score_statistic(model, d, x[flat], x_next[child], y_t)
    elif inside and stat == "suff":
        add = po.sufficient_statistic(model, x[flat], x_next[child])
    else:
        add = np.zeros((N * Ntilde, h))
    add = add[:, :h] * float(weight_t)
    new_stats = np.mean(np.reshape(stats[flat] + add, (N, Ntilde, h)), axis=1)
    dll = float(weight_t) * np.log(np.mean(np.exp(new_logw))) if inside else 0.0
    return new_logw, new_stats, dll


def forced_paris_steps(model, kernel, theta, y, all_x, all_logw, all_stats, all_anc, all_J, stat="score", t1=0, tL=None,
                       weights=None):
    """forced_paris_step for t = 0 .. T - 1 on a PaRIS window's trace (as forced_steps; all_J [T, N, Ntilde]) ->
    (log-weights [T, N], statistics [T, N, h], log-likelihood increments [T]); entry t is what the trace must hold at
    t + 1.  Every step starts from the trace: nothing of one recomputed step enters the next."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    T = y.shape[0]
    tL = T if tL is None else tL
    d = po.derived(model, theta)
    lws, sts, dlls = [], [], []
    for t in range(T):
        inside = t1 <= t < tL
        wt = float(weights[t - t1]) if inside and weights is not None else 1.0
        lw, st, dll = forced_paris_step(model, kernel, d, all_x[t], all_logw[t], all_stats[t], all_anc[t], all_J[t],
                                        all_x[t + 1], y[t], stat, inside, wt)
        lws.append(lw); sts.append(st); dlls.append(dll)
    return np.array(lws), np.array(sts), np.array(dlls)


def backward_law(model, d, x, logw, x_next):
    """beta [N children, N parents]: row i is the exact backward law of child i,
    log_normalize(logw + prior_log_density(x -> x_next[i])) (pf.py:226-236, :329-338)."""
    x, x_next = np.asarray(x, dtype=np.float64), np.asarray(x_next, dtype=np.float64)
    logw = np.asarray(logw, dtype=np.float64)
    N = x.shape[0]
    parent = np.tile(np.arange(N), N)           # row i * N + k: child i, parent k
    child = np.repeat(np.arange(N), N)
    lb = logw[None, :] + np.reshape(po.prior_log_density(model, d, x[parent], x_next[child]), (N, N))
    b = np.exp(lb - np.max(lb, axis=1, keepdims=True))
    return b / np.sum(b, axis=1, keepdims=True)


def backward_law_scores(model, d, all_x, all_logw, all_J):
    """(Z_p, Z_x, #terms) of a PaRIS trace against the exact backward law; all_J [T, N, Ntilde].

    Given the traced particles and log-weights, J_ij of step t is a draw from beta_i = backward_law(...)[i], independent
    over (t, i, j).  With f(k) = beta_i(k), f(J) has mean sum_k beta_i(k)^2 and variance sum beta^3 - (sum beta^2)^2; with
    f(k) = x_t[k, 0] -- the conditional mean the score is carried through -- the mean is sum_k beta_i(k) x_t[k, 0] and the
    variance Var_beta(x).  The centred sums over all (t, j, i), divided by the root of the summed variances,
        Z_p = sum (beta_i[J] - sum_k beta_i(k)^2) / sqrt(sum (sum beta^3 - (sum beta^2)^2))
        Z_x = sum (x_t[J, 0] - sum_k beta_i(k) x_t[k, 0]) / sqrt(sum Var_beta(x))
    are asymptotically N(0, 1).  A term whose variance vanishes in either sum (beta_i uniform or a point mass, all
    parents equal) is constant and enters neither; #terms counts the rest."""
    all_J = np.asarray(all_J)
    T, N, Ntilde = all_J.shape
    num_p = num_x = var_p = var_x = 0.0
    terms = 0
    for t in range(T):
        beta = backward_law(model, d, all_x[t], all_logw[t], all_x[t + 1])
        xk = np.asarray(all_x[t], dtype=np.float64)[:, 0]
        s2, s3 = np.sum(beta ** 2, axis=1), np.sum(beta ** 3, axis=1)
        vp = s3 - s2 ** 2
        mx = beta @ xk
        vx = beta @ (xk ** 2) - mx ** 2
        ok = (vp > 1e-12 * s2 ** 2) & (vx > 1e-12 * np.maximum(beta @ (xk ** 2), 1e-300))
        rows = np.arange(N)
        for j in range(Ntilde):
            Jj = all_J[t][:, j]
            num_p += np.sum((beta[rows, Jj] - s2)[ok])
            num_x += np.sum((xk[Jj] - mx)[ok])
        var_p += Ntilde * np.sum(vp[ok])
        var_x += Ntilde * np.sum(vx[ok])
        terms += Ntilde * int(np.sum(ok))
    assert terms > 0, "no term with a varying backward law"
    return float(num_p / np.sqrt(var_p)), float(num_x / np.sqrt(var_x)), terms
