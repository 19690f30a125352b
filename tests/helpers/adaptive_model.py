"""ESS-triggered ("adaptive") resampling (PFG_FLAG_ADAPTIVE_RESAMPLING, ess_threshold=tau) restated on the pinned CPU oracle.

At timestep t, with p = log_normalize(logw) and S = sum_i p_i stats_i from the CURRENT weights (as always):

    ESS < tau N:  anc = the multinomial draw of the oracle on p with u[t];  base = 0
    otherwise:    anc = arange(N);  base_i = (logw_i - m) - log(sum_j exp(logw_j - m)) + log(N),  m = max(logw)
    x_next, new_logw, add from parents = x[anc] exactly as the oracle;  stats = lambduh stats[anc] + (1 - lambduh) S + add
    logw = base + new_logw;  inside the window: loglik += weight_t log(mean(exp(logw)))

The decision is (sum w)^2 < tau N sum w^2 in fp64 with w = exp(logw - m); `base` lives in the log domain, so a particle whose
weight underflows keeps a finite log-weight.  With `always=True` every step resamples with base = 0: `oracle.pf_oracle.pf_window`
bit for bit (tests/test_adaptive_host.py).  The DEVICE instantiations record the uniform every child searched with (rec_ud);
their CDF layouts are restated by `device_ancestors` below."""
import numpy as np

from oracle import pf_oracle as po

# CDF slots of the DEVICE instantiations, by variant name (pfg_last_variant)
SLOTS = {"adaptive256x4": 1024, "big4096_adaptive": 4096, "big16384_adaptive": 16384}


def ess_decision(logw, tau):
    """(resample?, ESS) of one step: the fp64 rule (sum w)^2 < tau N sum w^2 with w = exp(logw - max logw)."""
    N = logw.shape[0]
    w = np.exp(logw - np.max(logw))
    s1, s2 = np.sum(w), np.sum(w * w)
    return bool(s1 * s1 < (tau * N) * s2), s1 * s1 / s2


def carried_base(logw):
    """The log-weights a step that keeps its particles carries on: log(N p_i), computed in the log domain."""
    m = np.max(logw)
    return ((logw - m) - np.log(np.sum(np.exp(logw - m)))) + np.log(logw.shape[0])


def pf_window(model, theta, y, N, z0, u, z, ess_threshold, always=False, resampler=None, decisions=None, kernel=None,
              pf="poyiadjis_N", lambduh=None, stat="score", t1=0, tL=None, weights=None, prior_mean=0.0, prior_var=1.0,
              save_all=True):
    """One buffered window with adaptive resampling, built from the oracle's pieces.  Returns the keys of
    po.pf_window(save_all=True) plus `resampled` [T] (bool), `ess` [T] and `margin` = min_t |ESS_t - tau N| / N.

    always: resample at every step (base = 0): po.pf_window.  resampler: (t, logw) -> ancestors of a step that resamples
    (DEVICE launches: `device_ancestors` on the recorded uniforms; u is then unused).  decisions: [T] bools that replace
    the rule (teacher forcing on a launch's own decisions)."""
    y = np.asarray(y, dtype=float).reshape(-1, 1)
    T = y.shape[0]
    tL = T if tL is None else tL
    kernel = po.DEFAULT_KERNEL[model] if kernel is None else kernel
    if pf == "poyiadjis_N":
        lambduh = 1.0
    elif pf == "nemeth":
        lambduh = 0.95 if lambduh is None else lambduh
    else:
        raise NotImplementedError("adaptive resampling is built for pf = 'poyiadjis_N' | 'nemeth'")
    if stat not in ("score", "suff", "none"):
        raise NotImplementedError("adaptive resampling is built for the score, sufficient or no statistic")
    d = po.derived(model, theta)
    h = 3 if stat == "none" else po.STAT_DIM[(model, stat)]
    x = po.sample_x0(model, prior_mean, prior_var, z0)
    logw = np.zeros(N)
    loglik = 0.0
    stats = np.zeros((N, h))
    all_x, all_lw, all_s, all_ll, all_anc = [x], [logw], [stats], [loglik], []
    resampled, ess, margin = np.zeros(T, dtype=bool), np.zeros(T), np.inf
    for t in range(T):
        inside = (t >= t1) and (t < tL)
        weight_t = float(weights[t - t1]) if inside and weights is not None else 1.0
        p = po.log_normalize(logw)
        S = np.sum(stats.T * p, axis=1)
        if always:
            res, ess[t] = True, np.nan
        else:
            res, ess[t] = ess_decision(logw, ess_threshold)
            margin = min(margin, abs(ess[t] - ess_threshold * N) / N)
            if decisions is not None:
                res = bool(decisions[t])
        resampled[t] = res
        if res:
            anc = po.multinomial_ancestors(p, u[t]) if resampler is None else resampler(t, logw)
            base = np.zeros(N)
        else:
            anc, base = np.arange(N), carried_base(logw)
        parents = x[anc]
        x_next = po.kernel_rv(model, kernel, d, parents, y[t], z[t])
        new_logw = po.kernel_reweight(model, kernel, d, parents, x_next, y[t])
        if inside and stat == "score":
            add = po.score_statistic(model, d, parents, x_next, y[t])
        elif inside and stat == "suff":
            add = po.sufficient_statistic(model, parents, x_next)
        else:
            add = np.zeros((N, h))
        add = add * weight_t
        stats = (lambduh * stats[anc] + (1.0 - lambduh) * np.outer(np.ones(N), S) + add)
        x, logw = x_next, base + new_logw
        if inside:
            loglik += weight_t * np.log(np.mean(np.exp(logw)))
        all_x.append(x); all_lw.append(logw); all_s.append(stats); all_ll.append(loglik); all_anc.append(anc)
    out = dict(x_t=x, log_weights=logw, statistics=stats, loglikelihood_estimate=loglik,
               mean_statistic=np.sum(stats.T * po.log_normalize(logw), axis=1), resampled=resampled, ess=ess, margin=margin)
    if save_all:
        out.update(all_x_t=np.array(all_x), all_log_weights=np.array(all_lw), all_statistics=np.array(all_s),
                   all_loglikelihood_estimate=np.array(all_ll), all_ancestors=np.array(all_anc, dtype=int).reshape(-1, N))
    return out


def device_ancestors(logw, ud, variant):
    """Ancestors of a step that resamples as the adaptive DEVICE instantiations lay the search out, from the uniforms the
    launch recorded.  All three keep the CDF in PARTICLE order (slot i <-> particle i: the 256 x 4 instantiation is not the
    thread-major layout of the plain multinomial unit; the large-N twins are pf_big_kernel's, sorted uniforms included),
    fp64 entries cs / W over `SLOTS[variant]` slots, slots >= N weighing nothing, against the uniform itself."""
    return po.device_ancestors(logw, ud, SLOTS[variant], 1, "f64_uniform")


def run_windows(problems, ctx=None, want_final=False):
    """Stand-in for particle_filters.run_windows on the CPU: tests/oracle_backend.run_windows_oracle, with the windows
    that carry `ess_threshold` evaluated by `pf_window` above."""
    from oracle_backend import run_windows_oracle
    outs = []
    for q in problems:
        tau = q.get("ess_threshold", None)
        if not tau:
            outs.extend(run_windows_oracle([q], ctx, want_final))
            continue
        if q["rng"] != "replay" or q["smoother"] != "nemeth":
            raise ValueError("the stand-in replays host streams of NEMETH windows")
        outs.append(pf_window(q["model"], q["theta"], q["y"], q["N"], q["z0"], q["u"], q["z"], tau, kernel=q["kernel"],
                              pf="nemeth", lambduh=q["lambduh"], stat=q["stat"], t1=q["t1"], tL=q["tL"], weights=q["weights"],
                              prior_mean=q["prior_mean"], prior_var=q["prior_var"], save_all=False))
    return outs
