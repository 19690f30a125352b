"""The predictive statistic (stat='predictive', PFG_STAT_PREDICTIVE: pf_mem_kernel's predictive branch) restated on a
TRACE, in np.longdouble.

The statistic is a function of the traced particles x_{t+1}, the traced log-weights and the lead normals alone:
  per particle and lead k   a_ik = w_t log Pr(y_{t+k} | x_{t+1,i})      oracle.pf_oracle.predictive_statistic, restated
                                                                         here in long double (svm/helper.py:352-395,
                                                                         lgssm/helper.py:1281-1336, garch/helper.py:374-412)
  per step                  stats_k += max_i a_ik + log sum_{i,k} W_i exp(a_ik - max_i a_ik)      pf.py:72-76, as
                                                                         oracle/pf_oracle.py states it: ONE sum over leads
                                                                         and particles, W = log_normalize(logw_{t+1})
with a_ik = 0 outside the window [t1, tL) and for leads past the series (t + k >= T): such a column has maximum 0 and
adds one unit to the sum, so a step outside the window adds log(K + 1) to every column.

LGSSM draws no lead normals; SVM's normal of lead 0 is multiplied by sqrt(0); GARCH's normal of lead k only moves the
state lead k + 1 is evaluated at.  So `pred_normals=None` is complete for LGSSM at any K and for every model at K = 0:
a traced device-generator launch then fixes the statistic to rounding (tests/test_gpu_predictive.py, section C).

`mutate` swaps in one deliberate error of the fold -- the ways a kernel's fold can be subtly wrong -- and is used by
tests/test_predictive_model_host.py alone, to show that the case list would notice each of them."""
import numpy as np

from oracle import pf_oracle as po

LD = np.longdouble
MUTATIONS = ("drop_unit_terms", "previous_weights", "one_maximum")
F32_UNIT = 2.0 ** -20           # eight f32 ulps of the magnitudes that enter a lead term


def _derived(model, theta):
    """po.derived in long double (scalars)."""
    th = dict(zip(po.THETA_NAMES[model], [LD(float(v)) for v in theta]))
    d = {"Rinv": th["LRinv"] * th["LRinv"] + LD(1e-16)}
    d["R"] = 1 / d["Rinv"]
    if model in ("svm", "lgssm"):
        d["A"] = th["A"]
        d["C"] = th.get("C", LD(1))
        d["Q"] = 1 / (th["LQinv"] * th["LQinv"] + LD(1e-16))
    else:
        expit = lambda v: 1 / (1 + np.exp(-v))
        mu, phi, lam = np.exp(th["log_mu"]), expit(th["logit_phi"]), expit(th["logit_lambduh"])
        d["alpha"], d["beta"], d["gamma"] = mu * (1 - phi), phi * lam, phi * (1 - lam)
    return d


def lead_terms(model, d, x_next, t, y, K, normals):
    """po.predictive_statistic in long double -> (a [N, K+1], leads evaluated, magnitude): a_ik = log Pr(y_{t+k} | x_next_i)
    for the leads with t + k < T, 0 past them; magnitude = max_{i,k} (|quadratic term| + |c0| + |log term|).
    `normals(k)`: the N lead normals of lead k, or None where they cannot matter (see the module docstring)."""
    x_next = np.asarray(x_next, dtype=LD)
    N, T = x_next.shape[0], y.shape[0]
    out = np.zeros((N, K + 1), dtype=LD)
    c0 = LD(-0.5) * np.log(2 * LD(np.pi))
    nact = min(K + 1, T - t)
    magnitude = LD(0)

    def need(k):
        z = normals(k) if normals is not None else None
        if z is None:
            raise ValueError("{0}: lead {1} of K = {2} needs its normals".format(model, k, K))
        return np.asarray(z, dtype=LD).reshape(N)

    mean, cov = x_next[:, 0].copy(), LD(0)
    s2 = x_next[:, 1].copy() if model == "garch" else None
    for k in range(nact):
        yk = LD(float(y[t + k]))
        if model == "svm":
            x_mc = mean if k == 0 and normals is None else mean + np.sqrt(cov) * need(k)
            ypc = d["R"] * np.exp(x_mc)
            quad, logt = LD(-0.5) * yk * yk / ypc, LD(-0.5) * np.log(ypc)
            mean, cov = d["A"] * mean, d["Q"] + d["A"] * d["A"] * cov
        elif model == "lgssm":
            diff = yk - mean * d["C"]
            ypc = d["R"] + d["C"] * cov * d["C"]
            quad, logt = LD(-0.5) * diff * diff / ypc, LD(-0.5) * np.log(ypc) * np.ones(N, dtype=LD)
            mean, cov = mean * d["A"], d["Q"] + d["A"] * cov * d["A"]
        else:
            diff = yk - mean
            quad, logt = LD(-0.5) * diff * diff / d["R"], LD(-0.5) * np.log(d["R"]) * np.ones(N, dtype=LD)
            if k + 1 < nact:                            # prior_kernel.rv: only the next lead reads it
                s2 = d["alpha"] + d["beta"] * mean * mean + d["gamma"] * s2
                mean = np.sqrt(s2) * need(k)
        out[:, k] = quad + c0 + logt
        magnitude = max(magnitude, np.max(np.abs(quad) + np.abs(c0) + np.abs(logt)))
    return out, nact, magnitude


def log_normalize(logw):
    """pf.py:374-377 in long double."""
    p = np.exp(np.asarray(logw, dtype=LD) - np.max(logw))
    return p / np.sum(p)


def predictive_from_trace(model, theta, y, all_x, all_logw, t1, tL, weights, K, pred_normals=None, mutate=None):
    """all_x [T+1, N, NS], all_logw [T+1, N] (a launch's or the oracle's trace) -> (statistic [K+1] float64, bound).

    pred_normals: None, or (t, k) -> the N normals of lead k at step t (what po.pf_window takes).
    bound: sum_t w_t max_{i,k}(|quadratic term| + |c0| + |log term|) 2^-20, the error that f32 arithmetic of the lead
    terms and of the exp leaves in an f32 launch replayed from its own trace (max + log(sum) is 1-Lipschitz in the
    maximum norm of a).
    mutate: None or one of MUTATIONS -- 'drop_unit_terms': the columns without a statistic add nothing to the sum;
    'previous_weights': the sum is weighted with logw_t instead of logw_{t+1}; 'one_maximum': one maximum over all leads
    instead of one per lead."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(mutate)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    T = y.shape[0]
    tL = T if tL is None else tL
    all_x = np.asarray(all_x, dtype=np.float64)
    all_logw = np.asarray(all_logw, dtype=np.float64)
    N = all_logw.shape[1]
    all_x = all_x.reshape(T + 1, N, -1)
    d = _derived(model, theta)
    stats = np.zeros(K + 1, dtype=LD)
    bound = LD(0)
    for t in range(T):
        inside = t1 <= t < tL
        add, nact = np.zeros((N, K + 1), dtype=LD), 0
        if inside:
            wt = LD(1.0 if weights is None else float(weights[t - t1]))
            normals = None if pred_normals is None else (lambda k, t=t: pred_normals(t, k))
            add, nact, magnitude = lead_terms(model, d, all_x[t + 1], t, y, K, normals)
            add = add * wt
            bound += wt * magnitude
        W = log_normalize(all_logw[t if mutate == "previous_weights" else t + 1])
        max_add = np.max(add, axis=0)
        if mutate == "one_maximum":
            max_add = np.full(K + 1, np.max(add), dtype=LD)
        cols = slice(0, nact) if mutate == "drop_unit_terms" else slice(0, K + 1)
        with np.errstate(divide="ignore"):
            stats = stats + max_add + np.log(np.sum(np.exp(add[:, cols] - max_add[cols]) * W[:, None]))
    return np.asarray(stats, dtype=np.float64), float(bound * F32_UNIT)


def tie_margin(all_logw, u):
    """The smallest |u[t, i] - cdf_t[j]| over the two CDF entries that bracket child i's uniform -- the neighbours of its
    ancestor --, with cdf_t the particle-order CDF of all_logw[t] as po.particle_order_ancestors restates pf_mem_kernel's."""
    return min([float(np.min(po.particle_order_ancestors(all_logw[t], u[t])[1])) for t in range(u.shape[0])], default=np.inf)
