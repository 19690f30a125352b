"""The REPLAY cases of the predictive statistic, shared by tests/test_predictive_model_host.py (the helper against the
oracle, the mutations, the tie margins) and tests/test_gpu_predictive.py (pf_mem_kernel's predictive branch against the
oracle).  Every input is generated here from a seed.

A row is (N, T, K, window, outlier).  The N list walks the kernel's edges: one particle, the one-wave sizes 63 / 64 / 65,
the 1024-particle chunk (1023 / 1024 / 1025, 2049, 4096 / 4097), np2 = 8192 against np2 = 16384 (8192 / 8193: the search's
index arithmetic changes there) and the maximum 16384.  K walks 0, 1, 5 and 15 = PFG_MAX_PRED - 1, with K >= T at T = 3
(leads cut off by the end of the series from the first step on).  Windows: 'full'; 'partial' = t1 > 0, tL < T with
importance weights from uniform(0.5, 10); 'empty' = t1 == tL, where every step adds log(K + 1).  `outlier` replaces two
observations by +-40 (x 0.4 for GARCH): one particle carries a column's maximum."""
import numpy as np

from oracle import pf_oracle as po

PAIRS = (("svm", "prior"), ("garch", "prior"), ("garch", "optimal"), ("lgssm", "prior"), ("lgssm", "optimal"))

ROWS = (
    (1, 4, 0, "full", False),
    (1, 3, 15, "partial", False),
    (2, 5, 1, "partial", False),
    (63, 6, 5, "full", False),
    (64, 3, 5, "full", False),
    (65, 3, 15, "partial", False),
    (300, 0, 5, "full", False),
    (1000, 12, 15, "full", False),
    (1000, 8, 0, "full", False),
    (1023, 7, 1, "empty", False),
    (1024, 8, 5, "partial", False),
    (1025, 9, 0, "partial", False),
    (1025, 10, 5, "full", True),
    (2049, 10, 15, "partial", False),
    (4096, 6, 1, "full", False),
    (4097, 11, 5, "partial", False),
    (4097, 3, 15, "full", False),
    (4097, 6, 5, "empty", False),
    (5000, 5, 15, "full", False),
    (5000, 4, 0, "empty", False),
    (8192, 4, 0, "partial", False),
    (8192, 12, 15, "full", False),
    (8193, 12, 1, "partial", False),
    (8193, 5, 15, "full", False),
    (16384, 4, 5, "full", False),
    (16384, 4, 0, "partial", False),
)

# (pair index, row index) -> seed offset: the seeds at which a uniform would land within 1e-10 of a CDF entry are
# stepped over (tests/test_predictive_model_host.py::test_no_near_ties holds every case to that margin)
SEED_STEPS = {(1, 20): 1, (1, 21): 2, (1, 22): 3, (1, 25): 2, (2, 25): 6, (4, 22): 2}

CASES = tuple((p, r) for p in range(len(PAIRS)) for r in range(len(ROWS)))


def case_id(case):
    p, r = case
    N, T, K, window, outlier = ROWS[r]
    return "{0}-{1}-N{2}-T{3}-K{4}-{5}{6}".format(PAIRS[p][0], PAIRS[p][1], N, T, K, window, "-outlier" if outlier else "")


def theta_of(model):
    from test_host_logic import default_params
    return default_params(model).theta()


def window_of(T, window):
    if window == "full" or T == 0:
        return 0, T
    if window == "empty":
        return T // 2, T // 2
    return max(1, T // 4), T - max(1, T // 5)


def problem(model, kernel, N, T, K, window, outlier, seed, dtype="f64"):
    """One REPLAY window as ctx.run_batch takes it (see `reference` for the oracle's run of the same dict)."""
    rs = np.random.RandomState(seed)
    y = rs.normal(size=T) * (0.6 if model == "garch" else 1.5)
    if outlier:
        y[T // 3], y[(2 * T) // 3] = (40.0 * (0.4 if model == "garch" else 1.0)) * np.array([1.0, -1.0])
    t1, tL = window_of(T, window)
    weights = rs.uniform(0.5, 10.0, size=tL - t1) if window == "partial" else None
    z0, u, z = po.draw_streams(rs, N, T)
    pred_z = rs.normal(size=(T, K + 1, N)) if model != "lgssm" else None
    return dict(model=model, kernel=kernel, smoother="filter", stat="predictive", dtype=dtype, rng="replay", N=N, t1=t1,
                tL=tL, prior_mean=-0.2, prior_var=1.3, y=y, weights=weights, theta=theta_of(model), z0=z0, u=u, z=z,
                pred_z=pred_z, num_steps_ahead=K)


def replay_problem(case):
    p, r = case
    model, kernel = PAIRS[p]
    return problem(model, kernel, *ROWS[r], seed=100003 * (p + 1) + 101 * r + 7919 * SEED_STEPS.get(case, 0))


# One launch of six windows that differ in everything a batch shares the sizing of: N (the scratch stride comes from the
# batch's largest N and PFG_MAX_PRED, not from the window's own N and K), K, T, window and weights.
BATCH_ROWS = (
    (200, 5, 0, "partial", False),
    (1025, 8, 15, "full", False),
    (3000, 3, 3, "partial", False),
    (64, 12, 7, "empty", False),
    (4097, 6, 1, "partial", False),
    (1, 4, 10, "full", False),
)


def batch_problems(p):
    model, kernel = PAIRS[p]
    return [problem(model, kernel, *row, seed=200003 * (p + 1) + 211 * b) for b, row in enumerate(BATCH_ROWS)]


def reference(q, stat="predictive", save_all=False):
    """po.pf_window on the problem dict q.  stat='none' gives the same trajectory without the statistic."""
    pz = q["pred_z"]
    with np.errstate(divide="ignore"):          # log(mean(exp(logw))) is -inf where every weight underflows
        return po.pf_window(q["model"], q["theta"], q["y"], q["N"], q["z0"], q["u"], q["z"], kernel=q["kernel"], pf="filter",
                            stat=stat, t1=q["t1"], tL=q["tL"], weights=q["weights"], prior_mean=q["prior_mean"],
                            prior_var=q["prior_var"], num_steps_ahead=q["num_steps_ahead"], save_all=save_all,
                            pred_normals=(lambda t, k: None) if pz is None else (lambda t, k: pz[t, k]))


def reference_loglik(q, ref):
    """The log-likelihood to hold a launch to.  The reference's log(mean(exp(logw))) is not max-stabilised
    (buffered_smoother.py:124-126): where the log-weights of a window step all sit below -600 its exp lands among the
    denormals or at zero and the reference's own value is inexact or -inf.  The kernel's is the max-stabilised form of
    the same sum (deviation (i)); there, that form on the oracle's log-weights is the expected value, as in
    tests/test_gpu_device_replay.py.  ref: reference(q, save_all=True)."""
    T = q["y"].shape[0]
    lw = ref["all_log_weights"][1:]
    steps = np.arange(T)
    inside = (steps >= q["t1"]) & (steps < q["tL"])
    if T == 0 or np.all(lw.max(axis=1)[inside] > -600.0):
        return ref["loglikelihood_estimate"]
    wt = np.zeros(T)
    wt[inside] = 1.0 if q["weights"] is None else q["weights"]
    mx = lw.max(axis=1)
    return float(np.sum(wt * (mx + np.log(np.mean(np.exp(lw - mx[:, None]), axis=1)))))
