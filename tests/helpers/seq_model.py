"""Host restatement of the reweight kernel of SMC^2 over resident PMMH chains (csrc/pfg_seq.hip; sgmcmc_ssm_amd/sequential.py),
NumPy long double, test-only.  Built on smc_model.py (the stage uniform, the systematic parents) and keyed_draws.py.

  reweight     one stage's population arithmetic: the evidence increment, the ESS, the trigger, the parents, the new logw
  cases        the weight patterns the GPU test runs, each with the smallest distance of a child's target to a CDF entry
"""
import numpy as np

import smc_model as sm
from keyed_draws import LD

NO_FINITE, NOT_A_NUMBER, BAD_B = 1, 2, 4
MIN_B, MAX_B = 2, 1 << 20
MIN_GAP = 1e-9          # every case the parents are compared on keeps its targets this far (relative to W) from the CDF


def reweight(logw, incr, tau, u):
    """logw, incr [B] (any float type; evaluated in long double) -> dict(status; and for status 0: increment, ess, resampled,
    vmax, W, cdf, parent, gap (None unless resampled), logw the new log-weights)."""
    logw, incr = np.asarray(logw, dtype=float).astype(LD), np.asarray(incr, dtype=float).astype(LD)
    B = logw.shape[0]
    if not MIN_B <= B <= MAX_B:
        return dict(status=BAD_B)
    if np.any(np.isnan(logw) | np.isposinf(logw) | np.isnan(incr) | np.isposinf(incr)):
        return dict(status=NOT_A_NUMBER)
    if not np.any(np.isfinite(logw)):
        return dict(status=NO_FINITE)
    lmax = logw.max()
    dead = np.isneginf(logw) | np.isneginf(incr)
    with np.errstate(invalid="ignore"):
        v = np.where(dead, LD(-np.inf), (logw - lmax) + incr)
    if not np.any(np.isfinite(v)):
        return dict(status=NO_FINITE)
    vmax = v.max()
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(dead, LD(0.0), np.exp(v - vmax))
        w0 = np.where(np.isneginf(logw), LD(0.0), np.exp(logw - lmax))
    cdf = np.cumsum(w)
    W = cdf[-1]
    ess = (W * W) / (w * w).sum()
    resampled = bool(ess < LD(tau) * LD(B))
    out = dict(status=0, increment=vmax + np.log(W / w0.sum()), ess=ess, resampled=resampled, vmax=vmax, W=W, cdf=cdf, weights=w)
    if resampled:
        out["parent"], out["gap"] = sm.systematic_parents(cdf, u)
        out["logw"] = np.zeros(B, dtype=LD)
    else:
        out["parent"], out["gap"] = np.arange(B, dtype=np.int64), None
        with np.errstate(invalid="ignore"):
            out["logw"] = np.where(dead, LD(-np.inf), v - vmax)
    return out


def normalised(logw):
    logw = np.asarray(logw).astype(LD)
    w = np.where(np.isneginf(logw), LD(0.0), np.exp(logw - logw[np.isfinite(logw)].max()))
    return w / w.sum()


PATTERNS = ("random", "equal", "one_minus_inf", "all_but_one_minus_inf", "below_target", "above_target")


def case(B, pattern):
    """(logw [B], incr [B], tau) of one weight pattern.  random: a spread that resamples at tau = 0.5 (B = 2: one side only);
    equal: the same incr everywhere on non-uniform weights; one_minus_inf / all_but_one_minus_inf: degenerate estimates;
    below_target / above_target: the same weights with tau just above and just below ESS / B."""
    rng = np.random.default_rng([B, PATTERNS.index(pattern), 0x5E02])
    logw = rng.normal(scale=0.7, size=B) - 3.0
    incr = rng.normal(scale=2.0, size=B) - 55.0
    tau = 0.5
    if pattern == "equal":
        incr = np.full(B, -41.25)
        tau = 1e-9
    elif pattern == "one_minus_inf":
        incr[B // 2] = -np.inf
    elif pattern == "all_but_one_minus_inf":
        keep = (2 * B) // 3
        incr[np.arange(B) != keep] = -np.inf
    elif pattern in ("below_target", "above_target"):
        r = reweight(logw, incr, 0.5, 0.5)
        frac = float(r["ess"]) / B
        tau = min(frac * 1.01, 1.0 - 1e-12) if pattern == "below_target" else frac * 0.99
    return logw, incr, tau


def move_off_the_cdf(logw, incr, tau, u, attempts=50):
    """The case with incr nudged until every child's target keeps MIN_GAP * W from the CDF entries (None if the case does not
    resample): the parents are then the same in double and long double, and no child has to be left out."""
    rng = np.random.default_rng(len(logw))
    for _ in range(attempts):
        r = reweight(logw, incr, tau, u)
        if r["status"] or not r["resampled"] or r["gap"].min() > MIN_GAP:
            return logw, incr, r
        live = np.isfinite(incr)
        incr = np.where(live, incr + rng.normal(scale=1e-3, size=len(incr)), incr)
    raise AssertionError("no input with targets off the CDF found")
