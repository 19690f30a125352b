"""Host restatement of the particle-MALA update rule of resident chains (pfg_pmala_propose_device,
pfg_pmala_accept_device; csrc/pfg_chains.hip), NumPy, test-only.  Built on keyed_draws.py (the Philox mirror, the prior
gradient of sgld_update_kernel) and pmmh_model.py (the support, the log-prior, the counter and seed conventions).

With s the proposal scales, g a score estimate in SCORE-COLUMN order (out[0..3] of a launch, verbatim) and
    d_j(theta, g) = grad_logprior_j(theta) + g_[column of j]
the rule of one chain and step is

    propose  theta'_j = theta_j + (s_j^2 / 2) d_j(theta, g_cur) + s_j z_j           (LGSSM: C stays 1, no normal)
    log q(b | a, g) = -sum_j (b_j - a_j - (s_j^2 / 2) d_j(a, g))^2 / (2 s_j^2)      (over the coordinates that move)
    log alpha = (ll' + logprior(theta')) - (ll + logprior(theta)) + log q(theta | theta', g') - log q(theta' | theta, g)

evaluated in np.longdouble; the draws are regenerated from the keys the kernel header documents: PMMH's counter layout
under the tags 0x4D4C0001 / 0x4D4C0002 (two normal pairs: z0, z1 and z2, z3) and 0x4D4C0003 (the accept uniform), PMMH's
slot assignment.  `hy` is the pfg_prior_hyper of the prior (ensemble.prior_hyper) or a dict of its fields."""
import numpy as np

import keyed_draws as kd
import pmmh_model as pm
from keyed_draws import LD, TOL_ULPS, ULP, normal_pair, uniform53

TAG_Z01, TAG_Z23, TAG_U = 0x4D4C0001, 0x4D4C0002, 0x4D4C0003
P_DIM, Z_SLOT, A_MAX = pm.P_DIM, pm.Z_SLOT, pm.A_MAX
SCORE_COL = kd.SCORE_COL            # score column of each theta slot
# the theta slots a proposal moves, and the score columns the drift reads
FREE = {"svm": (0, 1, 2), "lgssm": (0, 2, 3), "garch": (0, 1, 2, 3)}
USED_COLS = {m: tuple(sorted(SCORE_COL[m][j] for j in FREE[m])) for m in FREE}
update_seed, step_counter, in_support, logprior = pm.update_seed, pm.step_counter, pm.in_support, pm.logprior


def proposal_normals(C, seed, chain_offset, ctr):
    """[C, 4] long-double normals z0..z3 of the counter value `ctr`."""
    r0, r1 = pm._draw(C, seed, chain_offset, ctr, TAG_Z01), pm._draw(C, seed, chain_offset, ctr, TAG_Z23)
    z0, z1 = normal_pair(r0[0], r0[1])
    z2, z3 = normal_pair(r1[0], r1[1])
    return np.column_stack([z0, z1, z2, z3])


def accept_uniform(C, seed, chain_offset, ctr):
    """[C] long-double uniforms in (0, 1) (exact: 53 bits)."""
    r = pm._draw(C, seed, chain_offset, ctr, TAG_U)
    return uniform53(r[0], r[1])


def _scale(model, scale):
    P = P_DIM[model]
    sc = np.asarray(scale, dtype=float).reshape(-1)
    return (np.full(P, sc[0]) if sc.size == 1 else sc[:P]).astype(LD)       # a scalar: every coordinate


def drift(model, theta, grad, hy):
    """d [C, P] (theta order; 0 where the coordinate does not move) and the sum of the absolute values of its terms."""
    P = P_DIM[model]
    th = np.asarray(theta)[:, :P].astype(LD)
    g = np.asarray(grad, dtype=float)[:, list(SCORE_COL[model])].astype(LD)
    gp, gmag = kd.prior_gradient(model, th, kd._hy(hy))
    d, mag = gp + g, gmag + np.abs(g)
    fixed = [j for j in range(P) if j not in FREE[model]]
    d[:, fixed], mag[:, fixed] = 0.0, 0.0
    return d, mag


def proposal_mean(model, theta, grad, scale, hy):
    """a_j + (s_j^2 / 2) d_j(a, g) [C, P] and the magnitude of its terms."""
    P = P_DIM[model]
    th, sc = np.asarray(theta)[:, :P].astype(LD), _scale(model, scale)
    d, dmag = drift(model, th, grad, hy)
    h = LD(0.5) * (sc * sc)
    return th + h * d, np.abs(th) + h * dmag


class Proposal(pm.Proposal):
    """pmmh_model.Proposal of the Langevin proposal."""


def propose(model, theta, grad, scale, seed, chain_offset, ctr, hy):
    """pmala_propose_kernel of C chains: theta [C, >= P] and grad [C, >= 4] (score columns) as the kernel reads them
    (double), scale a scalar or [>= P].  tol: TOL_ULPS ulps of the terms' magnitudes; amb: the support test lies within
    tol of an edge."""
    P = P_DIM[model]
    th = np.asarray(theta, dtype=float)[:, :P].astype(LD)
    sc = _scale(model, scale)
    C = th.shape[0]
    z = proposal_normals(C, seed, chain_offset, ctr)
    mean, mag = proposal_mean(model, th, grad, scale, hy)
    raw = th.copy()
    for j, k in enumerate(Z_SLOT[model]):
        if k is None:
            raw[:, j], mag[:, j] = 1.0, np.abs(th[:, j])
            continue
        raw[:, j] = mean[:, j] + sc[j] * z[:, k]
        mag[:, j] = mag[:, j] + np.abs(sc[j] * z[:, k])
    tol = TOL_ULPS * ULP * mag
    valid = in_support(model, raw)
    amb = np.zeros(C, bool)
    if model != "garch":
        amb |= np.abs(np.abs(raw[:, 0]) - LD(A_MAX)) <= tol[:, 0]
        chol = (P - 2, P - 1)
    else:
        chol = (3,)
    for j in chol:
        amb |= np.abs(raw[:, j]) <= tol[:, j]
    prop = np.where(valid[:, None], raw, th)
    return Proposal(prop, valid, tol, amb, raw)


def log_q(model, b, a, grad_a, scale, hy):
    """[C] long double: log q(b | a, g_a) less the constant of the scales."""
    P = P_DIM[model]
    b = np.asarray(b)[:, :P].astype(LD)
    sc = _scale(model, scale)
    mean, _ = proposal_mean(model, a, grad_a, scale, hy)
    q = np.zeros(b.shape[0], dtype=LD)
    for j in FREE[model]:
        r = b[:, j] - mean[:, j]
        q = q + (r * r) / (LD(2) * (sc[j] * sc[j]))
    return -q


def log_alpha(model, prior, hy, scale, theta, theta_prop, ll_cur, ll_prop, g_cur, g_prop):
    """[C] long double: the acceptance ratio of the move theta -> theta_prop (see the module docstring)."""
    lp_c, lp_p = logprior(model, prior, theta).astype(LD), logprior(model, prior, theta_prop).astype(LD)
    target = (np.asarray(ll_prop, dtype=float).astype(LD) + lp_p) - (np.asarray(ll_cur, dtype=float).astype(LD) + lp_c)
    return (target + log_q(model, theta, theta_prop, g_prop, scale, hy)) - log_q(model, theta_prop, theta, g_cur, scale, hy)


def accept(model, prior, hy, scale, theta, theta_prop, valid, ll_cur, ll_prop, g_cur, g_prop, seed, chain_offset, ctr):
    """pmala_accept_kernel's decision of C chains -> (accepted [C] bool, margin [C] = |log u - log alpha|, inf where the
    decision does not depend on the comparison: an invalid proposal, or an estimate (ll_prop, a used component of
    g_prop) that is not finite)."""
    theta, theta_prop = np.asarray(theta, dtype=float), np.asarray(theta_prop, dtype=float)
    g_cur, g_prop = np.asarray(g_cur, dtype=float), np.asarray(g_prop, dtype=float)
    C = theta.shape[0]
    llp = np.asarray(ll_prop, dtype=float)
    live = np.asarray(valid).astype(bool) & np.isfinite(llp) & np.all(np.isfinite(g_prop[:, list(USED_COLS[model])]), axis=1)
    la = np.full(C, np.nan, dtype=LD)
    if live.any():
        with np.errstate(all="ignore"):
            la[live] = log_alpha(model, prior, hy, scale, theta[live], theta_prop[live], np.asarray(ll_cur, dtype=float)[live],
                                 llp[live], g_cur[live], g_prop[live])
    logu = np.log(accept_uniform(C, seed, chain_offset, ctr))
    with np.errstate(invalid="ignore"):
        acc = live & (logu < la)            # a NaN log alpha rejects
        margin = np.where(live & ~np.isnan(la), np.abs(logu - la), np.inf)
    return acc, margin.astype(float)


def run_chains(model, prior, hy, theta0, scale, loglik_and_score, seed, chain_offset, steps, first_step=0,
               force_invalid=False):
    """The whole rule on the host: C chains from theta0 [C, P], `steps` steps; loglik_and_score(theta_prop [C, P] double,
    ctr) -> (ll [C], g [C, 4] in score columns), the estimates of the launch at counter ctr (the init pass calls it with
    ctr 0).  Returns (theta [C, P], ll [C], g [C, 4], n_accept [C], trace of theta [steps, C, P]).  force_invalid: every
    proposal is treated as outside the support."""
    P = P_DIM[model]
    th = np.array(theta0, dtype=float)[:, :P].copy()
    C = th.shape[0]
    ll, g = loglik_and_score(th.copy(), 0)
    ll, g = np.asarray(ll, dtype=float).copy(), np.asarray(g, dtype=float).copy()
    n_acc = np.zeros(C, dtype=np.int64)
    trace = np.zeros((steps, C, P))
    useed = update_seed(seed)
    for s in range(first_step, first_step + steps):
        ctr = step_counter(s)
        pr = propose(model, th, g, scale, useed, chain_offset, ctr, hy)
        valid = pr.valid & (not force_invalid)
        prop = np.where(valid[:, None], pr.raw, th.astype(LD)).astype(float)
        llp, gp = loglik_and_score(prop.copy(), ctr)
        llp, gp = np.asarray(llp, dtype=float), np.asarray(gp, dtype=float)
        acc, _ = accept(model, prior, hy, scale, th, prop, valid, ll, llp, g, gp, useed, chain_offset, ctr)
        th[acc], ll[acc], g[acc] = prop[acc], llp[acc], gp[acc]
        n_acc += acc
        trace[s - first_step] = th
    return th, ll, g, n_acc, trace
