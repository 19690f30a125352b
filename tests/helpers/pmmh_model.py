"""Host restatement of the PMMH update rule of resident chains (pfg_pmmh_propose_device, pfg_pmmh_accept_device;
csrc/pfg_chains.hip), NumPy, test-only.

The draws are regenerated from the keys the kernel header documents -- Philox4x32-10, counter {gid_lo, step_lo,
step_hi ^ gid_hi, tag} under (seed_lo, seed_hi), tags 0x504D0001 / 0x504D0002 (two normal pairs: z0, z1 and z2, z3) and
0x504D0003 (the accept uniform, uniform53 of the first two words) -- the update is evaluated in np.longdouble, and the
log-prior is the host's Prior.logprior (base_parameters.py), in the raw coordinates, without Jacobian terms.

The counter: ChainEnsemble's init pass consumes counter value 0, so step s (from 0) of an ensemble draws with s + 1
(`step_counter`); the update kernels are keyed by seed ^ 0x5DEECE66D (`update_seed`), the particle filters by the seed."""
import numpy as np

from keyed_draws import LD, TOL_ULPS, ULP, _hi, _lo, MASK32, chain_ids, normal_pair, philox4x32_10, split_seed, uniform53

TAG_Z01, TAG_Z23, TAG_U = 0x504D0001, 0x504D0002, 0x504D0003
P_DIM = {"svm": 3, "garch": 4, "lgssm": 4}
# which normal moves which theta slot (LGSSM's C takes none: it stays 1)
Z_SLOT = {"svm": (0, 1, 2), "lgssm": (0, None, 2, 3), "garch": (0, 1, 2, 3)}
A_MAX = 0.9999


def update_seed(seed):
    """The seed ChainEnsemble keys its update kernels with."""
    return (int(seed) ^ 0x5DEECE66D) & 0xFFFFFFFFFFFFFFFF


def step_counter(step):
    """The counter value of step `step` (from 0) of an ensemble: the init pass took 0."""
    return int(step) + 1


def _draw(C, seed, chain_offset, ctr, tag):
    gid = chain_ids(C, chain_offset)
    s = int(ctr or 0)
    return philox4x32_10((_lo(gid), s & MASK32, _hi([s]) ^ _hi(gid), tag), split_seed(seed))


def proposal_normals(C, seed, chain_offset, ctr):
    """[C, 4] long-double normals z0..z3 of the counter value `ctr`."""
    r0, r1 = _draw(C, seed, chain_offset, ctr, TAG_Z01), _draw(C, seed, chain_offset, ctr, TAG_Z23)
    z0, z1 = normal_pair(r0[0], r0[1])
    z2, z3 = normal_pair(r1[0], r1[1])
    return np.column_stack([z0, z1, z2, z3])


def accept_uniform(C, seed, chain_offset, ctr):
    """[C] long-double uniforms in (0, 1) (exact: 53 bits)."""
    r = _draw(C, seed, chain_offset, ctr, TAG_U)
    return uniform53(r[0], r[1])


def in_support(model, th):
    """[C] bool: project_parameters leaves the rows of th [C, P] unchanged -- |A| <= 0.9999, every Cholesky factor > 0."""
    th = np.asarray(th)
    ok = np.all(np.isfinite(th.astype(float)), axis=1)
    if model == "garch":
        return ok & (th[:, 3] > 0)
    P = P_DIM[model]
    return ok & (np.abs(th[:, 0]) <= LD(A_MAX)) & (th[:, P - 2] > 0) & (th[:, P - 1] > 0)


class Proposal(object):
    """theta_prop [C, P] (long double; the current theta where invalid), valid [C], tol [C, P] (TOL_ULPS ulps of the
    terms' magnitudes), amb [C]: the support test lies within tol of an edge, either answer is a correct rounding."""

    def __init__(self, theta_prop, valid, tol, amb, raw):
        self.theta_prop, self.valid, self.tol, self.amb, self.raw = theta_prop, valid, tol, amb, raw


def propose(model, theta, scale, seed, chain_offset, ctr):
    """pmmh_propose_kernel of C chains: theta [C, >= P] as the kernel reads it (double), scale a scalar or [>= P]."""
    P = P_DIM[model]
    th = np.asarray(theta, dtype=float)[:, :P].astype(LD)
    sc = np.asarray(scale, dtype=float).reshape(-1)
    sc = (np.full(P, sc[0]) if sc.size == 1 else sc[:P]).astype(LD)       # a scalar: every coordinate
    C = th.shape[0]
    z = proposal_normals(C, seed, chain_offset, ctr)
    raw, mag = th.copy(), np.abs(th)
    for j, k in enumerate(Z_SLOT[model]):
        if k is None:
            raw[:, j] = 1.0
            continue
        raw[:, j] = th[:, j] + sc[j] * z[:, k]
        mag[:, j] = np.abs(th[:, j]) + np.abs(sc[j] * z[:, k])
    tol = TOL_ULPS * ULP * mag
    valid = in_support(model, raw)
    # near an edge: would another correctly rounded value of the components decide the other way?
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


def from_theta(model, th):
    from sgmcmc_ssm_amd.models.svm import SVMParameters
    from sgmcmc_ssm_amd.models.garch import GARCHParameters
    from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters
    th = [float(v) for v in th]
    if model == "svm":
        return SVMParameters(A=np.eye(1) * th[0], LQinv=np.eye(1) * th[1], LRinv=np.eye(1) * th[2])
    if model == "lgssm":
        return LGSSMParameters(A=np.eye(1) * th[0], C=np.eye(1) * th[1], LQinv=np.eye(1) * th[2], LRinv=np.eye(1) * th[3])
    return GARCHParameters(log_mu=th[0], logit_phi=th[1], logit_lambduh=th[2], LRinv=np.eye(1) * th[3])


def logprior(model, prior, theta):
    """[C] Prior.logprior of the raw rows theta [C, >= P] (double: the host function is the specification)."""
    P = P_DIM[model]
    return np.array([prior.logprior(from_theta(model, row[:P])) for row in np.asarray(theta, dtype=float)])


def log_alpha(model, prior, theta, theta_prop, ll_cur, ll_prop):
    """[C] long double: (ll_prop + logprior(theta_prop)) - (ll_cur + logprior(theta))."""
    lp_c, lp_p = logprior(model, prior, theta).astype(LD), logprior(model, prior, theta_prop).astype(LD)
    return (np.asarray(ll_prop, dtype=float).astype(LD) + lp_p) - (np.asarray(ll_cur, dtype=float).astype(LD) + lp_c)


def accept(model, prior, theta, theta_prop, valid, ll_cur, ll_prop, seed, chain_offset, ctr):
    """pmmh_accept_kernel's decision of C chains -> (accepted [C] bool, margin [C] = |log u - log alpha|, inf where the
    decision does not depend on the comparison: an invalid proposal or an estimate that is not finite)."""
    theta, theta_prop = np.asarray(theta, dtype=float), np.asarray(theta_prop, dtype=float)
    C = theta.shape[0]
    valid = np.asarray(valid).astype(bool)
    llp = np.asarray(ll_prop, dtype=float)
    live = valid & np.isfinite(llp)
    la = np.full(C, np.nan, dtype=LD)
    if live.any():
        la[live] = log_alpha(model, prior, theta[live], theta_prop[live], np.asarray(ll_cur, dtype=float)[live], llp[live])
    logu = np.log(accept_uniform(C, seed, chain_offset, ctr))
    with np.errstate(invalid="ignore"):
        acc = live & (logu < la)            # a NaN log alpha rejects
        margin = np.where(live & ~np.isnan(la), np.abs(logu - la), np.inf)
    return acc, margin.astype(float)


def run_chains(model, prior, theta0, scale, loglik, seed, chain_offset, steps, first_step=0, force_invalid=False):
    """The whole rule on the host: C chains from theta0 [C, P], `steps` steps, loglik(theta_prop [C, P] double, ctr) -> [C]
    the estimate of the launch at counter ctr (the init pass calls it with ctr 0).  Returns (theta [C, P], ll [C],
    n_accept [C], trace of theta [steps, C, P]).  force_invalid: every proposal is treated as outside the support."""
    P = P_DIM[model]
    th = np.array(theta0, dtype=float)[:, :P].copy()
    C = th.shape[0]
    ll = np.asarray(loglik(th.copy(), 0), dtype=float).copy()
    n_acc = np.zeros(C, dtype=np.int64)
    trace = np.zeros((steps, C, P))
    useed = update_seed(seed)
    for s in range(first_step, first_step + steps):
        ctr = step_counter(s)
        pr = propose(model, th, scale, useed, chain_offset, ctr)
        valid = pr.valid & (not force_invalid)
        prop = np.where(valid[:, None], pr.raw, th.astype(LD)).astype(float)
        llp = np.asarray(loglik(prop.copy(), ctr), dtype=float)
        acc, _ = accept(model, prior, th, prop, valid, ll, llp, useed, chain_offset, ctr)
        th[acc], ll[acc] = prop[acc], llp[acc]
        n_acc += acc
        trace[s - first_step] = th
    return th, ll, n_acc, trace
