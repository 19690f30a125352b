"""Generate tests/golden/kalman.npz -- the reference's exact (Kalman) LGSSM gradient, kind='marginal' -- by running
the REFERENCE itself, imported read-only from a checkout named by SGMCMC_REFERENCE (it never travels to the GPU box):

    SGMCMC_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_kalman_golden.py

Data only: inputs (observations, raw parameters, messages, weights, seeds, sampler arguments) and the reference's
outputs.  Gradients are stored in the order [A, C, LQinv_vec, LRinv_vec].
  helper/*   LGSSMHelper.gradient_marginal_loglikelihood / marginal_loglikelihood over a theta grid
  sampler/*  noisy_gradient / noisy_loglikelihood(kind='marginal') after np.random.seed
  traj/*     10-step fits: the KF row of the LGSSM experiment (SGRLD) and an SGLD run
  seq/*      SeqLGSSMSampler on three sequences (gradients and a fit)
  cv/*       sample_sgld_cv
"""
import itertools
import json
import os
import sys
import warnings

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
if "SGMCMC_REFERENCE" not in os.environ:
    sys.exit("set SGMCMC_REFERENCE to a checkout of the reference (the directory holding sgmcmc_ssm/)")
sys.path.insert(0, os.environ["SGMCMC_REFERENCE"])
import numpy as np  # noqa: E402

from sgmcmc_ssm.models.lgssm import (  # noqa: E402
    LGSSMParameters, LGSSMHelper, LGSSMSampler, SeqLGSSMSampler, generate_lgssm_data)

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("A", "C", "LQinv_vec", "LRinv_vec")


def params(A, C, Q, R):
    return LGSSMParameters(A=np.eye(1) * A, C=np.eye(1) * C, Q=np.eye(1) * Q, R=np.eye(1) * R)


def theta(p):
    return np.array([p.A[0, 0], p.C[0, 0], p.LQinv[0, 0], p.LRinv[0, 0]])


def vec(g):
    return np.array([float(np.asarray(g[k]).reshape(-1)[0]) for k in NAMES])


def helper_cases(out, meta):
    """(a): every (A, C, Q, R) of the grid, the window length / prior precision / weights cycling through all their
    combinations; odd cases carry a non-zero mean_precision and log_constant in the forward message."""
    lengths, precs = (1, 2, 17, 200, 1000), (0.1, 2.5)
    grid = list(itertools.product((-0.95, 0.3, 0.9, 0.999), (1.0, 0.6, -1.4), (0.1, 1.0, 3.0), (0.1, 1.0, 3.0)))
    helper = LGSSMHelper(n=1, m=1)
    for i, (A, C, Q, R) in enumerate(grid):
        L, prec, weighted = lengths[i % 5], precs[(i // 5) % 2], (i // 10) % 2 == 1
        p = params(A, C, Q, R)
        np.random.seed(1000 + i)
        y = generate_lgssm_data(T=L, parameters=params(max(min(A, 0.99), -0.99), C, Q, R))["observations"]
        w = np.random.uniform(0.5, 3.0, size=L) if weighted else None
        mp, lc = (0.7 * prec, 0.25) if i % 2 else (0.0, 0.0)
        fm = dict(log_constant=lc, mean_precision=np.ones(1) * mp, precision=np.eye(1) * prec)
        g = helper.gradient_marginal_loglikelihood(observations=y, parameters=p, forward_message=fm, weights=w)
        ll = helper.marginal_loglikelihood(observations=y, parameters=p, forward_message=fm, weights=w)
        key = "helper/{0}".format(i)
        out[key + "/y"] = y[:, 0]
        out[key + "/theta"] = theta(p)
        out[key + "/weights"] = np.zeros(0) if w is None else w
        out[key + "/message"] = np.array([lc, mp, prec])
        out[key + "/grad"] = vec(g)
        out[key + "/loglike"] = np.float64(ll)
        meta.append(dict(kind="helper", key=key, L=L, A=A, C=C, Q=Q, R=R, prec=prec, weighted=weighted))


def kf_row_data(T, seed):
    p = params(0.9, 1.0, 0.1, 1.0)
    p.project_parameters()
    np.random.seed(seed)
    return p, generate_lgssm_data(T=T, parameters=p)["observations"]


def sampler_cases(out, meta):
    """(b): seeded noisy_gradient / noisy_loglikelihood, T = 800 (every S below divides it: 'strict' partitions)."""
    p0, y = kf_row_data(800, 4242)
    p = params(0.7, 1.0, 0.3, 1.5)
    out["sampler/y"] = y[:, 0]
    out["sampler/theta"] = theta(p)
    c = 0
    for (S, B), mb, style in itertools.product(((-1, -1), (40, -1), (16, 4), (16, 0), (1, 3)), (1, 3),
                                               ("uniform", "strict")):
        sampler = LGSSMSampler(n=1, m=1, observations=y, parameters=p.copy(), partition_style=style)
        seed = 500 + c
        np.random.seed(seed)
        g = sampler.noisy_gradient(kind="marginal", subsequence_length=S, buffer_length=B, minibatch_size=mb)
        ll = sampler.noisy_loglikelihood(kind="marginal", subsequence_length=S, buffer_length=B, minibatch_size=mb)
        key = "sampler/{0}".format(c)
        out[key + "/grad"] = vec(g)
        out[key + "/loglike"] = np.float64(ll)
        meta.append(dict(kind="sampler", key=key, S=S, B=B, minibatch_size=mb, partition_style=style, seed=seed))
        c += 1


def trajectory_cases(out, meta):
    """(c): the KF row (SGRLD, eps .1, S = 40, buffer -1, T = 1000, A .9, Q .1, R 1) and an SGLD run, 10 steps."""
    p0, y = kf_row_data(1000, 8080)
    out["traj/y"] = y[:, 0]
    runs = (("kf_row", dict(iter_type="SGRLD", epsilon=0.1, subsequence_length=40, buffer_length=-1, minibatch_size=1)),
            ("sgld", dict(iter_type="SGLD", epsilon=0.002, subsequence_length=16, buffer_length=4, minibatch_size=2)))
    for c, (name, kw) in enumerate(runs):
        start = params(0.5, 1.0, 0.5, 2.0)
        sampler = LGSSMSampler(n=1, m=1, observations=y, parameters=start.copy())
        seed = 9000 + c
        np.random.seed(seed)
        hist = sampler.fit(num_iters=10, output_all=True, kind="marginal", **kw)
        key = "traj/" + name
        out[key + "/theta0"] = theta(start)
        out[key + "/trajectory"] = np.stack([theta(h) for h in hist])
        meta.append(dict(kind="traj", key=key, seed=seed, **kw))


def seq_cases(out, meta):
    """(d): three sequences of different lengths."""
    p = params(0.8, 1.0, 0.4, 1.2)
    np.random.seed(31)
    ys = [generate_lgssm_data(T=T, parameters=p)["observations"] for T in (120, 75, 200)]
    for k, yk in enumerate(ys):
        out["seq/y{0}".format(k)] = yk[:, 0]
    start = params(0.6, 1.0, 0.6, 1.0)
    out["seq/theta"] = theta(start)
    c = 0
    for ns, (S, B) in itertools.product((-1, 2), ((-1, -1), (16, 4))):
        sampler = SeqLGSSMSampler(n=1, m=1, observations=ys, parameters=start.copy())
        seed = 700 + c
        np.random.seed(seed)
        g = sampler.noisy_gradient(kind="marginal", subsequence_length=S, buffer_length=B, num_sequences=ns)
        # (no noisy_loglikelihood: the reference's Seq version re-checks one sequence as a list of sequences and
        # raises IndexError for LGSSM, lgssm/sampler.py:61)
        key = "seq/{0}".format(c)
        out[key + "/grad"] = vec(g)
        meta.append(dict(kind="seq", key=key, S=S, B=B, num_sequences=ns, seed=seed))
        c += 1
    sampler = SeqLGSSMSampler(n=1, m=1, observations=ys, parameters=start.copy())
    np.random.seed(777)
    kw = dict(iter_type="SGLD", epsilon=0.002, subsequence_length=16, buffer_length=4, num_sequences=1)
    hist = sampler.fit(num_iters=5, output_all=True, kind="marginal", **kw)
    out["seq/fit/trajectory"] = np.stack([theta(h) for h in hist])
    meta.append(dict(kind="seq_fit", key="seq/fit", seed=777, **kw))


class CVSampler(LGSSMSampler):
    """The reference's noisy_gradient hands `parameters` to grad_logprior twice when it is given (TypeError,
    sgmcmc_sampler.py:447-450), so its sample_sgld_cv cannot run as is; this is its body with that one call fixed."""

    def noisy_gradient(self, preconditioner=None, is_scaled=True, **kwargs):
        assert preconditioner is None
        grad_loglike = self._noisy_grad_loglikelihood(**kwargs)
        grad_prior = self.prior.grad_logprior(parameters=kwargs.get('parameters', self.parameters))
        grad = {var: grad_prior[var] + grad_loglike[var] for var in grad_prior}
        if is_scaled:
            for var in grad:
                grad[var] /= self._get_T(**kwargs)
        return grad


def cv_cases(out, meta):
    """(e): sample_sgld_cv: the centering gradient is the exact one at centering_parameters."""
    p0, y = kf_row_data(400, 5151)
    out["cv/y"] = y[:, 0]
    start, centre = params(0.6, 1.0, 0.5, 1.5), params(0.85, 1.0, 0.15, 1.1)
    sampler = CVSampler(n=1, m=1, observations=y, parameters=start.copy())
    np.random.seed(60)
    cg = sampler.noisy_gradient(kind="marginal", subsequence_length=-1, buffer_length=-1, parameters=centre)
    traj = [theta(sampler.parameters)]
    for _ in range(5):
        sampler.sample_sgld_cv(epsilon=0.002, centering_parameters=centre, centering_gradient=cg,
                               subsequence_length=16, buffer_length=4, kind="marginal")
        sampler.project_parameters()
        traj.append(theta(sampler.parameters))
    out["cv/theta0"] = theta(start)
    out["cv/centre"] = theta(centre)
    out["cv/centering_grad"] = vec(cg)
    out["cv/trajectory"] = np.stack(traj)
    meta.append(dict(kind="cv", key="cv", seed=60, epsilon=0.002, S=16, B=4))


def main():
    out, meta = {}, []
    helper_cases(out, meta)
    sampler_cases(out, meta)
    trajectory_cases(out, meta)
    seq_cases(out, meta)
    cv_cases(out, meta)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "kalman.npz"), **out)
    print("wrote kalman.npz: {0} cases".format(len(meta)))


if __name__ == "__main__":
    main()
