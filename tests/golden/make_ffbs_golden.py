"""Generate tests/golden/ffbs.npz -- the reference's FFBS latent paths (LGSSMHelper.latent_var_sample, distr='joint'),
its complete-data gradient, kind='complete' and Gibbs -- by running the REFERENCE itself, imported read-only from a
checkout named by SGMCMC_REFERENCE (it never travels to the GPU box):

    SGMCMC_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ffbs_golden.py

As shipped, the reference's gradient_complete_data_loglikelihood (models/lgssm/helper.py:422-491) raises
KeyError('LQinv'): it builds `grad` from parameters.as_dict() (keys LQinv_vec, LRinv_vec) and then adds to
grad['LQinv'] / grad['LRinv'].  That one method is wrapped so that it sees a parameters shim whose as_dict() returns
{A, C, LQinv, LRinv} as matrices -- what its last two lines (grad.pop('LQinv')[tril]) intend; everything else runs
unmodified.

Data only: inputs (observations, raw parameters, messages, weights, seeds, sampler arguments) and the reference's
outputs.  Gradients are stored in the order [A, C, LQinv_vec, LRinv_vec].
  paths/*    latent_var_sample over a grid of theta, T, num_samples and forward messages, and the complete-data
             gradient on those paths: the whole buffer (no x_prev) and a weighted inner window (with x_prev)
  grad/*     noisy_gradient(kind='complete', num_samples) after np.random.seed, and the next np.random draw
  traj/*     5-step fits: SGRLD (the MC_100 row of the LGSSM experiment) and SGLD with kind='complete',
             num_samples=100, and Gibbs
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
    LGSSMParameters, LGSSMHelper, LGSSMSampler, generate_lgssm_data)

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("A", "C", "LQinv_vec", "LRinv_vec")


class _MatrixDictParameters(object):
    """The parameters as gradient_complete_data_loglikelihood needs them: as_dict() with matrix-shaped LQinv / LRinv."""

    def __init__(self, parameters):
        self._p = parameters

    def __getattr__(self, name):
        return getattr(self._p, name)

    def as_dict(self):
        return dict(A=self._p.A, C=self._p.C, LQinv=self._p.LQinv, LRinv=self._p.LRinv)


_gradient_complete = LGSSMHelper.gradient_complete_data_loglikelihood


def _gradient_complete_fixed(self, observations, latent_vars, parameters, **kwargs):
    return _gradient_complete(self, observations=observations, latent_vars=latent_vars,
                              parameters=_MatrixDictParameters(parameters), **kwargs)


LGSSMHelper.gradient_complete_data_loglikelihood = _gradient_complete_fixed


def params(A, C, Q, R):
    return LGSSMParameters(A=np.eye(1) * A, C=np.eye(1) * C, Q=np.eye(1) * Q, R=np.eye(1) * R)


def theta(p):
    return np.array([p.A[0, 0], p.C[0, 0], p.LQinv[0, 0], p.LRinv[0, 0]])


def vec(g):
    return np.array([float(np.asarray(g[k]).reshape(-1)[0]) for k in NAMES])


def path_cases(out, meta):
    """(a): one case per (T, S), theta / forward message cycling; odd cases carry a non-zero mean_precision."""
    shapes = ((1, None), (2, 1), (3, 7), (17, None), (17, 7), (17, 100), (200, 1), (200, 7), (200, 100),
              (1000, None), (1000, 1), (1000, 7))
    thetas = ((0.9, 1.0, 0.1, 1.0), (-0.95, 0.6, 3.0, 0.1), (0.3, -1.4, 1.0, 3.0), (0.999, 1.0, 0.1, 0.1))
    precs = (0.1, 2.5)
    helper = LGSSMHelper(n=1, m=1)
    for i, (T, S) in enumerate(shapes):
        A, C, Q, R = thetas[i % len(thetas)]
        prec = precs[(i // 2) % 2]
        mp = 0.7 * prec if i % 2 else 0.0
        p = params(A, C, Q, R)
        np.random.seed(2000 + i)
        y = generate_lgssm_data(T=T, parameters=params(max(min(A, 0.99), -0.99), C, Q, R))["observations"]
        fm = dict(log_constant=0.0, mean_precision=np.ones(1) * mp, precision=np.eye(1) * prec)
        seed = 3000 + i
        np.random.seed(seed)
        x = helper.latent_var_sample(observations=y, parameters=p, forward_message=fm, distr='joint', num_samples=S)
        key = "paths/{0}".format(i)
        out[key + "/y"] = y[:, 0]
        out[key + "/theta"] = theta(p)
        out[key + "/message"] = np.array([mp, prec])
        out[key + "/paths"] = np.reshape(x, (T, -1))
        # the complete-data gradient on these paths: the whole buffer, then a weighted inner window given x_prev
        g0 = helper.gradient_complete_data_loglikelihood(observations=y, latent_vars=x, parameters=p)
        out[key + "/grad_all"] = vec(g0)
        t1, tL = T // 3, T - T // 4
        if 0 < t1 < tL:
            w = np.random.uniform(0.5, 3.0, size=tL - t1)
            g1 = helper.gradient_complete_data_loglikelihood(
                observations=y[t1:tL], latent_vars=x[t1:tL], parameters=p, weights=w,
                forward_message=dict(x_prev=x[t1 - 1]))
            out[key + "/weights"] = w
            out[key + "/grad_window"] = vec(g1)
        meta.append(dict(kind="paths", key=key, T=T, S=S, seed=seed, t1=t1, tL=tL, window=bool(0 < t1 < tL)))


def mc_row_data(T, seed):
    p = params(0.9, 1.0, 0.1, 1.0)
    p.project_parameters()
    np.random.seed(seed)
    return p, generate_lgssm_data(T=T, parameters=p)["observations"]


def grad_cases(out, meta):
    """(b): seeded noisy_gradient(kind='complete'), T = 400, and the next np.random draw after it."""
    p0, y = mc_row_data(400, 4343)
    p = params(0.7, 1.0, 0.3, 1.5)
    out["grad/y"] = y[:, 0]
    out["grad/theta"] = theta(p)
    c = 0
    for (S, B), ns, mb in itertools.product(((-1, -1), (40, -1), (16, 4), (16, 0), (398, 0)), (1, 7, 100), (1, 2)):
        if mb == 2 and ns == 100:
            continue
        sampler = LGSSMSampler(n=1, m=1, observations=y, parameters=p.copy())
        seed = 600 + c
        np.random.seed(seed)
        g = sampler.noisy_gradient(kind="complete", num_samples=ns, subsequence_length=S, buffer_length=B,
                                   minibatch_size=mb)
        key = "grad/{0}".format(c)
        out[key + "/grad"] = vec(g)
        out[key + "/next"] = np.float64(np.random.rand())
        meta.append(dict(kind="grad", key=key, S=S, B=B, num_samples=ns, minibatch_size=mb, seed=seed))
        c += 1


def trajectory_cases(out, meta):
    """(c): the MC_100 row (SGRLD, eps .1, S = 40, buffer -1, T = 1000, A .9, Q .1, R 1), an SGLD run and Gibbs,
    5 steps each."""
    p0, y = mc_row_data(1000, 8181)
    out["traj/y"] = y[:, 0]
    runs = (("mc_row", dict(iter_type="SGRLD", epsilon=0.1, subsequence_length=40, buffer_length=-1,
                            kind="complete", num_samples=100)),
            ("sgld", dict(iter_type="SGLD", epsilon=0.002, subsequence_length=16, buffer_length=4,
                          kind="complete", num_samples=100)),
            ("gibbs", dict(iter_type="Gibbs")))
    for c, (name, kw) in enumerate(runs):
        start = params(0.5, 1.0, 0.5, 2.0)
        sampler = LGSSMSampler(n=1, m=1, observations=y, parameters=start.copy())
        seed = 9100 + c
        np.random.seed(seed)
        hist = sampler.fit(num_iters=5, output_all=True, **kw)
        key = "traj/" + name
        out[key + "/theta0"] = theta(start)
        out[key + "/trajectory"] = np.stack([theta(h) for h in hist])
        meta.append(dict(kind="traj", key=key, seed=seed, fit=kw))


def main():
    out, meta = {}, []
    path_cases(out, meta)
    grad_cases(out, meta)
    trajectory_cases(out, meta)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "ffbs.npz"), **out)
    print("wrote ffbs.npz: {0} cases".format(len(meta)))


if __name__ == "__main__":
    main()
