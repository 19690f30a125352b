"""Generate tests/golden/optim_rules.npz -- the reference's own fit('SGD') and fit('ADAGRAD') on LGSSM with the exact
(kind='marginal') gradient of the full series -- by running the REFERENCE itself, imported read-only from a checkout
named by SGMCMC_REFERENCE (it never travels to the GPU box):

    SGMCMC_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_optim_golden.py

Both rules draw nothing and the full-series Kalman gradient is exact, so the trajectories are deterministic: 5 steps
(step_sgd | step_adagrad, then project_parameters) from three start points on one series of T = 30.

Data only: y [30]; theta0 [3, 4] raw (A, C, LQinv, LRinv); the prior's hyper-parameters (the sampler's default prior);
epsilon per rule; sgd/trajectory and adagrad/trajectory [3, 6, 4], the start included.
"""
import os
import sys
import warnings

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
if "SGMCMC_REFERENCE" not in os.environ:
    sys.exit("set SGMCMC_REFERENCE to a checkout of the reference (the directory holding sgmcmc_ssm/)")
sys.path.insert(0, os.environ["SGMCMC_REFERENCE"])
import numpy as np  # noqa: E402

from sgmcmc_ssm.models.lgssm import LGSSMParameters, LGSSMSampler, generate_lgssm_data  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
T, STEPS = 30, 5
STARTS = ((0.5, 1.0, 0.5, 2.0), (0.9, 1.0, 0.1, 1.0), (-0.3, 1.0, 2.0, 0.4))       # A, C, Q, R
EPSILON = dict(sgd=0.05, adagrad=0.1)
HYPER = ("df_Qinv", "scale_Qinv", "df_Rinv", "scale_Rinv", "mean_A", "var_col_A", "mean_C", "var_col_C")


def params(A, C, Q, R):
    return LGSSMParameters(A=np.eye(1) * A, C=np.eye(1) * C, Q=np.eye(1) * Q, R=np.eye(1) * R)


def theta(p):
    return np.array([p.A[0, 0], p.C[0, 0], p.LQinv[0, 0], p.LRinv[0, 0]])


def main():
    np.random.seed(4242)
    y = generate_lgssm_data(T=T, parameters=params(0.8, 1.0, 0.3, 0.6))["observations"]
    out = dict(y=np.reshape(y, -1), theta0=np.stack([theta(params(*s)) for s in STARTS]))
    for rule, iter_type in (("sgd", "SGD"), ("adagrad", "ADAGRAD")):
        traj = []
        for s in STARTS:
            sampler = LGSSMSampler(n=1, m=1, observations=y, parameters=params(*s))
            hist = sampler.fit(iter_type=iter_type, num_iters=STEPS, output_all=True, epsilon=EPSILON[rule],
                               subsequence_length=-1, buffer_length=-1, kind="marginal")
            traj.append(np.stack([theta(h) for h in hist]))
        out[rule + "/trajectory"] = np.stack(traj)
        out[rule + "/epsilon"] = np.float64(EPSILON[rule])
    hp = sampler.prior.hyperparams
    for k in HYPER:
        out["hyper/" + k] = np.float64(np.reshape(hp[k], -1)[0])
    np.savez_compressed(os.path.join(HERE, "optim_rules.npz"), **out)
    print("wrote optim_rules.npz:", {k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
