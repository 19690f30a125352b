"""1-D linear-Gaussian SSM:  x_t = A x_{t-1} + N(0, Q),   y_t = C x_t + N(0, R).

Exports LGSSMParameters, LGSSMPrior, LGSSMHelper, LGSSMSampler, SeqLGSSMSampler,
generate_lgssm_data (reference: models/lgssm/{parameters,helper,sampler}.py).  Particle-filter
entries: the "prior" and "optimal" proposals (models/lgssm/kernels.py:11-122) and the score
(helper.py:1270-1277) are model id PFG_MODEL_LGSSM in libpfgrad.so.  The exact gradient of the
reference's kind='marginal' -- buffered Kalman messages and the smoothed score
(helper.py:53-192, 312-420) -- is PFG_SMOOTHER_KALMAN (csrc/pfg_kalman.hip): every sampler entry
(noisy_gradient, noisy_loglikelihood, sample_sgld / sgrld / sgld_cv, fit*) accepts
kind='marginal', and LGSSMHelper.gradient_marginal_loglikelihood / marginal_loglikelihood run
one window on the GPU.  Forward-filtering backward-sampling of the latent path (helper.py:650-698)
is PFG_SMOOTHER_KALMAN_FFBS (csrc/pfg_ffbs.hip): LGSSMHelper.latent_var_sample, LGSSMSampler.sample_x
and predict(kind='analytic') with samples, kind='complete' gradients (num_samples paths per window)
and the blocked Gibbs sampler (sample_gibbs, iter_type='Gibbs').  Not built:
predictive_loglikelihood(kind='marginal'), noisy_loglikelihood(kind='complete'), smoothed marginals
(predict(kind='analytic', return_distr=True)), non-zero backward messages for kind='marginal',
include_init=False."""
import numpy as np

from .. import particle_filters as _pf
from ..base_parameters import (BaseParameters, BasePrior, MatrixVar, CholPrecisionVar,
                               WishartPrecisionPrior, MatrixNormalPrior, install_properties,
                               BasePreconditioner, MatrixPrecond, CholPrecisionPrecond)
from ..sgmcmc_sampler import SGMCMCSampler, SeqSGMCMCSampler, PFHelper
from .svm import stationary_precision


@install_properties
class LGSSMParameters(BaseParameters):
    """A, C (1x1), LQinv_vec, LRinv_vec."""
    _specs = (MatrixVar('A', ('n',)), MatrixVar('C', ('m', 'n'), stable=False),
              CholPrecisionVar('Q', 'n'), CholPrecisionVar('R', 'm'))

    def __str__(self):
        return "LGSSMParameters:\nA:\n{0}\nC:\n{1}\nQ:\n{2}\nR:\n{3}".format(self.A, self.C, self.Q, self.R)

    def project_parameters(self, **kwargs):
        # C is pinned to the identity unless told otherwise (lgssm/parameters.py:39-42)
        if 'C' not in kwargs:
            kwargs['C'] = dict(fixed_eye=True)
        return super().project_parameters(**kwargs)


class LGSSMPrior(BasePrior):
    _Parameters = LGSSMParameters
    _blocks = (WishartPrecisionPrior('Q', 'n', matrix_name='A'), WishartPrecisionPrior('R', 'm', matrix_name='C'),
               MatrixNormalPrior('A', ('n',), row_cov='Q'),
               MatrixNormalPrior('C', ('m', 'n'), row_cov='R'))


class LGSSMPreconditioner(BasePreconditioner):
    """SGRLD / SGRD preconditioner (lgssm/parameters.py:58-67); noise is drawn A, C, Q, R."""
    _blocks = (MatrixPrecond('A', 'Q'), MatrixPrecond('C', 'R'),
               CholPrecisionPrecond('Q'), CholPrecisionPrecond('R'))


def generate_lgssm_data(T, parameters, initial_message=None, tqdm=None):
    """Simulate T steps with the reference's np.random call order (lgssm/parameters.py:67-129)."""
    A, C, Q, R = parameters.A, parameters.C, parameters.Q, parameters.R
    m, n = np.shape(C)
    if initial_message is None:
        initial_message = dict(log_constant=0.0, mean_precision=np.zeros(n),
                               precision=stationary_precision(parameters.Qinv, A, 10))
    x_prev = np.random.multivariate_normal(
        mean=np.linalg.solve(initial_message['precision'], initial_message['mean_precision']),
        cov=np.linalg.inv(initial_message['precision']))
    x = np.zeros((T, n), dtype=float)
    y = np.zeros((T, m), dtype=float)
    for t in range(T):
        x[t] = np.random.multivariate_normal(mean=np.dot(A, x_prev), cov=Q)
        y[t] = np.random.multivariate_normal(mean=np.dot(C, x[t]), cov=R)
        x_prev = x[t]
    return dict(observations=y, latent_vars=x, parameters=parameters, initial_message=initial_message)


class LGSSMHelper(PFHelper):
    """pf_gradient_estimate -> dict(LRinv_vec, LQinv_vec, C, A)  (models/lgssm/helper.py:1136-1142);
    default kernel 'optimal' for n*m = 1 (:1200-1214).  The exact (Kalman) gradient and marginal
    log-likelihood of a window: kalman_problem, gradient_marginal_loglikelihood, marginal_loglikelihood."""
    model = "lgssm"
    exact = True
    default_kernel = "optimal"
    kernels = ("prior", "optimal")
    score_names = ("LRinv_vec", "LQinv_vec", "C", "A")

    @staticmethod
    def _scalar_observations(observations):
        y = np.ascontiguousarray(observations, dtype=float)
        if y.ndim == 2:
            if y.shape[1] != 1:
                raise ValueError("the exact LGSSM kernels support m = 1 observations only")
            y = y[:, 0]
        return y

    def _message_prior(self, forward_message):
        """The message of x_{-1} as the kernels take it: (prior_mean, prior_var) = (mean_precision, 1) / precision."""
        if forward_message is None:
            forward_message = self.default_forward_message
        precision = float(np.reshape(forward_message['precision'], -1)[0])
        mean_precision = float(np.reshape(forward_message['mean_precision'], -1)[0])
        if not (0.0 < precision < np.inf):
            raise ValueError("the forward message needs a finite precision > 0, got {0}".format(precision))
        return mean_precision / precision, 1.0 / precision

    def ffbs_problem(self, observations, parameters, num_samples, subsequence_start=0, subsequence_end=None,
                     weights=None, forward_message=None, stat="score", rng="replay", z=None, seed=0, stream=0, step=0):
        """num_samples FFBS paths of the buffer `observations` as a PFG_SMOOTHER_KALMAN_FFBS problem: forward messages
        from `forward_message` (the message of x_{-1}), backward sampling, and (stat='score') the complete-data score
        over [subsequence_start, subsequence_end) averaged over the paths.  rng='replay' draws the T * num_samples
        normals from np.random now, in the reference's order, unless `z` is given."""
        prior_mean, prior_var = self._message_prior(forward_message)
        y = self._scalar_observations(observations)
        T, S = y.shape[0], int(num_samples)
        if S < 1:
            raise ValueError("num_samples must be >= 1")
        if rng == "replay" and z is None:
            z = np.random.standard_normal(T * S)
        return dict(model="lgssm", kernel=self.default_kernel, smoother="kalman_ffbs", stat=stat, dtype="f64",
                    rng=rng, N=S, t1=int(subsequence_start), tL=T if subsequence_end is None else int(subsequence_end),
                    lambduh=1.0, prior_mean=prior_mean, prior_var=prior_var, y=y, weights=weights,
                    theta=parameters.theta(), z=z if rng == "replay" else None, seed=seed, stream=stream, step=step,
                    flags=0)

    def latent_var_sample(self, observations, parameters, forward_message=None, backward_message=None,
                          distr='joint', lag=None, num_samples=None, tqdm=None, include_init=False, **kwargs):
        """Draws of the latent path from Pr(x | y) by forward filtering, backward sampling (helper.py:650-698):
        shape (T, 1), or (T, 1, num_samples).  As in the reference, the joint draw ignores `backward_message`."""
        if distr == 'joint' and lag is not None:
            raise ValueError("Must set distr to 'marginal' for lag != None")
        if distr != 'joint':
            raise NotImplementedError("latent_var_sample(distr='{0}') is not built: FFBS draws the joint path".format(distr))
        if include_init:
            raise NotImplementedError("include_init=True (a draw of x_{-1} too) is not built")
        S = 1 if num_samples is None else int(num_samples)
        q = self.ffbs_problem(observations, parameters, S, forward_message=forward_message, stat="none")
        paths = _pf.run_windows([q], want_paths=True)[0]["paths"]
        T = q["y"].shape[0]
        return paths.reshape(T, 1) if num_samples is None else paths.reshape(T, 1, S)

    def calc_gibbs_sufficient_statistic(self, observations, latent_vars, **kwargs):
        """Sufficient statistics of (A, Q) and (C, R) given one latent path (helper.py:502-555)."""
        x = latent_vars
        y = observations
        PsiT, PsiT_prev = x[1:], x[:-1]
        transition_count = len(PsiT)
        Sx_prevprev = PsiT_prev.T.dot(PsiT_prev)
        Sx_curprev = PsiT.T.dot(PsiT_prev)
        Sx_curcur = PsiT.T.dot(PsiT)
        PsiT, PsiT_prev = y, x
        emission_count = len(PsiT)
        S_prevprev = PsiT_prev.T.dot(PsiT_prev)
        S_curprev = PsiT.T.dot(PsiT_prev)
        S_curcur = PsiT.T.dot(PsiT)
        return dict(A=dict(S_prevprev=Sx_prevprev, S_curprev=Sx_curprev),
                    Q=dict(S_count=transition_count, S_prevprev=Sx_prevprev, S_curprev=Sx_curprev, S_curcur=Sx_curcur),
                    R=dict(S_count=emission_count, S_prevprev=S_prevprev, S_curprev=S_curprev, S_curcur=S_curcur),
                    C=dict(S_prevprev=S_prevprev, S_curprev=S_curprev))

    def parameters_gibbs_sample(self, observations, latent_vars, prior, **kwargs):
        """theta ~ Pr(theta | y, x) (sgmcmc_sampler.py:1663-1685)."""
        return prior.sample_posterior(self.calc_gibbs_sufficient_statistic(observations, latent_vars))

    def kalman_problem(self, observations, parameters, subsequence_start=0, subsequence_end=None,
                       weights=None, forward_message=None, backward_message=None):
        """One buffered window as a PFG_SMOOTHER_KALMAN problem: forward messages over [0, subsequence_start) from
        `forward_message` (the message of x_{-1}), backward messages over [subsequence_end, T) from
        `backward_message`, the exact score and the forward log-likelihood over the window."""
        if backward_message is not None and (np.any(np.asarray(backward_message['precision']) != 0)
                                             or np.any(np.asarray(backward_message['mean_precision']) != 0)):
            raise NotImplementedError("kind='marginal' is built for the zero backward message")
        prior_mean, prior_var = self._message_prior(forward_message)
        y = self._scalar_observations(observations)
        T = y.shape[0]
        return dict(model="lgssm", kernel=self.default_kernel, smoother="kalman", stat="score", dtype="f64",
                    rng="device", N=1, t1=int(subsequence_start), tL=T if subsequence_end is None else int(subsequence_end),
                    lambduh=1.0, prior_mean=prior_mean, prior_var=prior_var,
                    y=y, weights=weights, theta=parameters.theta(), flags=0)

    def gradient_marginal_loglikelihood(self, observations, parameters, forward_message=None,
                                        backward_message=None, weights=None, include_init=True, tqdm=None):
        """Exact gradient of the (weighted) marginal log-likelihood of `observations`
        (models/lgssm/helper.py:312-420) -> dict(A, LQinv_vec, C, LRinv_vec)."""
        if not include_init:
            raise NotImplementedError("include_init=False is not built (the transition term from x_{-1} is always in)")
        q = self.kalman_problem(observations, parameters, weights=weights, forward_message=forward_message,
                                backward_message=backward_message)
        g = dict(zip(self.score_names, _pf.run_windows([q])[0]["mean_statistic"]))
        return {var: np.reshape(g[var], np.shape(value)) for var, value in parameters.as_dict().items()}

    def marginal_loglikelihood(self, observations, parameters, forward_message=None, backward_message=None,
                               weights=None, tqdm=None, **kwargs):
        """log Pr(y | theta) of `observations` given the forward message, whose log_constant is included
        (models/lgssm/helper.py:195-233; with the zero backward message the combination term is 0)."""
        if forward_message is None:
            forward_message = self.default_forward_message
        q = self.kalman_problem(observations, parameters, weights=weights, forward_message=forward_message,
                                backward_message=backward_message)
        return forward_message['log_constant'] + _pf.run_windows([q])[0]["loglikelihood_estimate"]


class LGSSMSampler(SGMCMCSampler):
    def __init__(self, n=1, m=1, observations=None, prior=None, parameters=None,
                 forward_message=None, backward_message=None, name="LGSSMSampler", **kwargs):
        self.options = kwargs
        self.n, self.m, self.name = n, m, name
        self.setup(observations=observations, prior=prior, parameters=parameters,
                   forward_message=forward_message, backward_message=backward_message)

    def setup(self, observations=None, prior=None, parameters=None, forward_message=None,
              backward_message=None):
        self.observations = observations
        self.prior = LGSSMPrior.generate_default_prior(n=self.n, m=self.m) if prior is None else prior
        self.parameters = self.prior.sample_prior() if parameters is None else parameters
        if forward_message is None:
            forward_message = dict(log_constant=0.0, mean_precision=np.zeros(self.n),
                                   precision=np.eye(self.n) / 10)
        self.forward_message = forward_message
        if backward_message is None:
            backward_message = dict(log_constant=0.0, mean_precision=np.zeros(self.n),
                                    precision=np.zeros((self.n, self.n)))
        self.backward_message = backward_message
        self.message_helper = LGSSMHelper(n=self.n, m=self.m, forward_message=forward_message,
                                          backward_message=backward_message)

    def _check_observation_shape(self, observations):
        if observations is None:
            return
        if np.shape(observations)[1] != self.m:
            raise ValueError("observations second dimension does not match m")

    def _get_preconditioner(self, preconditioner=None):
        return LGSSMPreconditioner() if preconditioner is None else preconditioner

    def predict(self, target='latent', distr=None, lag=None, return_distr=None, num_samples=None,
                kind='pf', observations=None, parameters=None, **kwargs):
        """kind='analytic', target='latent' draws latent paths (num_samples given, or return_distr=False) by FFBS
        (sgmcmc_sampler.py:956-1040); the smoothed marginals (return_distr=True) are not built.  kind='pf': the
        particle smoother's marginals, as for every model."""
        if kind != 'analytic':
            return super().predict(target=target, distr=distr, lag=lag, return_distr=return_distr,
                                   num_samples=num_samples, kind=kind, observations=observations,
                                   parameters=parameters, **kwargs)
        if return_distr is None:
            return_distr = num_samples is None
        if return_distr or target != 'latent':
            raise NotImplementedError("predict(kind='analytic') draws latent paths only (target='latent', "
                                      "return_distr=False or num_samples): smoothed marginals and y are not built")
        observations = self._get_observations(observations)
        if parameters is None:
            parameters = self.parameters
        return self.message_helper.latent_var_sample(
            distr='joint' if distr is None else distr, lag=lag, num_samples=num_samples,
            observations=observations, parameters=parameters, **kwargs)

    def sample_x(self, observations=None, parameters=None, tqdm=None, num_samples=None, **kwargs):
        """Latent paths drawn by FFBS (lgssm/sampler.py:70-77)."""
        return self.predict(target='latent', kind='analytic', return_distr=False, observations=observations,
                            parameters=parameters, num_samples=num_samples, **kwargs)

    def sample_gibbs(self, parameters=None, observations=None, tqdm=None):
        """One step of the blocked Gibbs sampler (lgssm/sampler.py:79-96): one FFBS path of the whole series, then
        the parameters from their conjugate posterior (Q, R, A, C)."""
        if parameters is None:
            parameters = self.parameters
        observations = self._get_observations(observations)
        x = self.sample_x(parameters=parameters, observations=observations)
        self.parameters = self.message_helper.parameters_gibbs_sample(
            observations=observations, latent_vars=x, prior=self.prior)
        return self.parameters

    def get_iter_step(self, iter_type, steps_per_iteration=1, **kwargs):
        if iter_type == 'Gibbs':        # sgmcmc_sampler.py:898-900
            names, kws = ['sample_gibbs', 'project_parameters'], [{}, kwargs.get("project_kwargs", {})]
            return names * steps_per_iteration, kws * steps_per_iteration
        return super().get_iter_step(iter_type, steps_per_iteration=steps_per_iteration, **kwargs)


class SeqLGSSMSampler(SeqSGMCMCSampler, LGSSMSampler):
    def sample_gibbs(self, parameters=None, observations=None, tqdm=None):
        # the reference's own Seq Gibbs step fails in _check_observation_shape on a list of sequences
        raise NotImplementedError("Gibbs over lists of sequences is not built")
