"""CPU: the restatement of the resident SGRLD / Gibbs chain rules (tests/helpers/lgssm_chain_rules.py) equals the host
classes -- LGSSMPreconditioner and LGSSMPrior.sample_posterior -- and the ensemble refuses what it does not build
before it looks for a GPU."""
import os
import sys

import numpy as np
import pytest
import scipy.stats

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import lgssm_chain_rules as rules  # noqa: E402

from sgmcmc_ssm_amd import _capi
from sgmcmc_ssm_amd.models.lgssm import LGSSMParameters, LGSSMPrior, LGSSMPreconditioner, LGSSMHelper


def _params(th):
    return LGSSMParameters(A=np.eye(1) * th[0], C=np.eye(1) * th[1], LQinv=np.eye(1) * th[2], LRinv=np.eye(1) * th[3])


def _random_thetas(rs, n):
    return np.column_stack([rs.uniform(-0.95, 0.95, n), rs.uniform(0.5, 1.5, n), rs.uniform(0.2, 4.0, n),
                            rs.uniform(0.2, 4.0, n)])


def test_stat_id():
    assert _capi.STAT["gibbs"] == 4


def test_sgrld_terms_equal_the_preconditioner():
    rs = np.random.RandomState(3)
    theta = _random_thetas(rs, 200)
    grad = rs.standard_normal((200, 4)) * 50.0
    T = 137.0
    pre = LGSSMPreconditioner()
    got_p = rules.sgrld_precondition(theta, grad, 1.0 / T)
    got_c = rules.sgrld_correction(theta, 1.0 / T)
    for i, th in enumerate(theta):
        p = _params(th)
        g = {v: np.reshape(grad[i, j], np.shape(p.var_dict[v])) for j, v in enumerate(rules.THETA)}
        ref_p = pre.precondition(g, p, scale=1.0 / T)
        ref_c = pre.correction_term(p, scale=1.0 / T)
        np.testing.assert_allclose(got_p[i], [float(np.reshape(ref_p[v], -1)[0]) for v in rules.THETA], rtol=1e-15, atol=0)
        np.testing.assert_allclose(got_c[i], [float(np.reshape(ref_c[v], -1)[0]) for v in rules.THETA], rtol=1e-15, atol=0)
        np.random.seed(100 + i)
        ref_n = pre.precondition_noise(p, scale=1.0 / T)
        np.random.seed(100 + i)
        z = np.random.normal(size=4)           # the noise is drawn A, C, Q, R: one normal each
        got_n = rules.sgrld_noise_factor(theta[i:i + 1])[0] * z * np.sqrt(1.0 / T)
        np.testing.assert_allclose(got_n, [float(np.reshape(ref_n[v], -1)[0]) for v in rules.THETA], rtol=1e-15, atol=0)


def test_sgrld_drift_is_the_host_step_without_noise():
    """eps * (noisy_gradient(preconditioner) + correction_term) of sample_sgrld, with the prior gradient at theta."""
    rs = np.random.RandomState(5)
    prior = LGSSMPrior.generate_default_prior(var=1.0, n=1, m=1)
    hy = rules.hyper_of(prior)
    theta = _random_thetas(rs, 50)
    ghat = rs.standard_normal((50, 4)) * 20.0
    eps, T = 0.1, 1000.0
    got = rules.sgrld_drift(theta, ghat, hy, eps, T)
    pre = LGSSMPreconditioner()
    for i, th in enumerate(theta):
        p = _params(th)
        gp = prior.grad_logprior(p)
        g = {v: gp[v] + ghat[i, rules.SCORE_COL[v]] for v in rules.THETA}
        d = pre.precondition(g, p, scale=1.0 / T)
        c = pre.correction_term(p, scale=1.0 / T)
        ref = [float(np.reshape(eps * (d[v] + c[v]), -1)[0]) for v in rules.THETA]
        np.testing.assert_allclose(got[i], ref, rtol=1e-14, atol=1e-300)


def test_gibbs_statistics_and_posterior_draws():
    """The restated record equals calc_gibbs_sufficient_statistic, and ~20k seeded host draws of sample_posterior
    follow the restated laws: Qinv / scale ~ chi2(df), Rinv likewise, (A - mean) sqrt((LQinv^2 + 1e-9) / var_unit)
    ~ N(0, 1)."""
    from sgmcmc_ssm_amd.models.lgssm import generate_lgssm_data
    np.random.seed(2)
    data = generate_lgssm_data(T=200, parameters=_params([0.9, 1.0, 1.0 / np.sqrt(0.1), 1.0]))
    x, y = data["latent_vars"], data["observations"]
    ss = LGSSMHelper(n=1, m=1).calc_gibbs_sufficient_statistic(y, x)
    rec = rules.gibbs_stats(x, y)
    ref = [ss["Q"]["S_prevprev"], ss["Q"]["S_curprev"], ss["Q"]["S_curcur"], ss["R"]["S_prevprev"],
           ss["R"]["S_curprev"], ss["R"]["S_curcur"], ss["R"]["S_count"]]
    np.testing.assert_allclose(rec[:7], [float(np.reshape(v, -1)[0]) for v in ref], rtol=1e-13)
    assert ss["Q"]["S_count"] == rec[6] - 1
    prior = LGSSMPrior.generate_default_prior(var=100.0, n=1, m=1)
    post = rules.gibbs_posterior(rec, rules.hyper_of(prior))
    np.random.seed(11)
    draws = np.array([prior.sample_posterior(ss).theta() for _ in range(20000)])
    qi, ri = draws[:, 2] ** 2, draws[:, 3] ** 2
    assert scipy.stats.kstest(qi / post["scale_Q"], "chi2", args=(post["df_Q"],)).pvalue > 1e-4
    assert scipy.stats.kstest(ri / post["scale_R"], "chi2", args=(post["df_R"],)).pvalue > 1e-4
    zA = (draws[:, 0] - post["mean_A"]) / np.sqrt(post["var_unit_A"] / (qi + 1e-9))
    zC = (draws[:, 1] - post["mean_C"]) / np.sqrt(post["var_unit_C"] / (ri + 1e-9))
    assert scipy.stats.kstest(zA, "norm").pvalue > 1e-4
    assert scipy.stats.kstest(zC, "norm").pvalue > 1e-4


@pytest.mark.parametrize("model", ["svm", "garch"])
def test_ensemble_refuses_sgrld_and_gibbs_off_lgssm(model):
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    with pytest.raises(NotImplementedError, match="No Default Preconditioner"):
        ChainEnsemble(model, np.zeros(20), np.zeros((2, _capi.THETA_DIM[model])), sampler="sgrld")
    with pytest.raises(NotImplementedError):
        ChainEnsemble(model, np.zeros(20), np.zeros((2, _capi.THETA_DIM[model])), sampler="gibbs")


def test_ensemble_gibbs_refuses_windows_sequence_lists_and_f32():
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    th = np.tile([0.7, 1.0, 1.5, 1.2], (2, 1))
    with pytest.raises(NotImplementedError, match="lists of sequences"):
        ChainEnsemble("lgssm", [np.zeros(20), np.zeros(30)], th, sampler="gibbs")
    with pytest.raises(NotImplementedError, match="whole series"):
        ChainEnsemble("lgssm", np.zeros(50), th, sampler="gibbs", subsequence_length=10)
    with pytest.raises(NotImplementedError, match="f64"):
        ChainEnsemble("lgssm", np.zeros(50), th, sampler="gibbs", dtype="f32")
