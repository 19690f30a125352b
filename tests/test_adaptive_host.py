"""CPU: ESS-triggered (adaptive) resampling, ess_threshold=tau (PFG_FLAG_ADAPTIVE_RESAMPLING) -- the restatement on the
oracle's pieces (tests/helpers/adaptive_model.py) against the oracle itself, what make_problem and ChainEnsemble's
device-free settings accept and refuse, the flag in the header and the binding, and the drop-in sampler on the stand-in."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from oracle import pf_oracle as po
from sgmcmc_ssm_amd import _capi, particle_filters
from sgmcmc_ssm_amd.ensemble import ChainEnsemble
from sgmcmc_ssm_amd.models.svm import SVMSampler
from test_host_logic import default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import adaptive_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
resolve = ChainEnsemble._resolve_settings
THETA = {"svm": [0.95, 1.4, 1.4], "garch": [0.0, 2.0, 2.0, 1.8], "lgssm": [0.9, 1.0, 1.2, 1.0]}
KERNEL = {"svm": "prior", "garch": "optimal", "lgssm": "optimal"}


@pytest.mark.parametrize("lam", [1.0, 0.9])
@pytest.mark.parametrize("model", ["svm", "garch", "lgssm"])
def test_always_resampling_is_the_oracle(model, lam):
    """always=True (base = 0 on every step) equals po.pf_window with absolute error 0: every trace, ancestors included."""
    N, T = 60, 14
    rs = np.random.RandomState(7)
    y = rs.normal(size=T)
    z0, u, z = po.draw_streams(rs, N, T)
    w = np.linspace(2.0, 3.0, 8)
    kw = dict(kernel=KERNEL[model], pf="nemeth", lambduh=lam, stat="score", t1=3, tL=11, weights=w, prior_mean=0.1, prior_var=2.0)
    got = adaptive_model.pf_window(model, THETA[model], y, N, z0, u, z, 0.5, always=True, **kw)
    ref = po.pf_window(model, THETA[model], y, N, z0, u, z, save_all=True, **kw)
    assert got["resampled"].all()
    for k in ("x_t", "log_weights", "statistics", "mean_statistic", "all_x_t", "all_log_weights", "all_statistics",
              "all_loglikelihood_estimate", "all_ancestors"):
        assert np.max(np.abs(np.asarray(got[k], dtype=float) - np.asarray(ref[k], dtype=float))) == 0.0, k
    assert got["loglikelihood_estimate"] == ref["loglikelihood_estimate"]


def test_adaptive_window_keeps_particles_and_carries_weights():
    """tau = 0.5: both branches run; a step that does not resample has identity ancestors and log-weights whose
    normalisation is the carried one (mean of exp(base) is 1), and the decision is the fp64 rule on the current weights."""
    N, T = 100, 24
    rs = np.random.RandomState(11)
    y = rs.normal(size=T)
    z0, u, z = po.draw_streams(rs, N, T)
    o = adaptive_model.pf_window("svm", THETA["svm"], y, N, z0, u, z, 0.5, t1=2, tL=22, prior_var=10.0)
    r = o["resampled"]
    assert 1 <= r.sum() <= T - 1 and o["margin"] > 0
    ident = np.all(o["all_ancestors"] == np.arange(N), axis=1)
    np.testing.assert_array_equal(ident, ~r)
    for t in range(T):
        lw = o["all_log_weights"][t]
        res, ess = adaptive_model.ess_decision(lw, 0.5)
        assert res == r[t] and (ess < 0.5 * N) == r[t]
        assert abs(np.mean(np.exp(adaptive_model.carried_base(lw))) - 1.0) < 1e-12
    # an underflowed weight keeps a finite carried log-weight
    base = adaptive_model.carried_base(np.array([0.0, -800.0, -5.0]))
    assert np.all(np.isfinite(base)) and base[1] < -790
    # tau = 1 resamples whenever the weights are not exactly uniform: from step 1 on
    one = adaptive_model.pf_window("svm", THETA["svm"], y, N, z0, u, z, 1.0, t1=2, tL=22, prior_var=10.0)
    assert not one["resampled"][0] and one["resampled"][1:].all()


def test_make_problem_off_is_todays_dict_and_on_draws_the_multinomial_stream():
    y, th = np.linspace(-1.0, 1.0, 12), default_params("svm").theta()
    qs = []
    for tau in ("absent", None, 0, 0.0):
        kw = {} if tau == "absent" else dict(ess_threshold=tau)
        qs.append(particle_filters.make_problem("svm", "prior", "poyiadjis_N", y, th, 100, t1=3, tL=9,
                                                random_state=np.random.RandomState(5), **kw))
    for q in qs[1:]:
        assert sorted(q) == sorted(qs[0]) and "ess_threshold" not in q and q["flags"] == qs[0]["flags"] == 0
        for k in q:
            if k != "_stream_bufs":
                np.testing.assert_array_equal(np.asarray(q[k]), np.asarray(qs[0][k]))
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    qm = particle_filters.make_problem("svm", "prior", "poyiadjis_N", y, th, 100, t1=3, tL=9, random_state=a)
    qa = particle_filters.make_problem("svm", "prior", "poyiadjis_N", y, th, 100, t1=3, tL=9, random_state=b, ess_threshold=0.5)
    assert (qa["smoother"], qa["ess_threshold"], qa["flags"]) == ("nemeth", 0.5, _capi.FLAG_ADAPTIVE_RESAMPLING)
    for k in ("z0", "u", "z"):
        np.testing.assert_array_equal(qm[k], qa[k])
    assert a.random_sample() == b.random_sample()
    qn = particle_filters.make_problem("garch", "optimal", "nemeth", y, [0.0, 2.0, 2.0, 1.8], 2000, rng="device", seed=3,
                                       stream=4, lambduh=0.9, ess_threshold=1.0, flags=_capi.FLAG_GARCH_STATIONARY_PRIOR)
    assert (qn["lambduh"], qn["ess_threshold"], qn["flags"]) == (0.9, 1.0, 17)


def test_make_problem_refusals():
    y, th = np.linspace(-1.0, 1.0, 12), default_params("svm").theta()
    mk = lambda pf="poyiadjis_N", N=100, **kw: particle_filters.make_problem(
        "svm", "prior", pf, y, th, N, rng="device", seed=1, stream=1, **kw)
    for pf in ("filter", "paris", "poyiadjis_N2"):
        with pytest.raises(NotImplementedError, match=r"built for pf = 'poyiadjis_N' \| 'nemeth', got pf = '{0}'".format(pf)):
            mk(pf, ess_threshold=0.5)
    with pytest.raises(NotImplementedError, match="not built for the predictive statistic"):
        mk(stat="predictive", ess_threshold=0.5)
    for mode in ("stratified", "systematic"):
        with pytest.raises(NotImplementedError, match="built for resampling='multinomial', got '{0}'".format(mode)):
            mk(resampling=mode, ess_threshold=0.5)
    with pytest.raises(NotImplementedError, match=re.escape("built for N <= 16384 (no whole-GPU windows)")):
        mk(N=16385, ess_threshold=0.5)
    for tau in (-0.1, 1.0001, 2, float("nan")):
        with pytest.raises(ValueError, match=re.escape("ess_threshold must be in (0, 1]")):
            mk(ess_threshold=tau)
    # elementwise statistics: refused by the Helper before anything is drawn
    sampler = SVMSampler(n=1, m=1, observations=y.reshape(-1, 1), parameters=default_params("svm"))
    state = np.random.get_state()[2]
    with pytest.raises(NotImplementedError, match="not built for elementwise statistics"):
        sampler.message_helper.pf_latent_var_distr(observations=y.reshape(-1, 1), parameters=sampler.parameters, N=50,
                                                   ess_threshold=0.5)
    assert np.random.get_state()[2] == state


@pytest.mark.parametrize("N", [64, 2000, 16384])
def test_resolve_settings_adaptive(N):
    svm = default_params("svm")
    s = resolve("svm", np.zeros(40), svm, num_chains=3, N=N, ess_threshold=0.5)
    assert (s.smoother, s.launch_smoother, s.lambduh, s.N, s.ess_threshold) == ("nemeth", "poyiadjis_n", 1.0, N, 0.5)
    s = resolve("svm", np.zeros(40), svm, num_chains=3, N=N, pf="nemeth", lambduh=0.9, ess_threshold=1)
    assert (s.smoother, s.lambduh, s.ess_threshold) == ("nemeth", 0.9, 1.0)
    s = resolve("svm", np.zeros(60), svm, num_chains=3, N=N, ess_threshold=0.25, minibatch_size=2, subsequence_length=10,
                buffer_length=2, window_sampling="device", sampler="sghmc")
    assert s.multi and s.W == 2 and s.ess_threshold == 0.25
    for off in (None, 0, 0.0):
        assert resolve("svm", np.zeros(40), svm, num_chains=3, N=N, ess_threshold=off).ess_threshold is None
    assert resolve("svm", np.zeros(40), svm, num_chains=3, N=N).ess_threshold is None


def test_resolve_settings_adaptive_refusals():
    svm, lg = default_params("svm"), default_params("lgssm")
    for pf in ("filter", "paris", "poyiadjis_N2"):
        with pytest.raises(NotImplementedError, match=r"built for pf = 'poyiadjis_N' \| 'nemeth', got pf = '{0}'".format(pf)):
            resolve("svm", np.zeros(40), svm, num_chains=2, N=100, pf=pf, ess_threshold=0.5)
    for mode in ("stratified", "systematic"):
        with pytest.raises(NotImplementedError, match="built for resampling='multinomial', got '{0}'".format(mode)):
            resolve("svm", np.zeros(40), svm, num_chains=2, N=100, resampling=mode, ess_threshold=0.5)
    with pytest.raises(NotImplementedError, match=re.escape("built for N <= 16384 (no whole-GPU windows), got N = 20000")):
        resolve("svm", np.zeros(40), svm, num_chains=2, N=20000, ess_threshold=0.5)
    with pytest.raises(NotImplementedError, match=re.escape("built for N <= 16384")):
        resolve("svm", np.zeros(40), svm, num_chains=2, N=16385, ess_threshold=0.5, minibatch_size=1)
    for kind in ("marginal", "complete"):
        with pytest.raises(NotImplementedError, match="needs a particle filter: kind='pf'"):
            resolve("lgssm", np.zeros(40), lg, num_chains=2, kind=kind, num_samples=2, ess_threshold=0.5)
    for tau in (-1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=re.escape("ess_threshold must be in (0, 1]")):
            resolve("svm", np.zeros(40), svm, num_chains=2, N=100, ess_threshold=tau)


def test_header_and_binding_agree_on_the_flag_and_the_abi_only_grew_at_the_end():
    src = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    m = re.search(r"#define\s+PFG_FLAG_ADAPTIVE_RESAMPLING\s+(\d+)u", src)
    assert m and int(m.group(1)) == 16 == _capi.FLAG_ADAPTIVE_RESAMPLING
    assert re.search(r"int\s+pfg_launch_device_adaptive\s*\(", src) and "pfg_launch_device_adaptive" in _capi.EXPORTS
    # no new smoother id, the same problem / descriptor sizes; the threshold sits where `reserved` sat.  (The flag came
    # without a version bump, at 125; 126 is pfg_result.trace_paris_J, appended behind everything that was there.)
    assert sorted(_capi.SMOOTHER.values()) == list(range(9))
    assert re.search(r"#define\s+PFG_VERSION\s+126\b", src)
    assert _capi.Result.trace_paris_J.offset == _capi.Result.paris_consumed.offset + 8 == C.sizeof(_capi.Result) - 8
    assert _capi.DEV_PROBLEM_DTYPE.itemsize == 376 and _capi.PROBLEM_DTYPE.itemsize == C.sizeof(_capi.Problem)
    assert _capi.Problem.reserved.offset == _capi.Problem.flags.offset + 4 == _capi.PROBLEM_DTYPE.fields["reserved"][1]
    assert _capi.Problem.reserved.size == 4 and _capi.Problem.lambduh.offset == _capi.Problem.flags.offset + 8
    f = _capi.DEV_PROBLEM_DTYPE.fields
    assert f["reserved"][1] == f["flags"][1] + 4 and f["paris_idx_u"][1] == f["flags"][1] + 8
    assert len(re.findall(r"int32_t reserved;", src)) == 2
    # the encoding the header states: the bits of an IEEE binary32
    assert [_capi.ess_threshold_bits(t) for t in (None, 0, 0.25, 0.5, 0.75, 1.0)] == \
        [0, 0, 0x3E800000, 0x3F000000, 0x3F400000, 0x3F800000] and "0x3F000000" in src
    assert [_capi.ess_threshold_from_bits(_capi.ess_threshold_bits(t)) for t in (0.25, 0.5, 0.75, 1.0)] == [0.25, 0.5, 0.75, 1.0]


def test_drop_in_fit_is_reproducible_and_differs_from_always_resampling(monkeypatch):
    """SVMSampler.fit(..., pf_kwargs=dict(ess_threshold=0.5)) on the stand-in: the same seed gives the same five steps,
    another trajectory than always-resampling from the first gradient on, and np.random ends where that run leaves it."""
    monkeypatch.setattr(particle_filters, "run_windows", adaptive_model.run_windows)
    np.random.seed(12)
    y = np.random.normal(size=(60, 1))

    def fit(**pf_kwargs):
        sampler = SVMSampler(n=1, m=1, observations=y, parameters=default_params("svm"))
        np.random.seed(4)
        plist = sampler.fit(iter_type="SGLD", num_iters=5, output_all=True, epsilon=0.01, subsequence_length=16,
                            buffer_length=4, kind="pf", pf_kwargs=dict(pf="poyiadjis_N", N=100, **pf_kwargs))
        return np.array([p.theta() for p in plist]), np.random.random_sample()

    a, ua = fit(ess_threshold=0.5)
    b, ub = fit(ess_threshold=0.5)
    m, um = fit()
    z, uz = fit(ess_threshold=0)
    assert a.shape == (6, 3) and np.all(np.isfinite(a))
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(m, z)
    assert ua == ub == um == uz
    np.testing.assert_array_equal(a[0], m[0])
    assert np.all(a[1] != m[1])
    # the helper's estimate is the restatement's on the same stream
    sampler = SVMSampler(n=1, m=1, observations=y, parameters=default_params("svm"))
    np.random.seed(3)
    g = sampler.message_helper.pf_gradient_estimate(observations=y, parameters=sampler.parameters, N=100,
                                                    subsequence_start=5, subsequence_end=50, ess_threshold=0.5)
    z0, u, zz = po.draw_streams(np.random.RandomState(3), 100, 60)
    ref = adaptive_model.pf_window("svm", default_params("svm").theta(), y, 100, z0, u, zz, 0.5, pf="poyiadjis_N", t1=5, tL=50,
                                   prior_mean=0.0, prior_var=10.0)
    assert 1 <= ref["resampled"].sum() <= 59
    got = np.array([float(np.reshape(g[k], -1)[0]) for k in ("LRinv_vec", "LQinv_vec", "A")])
    np.testing.assert_allclose(got, ref["mean_statistic"], rtol=1e-12)
