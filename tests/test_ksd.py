"""KSD evaluation: batched trace gradients + IMQ kernel Stein discrepancy."""
import numpy as np
import pytest

from oracle import ksd_oracle
from conftest import Golden
from test_host_logic import default_params, vec, SAMPLERS, run_windows_oracle
from sgmcmc_ssm_amd import particle_filters


@pytest.fixture(scope="module")
def golden_ksd():
    return Golden("ksd.npz")


def test_ksd_oracle_matches_reference(golden_ksd):
    for m in golden_ksd.meta:
        v = ksd_oracle.imq_ksd(golden_ksd.get(m["key"], "x"), golden_ksd.get(m["key"], "g"), c=m["c"], beta=m["beta"])
        ref = float(golden_ksd.get(m["key"], "value"))
        assert abs(v - ref) <= 1e-12 * ref, (m, v, ref)       # same terms, different summation order


def test_ksd_terms_match_oracle(golden_ksd):
    """imq_ksd_terms (longdouble sums of the signed and the absolute terms) restates imq_ksd: sqrt(tot) / K is its value
    on the four reference fixtures, also when several (c, beta) share one pass; abs_tot bounds |tot|."""
    assert len(golden_ksd.meta) == 4
    for m in golden_ksd.meta:
        x, g = golden_ksd.get(m["key"], "x"), golden_ksd.get(m["key"], "g")
        tot, abs_tot = ksd_oracle.imq_ksd_terms(x, g, c=m["c"], beta=m["beta"])
        assert tot.dtype == np.longdouble and 0 < tot <= abs_tot
        v = ksd_oracle.imq_ksd(x, g, c=m["c"], beta=m["beta"])
        assert abs(float(np.sqrt(tot) / x.shape[0]) - v) <= 1e-13 * v, (m, tot, v)
        ref = float(golden_ksd.get(m["key"], "value"))
        assert abs(float(np.sqrt(tot) / x.shape[0]) - ref) <= 1e-12 * ref, (m, tot, ref)
        both = ksd_oracle.imq_ksd_terms(x, g, c=[m["c"], 2.0], beta=[m["beta"], 0.3], rows=7)
        assert abs(both[0][0] - tot) <= 1e-17 * abs_tot and abs(both[0][1] - abs_tot) <= 1e-17 * abs_tot
        assert abs(float(np.sqrt(both[1][0]) / x.shape[0]) - ksd_oracle.imq_ksd(x, g, c=2.0, beta=0.3)) <= 1e-13 * v
    with pytest.raises(ValueError):
        ksd_oracle.imq_ksd_terms(np.zeros((3, 2)), np.zeros((3, 1)))


def _trace(model, K=5):
    rs = np.random.RandomState(8)
    plist = []
    for _ in range(K):
        p = default_params(model)
        for k in p.var_dict:
            p.var_dict[k] = p.var_dict[k] * rs.uniform(0.9, 1.05)
        plist.append(p.project_parameters())
    return plist


def _check_trace_equals_loop(model, seq, cmp):
    from test_host_logic import GEN
    np.random.seed(5)
    y = GEN[model](T=120, parameters=default_params(model))["observations"]
    Sampler, SeqSampler = SAMPLERS[model]
    if seq:
        sampler = SeqSampler(n=1, m=1, observations=[y[:50], y[50:90], y[90:]], parameters=default_params(model))
        kw = dict(kind="pf", pf="poyiadjis_N", N=64, subsequence_length=8, buffer_length=2, num_sequences=2,
                  is_scaled=False)
    else:
        sampler = Sampler(n=1, m=1, observations=y, parameters=default_params(model))
        kw = dict(kind="pf", pf="nemeth", N=64, subsequence_length=16, buffer_length=3, minibatch_size=2)
    plist = _trace(model)
    before = sampler.parameters
    np.random.seed(42)
    batched = sampler.noisy_gradient_trace(plist, **kw)
    assert sampler.parameters is before
    np.random.seed(42)
    looped = []
    for p in plist:
        sampler.parameters = p
        looped.append(sampler.noisy_gradient(**kw))
    for a, b in zip(batched, looped):
        cmp(vec(model, a), vec(model, b))


@pytest.mark.parametrize("model,seq", [("svm", False), ("garch", True), ("lgssm", False), ("svm", True)])
def test_gradient_trace_equals_loop_cpu(monkeypatch, model, seq):
    monkeypatch.setattr(particle_filters, "run_windows", run_windows_oracle)
    _check_trace_equals_loop(model, seq, np.testing.assert_array_equal)


@pytest.mark.gpu
def test_imq_ksd_kernel_matches_reference(golden_ksd):
    from sgmcmc_ssm_amd.trace_metric_functions import IMQ_KSD, compute_KSD
    for m in golden_ksd.meta:
        x, g = golden_ksd.get(m["key"], "x"), golden_ksd.get(m["key"], "g")
        v = IMQ_KSD(x, g, c=m["c"], beta=m["beta"])
        ref = float(golden_ksd.get(m["key"], "value"))
        assert abs(v - ref) <= 1e-10 * ref, (m, v, ref)
    # compute_KSD on a Parameters trace
    plist = _trace("svm", 12)
    rs = np.random.RandomState(2)
    grads = [[rs.normal(size=(1, 1)), rs.normal(size=1), rs.normal(size=1)] for _ in plist]
    res = compute_KSD(plist, grads, variables=["A", "LQinv_vec", "LRinv_vec"])
    for ii, var in enumerate(["A", "LQinv_vec", "LRinv_vec"]):
        x = np.array([np.asarray(getattr(p, var)).flatten() for p in plist])
        g = np.array([np.asarray(gr[ii]).flatten() for gr in grads])
        assert abs(res[var] - ksd_oracle.imq_ksd(x, g)) <= 1e-10 * res[var]
    with pytest.raises(ValueError):
        IMQ_KSD(np.zeros((3, 2)), np.zeros((3, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("model,seq", [("svm", False), ("garch", True)])
def test_gradient_trace_equals_loop_gpu(model, seq):
    _check_trace_equals_loop(model, seq, lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9))


# ---- imq_ksd_kernel past one block, one wave and one grid stride -------------------------------------------------------
_CB = [(1.0, 0.5), (0.1, 0.05), (10.0, 0.95)]
_KD = [(1, 3), (2, 1), (63, 8), (64, 8), (65, 8), (255, 5), (256, 5), (257, 5), (1023, 1), (1024, 1), (1025, 1), (2500, 8)]


def _ksd_bound(K, d, abs_tot):
    """|tot_kernel - tot| <= (A + 4 d + 32) 2^-53 abs_tot, derived from the kernel's summation and not measured: A serial
    additions on the longest path -- ceil(K / 256) * ceil(K / nblk) per thread, 6 for the wave sum, 3 across the waves,
    nblk in the host loop (nblk = min(K, 1024) blocks) --, 4 d roundings in the inner products of one term, and 32 for
    pow, the divisions, the term's own additions and the square root taken and undone.  One pair dropped or counted
    twice at K = 2500 moves tot by about 1e-7 of abs_tot, six orders above this."""
    nblk = min(K, 1024)
    A = -(-K // 256) * -(-K // nblk) + 6 + 3 + nblk
    return (A + 4 * d + 32) * 2.0 ** -53 * abs_tot


def _check_tot(ctx, x, g, c, beta, terms=None):
    K, d = x.shape
    tot, abs_tot = terms if terms is not None else ksd_oracle.imq_ksd_terms(x, g, c, beta)
    v = ctx.imq_ksd(x, g, c=c, beta=beta)
    tot_kernel = np.longdouble(K * v) ** 2           # the signed sum itself: the square root hides cancellation
    err, bound = abs(tot_kernel - tot), _ksd_bound(K, d, abs_tot)
    print("ksd K={0} d={1} c={2} beta={3}: |tot_kernel - tot| / abs_tot = {4:.3g} (bound {5:.3g}), tot / abs_tot = {6:.3g}"
          .format(K, d, c, beta, float(err / abs_tot), float(bound / abs_tot), float(tot / abs_tot)))
    assert np.isfinite(v) and err <= bound, (K, d, c, beta, float(tot_kernel), float(tot), float(err), float(bound))


@pytest.fixture(scope="module")
def ksd_ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


@pytest.mark.gpu
@pytest.mark.parametrize("c,beta", _CB)
@pytest.mark.parametrize("K,d", _KD)
def test_imq_ksd_kernel_sum_over_all_pairs(ksd_ctx, K, d, c, beta):
    """K = 1, 2 (lanes and waves that add nothing), 63..65 at d = 8 (the xi[] / gi[] arrays' size), 255..257 (the
    j stride), 1023..1025 and 2500 (nblk = 1024 blocks, the grid stride over i), at beta near 0 and 1."""
    rs = np.random.RandomState(1000 * K + d)
    _check_tot(ksd_ctx, rs.normal(size=(K, d)), rs.normal(size=(K, d)), c, beta)


def _ksd_special(name):
    rs = np.random.RandomState(17)
    if name == "duplicated":                 # every row twice: diff2 = 0 off the diagonal
        x, g = rs.normal(size=(65, 3)), rs.normal(size=(65, 3))
        return np.repeat(x, 2, axis=0), np.repeat(g, 2, axis=0)
    if name == "clusters":                   # two clusters 1e3 apart: base spans six orders
        x = rs.normal(size=(300, 2))
        x[150:] += 1e3
        return x, rs.normal(size=(300, 2))
    x = rs.normal(size=(1500, 4))            # the exact score of a standard normal: the terms cancel
    return x, -x


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["duplicated", "clusters", "exact_score"])
def test_imq_ksd_kernel_special_inputs(ksd_ctx, name):
    x, g = _ksd_special(name)
    terms = ksd_oracle.imq_ksd_terms(x, g, [c for c, _ in _CB], [b for _, b in _CB])
    for (c, beta), t in zip(_CB, terms):
        _check_tot(ksd_ctx, x, g, c, beta, terms=t)


@pytest.mark.gpu
def test_imq_ksd_refusals(ksd_ctx):
    from sgmcmc_ssm_amd.trace_metric_functions import IMQ_KSD
    x = np.random.RandomState(3).normal(size=(5, 9))
    for call in (ksd_ctx.imq_ksd, IMQ_KSD):
        with pytest.raises(ValueError, match="need K >= 1 and 1 <= d <= 8"):
            call(x, x)
        for beta in (0.0, 1.0):
            with pytest.raises(ValueError, match=r"beta must be in \(0,1\)"):
                call(x[:, :3], x[:, :3], beta=beta)
        with pytest.raises(ValueError, match="need K >= 1 and 1 <= d <= 8"):
            call(np.zeros((0, 3)), np.zeros((0, 3)))
        with pytest.raises(ValueError, match="x and gradlogp dimensions do not match"):
            call(x[:, :3], x[:, :2])
        with pytest.raises(ValueError, match="x and gradlogp dimensions do not match"):
            call(x[:4, :3], x[:, :3])
    assert np.isfinite(ksd_ctx.imq_ksd(x[:, :8], x[:, :8]))          # d = 8 is the last size served


@pytest.mark.gpu
def test_imq_ksd_leaves_the_context_buffers_usable(ksd_ctx):
    """pfg_imq_ksd borrows the context's input and output buffers: a window run after a large KSD call gives what it
    gave just before it, bit for bit."""
    from oracle import pf_oracle as po
    rs = np.random.RandomState(4)
    N, T = 100, 6
    z0, u, z = po.draw_streams(rs, N, T)
    q = dict(model="svm", kernel="prior", smoother="nemeth", stat="score", dtype="f64", rng="replay", N=N, t1=1, tL=5,
             lambduh=0.9, prior_mean=0.0, prior_var=1.0, y=rs.normal(size=T), theta=[0.9, 1.3, 0.8], z0=z0, u=u, z=z)
    before = ksd_ctx.run_batch([dict(q)])[0]
    x, g = rs.normal(size=(2500, 8)), rs.normal(size=(2500, 8))
    v = ksd_ctx.imq_ksd(x, g)
    after = ksd_ctx.run_batch([dict(q)])[0]
    assert np.all(np.isfinite(before["mean_stat"])) and np.any(before["mean_stat"] != 0.0) and np.isfinite(before["loglik"])
    assert np.array_equal(after["mean_stat"], before["mean_stat"]) and after["loglik"] == before["loglik"]
    assert ksd_ctx.imq_ksd(x, g) == v            # and the KSD after a window, on buffers the window resized or refilled
