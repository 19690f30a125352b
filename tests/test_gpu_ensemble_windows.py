"""GPU: ChainEnsemble with several windows per chain and step (minibatch_size, num_sequences) -- the multi-window path:
pfg_sample_windows_multi_device writes C * W descriptors, one particle-filter launch runs them, pfg_reduce_windows_device
combines each chain's W records in the reference's order.  One step is checked bitwise against ctx.run_batch of the
device-written windows and the NumPy restatement of the reduction (tests/helpers/window_reduce.py); the sampler against
its invariants and chi-square tests; the mean gradient against the drop-in Seq sampler; replay, partitions and resume
bitwise; the exchange-rate LD row (every EUR/USD segment, whole, PaRIS) end to end."""
import os
import sys

import numpy as np
import pytest
import scipy.stats

from test_host_logic import default_params, GEN, eurus_segments, vec

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import device_windows  # noqa: E402
import window_reduce  # noqa: E402

pytestmark = pytest.mark.gpu


def _series(model, T, seed=5):
    np.random.seed(seed)
    return GEN[model](T=T, parameters=default_params(model))["observations"]


def _segments(model, lengths, seed=6):
    y = _series(model, int(sum(lengths)), seed=seed)
    cuts = np.concatenate([[0], np.cumsum(lengths)])
    return [y[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


_device_windows = device_windows.ensemble_windows       # (records, y offset, weights offset or -1, sequence lengths)


def _restate_step(ens, y_host, theta, pf, dtype):
    """run_batch of the windows the device wrote at step 0 (seed, stream = g * W + w) + the host reduction."""
    from sgmcmc_ssm_amd import _capi
    from sgmcmc_ssm_amd.particle_filters import make_problem
    d, yoff, woff, seq_len = _device_windows(ens)
    wtab = ens.weights_dev.cpu().numpy() if ens.weights_dev is not None else None
    probs = []
    for i in range(ens.C * ens.W):
        T, t1, tL = int(d["T"][i]), int(d["t1"][i]), int(d["tL"][i])
        w = None if woff[i] < 0 else wtab[woff[i]:woff[i] + (tL - t1)]
        kw = dict(Ntilde=int(d["Ntilde"][i]), max_accept_reject=int(d["max_accept_reject"][i])) if pf == "paris" else {}
        if pf == "nemeth":
            kw["lambduh"] = float(d["lambduh"][i])
        probs.append(make_problem(ens.model, ens.kernel, pf, y_host[yoff[i]:yoff[i] + T], theta, ens.N, t1=t1, tL=tL,
                                  weights=w, prior_mean=float(d["prior_mean"][i]), prior_var=float(d["prior_var"][i]),
                                  flags=int(d["flags"][i]), dtype=dtype, rng="device", seed=ens.seed,
                                  stream=int(d["stream"][i]), **kw))
    outs = ens.ctx.run_batch(probs)
    h = _capi.STAT_DIM[ens.model]
    recs = np.zeros((len(probs), 8))
    recs[:, :h] = [o["mean_stat"] for o in outs]
    recs[:, 4] = [o["loglik"] for o in outs]
    red = window_reduce.reduce_windows(recs, seq_len, ens.K_eff, ens.M, ens._rescale, ens.T)
    return red, recs, d, yoff, seq_len


def _check_step(ens, y_host, theta, pf, dtype):
    ens.step(1)
    ens.synchronize()
    variant = ens.ctx.last_variant()
    g, ll = ens.last_gradient_statistics()
    win, _ = ens.window_statistics()
    red, recs, d, yoff, seq_len = _restate_step(ens, y_host, theta, pf, dtype)
    assert ens.ctx.last_variant() == variant            # the same kernel served both (the batch size takes part)
    h = g.shape[1]
    np.testing.assert_array_equal(win.reshape(-1, 8)[:, :h], recs[:, :h])
    np.testing.assert_array_equal(win.reshape(-1, 8)[:, 4], recs[:, 4])
    assert g.tobytes() == red[:, :h].tobytes() and ll.tobytes() == red[:, 4].tobytes()
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(ll))
    return variant, d, yoff, seq_len


CASES = [
    # model, list lengths (None = one series of T), K, M, S, B, pf, dtype, N, C, variant
    ("svm", None, None, 3, 20, 5, "poyiadjis_N", "f64", 100, 64, None),
    ("garch", [40, 12, 25, 60, 33], 3, 2, 16, 4, "nemeth", "f64", 128, 48, None),
    ("svm", [40, 12, 25, 60, 33], -1, 1, 16, 4, "paris", "f64", 100, 32, "paris64x2"),
    ("lgssm", [40, 12, 25, 60, 33], 3, 1, -1, 0, "poyiadjis_N", "f32", 200, 40, None),
    ("svm", [40, 12, 25, 60], -1, 1, -1, 0, "paris", "f64", 2000, 2, "paris_mem1024"),
    ("svm", None, None, 1, -1, 0, "paris", "f64", 1500, 3, "paris_mem1024"),
]


@pytest.mark.parametrize("case", CASES, ids=["single_M3", "garch_K3_M2_nemeth", "paris_all", "lgssm_f32_K3",
                                             "paris_N2000", "paris_W1_N1500"])
def test_one_step_equals_run_batch(case):
    """Every window record and every chain's reduced record after one step equal ctx.run_batch of the device-written
    windows (device generator, seed, stream = global chain * W + window, step 0) reduced on the host, bit for bit."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    model, lengths, K, M, S, B, pf, dtype, N, C, variant = case
    p = default_params(model)
    if lengths is None:
        obs = _series(model, 200).reshape(-1)
        y_host = obs
    else:
        obs = [s.reshape(-1) for s in _segments(model, lengths)]
        y_host = np.concatenate(obs)
    ens = ChainEnsemble(model, obs, p, num_chains=C, N=N, pf=pf, epsilon=1e-4, dtype=dtype, seed=17, chain_offset=5,
                        subsequence_length=S, buffer_length=B, minibatch_size=M, num_sequences=K,
                        window_sampling="device")
    assert ens._multi and ens.W == M * (1 if lengths is None else (len(lengths) if K == -1 else K))
    got, d, yoff, seq_len = _check_step(ens, y_host, p.theta(), pf, dtype)
    if variant:
        assert got == variant
    assert np.all(d["stream"] == (np.repeat(np.arange(C), ens.W) + 5) * ens.W + np.tile(np.arange(ens.W), C))


def test_sampler_invariants_and_uniformity():
    """Windows stay inside their sequence, a chain's sequences are distinct, a sequence no longer than S is taken whole;
    over many chains the sequence counts and the window starts are uniform (chi-square)."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    lengths = [40, 12, 25, 60, 33, 9, 50]
    segs = [s.reshape(-1) for s in _segments("svm", lengths)]
    cuts = np.concatenate([[0], np.cumsum(lengths)])
    S, B, K, M, C = 16, 4, 3, 4, 4096
    ens = ChainEnsemble("svm", segs, default_params("svm"), num_chains=C, N=32, epsilon=1e-4, seed=29,
                        subsequence_length=S, buffer_length=B, minibatch_size=M, num_sequences=K, window_sampling="device")
    ens.launch_windows()
    ens.synchronize()
    d, yoff, _, seq_len = _device_windows(ens)
    seq = np.searchsorted(cuts, yoff, side="right") - 1
    lo, hi = cuts[seq], cuts[seq + 1]
    assert np.all(yoff >= lo) and np.all(yoff + d["T"] <= hi)
    assert np.all(seq_len == hi - lo)
    per = seq.reshape(C, K, M)
    assert np.all(per == per[:, :, :1])                               # the M windows of a sequence share it
    first = per[:, :, 0]
    assert all(len(set(r)) == K for r in first)                       # distinct within a chain-step
    start = yoff + d["t1"] - lo
    length = d["tL"] - d["t1"]
    short = (hi - lo) <= S
    assert np.all(length[short] == (hi - lo)[short]) and np.all(start[short] == 0) and np.all(length[~short] == S)
    assert np.all(d["t1"][~short] == np.minimum(start[~short], B))
    # sequence counts: each of the n_seq sequences is in a chain's K draws with probability K / n_seq
    counts = np.bincount(first.reshape(-1), minlength=len(lengths))
    assert scipy.stats.chisquare(counts).pvalue > 1e-4, counts
    # the first draw alone is uniform too (the order is random)
    assert scipy.stats.chisquare(np.bincount(first[:, 0], minlength=len(lengths))).pvalue > 1e-4
    # window starts inside the longest sequence: uniform on 0..T_k - S
    k = int(np.argmax(lengths))
    st = start[seq == k]
    assert scipy.stats.chisquare(np.bincount(st, minlength=lengths[k] - S + 1)).pvalue > 1e-4
    # the next step draws other windows; the same step again the same ones
    before = ens.desc_dev.clone()
    ens.launch_windows()
    assert bool((ens.desc_dev == before).all())
    ens.step_ctr.add_(1)
    ens.launch_windows()
    assert not bool((ens.desc_dev == before).all())


def test_mean_gradient_matches_drop_in():
    """The mean reduced gradient of 2048 chains against SeqSVMSampler._noisy_grad_loglikelihood(num_sequences=K,
    minibatch_size=M, rng='device') over 300 draws, within 5 standard errors."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    from sgmcmc_ssm_amd.models.svm import SeqSVMSampler
    p = default_params("svm")
    segs = _segments("svm", [40, 12, 25, 60, 33])
    S, B, K, M, N, C = 16, 4, 2, 3, 128, 2048
    ens = ChainEnsemble("svm", [s.reshape(-1) for s in segs], p, num_chains=C, N=N, epsilon=1e-4, seed=41,
                        subsequence_length=S, buffer_length=B, minibatch_size=M, num_sequences=K, window_sampling="device")
    ens.step(1)
    g, _ = ens.last_gradient_statistics()
    sampler = SeqSVMSampler(n=1, m=1, observations=segs, parameters=p.copy())
    np.random.seed(3)
    ref = np.array([vec("svm", sampler._noisy_grad_loglikelihood(
        num_sequences=K, minibatch_size=M, kind="pf", pf="poyiadjis_N", N=N, subsequence_length=S, buffer_length=B,
        rng="device")) for _ in range(300)])
    got = g[:, [2, 1, 0]]                            # score columns [LRinv, LQinv, A] -> var_dict order
    se = np.sqrt(got.var(axis=0) / C + ref.var(axis=0) / len(ref))
    z = np.abs(got.mean(axis=0) - ref.mean(axis=0)) / se
    assert np.all(z < 5.0), (z, got.mean(axis=0), ref.mean(axis=0))


def test_replay_partitions_and_resume_are_bitwise():
    """Graph replay of a device-sampled list ensemble equals eager steps; two chain_offset partitions equal one
    ensemble; a state_dict resume continues bit for bit."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    p = default_params("svm")
    segs = [s.reshape(-1) for s in _segments("svm", [40, 12, 25, 60, 33])]
    kw = dict(N=64, epsilon=1e-3, seed=9, subsequence_length=16, buffer_length=4, minibatch_size=2, num_sequences=2,
              window_sampling="device")
    a = ChainEnsemble("svm", segs, p, num_chains=96, **kw).run(6, thin=2, graph_steps=2)
    b = ChainEnsemble("svm", segs, p, num_chains=96, **kw).run(6, thin=2)
    assert np.all(np.isfinite(a))
    np.testing.assert_array_equal(a, b)
    # the demos' SGLD row on the list (one sequence, one window per step), device-sampled: replay = eager
    one = dict(kw, minibatch_size=1, num_sequences=1)
    e1 = ChainEnsemble("svm", segs, p, num_chains=64, **one)
    assert e1._multi and e1.W == 1
    np.testing.assert_array_equal(e1.run(4, thin=4, graph_steps=4), ChainEnsemble("svm", segs, p, num_chains=64, **one).run(4, thin=4))
    # partitions
    lo = ChainEnsemble("svm", segs, p, num_chains=40, chain_offset=0, **kw)
    hi = ChainEnsemble("svm", segs, p, num_chains=56, chain_offset=40, **kw)
    lo.step(3)
    hi.step(3)
    one_ensemble = ChainEnsemble("svm", segs, p, num_chains=96, **kw).run(3, thin=3)[-1]
    np.testing.assert_array_equal(np.concatenate([lo.theta(), hi.theta()]), one_ensemble)
    # resume
    full = ChainEnsemble("svm", segs, p, num_chains=32, sampler="sghmc", **kw)
    full.step(2)
    st = full.state_dict()
    full.step(3)
    again = ChainEnsemble("svm", segs, p, num_chains=32, sampler="sghmc", **kw)
    again.load_state_dict(st)
    again.step(3)
    np.testing.assert_array_equal(full.theta(), again.theta())


@pytest.mark.parametrize("model", ["svm", "garch"])
def test_exchange_rate_ld_row(model):
    """The LD row of the exchange-rate demos (fit_timed(iter_type='SGLD', subsequence_length=-1, num_sequences=-1,
    buffer_length=0, pf='paris')) on the 49 EUR/USD segments: every segment whole, W = 49 windows per chain; N = 256 and
    N = 2000 (paris_mem1024); SGLD and SGHMC steps stay finite, and the first step equals the run_batch restatement."""
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    _, segs = eurus_segments()
    segs = [s.reshape(-1) for s in segs]
    y_host = np.concatenate(segs)
    p = default_params(model)
    for N, C in ((256, 4), (2000, 2)):
        kw = dict(N=N, pf="paris", epsilon=0.1 / 5907, subsequence_length=-1, buffer_length=0, num_sequences=-1, seed=N)
        ens = ChainEnsemble(model, segs, p, num_chains=C, **kw)
        assert ens.W == 49 and not ens._draws and not ens._rescale
        variant, d, _, seq_len = _check_step(ens, y_host, p.theta(), "paris", "f64")
        assert variant == ("paris_mem1024" if N > 1024 else "paris256x1")
        assert np.all(d["t1"] == 0) and np.all(d["tL"] == d["T"]) and np.all(d["T"] == seq_len)
        assert sorted(seq_len[:49]) == sorted(len(s) for s in segs)
        s = ens.run(2, thin=1, graph_steps=1)
        assert np.all(np.isfinite(s))
        h = ChainEnsemble(model, segs, p, num_chains=C, sampler="sghmc", **kw)
        assert np.all(np.isfinite(h.run(3, thin=3)))


def test_refusals():
    from sgmcmc_ssm_amd.ensemble import ChainEnsemble
    y = _series("svm", 60).reshape(-1)
    p = default_params("svm")
    segs = [s.reshape(-1) for s in _segments("svm", [20, 30, 10])]
    lg = _series("lgssm", 40).reshape(-1)
    plg = default_params("lgssm")
    with pytest.raises(NotImplementedError, match="gibbs"):
        ChainEnsemble("lgssm", lg, plg, num_chains=4, sampler="gibbs", minibatch_size=2)
    with pytest.raises(NotImplementedError, match="kind='pf' only"):
        ChainEnsemble("lgssm", lg, plg, num_chains=4, kind="marginal", minibatch_size=2, subsequence_length=10)
    with pytest.raises(NotImplementedError, match="window_sampling='device'"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, minibatch_size=2, subsequence_length=10, buffer_length=2)
    with pytest.raises(NotImplementedError, match="window_sampling='device'"):
        ChainEnsemble("svm", segs, p, num_chains=4, N=64, num_sequences=2)
    for K in (0, 4, -2):
        with pytest.raises(ValueError, match="num_sequences"):
            ChainEnsemble("svm", segs, p, num_chains=4, N=64, num_sequences=K, window_sampling="device")
    with pytest.raises(ValueError, match="num_sequences = 1"):
        ChainEnsemble("svm", y, p, num_chains=4, N=64, num_sequences=2)
    with pytest.raises(NotImplementedError, match="16384"):
        ChainEnsemble("svm", segs, p, num_chains=2, N=20000, pf="paris", num_sequences=-1)
    with pytest.raises(NotImplementedError, match="16384"):
        ChainEnsemble("svm", y, p, num_chains=2, N=20000, minibatch_size=2)
    # whole sequences with nothing to draw: 'host' is fine (no window is drawn)
    e = ChainEnsemble("svm", segs, p, num_chains=2, N=64, num_sequences=-1, subsequence_length=-1, buffer_length=0)
    assert e._multi and not e._draws
    # the single-window path keeps its limits when neither argument is passed
    with pytest.raises(NotImplementedError, match="N <= 1024"):
        ChainEnsemble("svm", y, p, num_chains=4, N=2000, pf="paris")
    assert e.ctx.scratch_bytes_smoother("svm", "f64", "device", "paris", 1000) == 0
    assert e.ctx.scratch_bytes_smoother("svm", "f64", "device", "paris", 2000) > 0
    assert e.ctx.scratch_bytes_smoother("svm", "f64", "device", "paris", 20000) == -1
