"""GPU: SMC^2 over resident PMMH chains -- the population kernels (csrc/pfg_seq.hip) against the long-double model
(tests/helpers/seq_model.py) and bitwise copies, the warm start the feature stands on, and SequentialPopulation: its
bookkeeping, determinism, checkpoints, extend(), the consistency of the particle systems after a move, and its law against
TemperedPopulation."""
import os
import sys

import numpy as np
import pytest

from test_host_logic import DATA_SEED, GEN, PRIORS, default_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
import seq_model as sq  # noqa: E402
import smc_model as sm  # noqa: E402

from test_seq_host import SEED, SHAPES  # noqa: E402

pytestmark = pytest.mark.gpu

LD = sq.LD


def _ctx():
    from sgmcmc_ssm_amd import _capi
    return _capi.default_context(0)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize(_dev())


# ---- 1. reweight against the model ----------------------------------------------------------------------------------------
def run_reweight(logw, incr, tau, seed, stage, stride=1, B=None):
    """pfg_seq_reweight_device -> dict(status, record [8], parent [B], logw [B], cdf); every output starts from a sentinel.
    stride 8: incr travels as column 4 of [B, 8] records, as the stage loop passes it."""
    import torch
    from sgmcmc_ssm_amd import _capi
    n = len(logw)
    B = n if B is None else B
    dev = _dev()
    logw_dev = torch.from_numpy(np.asarray(logw, dtype=np.float64).copy()).to(dev)
    if stride <= 1:
        incr_dev = torch.from_numpy(np.asarray(incr, dtype=np.float64).copy()).to(dev)
        incr_ptr = incr_dev.data_ptr()
    else:
        rec = np.full((n, stride), 777.0)
        rec[:, 4] = incr
        incr_dev = torch.from_numpy(rec).to(dev)
        incr_ptr = incr_dev.data_ptr() + 8 * 4
    record = torch.full((_capi.SEQ_RECORD_DOUBLES,), -7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    parent = torch.full((n,), -1, dtype=torch.int32, device=dev)
    cdf = torch.full((max(_capi.smc_scratch_bytes(n), 256) // 8,), -7.0, dtype=torch.float64, device=dev)
    _ctx().seq_reweight_device(B, logw_dev.data_ptr(), incr_ptr, stride, tau, seed, stage, record.data_ptr(), status.data_ptr(),
                               parent.data_ptr(), cdf.data_ptr(), _stream())
    _sync()
    return dict(status=int(status.item()), record=record.cpu().numpy(), parent=parent.cpu().numpy().astype(np.int64),
                logw=logw_dev.cpu().numpy(), cdf=cdf.cpu().numpy())


def _untouched(out, logw):
    return (np.all(out["record"] == -7.0) and np.all(out["parent"] == -1) and np.all(out["cdf"] == -7.0)
            and np.array_equal(out["logw"], np.asarray(logw, dtype=np.float64), equal_nan=True))


@pytest.mark.parametrize("B", SHAPES)
def test_reweight_kernel_matches_the_model(B):
    """Every weight pattern at one population size: one chain per thread (B <= 1024), the 1 -> 2 chains-per-thread switch
    (1025), idle threads and a ragged last thread (4097).  The evidence increment and the ESS agree with the long-double
    model to 1e-12 relative; a new log-weight, a difference of numbers of size up to 60 whose operands are rounded to
    2^-52 of that, to 1e-12 of max(|logw|, 1) with -inf exactly -inf; the trigger is the model's; the uniform is the keyed one;
    EVERY parent is the one the model's search selects -- the inputs keep each target 1e-9 W off the CDF entries
    (tests/test_seq_host.py checks that on the CPU), so no child is exempt.  incr is read with stride 1 and, as the stage loop
    passes it, as column 4 of [B, 8] records."""
    for k, pattern in enumerate(sq.PATTERNS):
        stage = 3 + k + (1 << 33) * (k % 2)                 # the high word of the stage takes part in the key
        u = sm.stage_uniform(SEED, stage)
        logw, incr, tau = sq.case(B, pattern)
        logw, incr, want = sq.move_off_the_cdf(logw, incr, tau, u)
        assert want["status"] == 0
        for stride in (1, 8):
            got = run_reweight(logw, incr, tau, SEED, stage, stride=stride)
            assert got["status"] == 0, (pattern, got["status"])
            increment, ess, resampled, u_dev, vmax, W = got["record"][:6]
            rel = lambda a, b: float(abs(LD(a) - b) / abs(b))
            print(B, pattern, stride, "incr", increment, "rel", rel(increment, want["increment"]), "ess", ess, "rel",
                  rel(ess, want["ess"]), "resampled", resampled, "min gap", None if want["gap"] is None else want["gap"].min())
            assert u_dev == float(u) and vmax == float(want["vmax"])
            assert rel(increment, want["increment"]) <= 1e-12 and rel(ess, want["ess"]) <= 1e-12
            assert bool(resampled) == want["resampled"] and resampled in (0.0, 1.0)
            np.testing.assert_array_equal(got["parent"], want["parent"])
            dead = np.isneginf(want["logw"].astype(float))
            np.testing.assert_array_equal(np.isneginf(got["logw"]), dead)
            err = np.abs(got["logw"][~dead].astype(LD) - want["logw"][~dead]) / np.maximum(np.abs(want["logw"][~dead]), 1)
            assert err.max() <= 1e-12, float(err.max())
            if want["resampled"]:
                assert not got["logw"].any()
                assert np.max(np.abs(got["cdf"][:B].astype(LD) - want["cdf"])) <= 1e-12 * want["W"]
            if pattern == "equal":
                assert increment == -41.25 and not resampled
                assert np.max(np.abs(sq.normalised(got["logw"]) - sq.normalised(logw))) <= 1e-15
            if pattern == "all_but_one_minus_inf":
                assert abs(ess - 1.0) <= 1e-15 and (B == 2 or np.all(got["parent"] == (2 * B) // 3))
            if pattern == "one_minus_inf" and want["resampled"]:
                assert B // 2 not in got["parent"]


def test_reweight_kernel_flags_and_errors():
    """No finite v (every incr -inf; every logw -inf; the two disjoint), a NaN or +inf in either array, and a B outside
    2 .. 2^20 set the status and store nothing else; a NULL argument, a negative stride and an ess_target outside (0, 1] are
    errors of the call."""
    z = np.zeros(1500)
    cases = [(z, np.full(1500, -np.inf), sq.NO_FINITE), (np.full(1500, -np.inf), z, sq.NO_FINITE),
             (np.r_[-np.inf, 0.0], np.r_[0.0, -np.inf], sq.NO_FINITE), (z, np.r_[z[:-1], np.nan], sq.NOT_A_NUMBER),
             (z, np.r_[np.inf, z[:-1]], sq.NOT_A_NUMBER), (np.r_[z[:70], np.nan], np.r_[z[:70], 0.0], sq.NOT_A_NUMBER),
             (np.r_[z[:70], np.inf], np.r_[z[:70], 0.0], sq.NOT_A_NUMBER)]
    for logw, incr, flag in cases:
        assert sq.reweight(logw, incr, 0.5, 0.5)["status"] == flag
        got = run_reweight(logw, incr, 0.5, SEED, 0)
        assert got["status"] == flag and _untouched(got, logw), (flag, got["status"])
    for B in (1, 0, -5, (1 << 20) + 1):
        got = run_reweight(np.zeros(4), np.zeros(4), 0.5, SEED, 0, B=B)
        assert got["status"] == sq.BAD_B and _untouched(got, np.zeros(4)), B
    for tau in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_target"):
            run_reweight(np.zeros(8), np.zeros(8), tau, SEED, 0)
    with pytest.raises(ValueError, match="incr_stride"):
        run_reweight(np.zeros(8), np.zeros(8), 0.5, SEED, 0, stride=-1)
    # ess_target = 1: any inequality among the weights resamples, equal weights do not
    assert run_reweight(np.zeros(64), np.zeros(64), 1.0, SEED, 0)["record"][2] == 0.0
    assert run_reweight(np.r_[np.zeros(63), 0.5], np.zeros(64), 1.0, SEED, 0)["record"][2] == 1.0


# ---- 2. gather, bitwise -----------------------------------------------------------------------------------------------------
ROWS = [2 * 2, 3 * 2, 127 * 2, 129 * 3, 1000 * 2, 1025 * 3, 4097 * 2]        # N (NS + 1): even and odd, NS = 1 and 2


@pytest.mark.parametrize("row", ROWS)
def test_gather_is_bitwise(row):
    """dst row b = src row parent[b], theta and ll with it, for C in {2, 65, 1024} and the parents identity, all 0, reversed
    and random; dst (and, at C = 65, src) starts 8 bytes off a 16-byte boundary, so that rows of odd length put both kinds of
    row alignment on either side; guard words around dst and every word of src stay as they were.  The payload carries NaN
    and -inf patterns: a copy moves bits."""
    import torch
    dev, ctx = _dev(), _ctx()
    for C in (2, 65, 1024):
        rng = np.random.default_rng([row, C])
        src = rng.normal(size=(C, row))
        src[0, 0], src[C - 1, row - 1], src[C // 2, row // 2] = np.nan, -np.inf, -0.0
        theta, ll = rng.normal(size=(C, 4)), rng.normal(size=C)
        guard, lead = 5, (3 if C != 1024 else 4)                # lead 3: dst starts 8 bytes off 16
        s_off = 1 if C == 65 else 0
        src_dev = torch.zeros(C * row + 2, dtype=torch.float64, device=dev)
        src_dev[s_off:s_off + C * row] = torch.from_numpy(src.reshape(-1)).to(dev)
        src_view = src_dev[s_off:s_off + C * row]
        for name, parent in (("identity", np.arange(C)), ("all 0", np.zeros(C, dtype=np.int64)), ("reversed", np.arange(C)[::-1]),
                             ("random", rng.integers(0, C, size=C))):
            flat = torch.full((lead + C * row + guard,), -7.25, dtype=torch.float64, device=dev)
            dst = flat[lead:lead + C * row]
            th_dev, ll_dev = torch.from_numpy(theta).to(dev), torch.from_numpy(ll).to(dev)
            th_tmp, ll_tmp = torch.zeros_like(th_dev), torch.zeros_like(ll_dev)
            par = torch.from_numpy(np.ascontiguousarray(parent, dtype=np.int32)).to(dev)
            ctx.seq_gather_device(C, par.data_ptr(), row, src_view.data_ptr(), dst.data_ptr(), th_dev.data_ptr(), th_tmp.data_ptr(),
                                  ll_dev.data_ptr(), ll_tmp.data_ptr(), _stream())
            _sync()
            out = flat.cpu().numpy()
            assert np.all(out[:lead] == -7.25) and np.all(out[lead + C * row:] == -7.25), (C, name)
            got = out[lead:lead + C * row].reshape(C, row)
            np.testing.assert_array_equal(got.view(np.uint64), src[parent].view(np.uint64), err_msg="{0} {1}".format(C, name))
            np.testing.assert_array_equal(th_dev.cpu().numpy(), theta[parent], err_msg=name)
            np.testing.assert_array_equal(ll_dev.cpu().numpy(), ll[parent], err_msg=name)
        np.testing.assert_array_equal(src_view.cpu().numpy().view(np.uint64), src.reshape(-1).view(np.uint64))
    with pytest.raises(ValueError, match="must not alias"):
        ctx.seq_gather_device(2, par.data_ptr(), row, dst.data_ptr(), dst.data_ptr(), th_dev.data_ptr(), th_tmp.data_ptr(),
                              ll_dev.data_ptr(), ll_tmp.data_ptr(), _stream())
    with pytest.raises(ValueError, match="2 <= B <= 2\\^20"):
        ctx.seq_gather_device(1, par.data_ptr(), row, src_view.data_ptr(), dst.data_ptr(), th_dev.data_ptr(), th_tmp.data_ptr(),
                              ll_dev.data_ptr(), ll_tmp.data_ptr(), _stream())


# ---- 3. adopt ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [3 * 2, 129 * 3, 1000 * 2])
def test_adopt_copies_the_rows_whose_count_moved(row):
    """Only the rows whose acceptance count differs from `seen` change, bitwise to the fresh row; `seen` follows the counts;
    a second run is a no-op, also on a fresh buffer that has changed meanwhile."""
    import torch
    dev, ctx = _dev(), _ctx()
    for C in (2, 65, 1024):
        rng = np.random.default_rng([row, C, 3])
        cur, fresh = rng.normal(size=(C, row)), rng.normal(size=(C, row))
        seen = rng.integers(0, 5, size=C)
        moved = rng.random(C) < 0.4
        moved[0], moved[C - 1] = True, False
        n_accept = seen + moved
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        lead = 3
        flat = torch.full((lead + C * row + 4,), -7.25, dtype=torch.float64, device=dev)
        flat[lead:lead + C * row] = t(cur.reshape(-1))
        cur_dev = flat[lead:lead + C * row]
        fresh_dev, n_dev, seen_dev = t(fresh), t(n_accept.astype(np.int64)), t(seen.astype(np.int64))
        want = np.where(moved[:, None], fresh, cur)
        for attempt in range(2):
            ctx.seq_adopt_device(C, n_dev.data_ptr(), seen_dev.data_ptr(), row, cur_dev.data_ptr(), fresh_dev.data_ptr(), _stream())
            _sync()
            out = flat.cpu().numpy()
            assert np.all(out[:lead] == -7.25) and np.all(out[lead + C * row:] == -7.25)
            np.testing.assert_array_equal(out[lead:lead + C * row].reshape(C, row), want, err_msg="run {0}".format(attempt))
            np.testing.assert_array_equal(seen_dev.cpu().numpy(), n_accept)
            fresh_dev.fill_(123.0)              # the second run must not read it into any row
        np.testing.assert_array_equal(n_dev.cpu().numpy(), n_accept)


# ---- 4. the ground the feature stands on ------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["svm", "garch"])
@pytest.mark.parametrize("N", [100, 1025])
def test_ground_chunked_launches_are_the_one_shot_launch(model, N):
    """THE GROUND THE FEATURE STANDS ON -- this test passes without SequentialPopulation and the pfg_seq_* kernels: through
    ctx.run_batch on REPLAY streams, T = 12, a window split into (1, 11), (5, 7) and (4, 4, 4) and chained through init_x /
    init_logw <- x_t / log_weights gives the one-shot launch's final particles and log-weights bitwise, and the sum of the
    chunks' loglik is the one-shot value to 1e-12 relative."""
    from test_gpu_device_replay import THETA, _series
    T = 12
    rs = np.random.RandomState(N + len(model))
    y = _series(model, T, seed=N)
    z0, u, z = rs.normal(size=N), rs.random_sample((T, N)), rs.normal(size=(T, N))
    base = dict(model=model, kernel="prior", smoother="nemeth", stat="none", dtype="f64", rng="replay", N=N, lambduh=1.0,
                prior_mean=0.0, prior_var=1.0, theta=THETA[model])
    whole = _ctx().run_batch([dict(base, y=y, z0=z0, u=u, z=z)], want_final=True)[0]
    assert np.isfinite(whole["loglik"]) and np.all(np.isfinite(whole["x_t"]))
    for split in ((1, 11), (5, 7), (4, 4, 4)):
        t, ll, state = 0, 0.0, {}
        for k in split:
            q = dict(base, y=y[t:t + k], u=u[t:t + k], z=z[t:t + k], **state)
            if not state:
                q["z0"] = z0
            o = _ctx().run_batch([q], want_final=True)[0]
            state = dict(init_x=o["x_t"].copy(), init_logw=o["log_weights"].copy())
            ll += o["loglik"]
            t += k
        np.testing.assert_array_equal(o["x_t"], whole["x_t"], err_msg=str(split))
        np.testing.assert_array_equal(o["log_weights"], whole["log_weights"], err_msg=str(split))
        print(model, N, split, "loglik", ll, "one shot", whole["loglik"], "rel", abs(ll - whole["loglik"]) / abs(whole["loglik"]))
        assert abs(ll - whole["loglik"]) <= 1e-12 * abs(whole["loglik"])


# ---- 5 .. 8. SequentialPopulation -------------------------------------------------------------------------------------------
def _series(model, T):
    np.random.seed(DATA_SEED[model])
    return GEN[model](T=T, parameters=default_params(model))["observations"].reshape(-1)


def _prior(model):
    return PRIORS[model].generate_default_prior(var=1.0, n=1, m=1)


def _population(model="lgssm", T=20, y=None, C=256, N=32, chunk=5, seed=SEED, **kw):
    from sgmcmc_ssm_amd.sequential import SequentialPopulation
    y = _series(model, T) if y is None else y
    return SequentialPopulation(model, y, default_params(model), num_chains=C, N=N, chunk=chunk, seed=seed, prior=_prior(model), **kw)


def _snapshot(pop):
    e = pop.ensemble
    e.synchronize()
    return dict(theta=e.theta_dev.cpu().numpy(), ll=e.ll_dev.cpu().numpy(), weights=pop.weights(), logw=pop.logw_dev.cpu().numpy(),
                increments=pop.evidence_increments(), rows=pop.state_rows(), ctr=int(e.step_ctr.item()), launches=pop.launches,
                scale=e.scale_dev.cpu().numpy(), n=pop.accept_dev.cpu().numpy(), origin=pop.row_origin(), t=pop.t)


def _same(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_bookkeeping_identity():
    """LGSSM T = 20, C = 256, N = 32, chunk = 5 and an ess_target no stage falls below: the evidence telescopes,
    log_evidence() = log((1 / C) sum_i e^(h0_i + ll_i)) + log m(q0) to 1e-12 relative with h0 and the sum taken on the host in long
    double from the population's own theta and ll; every chain's ll is the sum of its extension records, bitwise; nothing
    moved, so theta is the initial population and the weights are the normalised e^(h0 + ll)."""
    pop = _population(ess_target=1e-6)
    e = pop.ensemble
    theta0 = e.theta()
    records = []
    assert pop.stage_index == 1 and pop.t == 0
    while pop.t < pop.T:
        assert pop.step(1) == 1
        records.append(e.out_dev[:, 4].cpu().numpy())
    assert pop.step(1) == 0 and pop.t == 20 and pop.stage_index == 5 and pop.launches == 4
    sched = pop.schedule()
    assert not sched["resampled"].any() and list(sched["t"]) == [0, 5, 10, 15, 20] and not sched["acceptance"].any()
    ll = np.zeros(256)
    for r in records:
        ll = ll + r
    np.testing.assert_array_equal(e.ll_dev.cpu().numpy(), ll)
    np.testing.assert_array_equal(e.theta(), theta0)
    h0 = sm.log_target("lgssm", sm.hyper_of("lgssm", _prior("lgssm")), theta0, np.zeros(256), pop.q0_mean, pop.q0_sd)
    v = h0 + ll.astype(LD)
    want = v.max() + np.log(np.exp(v - v.max()).sum() / LD(256)) + LD(sm.log_q0_mass("lgssm", pop.q0_mean, pop.q0_sd))
    print("log evidence", pop.log_evidence(), "host", float(want), "rel", float(abs(LD(pop.log_evidence()) - want) / abs(want)))
    assert abs(LD(pop.log_evidence()) - want) <= 1e-12 * abs(want)
    assert abs(pop.log_evidence() - (pop.evidence_increments().sum() + sm.log_q0_mass("lgssm", pop.q0_mean, pop.q0_sd))) < 1e-12
    assert np.max(np.abs(pop.weights() - sq.normalised(v))) <= 1e-12
    assert abs(pop.ess() - 1.0 / np.sum(pop.weights() ** 2)) < 1e-9
    assert np.max(np.abs(pop.posterior_mean() - (pop.weights()[:, None] * theta0).sum(0))) <= 1e-12


def test_determinism_checkpoints_and_extend():
    """ess_target = 0.9, so that stages resample on either side of every boundary used.  Two runs with one seed are bitwise
    equal in theta, weights, increments and particle systems; save after stage 2 (t = 10), load into a fresh population and
    continue is the uninterrupted run, bitwise; a population constructed on y[:10], run, extended by y[10:] and run is the one
    constructed on the whole series; a checkpoint of another chunk, tau or N is refused."""
    y = _series("lgssm", 20)
    kw = dict(ess_target=0.9, moves=2)
    whole = _population(y=y, **kw)
    info = whole.run()
    assert whole.t == 20 and info["resampled"][1:3].any() and info["resampled"][3:].any(), info["resampled"]
    assert 0.0 < info["acceptance"][info["resampled"] == 1].min() and info["acceptance"].max() < 1.0
    twin = _population(y=y, **kw)
    twin.run()
    a = _snapshot(whole)
    _same(a, _snapshot(twin))
    assert a["ctr"] == 1 + 2 * int(info["resampled"].sum()) and a["launches"] == 4 + 2 * int(info["resampled"].sum())

    first = _population(y=y, **kw)
    assert first.step(2) == 2 and first.t == 10
    state = first.state_dict()
    assert set(state) - {"sequential"} == set(first.ensemble.state_dict())
    resumed = _population(y=y, **kw)
    resumed.load_state_dict(state)
    _same(_snapshot(first), _snapshot(resumed))
    resumed.run()
    _same(a, _snapshot(resumed))
    again = resumed.schedule()
    for k in info:
        np.testing.assert_array_equal(info[k], again[k], err_msg=k)
    assert whole.log_evidence() == resumed.log_evidence()

    grown = _population(y=y[:10], **kw)
    grown.run()
    assert grown.t == 10 and grown.step(1) == 0
    _same(_snapshot(first), _snapshot(grown))
    grown.extend(y[10:])
    grown.run()
    _same(a, _snapshot(grown))
    for other in (dict(chunk=4), dict(ess_target=0.8, moves=2), dict(N=64)):
        wrong = _population(y=y, **{**kw, **other})
        with pytest.raises(ValueError, match="does not match the population"):
            wrong.load_state_dict(state)


def test_finish_leaves_a_plain_pmmh_ensemble():
    """finish() forces a resample-move when the weights are not all equal and points the ensemble at the series taken so far:
    equal weights afterwards, the evidence unchanged, and the ensemble steps as a plain PMMH ensemble on y[0 : t) whose
    acceptance counts start at 0."""
    pop = _population(ess_target=1e-6, T=20)
    pop.step(2)
    lz = pop.log_evidence()
    assert pop.ess() < 255.0
    ens = pop.finish()
    assert ens is pop.ensemble and ens.T == 10 and pop.log_evidence() == lz
    np.testing.assert_array_equal(pop.weights(), np.full(256, 1.0 / 256))
    assert pop.schedule()["resampled"][-1] == 1 and pop.evidence_increments()[-1] == 0.0
    assert ens.steps_done == 0 and not ens.accept_dev.any().item()
    ens.step(5)
    ens.synchronize()
    assert np.all(np.isfinite(ens.loglik())) and 0.0 < ens.acceptance_rate().mean() < 1.0
    with pytest.raises(ValueError, match="finished"):
        pop.step(1)


@pytest.mark.parametrize("model", ["lgssm", "garch"])
def test_the_move_keeps_every_particle_system_consistent(model):
    """One forced resample-move at t = 10 (chunk = 10, ess_target = 0.999, moves = 2).  For every chain, a filter relaunched
    from scratch on y[0 : 10) at the chain's theta, under the counter and the key chain row_origin() records, reproduces its
    row of the current buffer bitwise: a chain that accepted replays the move's launch, one that rejected both proposals the
    extension launch of the parent it descends from, and its ll is that launch's estimate."""
    import torch
    pop = _population(model=model, T=10, chunk=10, C=257, N=32, ess_target=0.999, moves=2)
    assert pop.step(1) == 1 and pop.schedule()["resampled"][-1] == 1
    e = pop.ensemble
    rows, origin, ll = pop.state_rows(), pop.row_origin(), e.ll_dev.cpu().numpy()
    theta = e.theta_dev.clone()
    assert set(np.unique(origin[:, 0])) == {0, 1, 2} and np.all(origin[:, 2] == 10)
    kept = origin[:, 0] == 0
    assert kept.any() and np.any(origin[kept, 1] != np.arange(257)[kept])         # rows that came from another chain
    assert np.all(origin[~kept, 1] == np.arange(257)[~kept])
    launches = pop.launches
    for ctr in (0, 1, 2):
        mine = origin[:, 0] == ctr
        pop._desc["stream"] = origin[:, 1].astype(np.uint64)
        pop.ctr_dev.fill_(ctr)
        pop.launch_filter(theta, 0, 10, None, 1 - pop._cur)
        _sync()
        again = pop.state_dev[1 - pop._cur].cpu().numpy()
        np.testing.assert_array_equal(again[mine].view(np.uint64), rows[mine].view(np.uint64), err_msg="counter {0}".format(ctr))
        np.testing.assert_array_equal(e.out_dev[:, 4].cpu().numpy()[mine], ll[mine])
        assert not np.array_equal(again[~mine], rows[~mine])
    pop._desc["stream"] = np.arange(257, dtype=np.uint64)
    pop.ctr_dev.fill_(launches)
    pop.launches = launches
    np.testing.assert_array_equal(pop.state_rows(), rows)


def _four_se(a, b, what):
    """Each difference of the two sets' means within 4 combined standard errors, taken across the seeds of either set."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    se = np.sqrt(a.var(0, ddof=1) / len(a) + b.var(0, ddof=1) / len(b))
    diff = a.mean(0) - b.mean(0)
    print(what, "smc2", a.mean(0), "sd", a.std(0, ddof=1), "tempered", b.mean(0), "sd", b.std(0, ddof=1), "difference", diff,
          "in combined standard errors", diff / se)
    assert np.all(np.abs(diff) <= 4.0 * se), (what, diff / se)


LAW = [("lgssm", dict(T=20, C=2048, N=64, chunk=5), dict(kind="marginal")),
       ("svm", dict(T=40, C=1024, N=128, chunk=5), dict(N=128))]


@pytest.mark.parametrize("model, shape, yardstick", LAW, ids=[c[0] for c in LAW])
def test_law_against_the_tempered_population(model, shape, yardstick):
    """K = 5 seeds of SequentialPopulation against 5 seeds of TemperedPopulation -- existing code, the yardstick -- on the same
    data, prior and q0: LGSSM against the exact Kalman likelihood (kind='marginal'), SVM against tempering with as many
    particles.  The weighted posterior means of the moving slots and log_evidence() each differ by at most 4 combined
    standard errors, computed here from the two sets of seeds.  (log of an unbiased evidence estimate carries a Jensen bias of
    about half its variance; across 1024 .. 2048 chains that is far below the standard error, so the rule covers it.)"""
    from sgmcmc_ssm_amd.tempering import TemperedPopulation
    y = _series(model, shape["T"])
    slots = list(sm.MOVING[model])
    seq, tmp = [], []
    for seed in range(5):
        pop = _population(model=model, y=y, C=shape["C"], N=shape["N"], chunk=shape["chunk"], seed=seed)
        pop.run()
        seq.append(np.r_[pop.posterior_mean()[slots], pop.log_evidence()])
        ref = TemperedPopulation(model, y, default_params(model), num_chains=shape["C"], seed=100 + seed, prior=_prior(model),
                                 **yardstick)
        ref.temper()
        tmp.append(np.r_[ref.ensemble.theta()[:, slots].mean(0), ref.log_evidence()])
    print(model, "stages resampled", pop.schedule()["resampled"], "acceptance", pop.schedule()["acceptance"])
    _four_se(seq, tmp, model + " (means of the moving slots, log evidence)")
