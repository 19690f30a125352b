"""Writes tests/golden/chain_rules.npz: the outputs of every entry point of csrc/pfg_chains.hip on fixed inputs, one launch
each (sghmc: three), so that tests/test_gpu_chain_rules_golden.py notices a last bit that moves.  The mirror tests accept
a band of a few ulps and the ensemble tests compare a build with itself; this file pins the values.  Needs a GPU:

    python tests/golden/make_chain_rules_golden.py

B = 130 chains (two 128-lane blocks, the second partial); theta and scores as _chain_inputs of test_gpu_keyed_draws.py
makes them (|A| on both sides of 0.9999, negative Cholesky factors, scores O(1) with +-1e3 and zero rows); a key whose
high words matter and one SGLD case with a NULL counter.  The accept cases take the proposals of the propose cases, with
out[4] = ll_cur + N(0, 1) and, on rows the proposal left valid, a NaN and a +-inf in out[4] and (pMALA) in a score column.
Only outputs are stored; run_cases() rebuilds the inputs, and check_coverage() refuses to write a file whose cases miss
the branches they were built for."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "helpers"),
                os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd")]

import keyed_draws as kd                                                                    # noqa: E402
from test_gpu_keyed_draws import _chain_inputs, _gibbs_hyper, _gibbs_stats, _hyper           # noqa: E402
from test_gpu_pgibbs import _hyper as _pgibbs_hyper, _records                                # noqa: E402

PATH = os.path.join(HERE, "chain_rules.npz")
B = 130
MODELS = ("svm", "garch", "lgssm")
EPS, TSCALE, ALPHA, SEED = 0.02, 50.0, 0.1, 0x5EED0000C0DE1234
OFF, STEP = 2 ** 32 - 100, 2 ** 32 + 3                  # the high words of the chain id and of the counter take part
GIBBS_CASES = ("paths", "short_small_df")
# proposal scales, large enough that some proposals leave the support (those of tests/test_gpu_pmala.py)
SCALE = {"svm": [0.3, 0.3, 0.3, 0.0], "lgssm": [0.2, 1.0, 0.4, 0.4], "garch": [0.3, 0.5, 0.5, 1.0]}
NAN_ROW, INF_ROW = 100, 101                             # of grad_cur, in the pMALA propose cases


def chain_inputs(model, seed):
    """(theta [B, 4], outs [B, 8]) with +-1e3 rows and zero rows among the scores"""
    th, g = _chain_inputs(model, n=B, seed=seed)
    assert (np.abs(g[:, :4]) == 1e3).all(axis=1).any() and (g[:, :4] == 0).all(axis=1).any(), "choose another seed"
    assert (np.abs(g[:, :4]) == 1e3).all(axis=1).sum() < B // 4
    return th, g


def propose_inputs(model):
    """(theta, grad_cur [B, 4]): grad_cur with one NaN and one -inf row"""
    th, g = chain_inputs(model, 11)
    grad = g[:, :4].copy()
    grad[NAN_ROW, 0], grad[INF_ROW, 1] = np.nan, -np.inf
    return th, grad


def accept_inputs(model, sampler, valid):
    """(outs, ll_cur, n_accept, rows) of an accept case on the proposals whose `valid` is given: out[4] = ll_cur + N(0, 1);
    on the first rows that are valid a NaN, a +inf and a -inf in out[4]; for pMALA a NaN and a +inf in a score column the
    drift uses and (LGSSM) a NaN in C's column, which it does not use, on a row whose out[4] accepts whatever else"""
    rs = np.random.RandomState(17)
    g = chain_inputs(model, 12)[1]
    ll = -40.0 + 3.0 * rs.standard_normal(B)
    g[:, 4] = ll + rs.standard_normal(B)
    ok = np.nonzero((np.asarray(valid) == 1) & (np.abs(g[:, :4]) < 10).all(axis=1))[0]
    assert len(ok) >= 6, "too few valid proposals: choose another seed"
    rows = dict(ll_nan=ok[0], ll_pinf=ok[1], ll_ninf=ok[2])
    g[ok[0], 4], g[ok[1], 4], g[ok[2], 4] = np.nan, np.inf, -np.inf
    if sampler == "pmala":
        rows.update(g_nan=ok[3], g_inf=ok[4])
        g[ok[3], 0], g[ok[4], 1] = np.nan, np.inf
        g[ok[3], 4] = g[ok[4], 4] = 1e6
        if model == "lgssm":
            rows.update(c_nan=ok[5])
            g[ok[5], 2], g[ok[5], 4] = np.nan, 1e6
    return g, ll, (np.arange(B) % 7).astype(np.int64), rows


def first_round_rejected(stats, hy):
    """per chain: did Marsaglia-Tsang reject round 0 of Qinv's or Rinv's draw (the host mirror's decision)"""
    keys = kd.ChainKeys(kd.chain_ids(B, OFF), SEED, STEP)
    _, _, shq, shr = kd.gibbs_expected(stats, hy, SEED, OFF, STEP)
    rej = np.zeros(B, bool)
    for var, shape in ((0, shq), (1, shr)):
        a = np.where(shape < 1, shape + 1, shape)
        d = a - kd.LD(1) / kd.LD(3)
        c = kd.LD(1) / np.sqrt(kd.LD(9) * d)
        r = keys.draw(var, 0)
        z, _ = kd.normal_pair(r[0], r[1])
        t = 1 + c * z
        v = np.where(t > 0, t * t * t, 1)
        rej |= (t <= 0) | ~(np.log(kd.uniform53(r[2], r[3])) < kd.LD(0.5) * z * z + d - d * v + d * np.log(v))
    return rej


def run_cases():
    """Every case through _capi on cuda:0.  Returns (outputs {name: array}, facts for check_coverage)."""
    import torch
    from sgmcmc_ssm_amd import _capi
    ctx = _capi.default_context()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    counter = lambda: torch.tensor([STEP], dtype=torch.int64, device="cuda")
    out, facts = {}, {}

    def put(case, **arrays):
        torch.cuda.synchronize()
        for k, v in arrays.items():
            out[case + "/" + k] = v.cpu().numpy()

    for model in MODELS:
        hy = _hyper(model)
        th0, g = chain_inputs(model, 1)
        # sgld, and three sghmc steps with the momentum carried
        theta, outs, ctr = dev(th0), dev(g), counter()
        ctx.sgld_update_device(model, B, theta.data_ptr(), outs.data_ptr(), hy, EPS, TSCALE, SEED, OFF, ctr.data_ptr())
        put("sgld/" + model, theta=theta, ctr=ctr)
        theta, ctr = dev(th0), counter()
        mom = torch.zeros((B, _capi.MAX_THETA), dtype=torch.float64, device="cuda")
        for _ in range(3):
            ctx.sghmc_update_device(model, B, theta.data_ptr(), mom.data_ptr(), outs.data_ptr(), hy, EPS, ALPHA, TSCALE, SEED,
                                    OFF, ctr.data_ptr())
        put("sghmc/" + model, theta=theta, momentum=mom, ctr=ctr)
        # logprior (NaN where a Cholesky factor is negative)
        theta, lp = dev(th0), torch.zeros(B, dtype=torch.float64, device="cuda")
        ctx.logprior_device(model, B, theta.data_ptr(), hy, lp.data_ptr())
        put("logprior/" + model, logprior=lp)
        # pmmh and pmala: propose, accept on those proposals, init
        scale = dev(np.array(SCALE[model]))
        th0, grad0 = propose_inputs(model)
        for sampler in ("pmmh", "pmala"):
            case = sampler + "_{0}/" + model
            theta, grad, ctr = dev(th0), dev(grad0), counter()
            prop = torch.full((B, _capi.MAX_THETA), -7.0, dtype=torch.float64, device="cuda")
            valid = torch.full((B,), -7, dtype=torch.int32, device="cuda")
            if sampler == "pmmh":
                ctx.pmmh_propose_device(model, B, theta.data_ptr(), prop.data_ptr(), valid.data_ptr(), scale.data_ptr(), SEED,
                                        OFF, ctr.data_ptr())
            else:
                ctx.pmala_propose_device(model, B, theta.data_ptr(), grad.data_ptr(), prop.data_ptr(), valid.data_ptr(),
                                         scale.data_ptr(), hy, SEED, OFF, ctr.data_ptr())
            put(case.format("propose"), theta_prop=prop, valid=valid, ctr=ctr)
            v = out[case.format("propose") + "/valid"]
            g, ll0, n0, rows = accept_inputs(model, sampler, v)
            grad0_ok = np.where(np.isfinite(grad0), grad0, 0.0)         # a chain's own estimate is always finite
            for init in (0, 1):
                theta, grad, outs, ll, n = dev(th0), dev(grad0_ok), dev(g), dev(ll0), dev(n0)
                if sampler == "pmmh":
                    ctx.pmmh_accept_device(model, B, theta.data_ptr(), prop.data_ptr(), valid.data_ptr(), outs.data_ptr(),
                                           ll.data_ptr(), n.data_ptr(), hy, init, SEED, OFF, ctr.data_ptr())
                else:
                    ctx.pmala_accept_device(model, B, theta.data_ptr(), prop.data_ptr(), valid.data_ptr(), outs.data_ptr(),
                                            ll.data_ptr(), grad.data_ptr(), n.data_ptr(), hy, scale.data_ptr(), init, SEED,
                                            OFF, ctr.data_ptr())
                name = case.format("init" if init else "accept")
                put(name, ll_cur=ll, n_accept=n, ctr=ctr)
                if init:                        # init leaves theta as it is: checked here, not stored
                    np.testing.assert_array_equal(theta.cpu().numpy(), th0, err_msg=name)
                else:
                    put(name, theta=theta)
                if sampler == "pmala":
                    put(name, grad_cur=grad)
            facts[sampler + "/" + model] = dict(valid=v, rows=rows, accepted=out[case.format("accept") + "/n_accept"] - n0,
                                                theta0=th0)

    # one SGLD case with a NULL counter
    th0, g = chain_inputs("svm", 1)
    theta, outs = dev(th0), dev(g)
    ctx.sgld_update_device("svm", B, theta.data_ptr(), outs.data_ptr(), _hyper("svm"), EPS, TSCALE, SEED, 0, None)
    put("sgld_null_counter/svm", theta=theta)

    th0, g = chain_inputs("lgssm", 3)
    theta, outs, ctr = dev(th0), dev(g), counter()
    ctx.sgrld_update_device("lgssm", B, theta.data_ptr(), outs.data_ptr(), _hyper("lgssm"), EPS, TSCALE, SEED, OFF,
                            ctr.data_ptr())
    put("sgrld/lgssm", theta=theta, ctr=ctr)

    start = np.tile([0.5, 1.0, 1.0, 1.0], (B, 1))
    for case in GIBBS_CASES:
        stats, hy = _gibbs_stats(case, n=B), _gibbs_hyper(case)
        theta, outs, ctr = dev(start), dev(stats), counter()
        ctx.gibbs_update_device("lgssm", B, theta.data_ptr(), outs.data_ptr(), hy, SEED, OFF, ctr.data_ptr())
        put("gibbs/" + case, theta=theta, ctr=ctr)
        facts["gibbs/" + case] = first_round_rejected(stats, hy)
    for model in ("svm", "lgssm"):
        theta, outs, ctr = dev(start), dev(_records(model, B)), counter()
        ctx.pgibbs_update_device(model, B, theta.data_ptr(), outs.data_ptr(), _pgibbs_hyper(model), SEED, OFF, ctr.data_ptr())
        put("pgibbs/" + model, theta=theta, ctr=ctr)
    return out, facts


def check_coverage(out, facts):
    """The branches the cases were built for were taken: a file that exercises nothing is not written."""
    for model in MODELS:
        assert (np.abs(chain_inputs(model, 1)[0][:, 0]) > 0.9999).any() or model == "garch"
        for sampler in ("pmmh", "pmala"):
            f = facts[sampler + "/" + model]
            valid, acc, rows = f["valid"], f["accepted"], f["rows"]
            what = (sampler, model)
            assert set(np.unique(valid)) == {0, 1}, what                        # some proposals left the support
            inv = valid == 0
            np.testing.assert_array_equal(out["{0}_propose/{1}/theta_prop".format(*what)][inv], f["theta0"][inv])
            assert set(np.unique(acc)) == {0, 1} and not acc[inv].any(), what   # both outcomes; none accepted unseen
            assert (acc[valid == 1] == 0).sum() > len(rows), what               # rejects beyond the rows built to reject
            for k, r in rows.items():
                assert acc[r] == (1 if k == "c_nan" else 0), (what, k)          # NaN and +-inf rows were rejected
            np.testing.assert_array_equal(out["{0}_accept/{1}/ctr".format(*what)], [STEP + 1])
            np.testing.assert_array_equal(out["{0}_init/{1}/ctr".format(*what)], [STEP + 1])    # init does not bump
            if sampler == "pmala":
                assert valid[NAN_ROW] == 0 and valid[INF_ROW] == 0, what
                if model == "lgssm":
                    assert np.isnan(out["pmala_accept/lgssm/grad_cur"][rows["c_nan"], 2])
    assert facts["gibbs/short_small_df"].any(), "no rejected Marsaglia-Tsang round under the boosted shapes"
    assert facts["gibbs/paths"].any(), "no rejected Marsaglia-Tsang round"
    for name, a in out.items():
        if name.endswith("/theta") and not name.startswith(("pmmh", "pmala", "sgld", "sghmc", "sgrld")):
            assert np.all(np.isfinite(a)), name
        if name.endswith("/ctr") and name.split("/")[0] in ("sgld", "sgrld", "gibbs", "pgibbs"):
            assert int(a[0]) == STEP + 1, name
        if name.startswith("sghmc") and name.endswith("/ctr"):
            assert int(a[0]) == STEP + 3, name


if __name__ == "__main__":
    out, facts = run_cases()
    check_coverage(out, facts)
    np.savez_compressed(PATH, **out)
    print("wrote chain_rules.npz:", len(out), "arrays,", os.path.getsize(PATH), "bytes")
