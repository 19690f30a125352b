"""Record what the size and name queries of the launch planner answer: tests/golden/plan_sizes.npz.

    python tests/golden/make_plan_sizes_golden.py [path]   (no GPU needed, with the library built)

For every model x dtype x generator and the eleven N of NS (each side of every size class of csrc/pfg_plan.hip: one wave,
256, the LDS-resident kernels' 1024, 4096, the one-workgroup kernels' 16384):

  * scratch_smoother [3, 2, 2, 9, 11]: pfg_scratch_bytes_smoother of every smoother id 0 ... 8 (-1: refused);
  * scratch [3, 2, 2, 11] and name [3, 2, 2, 11]: pfg_scratch_bytes and pfg_variant_name of plain windows.

tests/test_plan_sizes_host.py calls record() again and compares for equality.  The fixture was written at the commit before
make_plan took a request struct and the resampling schemes became rows of one table; it is this library's own output.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(HERE, "plan_sizes.npz")
MODELS = ("svm", "garch", "lgssm")
DTYPES = ("f64", "f32")
RNGS = ("replay", "device")
SMOOTHERS = tuple(range(9))
NS = (1, 128, 129, 256, 257, 1024, 1025, 4096, 4097, 16384, 16385)


def record(lib):
    """The three arrays; PFGRAD_VARIANT and PFGRAD_NO_SCORE1 must be unset (the planner reads them)."""
    from sgmcmc_ssm_amd import _capi
    shape = (len(MODELS), len(DTYPES), len(RNGS), len(NS))
    smo = np.zeros(shape[:3] + (len(SMOOTHERS), len(NS)), dtype=np.int64)
    scratch = np.zeros(shape, dtype=np.int64)
    name = np.zeros(shape, dtype="U32")
    for i, model in enumerate(MODELS):
        for j, dtype in enumerate(DTYPES):
            for k, rng in enumerate(RNGS):
                m, d, r = _capi.MODEL[model], _capi.DTYPE[dtype], _capi.RNG[rng]
                for n, N in enumerate(NS):
                    scratch[i, j, k, n] = lib.pfg_scratch_bytes(m, d, r, N)
                    name[i, j, k, n] = lib.pfg_variant_name(m, 0, d, r, N).decode()
                    for s in SMOOTHERS:
                        smo[i, j, k, s, n] = lib.pfg_scratch_bytes_smoother(m, d, r, s, N)
    return dict(scratch_smoother=smo, scratch=scratch, name=name)


if __name__ == "__main__":
    from sgmcmc_ssm_amd import _capi
    for var in ("PFGRAD_VARIANT", "PFGRAD_NO_SCORE1"):
        assert var not in os.environ, var
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(path, **record(_capi.load_library()))
    print(path)
