"""Launch sizing is monotone in N (no GPU needed).

Every launch path sizes what a batch shares -- the per-window HBM scratch stride, the dynamic LDS -- once, from the
batch's LARGEST window, while each kernel lays out its own window from that window's own N.  That is only safe if
every size a window needs is non-decreasing in N inside the kernel family (and grid tile class) the plan picked for
n_max: a window smaller than n_max must never need more than the plan allotted.  pfg_scratch_bytes is the plan's
per-window stride; pfg_variant_name names the family it was computed for.
"""
import os
import sys

import numpy as np
import pytest

from sgmcmc_ssm_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
from grid_layout import grid_layout, grid_step_lds_coarse  # noqa: E402

MODELS = ("svm", "garch", "lgssm")
DTYPES = ("f64", "f32")
GRID_MAX_N = 1 << 22

# every place a size formula changes regime: the one-workgroup kernels' limits, the grid tile classes, the coarse
# table's stride doublings (C = ceil(N / S) would drop at 2^20 + 1 and 2^21 + 1), the supported maximum
BOUNDARIES = (1024, 4096, 16384, 1 << 19, 1 << 20, 1 << 21, GRID_MAX_N)


def sample_ns():
    ns = set()
    for b in BOUNDARIES:
        ns.update(n for n in range(b - 3, b + 4) if 1 <= n <= GRID_MAX_N)
    ns.update(int(round(v)) for v in np.logspace(0, 22 * np.log10(2), 240))
    return sorted(n for n in ns if 1 <= n <= GRID_MAX_N)


NS = sample_ns()


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def test_samples_cover_every_boundary():
    for n in (1024, 1025, 4096, 4097, 16384, 16385, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, (1 << 20) - 1, 1 << 20,
              (1 << 20) + 1, (1 << 20) + 2, (1 << 21) - 1, (1 << 21) + 1, GRID_MAX_N - 1, GRID_MAX_N):
        assert n in NS, n
    assert len(NS) > 250


@pytest.mark.parametrize("rng", ["replay", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_scratch_stride_is_monotone_inside_each_family(lib, model, dtype, rng):
    """pfg_scratch_bytes(N) never decreases while pfg_variant_name(N) stays the same (a grid name also fixes the tile
    class).  Fails at N = 2^20 + 1 and 2^21 + 1 (REPLAY) if the whole-GPU layout sizes its coarse table from ceil(N / S)."""
    m, d, r = _capi.MODEL[model], _capi.DTYPE[dtype], _capi.RNG[rng]
    drops = []
    prev = None
    for n in NS:
        name = lib.pfg_variant_name(m, 0, d, r, n)
        size = lib.pfg_scratch_bytes(m, d, r, n)
        assert size >= 0 and name != b"none", (model, dtype, rng, n, name, size)
        if prev is not None and prev[1] == name and size < prev[2]:
            drops.append((prev[0], n, name.decode(), prev[2], size))
        prev = (n, name, size)
    assert not drops, drops


@pytest.mark.parametrize("replay", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_grid_layout_mirror_is_monotone_and_covers_every_window(model, dtype, replay):
    """The Python mirror of the whole-GPU layout: every offset and the total are non-decreasing in N inside a tile class,
    and the coarse table a window reserves (and the step kernel's LDS is sized from) holds the C = ceil(N / S) entries
    the kernels fill, for the window itself and for every smaller window of its class."""
    keys = ("lw", "rec", "part", "rng", "head", "cdf", "coarse", "walk_i", "walk_p", "walk_q", "walk_s", "cdfx", "cs",
            "tab", "consts", "bytes")
    prev = None
    for n in (x for x in NS if x > 16384):
        L = grid_layout(model, dtype, n, replay)
        assert L["C"] == (n + L["S"] - 1) // L["S"] and L["C"] <= 16384
        if replay:
            assert L["C"] <= L["CR"] <= 16384 and L["CR"] == grid_step_lds_coarse(n)
        if prev is not None and prev["TILE"] == L["TILE"]:
            for k in keys:
                if k in L:
                    assert np.all(np.asarray(L[k]) >= np.asarray(prev[k])), (model, dtype, replay, prev["N"], n, k)
            if replay:
                assert L["CR"] >= prev["C"]
        prev = L


@pytest.mark.parametrize("rng", ["replay", "device"])
def test_grid_scratch_matches_the_mirror_across_the_stride_doublings(lib, rng):
    """pfg_scratch_bytes of the whole-GPU window equals the mirror at each side of every coarse-stride doubling."""
    for model in MODELS:
        for dtype in DTYPES:
            for n in (1 << 20, (1 << 20) + 1, (1 << 20) + 2, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, GRID_MAX_N - 1):
                got = lib.pfg_scratch_bytes(_capi.MODEL[model], _capi.DTYPE[dtype], _capi.RNG[rng], n)
                assert got == grid_layout(model, dtype, n, rng == "replay")["bytes"], (model, dtype, rng, n)
