"""The 256 x 4 kernel's map from the search's final byte offset to the parent's gather address (GADDR in
csrc/pfg_reg_kernel.hpp), restated in NumPy with the kernel's 32-bit / 24-bit integer operations, against the general
form it replaces: physical CDF position -> CDF position (p - p * 993 >> 15, undoing one pad slot per 32 entries) ->
particle index (thread-major position tid * 4 + k <-> particle k * 256 + tid) -> clamp to the last particle.  Exact
equality on every physical position of the padded CDF -- the pad slots and the past-the-end offset the search reaches
when every compare succeeds included -- and for every `last` at which the clamp can cut differently."""
import numpy as np
import pytest

NT, PPT = 256, 4
SLOTS = NT * PPT
PHYS = SLOTS + SLOTS // 32          # 1056 physical positions


def _general(phys, last):
    """today's form: anc = particle index of the CDF position, clamped"""
    p = phys.astype(np.uint32)
    p = p - ((p * np.uint32(993)) >> np.uint32(15))
    anc = ((p << np.uint32(8)) & np.uint32((PPT - 1) * NT)) | (p >> np.uint32(2))
    return np.minimum(anc.astype(np.int64), last)


def _gather_address(phys, last):
    """the kernel's short form on the byte offset off = 4 * phys: the gather's byte address / 16 is the ancestor"""
    off = (4 * phys).astype(np.uint32)
    assert np.all(off.astype(np.uint64) * 993 < 1 << 24)                # v_mul_u32_u24 is exact
    q = (off * np.uint32(993)) >> np.uint32(17)
    p4 = (off.astype(np.int64) + q.astype(np.int64) * -4).astype(np.uint32)   # v_mad_i32_i24
    assert np.all(p4 < 1 << 13)
    a = (p4 * np.uint32(1025)) & np.uint32(0x3FF0)
    return np.minimum(a, np.uint32(16 * last))


def _search_end(cdf_phys_u32, word):
    """the kernel's unrolled search on the padded 32-bit CDF: the physical position it ends on"""
    pos = 0
    step = SLOTS >> 1
    while step >= 1:
        probe = step - 1 + ((step >> 5) - 1 if step >= 32 else 0)
        if cdf_phys_u32[pos + probe] <= word:
            pos += step + (step >> 5)
        step >>= 1
    return pos


@pytest.mark.parametrize("last", [0, 1, 255, 256, 999, 1022, 1023])
def test_gather_address_equals_general_form(last):
    phys = np.arange(PHYS, dtype=np.int64)
    a = _gather_address(phys, last)
    assert np.all(a % 16 == 0)
    assert np.array_equal(a.astype(np.int64) // 16, _general(phys, last))
    # the address stays inside one state array of 1024 sixteen-byte records
    assert a.max() <= 16 * last


def test_search_reaches_the_past_the_end_offset_and_it_maps_to_the_last_slot():
    """every compare succeeds (all entries <= word): the search ends on physical position 1054, CDF position 1023"""
    cdf = np.zeros(PHYS, dtype=np.uint32)
    end = _search_end(cdf, np.uint32(0xFFFFFFFF))
    assert end == 1054
    for last in (0, 1, 255, 256, 999, 1022, 1023):
        got = int(_gather_address(np.array([end]), last)[0])
        assert got == 16 * min(last, ((1023 & 3) << 8) | (1023 >> 2)) == int(_general(np.array([end]), last)[0]) * 16
    # no compare succeeds: position 0, particle 0
    assert _search_end(np.full(PHYS, 0xFFFFFFFF, dtype=np.uint32), np.uint32(0)) == 0
    assert int(_gather_address(np.array([0]), 1023)[0]) == 0


def test_every_cdf_position_round_trips():
    """physical position of CDF position p is p + p // 32; the address is 16 x the particle of thread-major position p"""
    p = np.arange(SLOTS, dtype=np.int64)
    a = _gather_address(p + p // 32, SLOTS - 1).astype(np.int64)
    assert np.array_equal(a // 16, (p % PPT) * NT + p // PPT)
