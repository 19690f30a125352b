"""PFG_OPT_EXPMAGIC (csrc/pfg_math.hpp, exp_tab_hot): the two argument reductions of the 128-entry table exp, modelled exactly.

    reference   kd = rint(fl(x c)),             k = (int)kd         (the product is rounded, then rounded to an integer)
    magic       s = fma(x, c, 1.5 * 2^52),      kd = s - 1.5 * 2^52, k = low word of s

s lies in [2^52, 2^53), where doubles are the integers, and 1.5 * 2^52 is even: the fma's single rounding IS round-half-even of
the EXACT product x c to an integer.  fractions.Fraction holds the exact product; float(Fraction) rounds correctly, which
gives fl(x c) and every fma below.  The two k differ only where fl(x c) is a half-integer that the exact product is not:

  * 10^6 seeded arguments uniform in [-1000, 64]: the same k in every case.  (A product has 36 or more fraction bits in
    this range, so a rounded product hits a half-integer about once in 2^35 arguments: 3e-5 expected cases.)
  * constructed ties: for half-integers p = h + 1/2 the doubles x next to p / c whose ROUNDED product is p exactly while the
    exact one is not.  There k differs by at most 1, both reductions are valid (|r| <= ln2/256 to rounding), and the two
    results differ by less than 1e-11 relative.  Bound: each result is 2^(k/128) (1 + expm1_3(r)) with the cubic
    expm1_3(r) = r + r^2/2 + r^3/6, whose error is r^4/24 (1 + r/5 + ...) <= 2.3e-12 at |r| = ln2/256 = 2.7e-3; the table
    entry, the fma chain and ldexp add a few ulp (< 1e-15), and the rounded constant ln2/128 enters both r alike up to one
    step of k (6e-19).  Two results, each within 2.3e-12 + 1e-15 of exp(x): their difference is below 4.7e-12 < 1e-11."""
from fractions import Fraction
import math

import numpy as np

C128 = 184.6649652337873            # 128 / ln 2, as in exp_tab
LN2_128 = 0.0054152123481245725     # ln 2 / 128
MAGIC = float.fromhex("0x1.8p52")
FC = Fraction(C128)


def k_reference(x):
    p = float(Fraction(x) * FC)                 # fl(x c)
    return int(round(Fraction(p)))              # rint: round-half-even of the rounded product


def k_magic(x):
    s = float(Fraction(x) * FC + Fraction(MAGIC))       # the fma, rounded once
    assert 2.0 ** 52 <= s < 2.0 ** 53
    kd = s - MAGIC                                       # exact
    low = int(s) & 0xFFFFFFFF                            # the low word of s, as two's complement
    k = low - (1 << 32) if low & 0x80000000 else low
    assert k == int(kd)
    return k


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def exp_from_k(x, k):
    """the rest of exp_tab's 128-entry form (cubic expm1), every fma rounded once"""
    r = fma(float(k), -LN2_128, x)
    t = float(2.0 ** ((k & 127) / 128.0))
    p = fma(r, 0.16666666666666666, 0.5)
    p = fma(p, r, 1.0)
    p = p * r
    return math.ldexp(fma(t, p, t), k >> 7), r


def test_same_k_on_a_million_arguments():
    x = np.random.RandomState(20250819).uniform(-1000.0, 64.0, size=1000000)
    ref = np.rint(x * C128).astype(np.int64)                 # IEEE: the product rounded, then rint
    # the exact product by integers: x = n / 2^a, c = m / 2^b
    m, d = FC.numerator, FC.denominator
    assert d & (d - 1) == 0
    sh_c = d.bit_length() - 1
    bad = []
    for i, xv in enumerate(x.tolist()):
        n, dx = xv.as_integer_ratio()
        num, sh = n * m, sh_c + dx.bit_length() - 1          # exact product = num / 2^sh
        q, rem = num >> sh, num & ((1 << sh) - 1)
        half = 1 << (sh - 1)
        km = q + (1 if rem > half or (rem == half and (q & 1)) else 0)       # round-half-even of the exact product
        if km != ref[i]:
            bad.append((xv, int(ref[i]), km))
    # the integer path is the Fraction model (checked on a sample, with the reference's product by Fraction as well)
    for xv in x[:2000].tolist():
        assert k_reference(xv) == int(np.rint(xv * C128))
    for xv, kr, km in bad:
        print("differs:", float.hex(xv), kr, km)
    assert not bad


def _ties(count):
    """doubles whose rounded product with c is a half-integer exactly and whose exact product is not"""
    out = []
    rs = np.random.RandomState(5)
    while len(out) < count:
        h = int(rs.randint(-129000, 11800))          # x in [-698, 64]: exp(x) is a normal double, a relative difference means something
        p = h + 0.5
        x0 = p / C128
        for step in range(-3, 4):
            x = x0
            for _ in range(abs(step)):
                x = math.nextafter(x, math.inf if step > 0 else -math.inf)
            exact = Fraction(x) * FC
            if float(exact) == p and exact != Fraction(p) and -1000.0 <= x <= 64.0:
                out.append(x)
    return out


def test_constructed_ties_differ_by_one_step_and_the_cubics_error():
    xs = _ties(400)
    differ = 0
    for x in xs:
        kr, km = k_reference(x), k_magic(x)
        assert abs(kr - km) <= 1, (float.hex(x), kr, km)
        differ += kr != km
        (vr, rr), (vm, rm) = exp_from_k(x, kr), exp_from_k(x, km)
        assert abs(rr) <= LN2_128 / 2 * (1 + 1e-9) and abs(rm) <= LN2_128 / 2 * (1 + 1e-9)     # both valid reductions
        assert abs(vr - vm) < 1e-11 * abs(vr), (float.hex(x), vr, vm)
        assert abs(vr - math.exp(x)) < 5e-12 * math.exp(x)
    print("ties:", len(xs), "with different k:", differ)
    assert differ > len(xs) // 8           # the construction does reach the case (about half of the ties)
