#!/usr/bin/env python
"""Compare the device listings of two builds kernel by kernel (no GPU needed).

    python tools/compare_listings.py DIR_A DIR_B [--pool] [--exact 'pf_reg_kernel<0, 0, double, 256, 4, 1, false, 0, false, false>' ...]

DIR_A / DIR_B hold one `hipcc --cuda-device-only -S` listing per instantiation unit (the recipe of
tools/isa_histogram.py::listing without -DPFG_ISA_MARKERS), under the same file names -- or, with --pool, under any
names: the kernels of all listings of a directory are pooled by name, so one that moved to another unit is still
compared (a name defined twice in a directory is an error).  Per kernel, one of
  identical   the same instructions in the same order (labels, symbols of the unit id and source paths aside);
  commuted    ... up to the order of the source operands of commutative instructions;
  reordered   the same multiset of instructions (commutative operands unordered; s_nop / s_waitcnt counted apart and
              reported when their numbers differ), in another order;
  DIFFERENT   anything else (the first differing mnemonic counts are printed).
Exit status 1 if a kernel is DIFFERENT, or if a kernel named with --exact is not identical / commuted.
"""
import argparse
import collections
import os
import re
import subprocess
import sys

COMMUTATIVE = re.compile(r"^v_(add|mul|max|min|fmac|mac)_(f|u|i)(16|32|64)(_e32|_e64)?$|^v_(and|or|xor)_b32(_e32|_e64)?$|^v_add_(co_)?u32(_e32|_e64)?$")
# (v_fmac / v_mac d, a, b: d is also the addend, a and b are the multiplicands -- the last two operands commute)
MULTIPLY_ADD = re.compile(r"^v_(fma|mad)_(f|u|i)(16|32|64)(_e64)?$")     # d, a, b, c: a and b commute
WAITS = ("s_nop", "s_waitcnt")


def kernels(path):
    """{demangled name: [(mnemonic, operands)]} of the .amdgpu functions of one listing."""
    out, name, body = {}, None, None
    for line in open(path):
        line = re.sub(r"__hip_cuid_\w+", "__hip_cuid", line.split(";")[0]).strip()
        m = re.match(r"^(_Z\w+):$", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif name and line and not line.startswith(".") and not line.endswith(":"):
            mn, _, ops = line.partition(" ")
            body.append((mn, re.sub(r"\.LBB\d+_\d+", ".LBB", ops.strip())))
    if not out:         # a unit without device functions (c++filt would wait for names on its input)
        return {}
    names = subprocess.run(["c++filt"] + list(out), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert len(names) == len(out), "c++filt returned {0} names for {1} symbols".format(len(names), len(out))
    return {n.replace("void pfg::", "").replace("(anonymous namespace)::", "").split("(")[0]: out[k] for k, n in zip(out, names)}


def canon(inst):
    mn, ops = inst
    if COMMUTATIVE.match(mn) and "dpp" not in ops and "sdwa" not in ops:
        parts = [p.strip() for p in ops.split(",")]
        if len(parts) >= 3:
            parts[-2:] = sorted(parts[-2:])
        return mn, ", ".join(parts)
    if MULTIPLY_ADD.match(mn):
        parts = [p.strip() for p in ops.split(",")]
        if len(parts) >= 4:
            parts[1:3] = sorted(parts[1:3])
        return mn, ", ".join(parts)
    return inst


def verdict(a, b):
    if a == b:
        return "identical", ""
    ca, cb = [canon(i) for i in a], [canon(i) for i in b]
    if ca == cb:
        return "commuted", "{0} instructions with swapped operands".format(sum(x != y for x, y in zip(a, b)))
    ma = collections.Counter(i for i in ca if i[0] not in WAITS)
    mb = collections.Counter(i for i in cb if i[0] not in WAITS)
    waits = ", ".join("{0} {1} -> {2}".format(w, sum(i[0] == w for i in a), sum(i[0] == w for i in b)) for w in WAITS
                      if sum(i[0] == w for i in a) != sum(i[0] == w for i in b))
    if ma == mb:
        return "reordered", waits
    na, nb = collections.Counter(i[0] for i in a), collections.Counter(i[0] for i in b)
    diff = ["{0} {1} -> {2}".format(k, na[k], nb[k]) for k in sorted(set(na) | set(nb)) if na[k] != nb[k]]
    return "DIFFERENT", "; ".join(diff[:8]) or "same mnemonic counts, other operands ({0} instructions)".format(sum((ma - mb).values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--exact", nargs="*", default=[], help="kernels that must be identical or commuted")
    ap.add_argument("--pool", action="store_true", help="pool the kernels of all listings of each directory by name")
    args = ap.parse_args()
    bad, tally = 0, collections.Counter()

    def pooled(d):
        out = {}
        for f in sorted(x for x in os.listdir(d) if x.endswith(".s")):
            for name, body in kernels(os.path.join(d, f)).items():
                if name in out:
                    raise SystemExit("{0} is defined twice in {1}".format(name, d))
                out[name] = body
        return out

    pairs = [("pooled", pooled(args.dir_a), pooled(args.dir_b))] if args.pool else \
            [(f, kernels(os.path.join(args.dir_a, f)), kernels(os.path.join(args.dir_b, f)))
             for f in sorted(x for x in os.listdir(args.dir_a) if x.endswith(".s"))]
    for f, ka, kb in pairs:
        for name in sorted(set(ka) | set(kb)):
            v, note = verdict(ka[name], kb[name]) if name in ka and name in kb else ("DIFFERENT", "in one build only")
            tally[v] += 1
            must = name in args.exact
            bad += v == "DIFFERENT" or (must and v not in ("identical", "commuted"))
            if v != "identical" or must:
                print("{0:<10} {1} {2}  [{3}]{4}".format(v, "!" if must else " ", name, f, "  " + note if note else ""))
    if not tally:
        raise SystemExit("no listing (*.s) in " + args.dir_a)
    print("# " + ", ".join("{0} {1}".format(n, v) for v, n in sorted(tally.items())))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
