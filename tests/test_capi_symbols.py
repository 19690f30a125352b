"""The C-ABI library builds, loads and exports every function include/pfgrad.h declares.
No compute calls here (no GPU in the CPU suite)."""
import ctypes
import os
import re

import pytest

from sgmcmc_ssm_amd import _capi, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?(?:int|void|int64_t|char)\s*\*?\s*(pfg_\w+)\s*\(", src, flags=re.M)
    return sorted(set(names))


def declared_prototypes():
    """name -> (return type, parameter types) of every pfg_* prototype of the header, as C spells them without `const`
    and the parameter names; every pointer is '*'."""
    src = open(os.path.join(ROOT, "include", "pfgrad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)

    def c_type(decl, named):
        if "*" in decl:
            return "char*" if "char" in decl else "*"
        words = [w for w in decl.split() if w != "const"]
        return " ".join(words[:-1] if named else words)
    protos = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?(?:int|void|int64_t|char)\s*\*?)\s*(pfg_\w+)\s*\(([^)]*)\)\s*;",
                                        src, flags=re.M):
        params = [] if params.strip() == "void" else params.split(",")
        protos[name] = (c_type(ret, False), [c_type(p, True) for p in params])
    return protos


C_SCALARS = {"int": ctypes.c_int, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
             "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}


def is_pointer_type(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def test_binding_types_match_the_header_prototypes():
    """Every prototype of include/pfgrad.h against the argtypes / restype the binding sets on the loaded library: the
    arity, each parameter's class (int, double, uint64_t, uint32_t, int64_t, size_t, or a pointer -- which must meet a
    ctypes pointer type or c_void_p, as an integer must meet its own ctypes integer) and the return type."""
    if _build.is_stale():
        _build.build_library()
    lib = _capi.load_library()
    protos = declared_prototypes()
    assert len(protos) >= 54 and set(protos) == set(declared_functions()), sorted(protos)
    returns = dict(C_SCALARS, void=None)
    for name, (ret, params) in protos.items():
        fn = getattr(lib, name)
        argtypes = list(fn.argtypes or ())
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for i, (c, t) in enumerate(zip(params, argtypes)):
            if c == "*":
                assert is_pointer_type(t), (name, i, c, t)
            else:
                assert t is C_SCALARS[c], (name, i, c, t)
        if ret == "char*":
            assert fn.restype is ctypes.c_char_p, (name, "return", fn.restype)
        elif ret == "*":
            assert fn.restype is ctypes.c_void_p, (name, "return", fn.restype)
        else:
            assert fn.restype is returns[ret], (name, "return", ret, fn.restype)


ABI_STRUCTS = (("pfg_problem", "PROBLEM_DTYPE"), ("pfg_result", "RESULT_DTYPE"), ("pfg_dev_problem", "DEV_PROBLEM_DTYPE"),
               ("pfg_prior_hyper", "PriorHyper"), ("pfg_csmc_problem", "CSMC_PROBLEM_DTYPE"),
               ("pfg_cpm_problem", "CPM_PROBLEM_DTYPE"), ("pfg_sqmc_problem", "SQMC_PROBLEM_DTYPE"))
ENUM_PREFIXES = (("MODEL", "PFG_MODEL_"), ("KERNEL", "PFG_KERNEL_"), ("SMOOTHER", "PFG_SMOOTHER_"), ("STAT", "PFG_STAT_"),
                 ("DTYPE", "PFG_"), ("RNG", "PFG_RNG_"))


def mirror_layout(mirror):
    """(size, [(field, offset, size)]) of a numpy structured dtype or a ctypes structure."""
    if isinstance(mirror, type) and issubclass(mirror, ctypes.Structure):
        return ctypes.sizeof(mirror), [(n, getattr(mirror, n).offset, getattr(mirror, n).size) for n, _ in mirror._fields_]
    return mirror.itemsize, [(n, mirror.fields[n][1], mirror.fields[n][0].itemsize) for n in mirror.names]


def enumerators(table, prefix):
    """C enumerator -> value behind one of the binding's name tables ("philox" is its alias of "device", not an enumerator)."""
    return {prefix + key.upper(): value for key, value in getattr(_capi, table).items() if (table, key) != ("RNG", "philox")}


def mirrored_values():
    """name -> value of everything the binding restates from the header: the struct layouts (the field names are the
    mirrors'), the constants and the enumerators; the keys are C expressions of type size_t or int."""
    want = {}
    for c_name, py_name in ABI_STRUCTS:
        size, fields = mirror_layout(getattr(_capi, py_name))
        want["sizeof({0})".format(c_name)] = size
        for field, offset, width in fields:
            want["offsetof({0}, {1})".format(c_name, field)] = offset
            want["sizeof((({0} *)0)->{1})".format(c_name, field)] = width
    for name in ("MAX_STAT", "MAX_THETA", "OUT_DOUBLES", "MAX_PRED", "STAMP_WORDS", "MAX_DRAWN_SEQUENCES", "SMC_RESULT_DOUBLES",
                 "FLAG_GARCH_STATIONARY_PRIOR", "FLAG_PARIS_NO_ACCEPT_REJECT", "FLAG_PARIS_RAW_STREAM", "FLAG_PARIS_RAW_CARRY",
                 "FLAG_ADAPTIVE_RESAMPLING"):
        want["PFG_" + name] = getattr(_capi, name)
    for name in ("GRID_PHASE_INIT", "GRID_PHASE_FINISH", "GRID_PHASE_ALL"):
        want["PFG_" + name] = getattr(_capi.Context, name)
    for name in ("PFG_OK", "PFG_ERR_INVALID", "PFG_ERR_UNSUPPORTED", "PFG_ERR_DEVICE", "PFG_ERR_NOMEM", "PFG_ERR_NUMERIC"):
        want[name] = getattr(_capi, name)
    for table, prefix in ENUM_PREFIXES:
        want.update(enumerators(table, prefix))
    return want


def test_binding_layouts_constants_and_enums_match_the_header(tmp_path):
    """A C99 program that includes pfgrad.h prints sizeof of the seven ABI structs, offsetof and the member size of every
    field of their mirrors, every constant and every enumerator the binding restates; each must equal the Python side.
    The fields are the mirrors', and a struct's sizeof must equal its mirror's size, so a field a mirror lacks shows too;
    the header's enums must hold no enumerator the binding lacks."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    want = mirrored_values()
    # the ctypes forms of pfg_problem / pfg_result (what pfg_run_batch is handed) lay out as their numpy forms do
    assert mirror_layout(_capi.Problem) == mirror_layout(_capi.PROBLEM_DTYPE)
    assert mirror_layout(_capi.Result) == mirror_layout(_capi.RESULT_DTYPE)
    assert _capi.RNG["philox"] == _capi.RNG["device"]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfgrad.h")).read(), flags=re.S)
    for table, prefix in ENUM_PREFIXES:
        declared = set(re.findall(r"\b" + (r"PFG_F\d+" if table == "DTYPE" else prefix + r"\w+") + r"\b", header))
        assert declared == set(enumerators(table, prefix)), (table, declared)
    src = tmp_path / "abi_layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"pfgrad.h\"\nint main(void) {\n" +
                   "".join("    printf(\"%ld\\n\", (long)({0}));\n".format(expr) for expr in want) +
                   "    return 0;\n}\n")
    exe = str(tmp_path / "abi_layout")
    res = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                          str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stderr)
    got = [int(line) for line in run.stdout.split()]
    assert len(got) == len(want)
    wrong = {expr: (c_value, py_value) for (expr, py_value), c_value in zip(want.items(), got) if c_value != py_value}
    assert not wrong, wrong          # expression -> (the header's value, the binding's)


def test_header_declares_expected_entry_points():
    names = declared_functions()
    assert set(names) == set(_capi.EXPORTS), (names, _capi.EXPORTS)


def test_library_exports_every_declared_symbol():
    if _build.is_stale():
        _build.build_library()
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in declared_functions():
        assert hasattr(lib, name), name


def test_binding_struct_sizes_version_and_grid_scratch():
    """ABI struct sizes, the version, the variant names of the plan, and pfg_scratch_bytes of the whole-GPU window equal
    to the Python mirror of its layout on both sides of every tile-class and coarse-stride boundary.  (The REPLAY layout
    reserves min(16384, ceil(N / 64)) coarse entries, so the sizes above 2^20 are those of a layout monotone in N.)"""
    lib = _capi.load_library()          # asserts the struct sizes against pfg_struct_size()
    assert lib.pfg_version() == 126
    assert lib.pfg_struct_size(2) == _capi.DEV_PROBLEM_DTYPE.itemsize == 376
    assert lib.pfg_struct_size(99) == -1
    assert lib.pfg_variant_name(0, 0, 0, 1, 1000) == b"wg256x4s"
    assert lib.pfg_variant_name(0, 0, 0, 1, 100) == b"wg64x2s"        # N <= 128, throughput: one wave per window
    assert lib.pfg_variant_name(0, 0, 0, 1, 200) == b"wg64x4s"         # 128 < N <= 256, device generator, many windows
    assert lib.pfg_variant_name(0, 0, 0, 0, 200) == b"wg256x1"         # ... the REPLAY units
    assert lib.pfg_variant_name(0, 0, 0, 1, 1024) == b"wg256x4s"
    assert lib.pfg_variant_name(0, 0, 0, 0, 1025) == b"mem1024"       # N > 1024: state in HBM scratch
    assert lib.pfg_variant_name(0, 0, 0, 1, 1025) == b"wg1024x4s"     # ... device generator, SVM fp64: still fits LDS (32-bit CDF)
    assert lib.pfg_variant_name(2, 1, 0, 1, 4096) == b"big4096"       # LGSSM fp64 (5 arrays) does not: fast large-N kernel
    assert lib.pfg_variant_name(2, 1, 1, 1, 4096) == b"wg1024x4s"     # ... in f32 it does
    assert lib.pfg_variant_name(0, 0, 0, 1, 10000) == b"big16384"
    assert lib.pfg_variant_name(1, 1, 0, 1, 1000) == b"wg512x2s"      # GARCH fp64 (n=2, h=4) still LDS-resident: 8 waves
    assert lib.pfg_variant_name(1, 1, 0, 0, 1000) == b"wg256x4s"      # ... the REPLAY units keep 256 x 4
    assert lib.pfg_variant_name(1, 1, 0, 0, 4000) == b"mem1024" and lib.pfg_variant_name(1, 1, 0, 1, 4000) == b"big4096"
    assert lib.pfg_variant_name(0, 0, 0, 0, 10000) == b"mem1024"
    # above the one-workgroup kernels' 16384: the whole-GPU window (tiles of 1024 particles up to 2^19, of 2048 above)
    assert lib.pfg_variant_name(0, 0, 0, 1, 20000) == b"grid1024" and lib.pfg_variant_name(0, 0, 0, 0, 500000) == b"grid1024" and lib.pfg_variant_name(0, 0, 0, 0, 1000000) == b"grid2048"
    assert lib.pfg_variant_name(0, 0, 0, 1, (1 << 22) + 1) == b"none"
    assert lib.pfg_scratch_bytes(0, 0, 1, 1000) == 0 and lib.pfg_scratch_bytes(0, 0, 1, (1 << 22) + 1) == -1
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "helpers"))
    from grid_layout import grid_layout
    for model, mname in enumerate(("svm", "garch", "lgssm")):
        for dtype, dname in enumerate(("f64", "f32")):
            for rng in (0, 1):
                for N in (16385, 100000, 1 << 19, (1 << 19) + 1, 1000000, 1 << 20, (1 << 20) + 1, 1 << 21, (1 << 21) + 1,
                          (1 << 22) - 1, 1 << 22):
                    assert lib.pfg_scratch_bytes(model, dtype, rng, N) == grid_layout(mname, dname, N, rng == 0)["bytes"]
    assert lib.pfg_scratch_bytes(0, 0, 1, 10000) == (10000 * 9 * 8 + 16 + 255) // 256 * 256


def test_no_cpu_fallback_without_gpu():
    """Without a HIP device the product path must fail loudly, never fall back."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(_capi.PfgError, match="no HIP device|no CPU fallback"):
        _capi.Context(0)
    assert "oracle" not in " ".join(open(os.path.join(os.path.dirname(_capi.__file__), f)).read()
                                    for f in os.listdir(os.path.dirname(_capi.__file__)) if f.endswith(".py")
                                    ).replace("oracle fixtures", "")


@pytest.mark.gpu
def test_plain_c_consumer_gpu(tmp_path):
    """The same C program on an MI355X: pfg_create + pfg_run from plain C reproduce the REFERENCE's numbers
    for the traced case pf_trace.npz:c0 (tests/c_abi/known_answer.h) at rtol 1e-9; the program returns non-zero
    and this test fails if log-likelihood or any gradient component differs."""
    out = _build_and_run_c_consumer(tmp_path)
    assert "run rc=0" in out and "known answer ok" in out and "differs" not in out, out


def test_plain_c_consumer(tmp_path):
    """include/pfgrad.h compiles as C99 with gcc and a C program links against libpfgrad.so
    (without a GPU it must report the missing device loudly)."""
    out = _build_and_run_c_consumer(tmp_path)
    assert "run rc=0" in out or "create failed as expected" in out, out


def _build_and_run_c_consumer(tmp_path):
    import shutil
    import subprocess
    if _build.is_stale():
        _build.build_library()
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path / "abi_check")
    libdir = os.path.dirname(_build.LIB_PATH)
    cmd = [gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "tests", "c_abi"),
           os.path.join(ROOT, "tests", "c_abi", "abi_check.c"), "-o", exe,
           "-L", libdir, "-lpfgrad", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    return run.stdout
