"""libspg.so loads on a CPU-only host and exports every entry point include/spg.h declares; without a
gfx950 device spg_init must fail loudly (no CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg.so")
HDR = os.path.join(ROOT, "include", "spg.h")


def declared_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(spg_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "spg_init" in syms and "spg_msm" in syms and "spg_commit_rows" in syms


def test_library_exports_all_symbols():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(LIB)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_init_without_device_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a device is present")
    lib = ctypes.CDLL(LIB)
    h = ctypes.c_void_p()
    assert lib.spg_init(0, ctypes.byref(h)) == -5  # SPG_E_NODEVICE


# ---- the Python binding takes its signatures from the header (spg._signatures / spg._bind)
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def header_param_count(text, name):
    """parameters of `name(...)` counted by top-level commas, independently of the binding's own parser"""
    start = re.search(r"\b%s\s*\(" % re.escape(name), text).end()
    depth, commas, i = 1, 0, start
    while depth:
        c = text[i]
        if c in "([":
            depth += 1
        elif c in ")]":
            depth -= 1
        elif c == "," and depth == 1:
            commas += 1
        i += 1
    body = text[start:i - 1].strip()
    return 0 if body in ("", "void") else commas + 1


def test_every_declared_symbol_is_bound():
    import spg

    text = header_text()
    lib = spg.lib()
    sigs = spg._signatures(open(HDR).read())
    syms = declared_symbols()
    assert sorted(sigs) == syms and len(syms) >= 123
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes is not None, s
        assert len(fn.argtypes) == header_param_count(text, s), s
        assert fn.restype is sigs[s][0] and list(fn.argtypes) == sigs[s][1], s


def test_pinned_signatures():
    import spg

    lib = spg.lib()
    for s in ("spg_buf_len", "spg_gens_n", "spg_points_n", "spg_poly_gens_n"):
        assert getattr(lib, s).restype is ctypes.c_size_t, s
        assert list(getattr(lib, s).argtypes) == [ctypes.c_void_p], s
    assert lib.spg_last_kernel_us.restype is ctypes.c_double
    assert lib.spg_last_error.restype is ctypes.c_char_p
    assert list(lib.spg_init.argtypes) == [ctypes.c_int, ctypes.c_void_p]
    assert lib.spg_init.restype is ctypes.c_int
    assert lib.spg_set_vmsm_host_max.argtypes[1] is ctypes.c_long
    assert list(lib.spg_comb_stats.argtypes) == [ctypes.c_void_p] * 4
    # a callback typedef and an array parameter are pointers; size_t stays by value between them
    assert list(lib.spg_set_comm.argtypes) == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_void_p]
    assert list(lib.spg_points_sum_compress.argtypes) == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]


def test_signatures_refuse_an_unmapped_type():
    import spg

    assert spg._signatures("int spg_x(void);\nsize_t spg_y(const spg_buf* b, uint64_t k);") == {
        "spg_x": (ctypes.c_int, []), "spg_y": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_uint64])}
    with pytest.raises(ValueError, match=r"spg_x.*float a"):
        spg._signatures("int spg_x(spg_ctx* ctx, float a);")
    with pytest.raises(ValueError, match=r"spg_x.*float"):
        spg._signatures("float spg_x(spg_ctx* ctx);")


def test_bad_argument_stops_in_ctypes():
    import spg

    with pytest.raises(ctypes.ArgumentError):
        spg.lib().spg_gens_n(1.5)
    with pytest.raises(ctypes.ArgumentError):
        spg.lib().spg_points_sum_compress(None, 1.5, None)
    with pytest.raises(ctypes.ArgumentError):
        spg.lib().spg_points_sum_compress(None, ctypes.c_int(1), None)


# ---- the header is C: it compiles as C99 on its own, and its plain structs have the layout of the ctypes mirrors
def header_struct_fields(text, name):
    """field names of `typedef struct { ... } name;` in declaration order"""
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % re.escape(name), text).group(1)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names += [re.findall(r"[A-Za-z_]\w*", d.split("[")[0])[-1] for d in decl.split(",")]
    return names


def test_header_is_c99_and_structs_match_ctypes_mirrors(tmp_path):
    import subprocess

    import spg
    import workload

    mirrors = {"spg_sparse_entry": workload.SparseEntry, "spg_r1cs_instance": workload.CInstance,
               "spg_witness_sec": workload.CWitnessSec, "spg_witness_comm": spg.CWitnessComm,
               "spg_snark_instance": workload.CSnarkInstance, "spg_snark_inputs": workload.CSnarkInputs,
               "spg_snark_public": workload.CSnarkPublic}
    text = header_text()
    fields = {s: header_struct_fields(text, s) for s in mirrors}
    lines = ['#include "spg.h"', "#include <stdio.h>", "int main(void) {"]
    for s, names in fields.items():
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in names]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    cc = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    for s, mirror in mirrors.items():
        assert [f[0] for f in mirror._fields_] == fields[s], s
        assert int(got[s]) == ctypes.sizeof(mirror), s
        for f in fields[s]:
            assert int(got[f"{s}.{f}"]) == getattr(mirror, f).offset, f"{s}.{f}"
