"""The host side of the satisfiability check (csrc/satcheck.hpp through libspg_hostcheck.so), the layout of its two
report structs, and the Python-integer reference the GPU tests compare against. CPU only."""
import ctypes
import os
import subprocess

import pytest

import sat_ref
import sparse_cases
from test_abi import HDR, header_struct_fields, header_text


@pytest.fixture(scope="module")
def hc():
    import spg

    lib = spg.hostcheck()
    lib.spgh_sat_merge.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.spgh_sat_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p]
    return lib


def _rec(rows, violations=0, p=0, q=0, row=0, tag=0):
    import spg

    r = spg.CSatReport(rows, violations, p, q, row)
    if violations:
        for i in range(4):
            r.az[i], r.bz[i], r.cz[i] = tag + i, tag + 10 + i, tag + 20 + i
    return r


def _merge(hc, recs):
    import spg

    arr = (spg.CSatReport * len(recs))(*recs)
    out = spg.CSatReport()
    assert hc.spgh_sat_merge(arr, len(recs), ctypes.byref(out)) == 0
    return out


def test_merge_sums_counts_and_keeps_the_lowest_row(hc):
    recs = [_rec(100, 2, p=3, q=1, row=7, tag=100), _rec(60), _rec(40, 5, p=1, q=2, row=0, tag=200),
            _rec(8, 1, p=1, q=0, row=9, tag=300)]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):  # whichever rank holds the lowest row
        out = _merge(hc, [recs[i] for i in order])
        assert (out.rows, out.violations) == (208, 8)
        assert (out.p, out.q, out.row) == (1, 0, 9)
        assert list(out.az) == [300, 301, 302, 303] and list(out.bz) == [310, 311, 312, 313]
        assert list(out.cz) == [320, 321, 322, 323]


def test_merge_orders_by_p_then_q_then_row(hc):
    a, b = _rec(1, 1, p=2, q=0, row=50, tag=1), _rec(1, 1, p=2, q=1, row=0, tag=2)
    assert _merge(hc, [b, a]).az[0] == 1
    c = _rec(1, 1, p=2, q=0, row=49, tag=3)
    assert _merge(hc, [a, b, c]).az[0] == 3
    d = _rec(1, 1, p=1, q=9, row=99, tag=4)
    assert _merge(hc, [a, d, c]).az[0] == 4


def test_merge_of_clean_ranks_is_all_zero(hc):
    import spg

    # a clean rank's p, q, row are not read (zero in what the library sends; made non-zero here)
    out = _merge(hc, [_rec(10, 0, p=5, q=5, row=5), _rec(22)])
    assert (out.rows, out.violations) == (32, 0)
    assert bytes(out)[16:] == bytes(ctypes.sizeof(spg.CSatReport) - 16)


def test_key_decoding_reverses_q_and_row(hc):
    """instance 1 of (4 x 8, 2 x 4, 1 x 2): rows [32, 40); the natural key 32 + 1 * 4 + 3 is (1, 1, 3), stored at
    32 + brev(1, 1 bit) * 4 + brev(3, 2 bits) = 32 + 4 + 3"""
    npf = (ctypes.c_size_t * 3)(4, 2, 1)
    nc = (ctypes.c_size_t * 3)(8, 4, 2)
    out = (ctypes.c_uint64 * 4)()
    assert hc.spgh_sat_decode(npf, nc, 3, 39, out) == 0 and list(out) == [1, 1, 3, 39]
    assert hc.spgh_sat_decode(npf, nc, 3, 32 + 1, out) == 0 and list(out) == [1, 0, 1, 32 + 2]
    assert hc.spgh_sat_decode(npf, nc, 3, 1 * 8 + 3, out) == 0 and list(out) == [0, 1, 3, 2 * 8 + 6]
    assert hc.spgh_sat_decode(npf, nc, 3, 41, out) == 0 and list(out) == [2, 0, 1, 41]  # lg_q = 0
    assert hc.spgh_sat_decode(npf, nc, 3, 42, out) == -1  # past the domain
    assert hc.spgh_sat_decode((ctypes.c_size_t * 1)(3), (ctypes.c_size_t * 1)(8), 1, 0, out) == -1  # not a power of two


def test_report_structs_match_their_ctypes_mirrors(tmp_path):
    import spg

    mirrors = {"spg_sat_report": spg.CSatReport, "spg_snark_report": spg.CSnarkReport}
    text = header_text()
    fields = {s: header_struct_fields(text, s) for s in mirrors}
    assert fields["spg_sat_report"] == ["rows", "violations", "p", "q", "row", "az", "bz", "cz"]
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


def test_error_code_and_constants():
    import spg

    assert spg.SPG_ERRORS[-8] == "SPG_E_UNSAT" and spg.SPG_E_UNSAT == -8
    assert "#define SPG_E_UNSAT -8" in open(HDR).read()
    assert (spg.SAT_BLOCK, spg.SAT_PAIRWISE, spg.SAT_PERM_ROOT) == (0, 1, 2)
    assert (spg.FIRST_NONE, spg.FIRST_PERM_EXEC, spg.FIRST_PERM_PHY, spg.FIRST_PERM_VIR, spg.FIRST_IO) == (-1, 3, 4, 5, 6)


def test_reference_accepts_the_satisfiable_workload():
    wl = sparse_cases.satisfiable()
    r = sat_ref.report(wl)
    assert r.rows == 4 * 64 + 2 * 16 and r.violations == 0 and r.p is None


def test_reference_names_a_changed_scalar():
    """the fresh column X + 15 of (instance 1, execution 1) carries (A z)[15]: changing it breaks exactly that row"""
    wl = sat_ref.tamper(sparse_cases.satisfiable(), 1, 1, 16 + 15)
    r = sat_ref.report(wl)
    assert (r.violations, r.p, r.q, r.row) == (1, 1, 1, 15)
    assert r.bz == 1 and r.cz == 12345 and r.az != r.cz


def test_reference_on_unsatisfied_workloads():
    """the structured cases' witnesses were never made to fit their matrices: most break many rows (below_cells_x256,
    whose C is empty and whose A and B share no row, breaks none: 0 * b == 0)"""
    for case in sparse_cases.CASES:
        r = sat_ref.report(sparse_cases.structured(case))
        assert r.rows == sum(x * q for x, q in zip(*sparse_cases.CASES[case][:2]))
        assert 0 <= r.violations < r.rows
        assert (r.violations > 0) == (case != "below_cells_x256"), case
        assert r.violations == 0 or (r.az * r.bz - r.cz) % sat_ref.Q != 0
