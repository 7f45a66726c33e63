"""The descriptor builders of the R1CS table kernels (csrc/r1cs_desc.hpp) without a GPU, through libspg_hostcheck.so:
every field of every SpDesc (k_spmv) and AbcDesc (k_abc) and the pqx_shape offsets, for the forms the prover's table
setup and the seams ask for, against values computed here from the definitions: offsets are prefix sums of
rows * secs * cols over the instances a caller holds, the logs are lg2 of the sizes, and the matrix index is the
caller's global instance index, or 0 when one matrix triple serves every instance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spartan-parallel_amd")
HC = os.environ.get("SPG_HOSTCHECK_LIB", os.path.join(PKG, "lib", "libspg_hostcheck.so"))
Z = ctypes.c_size_t
VP = ctypes.c_void_p

# (num_cons, num_proofs, num_inputs, sections, one matrix triple for every instance, the rank's range [p0, p1)).
# The shared shape's inputs and sections are free; 2 sections and unequal widths keep every field distinct.
SHAPES = {
    "ragged": ([16, 8, 4], [4, 1, 2], [8, 4, 2], 3, False, (0, 3)),
    "shared": ([8, 8], [2, 4], [4, 2], 2, True, (0, 2)),
    "rank_range": ([16, 8, 4], [4, 1, 2], [8, 4, 2], 3, False, (1, 3)),
}


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(HC):
        subprocess.check_call(["make", "-s", "-C", PKG, "lib/libspg_hostcheck.so"])
    lib = ctypes.CDLL(HC)
    lib.spgh_pqx_shape.restype = None
    lib.spgh_pqx_shape.argtypes = [Z, VP, Z, VP, VP, VP]
    lib.spgh_r1cs_sp_descs.restype = Z
    lib.spgh_r1cs_sp_descs.argtypes = [VP, VP, VP, Z, Z, ctypes.c_int, ctypes.c_int, VP]
    lib.spgh_r1cs_abc_descs.restype = None
    lib.spgh_r1cs_abc_descs.argtypes = [VP, Z, Z, Z, VP]
    lib.spgh_r1cs_mat_descs.restype = None
    lib.spgh_r1cs_mat_descs.argtypes = [Z, VP, VP, VP]
    return lib


def _sz(v):
    return np.asarray(v, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(VP)


def lg2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


def prefix(sizes):
    """offsets of blocks packed one after another, and their total"""
    off, o = [], 0
    for s in sizes:
        off.append(o)
        o += s
    return off, o


def sp_descs(hc, cons, proofs, inputs, p0, p1, single, log_ni):
    out = np.zeros((p1 - p0, 8), np.uint64)
    n = hc.spgh_r1cs_sp_descs(_p(_sz(proofs)), _p(_sz(cons)), _p(_sz(inputs)), p0, p1, int(single), int(log_ni), _p(out))
    assert n == p1 - p0
    keys = ("dom_off", "out_off", "pi", "lg_q", "nrows", "lg_rows", "ni", "lg_ni")
    return [dict(zip(keys, (int(v) for v in row))) for row in out]


def abc_descs(hc, inputs, pi0, n, secs):
    out = np.zeros((n, 6), np.uint64)
    hc.spgh_r1cs_abc_descs(_p(_sz(inputs)), pi0, n, secs, _p(out))
    keys = ("dom_off", "out_off", "pi", "ni", "lg_ni", "pad")
    return [dict(zip(keys, (int(v) for v in row))) for row in out]


def pqx_shape(hc, rows, secs, cols):
    off = np.zeros(len(rows), np.uint64)
    total = np.zeros(1, np.uint64)
    hc.spgh_pqx_shape(len(rows), _p(_sz(rows)), secs, _p(_sz(cols)), _p(off), _p(total))
    return [int(v) for v in off], int(total[0])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_sp_descs(hc, name):
    cons, proofs, inputs, _, single, (p0, p1) = SHAPES[name]
    loc = range(p0, p1)
    off, _ = prefix([proofs[p] * cons[p] for p in loc])  # the rank's own Az, Bz, Cz: offsets are local
    want = [dict(dom_off=off[k], out_off=off[k], pi=0 if single else p, lg_q=lg2(proofs[p]), nrows=cons[p],
                 lg_rows=lg2(cons[p]), ni=inputs[p], lg_ni=lg2(inputs[p])) for k, p in enumerate(loc)]
    got = sp_descs(hc, cons, proofs, inputs, p0, p1, single, True)
    assert got == want
    if name == "rank_range":  # pi is the caller's instance index while the offsets start at the rank's first instance
        assert [d["pi"] for d in got] == [1, 2] and got[0]["dom_off"] == 0 and got[1]["dom_off"] == proofs[1] * cons[1]
    # the multiply_vec_block seam: the same list but for lg_ni, which k_spmv does not read
    seam = sp_descs(hc, cons, proofs, inputs, p0, p1, single, False)
    assert [d["lg_ni"] for d in seam] == [0] * len(want)
    assert [dict(d, lg_ni=w["lg_ni"]) for d, w in zip(seam, want)] == want
    assert [(d["dom_off"], d["out_off"]) for d in seam] == [(d["dom_off"], d["out_off"]) for d in got]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_abc_descs(hc, name):
    _, _, inputs, secs, single, (p0, p1) = SHAPES[name]
    # the prover's ABC: the shared matrix once, or the rank's own matrices; the seams: every matrix of the handle
    pi0, n = (0, 1) if single else (p0, p1 - p0)
    forms = [(pi0, n)] + ([] if single else [(0, len(inputs))])
    for first, count in forms:
        off, _ = prefix([secs * inputs[first + k] for k in range(count)])
        want = [dict(dom_off=off[k], out_off=off[k], pi=first + k, ni=inputs[first + k], lg_ni=lg2(inputs[first + k]),
                     pad=0) for k in range(count)]
        assert abc_descs(hc, inputs, first, count, secs) == want, (first, count)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_pqx_shape_offsets(hc, name):
    cons, proofs, inputs, secs, _, (p0, p1) = SHAPES[name]
    lp, lc, li = proofs[p0:p1], cons[p0:p1], inputs[p0:p1]
    ones = [1] * len(lp)
    for rows, s, cols in ((lp, secs, li), (lp, 1, lc), (ones, secs, li), (ones, 1, ones)):  # Z, Az, ABC, compact
        assert pqx_shape(hc, rows, s, cols) == prefix([r * s * c for r, c in zip(rows, cols)])


def test_mat_descs(hc):
    rp = _sz([0, 17, 34, 51, 60, 69])  # [3 p + m]
    cp = _sz([0, 33])
    out = np.zeros((2, 4), np.uint64)
    hc.spgh_r1cs_mat_descs(2, _p(rp), _p(cp), _p(out))
    assert out.tolist() == [[0, 17, 34, 0], [51, 60, 69, 33]]
