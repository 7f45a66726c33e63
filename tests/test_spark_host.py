"""The host-only pieces of the SPARK prover without a GPU, through libspg_hostcheck.so: the shape both multi_commit and
the prover derive from sizes (csrc/spark_shape.hpp) against the oracle's commitments, the sharded product trees' top
levels against the oracle's ProductCircuit, the decoders of the grids that two and three sumcheck rounds in one launch
post (csrc/hostmath.hpp) against direct evaluation, and the workspace slot table (csrc/ws_slots.hpp)."""
import ctypes
import itertools
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import fieldref as fr
from r1cs_cases import SPARK_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spartan-parallel_amd")
HC = os.environ.get("SPG_HOSTCHECK_LIB", os.path.join(PKG, "lib", "libspg_hostcheck.so"))
Z = ctypes.c_size_t
Q = fr.Q


@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(HC):
        subprocess.check_call(["make", "-s", "-C", PKG, "lib/libspg_hostcheck.so"])
    lib = ctypes.CDLL(HC)
    lib.spgh_ws_table.restype = Z
    lib.spgh_ws_table.argtypes = [ctypes.c_char_p, Z]
    lib.spgh_spark_shape.restype = None
    lib.spgh_spark_shape.argtypes = [Z] * 8 + [ctypes.c_void_p]
    lib.spgh_spark_commit_refusal.argtypes = [Z] * 9 + [ctypes.c_char_p, Z]
    lib.spgh_spark_comm_refusal.argtypes = [Z] * 9 + [ctypes.c_char_p, Z]
    for f in (lib.spgh_tree_tops, lib.spgh_pair_rounds, lib.spgh_triple_rounds):
        f.restype = None
    lib.spgh_tree_tops.argtypes = [ctypes.c_void_p, Z, ctypes.c_void_p]
    lib.spgh_pair_rounds.argtypes = [ctypes.c_void_p] * 3
    lib.spgh_triple_rounds.argtypes = [ctypes.c_void_p] * 3
    lib.spgh_fold_corners.restype = None
    lib.spgh_fold_corners.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def mont(vals):
    return fr.arr_u64([fr.to_mont(v % Q) for v in vals])


def plain(a):
    return [fr.from_mont(v) for v in fr.ints(a)]


# ---------------------------------------------------------------- 1. shape
SHAPE_FIELDS = ("N", "cells", "nv_ops", "nv_mem", "nv_der", "ops_len", "mem_len", "der_len", "gens_n", "ops_rows",
                "mem_rows")


def shape(hc, B, max_nnz, nvx, nvy, gens_nvx, gens_nvy, gens_nnz, gens_batch):
    out = np.zeros(len(SHAPE_FIELDS), np.uint64)
    hc.spgh_spark_shape(B, max_nnz, nvx, nvy, gens_nvx, gens_nvy, gens_nnz, gens_batch, _p(out))
    return dict(zip(SHAPE_FIELDS, (int(v) for v in out)))


def parse_commitment(comm):
    """bincode(SparseMatPolyCommitment): batch_size, num_ops, num_mem_cells, comm_comb_ops, comm_comb_mem (each a
    u64 count of 32-byte row commitments)"""
    B, N, cells, n_ops = struct.unpack_from("<4Q", comm, 0)
    (n_mem,) = struct.unpack_from("<Q", comm, 32 + 32 * n_ops)
    assert len(comm) == 40 + 32 * (n_ops + n_mem)
    return B, N, cells, n_ops, n_mem


@pytest.mark.parametrize("case", sorted(SPARK_CASES))
def test_shape_matches_oracle_commitment(hc, oracle, case):
    import workload
    from test_oracle_spark import spark_inputs

    wl, rx, ry = spark_inputs(oracle, case)
    comm, _, ok = oracle.spark_prove(wl, rx, ry, workload.tape_seed())
    assert ok
    # the inputs pyoracle.spark_prove gives the reference: the batch [A_0, B_0, C_0, ...], R1CSCommitmentGens' sizes
    max_nnz = max(int(m.shape[0]) for mats in wl.entries for m in mats)
    nvx, nvy = (wl.max_num_cons - 1).bit_length(), (wl.num_vars - 1).bit_length()
    sp = shape(hc, 3 * len(wl.entries), max_nnz, nvx, nvy, nvx, nvy, len(wl.entries) * max_nnz, 3)
    assert parse_commitment(comm) == (3 * len(wl.entries), sp["N"], sp["cells"], sp["ops_rows"], sp["mem_rows"])
    # .. and what the handle derives from them
    B, N, cells = 3 * len(wl.entries), sp["N"], sp["cells"]
    assert sp["ops_len"] == 1 << (5 * B * N - 1).bit_length() and sp["mem_len"] == 2 * cells
    assert sp["der_len"] == 1 << (2 * B * N - 1).bit_length()
    assert sp["gens_n"] == max(1 << (nv - nv // 2) for nv in (sp["nv_ops"], sp["nv_mem"], sp["nv_der"]))


def refusal(fn, *args):
    msg = ctypes.create_string_buffer(128)
    rc = fn(*args, msg, len(msg))
    assert bool(rc) == bool(msg.value)
    return msg.value.decode()


def test_refusals_at_their_bounds(hc):
    TOO_SMALL = "SPARK generators (gens_nnz, gens_batch) too small for the batch"
    # B = 3 matrices of N = 16 ops over 2^4 x 2^4: comb_ops has npow2(240) = 2^8 entries, the derefs 2^7, the memory 2^5.
    # gens_batch = 3 gives nv_ops = lg(npow2(gens_nnz)) + 4 and nv_der = lg(npow2(gens_nnz)) + 3: gens_nnz = 16 just fits
    B, N, cells, nv = 3, 16, 16, 4
    commit = lambda gx, gy, gnnz: refusal(hc.spgh_spark_commit_refusal, B, N, cells, nv, nv, gx, gy, gnnz, 3)
    assert commit(4, 4, 16) == "" and commit(4, 4, 9) == ""  # (npow2(9) = 16)
    assert commit(4, 4, 8) == TOO_SMALL
    assert commit(3, 4, 16) == "" and commit(3, 3, 16) == TOO_SMALL  # nv_mem = max(gens_nvx, gens_nvy) + 1
    assert refusal(hc.spgh_spark_commit_refusal, 1 << 15, 1 << 16, cells, nv, nv, 4, 4, 1 << 40, 3) == "SPARK batch too large"
    assert refusal(hc.spgh_spark_commit_refusal, (1 << 15) - 1, 1 << 16, cells, nv, nv, 4, 4, 1 << 40, 1 << 20) == ""
    # a commitment read back: 2^(8 / 2) rows of comb_ops, 2^(5 / 2) of comb_mem, and nothing else
    ROWS = "SPARK commitment row counts do not match its sizes"
    FIT = "SPARK commitment sizes do not fit the generators"
    comm = lambda ro, rm, gnnz=16, n=N, c=cells: refusal(hc.spgh_spark_comm_refusal, B, n, c, ro, rm, 4, 4, gnnz, 3)
    assert comm(16, 4) == ""
    for ro, rm in ((15, 4), (17, 4), (32, 4), (16, 3), (16, 5), (16, 8), (0, 4), (16, 0)):
        assert comm(ro, rm) == ROWS, (ro, rm)
    assert comm(16, 4, gnnz=8) == FIT
    assert comm(16, 4, n=12) == FIT and comm(16, 4, n=1) == FIT and comm(16, 4, c=24) == FIT
    assert comm(16, 4, c=32) == FIT  # 2^6 memory entries against nv_mem = 5
    assert comm(16, 4, n=1 << 33) == FIT and comm(16, 4, c=1 << 33) == FIT  # (ranges checked before any length forms)


# ---------------------------------------------------------------- 2. sharded tree tops
@pytest.mark.parametrize("W", [2, 4, 8])  # 2: no inner level; 8: the smallest with two
def test_tree_tops_match_product_circuit(hc, W):
    import prodc_ref

    rng = np.random.default_rng(100 + W)
    for _ in range(2):
        leaves = mont([int.from_bytes(rng.bytes(40), "little") for _ in range(W)])
        ls, rs, product = prodc_ref.circuit_layers(leaves)
        v = np.zeros((2 * W, 4), np.uint64)
        v[:W] = leaves
        prod = np.zeros(4, np.uint64)
        hc.spgh_tree_tops(_p(v), W, _p(prod))
        assert np.array_equal(prod, product)
        assert len(ls) == W.bit_length() - 1
        o = 0
        for left, right in zip(ls, rs):  # level k = left ++ right, back to back
            n = 2 * len(left)
            assert np.array_equal(v[o:o + n], np.concatenate([left, right])), o
            o += n
        assert o == 2 * W - 2 and not v[o:].any()


# ---------------------------------------------------------------- 3. multi-round grids
def poly3(rng, nvars):
    """a random polynomial of degree 3 in each variable: coefficients c[a][b][..] of x^a y^b .."""
    c = np.empty((4,) * nvars, dtype=object)
    for idx in itertools.product(range(4), repeat=nvars):
        c[idx] = int.from_bytes(rng.bytes(40), "little") % Q
    return c


def ev(c, *pt):
    return sum(c[idx] * math.prod(pow(x, e, Q) for x, e in zip(pt, idx))
               for idx in itertools.product(range(4), repeat=len(pt))) % Q


def challenges(rng, n):
    """every n-tuple over the edge values 0, 1, q - 1 and one random value"""
    return list(itertools.product([0, 1, Q - 1, int.from_bytes(rng.bytes(40), "little") % Q], repeat=n))


def test_pair_grid(hc):
    rng = np.random.default_rng(7)
    F = poly3(rng, 2)  # F(t, s): t round j's variable, s round j + 1's
    grid = [ev(F, t, Y) for Y in (0, 2, 3) for t in range(4)] + [ev(F, X, 1) for X in (0, 2, 3)]
    corners = [ev(F, t, s) for t in (0, 1) for s in (0, 1)]
    for rj, rj1 in challenges(rng, 2):
        out = np.zeros((6, 4), np.uint64)
        hc.spgh_pair_rounds(_p(mont(grid)), _p(mont([rj])), _p(out))
        want = [(ev(F, X, 0) + ev(F, X, 1)) % Q for X in (0, 2, 3)] + [ev(F, rj, Y) for Y in (0, 2, 3)]
        assert plain(out) == want, (rj, rj1)
        fold = np.zeros(4, np.uint64)
        hc.spgh_fold_corners(2, _p(mont(corners)), _p(mont([rj, rj1])), _p(fold))
        ml = sum(corners[2 * t + s] * (rj if t else 1 - rj) * (rj1 if s else 1 - rj1) for t in (0, 1) for s in (0, 1)) % Q
        assert plain(fold) == [ml], (rj, rj1)


def test_triple_grid(hc):
    rng = np.random.default_rng(8)
    F = poly3(rng, 3)  # F(t, s, u), the variables of rounds j, j + 1, j + 2
    grid = [ev(F, t, s, u) for u in range(4) for s in range(4) for t in range(4)]  # ev[t + 4 s + 16 u]
    corners = [ev(F, t, s, u) for t in (0, 1) for s in (0, 1) for u in (0, 1)]     # w[4 t + 2 s + u]
    for rj, rj1, rj2 in challenges(rng, 3):
        out = np.zeros((9, 4), np.uint64)
        hc.spgh_triple_rounds(_p(mont(grid)), _p(mont([rj, rj1])), _p(out))
        want = [sum(ev(F, X, s, u) for s in (0, 1) for u in (0, 1)) % Q for X in (0, 2, 3)]
        want += [(ev(F, rj, Y, 0) + ev(F, rj, Y, 1)) % Q for Y in (0, 2, 3)]
        want += [ev(F, rj, rj1, Zv) for Zv in (0, 2, 3)]
        assert plain(out) == want, (rj, rj1, rj2)
        fold = np.zeros(4, np.uint64)
        hc.spgh_fold_corners(3, _p(mont(corners)), _p(mont([rj, rj1, rj2])), _p(fold))
        ml = sum(corners[4 * t + 2 * s + u] * (rj if t else 1 - rj) * (rj1 if s else 1 - rj1) * (rj2 if u else 1 - rj2)
                 for t in (0, 1) for s in (0, 1) for u in (0, 1)) % Q
        assert plain(fold) == [ml], (rj, rj1, rj2)


# ---------------------------------------------------------------- 4. slot table
def test_slot_table(hc):
    n = hc.spgh_ws_table(None, 0)
    buf = ctypes.create_string_buffer(n)
    assert hc.spgh_ws_table(buf, n) == n
    rows = [line.split("\t") for line in buf.raw.decode().splitlines()]
    assert rows and all(len(r) == 3 for r in rows)
    names = [r[0] for r in rows]
    assert all(nm and nm != "?" and nm.isidentifier() for nm in names), names
    assert len(set(names)) == len(names), "a slot is declared twice"
    csrc = os.path.join(PKG, "csrc")
    for _, owner, what in rows:
        assert what.strip()
        assert all(os.path.exists(os.path.join(csrc, f.strip())) for f in owner.split(",")), owner
