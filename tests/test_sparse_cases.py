"""Structured sparse matrices (tests/sparse_cases.py) on the CPU: the cases have the structure they are there for,
the oracle's SPARK round trip verifies on every one, R1CSProof::prove runs on them and does not depend on the order
of a matrix's entry list, and the satisfiable case passes prove -> verify. Bytes frozen in
tests/golden/spark_proofs.json and r1cs_proofs.json under structured_<case>."""
import hashlib
import json
import os

import numpy as np
import pytest

import sparse_cases
from sparse_cases import CASES

G = os.path.join(os.path.dirname(__file__), "golden")
Q = sparse_cases.Q


def _golden(name, case):
    return json.load(open(os.path.join(G, name)))["structured_" + case]


def test_cases_are_structured():
    """ragged nnz (0, 1, 37, > num_cons, > cells), hot rows and columns beyond a workgroup, duplicates, the special
    values, shuffled order, one tiled and one shared case, N on both sides of the number of cells"""
    seen = set()
    for case, (nc, npf, nws, shared, nnz) in CASES.items():
        wl = sparse_cases.structured(case)
        cells = 1 << max((wl.max_num_cons - 1).bit_length(), (wl.num_vars - 1).bit_length())
        N = 1 << (max(nnz) - 1).bit_length()
        seen.add("N>cells" if N > cells else "N<cells")
        assert len(wl.entries) == (1 if shared else len(nc)) and len(set(nnz)) == len(nnz)
        for p, mats in enumerate(wl.entries):
            for m, M in enumerate(mats):
                n = nnz[3 * p + m]
                assert M.shape == (n, 6)
                seen.add({0: "empty", 1: "single", 37: "37"}.get(n, "other"))
                if n > wl.num_cons[p]:
                    seen.add("nnz>num_cons")
                if n > cells:
                    seen.add("nnz>cells")
                if n == 0:
                    continue
                assert int(M[:, 0].max()) < wl.num_cons[p]
                assert all(int(c) // wl.max_num_inputs < nws and int(c) % wl.max_num_inputs < wl.num_inputs[p]
                           for c in M[:, 1]), "a column outside the instance's witness width"
                if n < 8:
                    continue
                rows, cols = np.bincount(M[:, 0].astype(np.int64)), np.bincount(M[:, 1].astype(np.int64))
                assert rows.max() >= n // 3 and cols.max() >= n // 3
                if n >= 770:
                    assert rows.max() > 256 and cols.max() > 256
                    seen.add("hot>256")
                assert len({(int(r), int(c)) for r, c in M[:, :2]}) < n, "no duplicate (row, col)"
                vals = set(sparse_cases._ints(M[:, 2:]))
                assert {0, 1, Q - 1} <= vals and len(vals) > 3
                order = M[:, 0].astype(np.int64) * (1 << 32) + M[:, 1].astype(np.int64)
                assert (np.diff(order) < 0).any(), "entries sorted by (row, col)"
        if min(wl.num_cons[:len(wl.entries)]) >= 256:
            seen.add("tiled")
        if shared:
            seen.add("shared")
    assert seen >= {"N>cells", "N<cells", "empty", "single", "37", "nnz>num_cons", "nnz>cells", "hot>256", "tiled",
                    "shared"}, seen


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_spark_roundtrip(oracle, case):
    import workload

    wl = sparse_cases.structured(case)
    rx, ry = sparse_cases.eval_point(oracle, wl)
    comm, proof, ok = oracle.spark_prove(wl, rx, ry, workload.tape_seed())
    assert ok, "the oracle's SPARK verifier rejected its own proof"
    assert _golden("spark_proofs.json", case) == {"comm_sha256": hashlib.sha256(comm).hexdigest(),
                                                  "proof_sha256": hashlib.sha256(proof).hexdigest(),
                                                  "proof_len": len(proof)}


def _eval_ref(M, rx, ry):
    """sum_e val_e eq(rx, row_e) eq(ry, col_e) on Python integers (challenge j binds bit j from the top)"""
    def eq(r, i):
        out = 1
        for j, x in enumerate(r):
            out = out * (x if (i >> (len(r) - 1 - j)) & 1 else 1 - x) % Q
        return out

    vals = sparse_cases._ints(M[:, 2:]) if len(M) else []
    return sum(v * eq(rx, int(e[0])) * eq(ry, int(e[1])) for e, v in zip(M, vals)) % Q


def test_oracle_multi_evaluate_against_integers(oracle):
    """the oracle's multi_evaluate itself, on matrices with duplicates and an empty matrix, against the definition"""
    wl = sparse_cases.structured("ragged_p2_x64")
    rx, ry = sparse_cases.eval_point(oracle, wl)
    got = sparse_cases._ints(oracle.r1cs_multi_evaluate(wl, rx, ry))
    rxi, ryi = sparse_cases._ints(rx), sparse_cases._ints(ry)
    want = [_eval_ref(M, rxi, ryi) for mats in wl.entries for M in mats]
    assert got == want and want[2] == 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_r1cs_prove_ignores_entry_order(oracle, case):
    import workload

    wl = sparse_cases.structured(case)
    pf, _ = oracle.r1cs_prove(wl, workload.tape_seed())
    assert _golden("r1cs_proofs.json", case) == {"len": len(pf), "sha256": hashlib.sha256(pf).hexdigest()}
    st = sparse_cases.sorted_entries(wl)
    assert any((a != b).any() for x, y in zip(wl.entries, st.entries) for a, b in zip(x, y))
    assert oracle.r1cs_prove(st, workload.tape_seed())[0] == pf


def test_satisfiable_case(oracle):
    """(A z) * (B z) = C z row by row on Python integers; the oracle proves and its verifier accepts"""
    import workload

    wl = sparse_cases.satisfiable()
    for p in range(wl.P):
        A, B, C = wl.entries[p]
        assert np.bincount(A[:, 0].astype(np.int64)).max() >= 16 and len(A) > 4 * wl.num_cons[p]
        z = [sparse_cases._ints(wl.sections[w][p][0]) for w in range(wl.nws)]  # execution 0
        mv = lambda M: [sum(v * z[int(e[1]) // wl.max_num_inputs][int(e[1]) % wl.max_num_inputs]
                            for e, v in zip(M, sparse_cases._ints(M[:, 2:])) if int(e[0]) == r) % Q
                        for r in range(wl.num_cons[p])]
        az, bz, cz = mv(A), mv(B), mv(C)
        assert all(a * b % Q == c for a, b, c in zip(az, bz, cz)) and any(az)
    pf, _ = oracle.r1cs_prove(wl, workload.tape_seed())
    assert oracle.r1cs_verify(wl, pf, workload.tape_seed()) == 1
    assert _golden("r1cs_proofs.json", "satisfiable") == {"len": len(pf), "sha256": hashlib.sha256(pf).hexdigest()}
