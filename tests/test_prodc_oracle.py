"""CPU: the checker of the product-circuit seams (tests/prodc_oracle, the oracle's ProductCircuit, hash layer,
prove_cubic_batched and ProductCircuitEvalProofBatched behind a C interface) pinned against the oracle's field ops and
the restatement of prove_cubic in test_gpu_seams.py, and the C-ABI surface of the seams (include/spg.h, libspg.so)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import prodc_ref
from test_gpu_seams import mont, prove_cubic_ref, rand_fq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg.so")
HDR = os.path.join(ROOT, "include", "spg.h")

NEW_SYMBOLS = ["spg_hash_layer", "spg_prodc_new", "spg_prodc_free", "spg_prodc_shape", "spg_prodc_evaluate",
               "spg_prodc_layer", "spg_prove_cubic_batched", "spg_prodc_prove_batched"]


def test_seams_declared_and_exported():
    """every seam entry is declared in include/spg.h and exported by libspg.so; the library exports exactly the
    header's spg_* declarations and no oracle symbol"""
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(spg_[a-z0-9_]+)\s*\(", src))
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(LIB)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()[-1].startswith(("spg_", "orc_", "po_"))}
    assert exported == declared


def fq_prod(oracle, v):
    acc = v[0]
    for x in v[1:]:
        acc = oracle.fq_op("mul", acc, x)[0]
    return acc


@pytest.mark.parametrize("M", [2, 8])
def test_circuit_layers(oracle, M):
    rng = np.random.default_rng(M)
    leaves = rand_fq(oracle, rng, M)
    ls, rs, ev = prodc_ref.circuit_layers(leaves)
    assert len(ls) == M.bit_length() - 1
    assert np.array_equal(ls[0], leaves[:M // 2]) and np.array_equal(rs[0], leaves[M // 2:])
    assert np.array_equal(ev, fq_prod(oracle, leaves))
    for k in range(len(ls) - 1):  # layer k + 1 = the element-wise product of layer k's halves
        nxt = oracle.fq_op("mul", ls[k], rs[k])
        assert np.array_equal(np.concatenate([ls[k + 1], rs[k + 1]]), nxt)


def hash_formula(oracle, addr, val, ts, rh, rms):
    n = addr.shape[0]
    rep = lambda x: np.repeat(x.reshape(1, 4), n, axis=0)  # noqa: E731
    rh2 = oracle.fq_op("mul", rh, rh)[0]
    s = oracle.fq_op("add", oracle.fq_op("mul", ts, rep(rh2)), oracle.fq_op("mul", val, rep(rh)))
    return oracle.fq_op("sub", oracle.fq_op("add", s, addr), rep(rms))


def test_hash_layer_formula(oracle):
    rng = np.random.default_rng(11)
    cells, n, ops = 8, 2, 4
    table, audit_ts = rand_fq(oracle, rng, cells), rand_fq(oracle, rng, cells)
    addrs, derefs, rts = (rand_fq(oracle, rng, n * ops).reshape(n, ops, 4) for _ in range(3))
    rh, rms = rand_fq(oracle, rng, 2)
    init, reads, writes, audit = prodc_ref.hash_layer(table, audit_ts, addrs, derefs, rts, rh, rms)
    idx = np.stack([mont(i) for i in range(cells)])
    zero, one = np.zeros((cells, 4), np.uint64), np.repeat(mont(1).reshape(1, 4), ops, axis=0)
    assert np.array_equal(init, hash_formula(oracle, idx, table, zero, rh, rms))
    assert np.array_equal(audit, hash_formula(oracle, idx, table, audit_ts, rh, rms))
    for k in range(n):
        assert np.array_equal(reads[k], hash_formula(oracle, addrs[k], derefs[k], rts[k], rh, rms))
        assert np.array_equal(writes[k], hash_formula(oracle, addrs[k], derefs[k], oracle.fq_op("add", rts[k], one), rh, rms))


def test_prove_batched_verifies_and_rejects_tampering(oracle):
    rng = np.random.default_rng(16)
    M, nc, nd = 16, 2, 2
    leaves = rand_fq(oracle, rng, nc * M).reshape(nc, M, 4)
    dotp = rand_fq(oracle, rng, nd * 3 * (M // 2)).reshape(nd, 3, M // 2, 4)
    proof, rand, check, ok = prodc_ref.prove_batched(b"prodc", leaves, dotp)
    assert ok and rand.shape == (4, 4) and len(check) == 64
    proof2, _, check2, ok2 = prodc_ref.prove_batched(b"prodc", leaves, dotp, tamper=True)
    assert proof2 == proof and check2 == check  # the prover's side is the same run
    assert not ok2  # one byte inside claims_prod_left changed: the verifier's final check fails


def test_cubic_batched_single_triple_is_prove_cubic(oracle):
    """n_par = 0, n_seq = 1, coeffs = [1]: prove_cubic_batched is prove_cubic (src/sumcheck.rs:193-262)"""
    rng = np.random.default_rng(4)
    ell = 4
    A, B, C = (rand_fq(oracle, rng, 1 << ell) for _ in range(3))
    claim = rand_fq(oracle, rng, 1)[0]
    polys, r, bound, _ = prodc_ref.cubic_batched(b"cubic", claim, ell, [], [], C.copy(), A[None], B[None], C[None],
                                                 mont(1).reshape(1, 4))
    tr = oracle.OracleTranscript(b"cubic")
    rpolys, rr, rclaims = prove_cubic_ref(oracle, claim, ell, A, B, C, tr)
    assert np.array_equal(polys, np.stack(rpolys))
    assert np.array_equal(r, np.stack(rr))
    assert np.array_equal(np.stack([bound["Aseq"][0, 0], bound["Bseq"][0, 0], bound["Cseq"][0, 0]]), rclaims)
