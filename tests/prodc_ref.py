"""TEST HELPER loader: ctypes bindings over tests/prodc_oracle/build/libprodc_oracle.so, the oracle's product-circuit
entries (tests/prodc_oracle/prodc_oracle.cpp, built from oracle/*.hpp as they stand) that pyoracle does not expose.
Scalars are Montgomery [u64; 4] rows, as everywhere in the tests."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prodc_oracle")
_LIB_PATH = os.path.join(_HERE, "build", "libprodc_oracle.so")
_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE], stdout=subprocess.DEVNULL)


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(_LIB_PATH)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _u(x, *shape):
    a = np.ascontiguousarray(x, dtype=np.uint64)
    return a.reshape(*shape) if shape else a


def hash_layer(eval_table, audit_ts, addrs, derefs, read_ts, r_hash, r_multiset):
    """addrs, derefs, read_ts: [n, ops, 4]. Returns init [cells, 4], reads [n, ops, 4], writes, audit."""
    cells = eval_table.shape[0]
    a, d, t = (_u(x) for x in (addrs, derefs, read_ts))
    n, ops = a.shape[0], a.shape[1]
    init, audit = np.zeros((cells, 4), np.uint64), np.zeros((cells, 4), np.uint64)
    reads, writes = np.zeros((n, ops, 4), np.uint64), np.zeros((n, ops, 4), np.uint64)
    rc = lib().po_hash_layer(_p(_u(eval_table)), _p(_u(audit_ts)), ctypes.c_size_t(cells), _p(a), _p(d), _p(t),
                             ctypes.c_size_t(n), ctypes.c_size_t(ops), _p(_u(r_hash)), _p(_u(r_multiset)), _p(init),
                             _p(reads), _p(writes), _p(audit))
    assert rc == 0
    return init, reads, writes, audit


def circuit_layers(leaves):
    """ProductCircuit::create of [M, 4] leaves: ([left_vec[k]], [right_vec[k]], evaluate())"""
    M = leaves.shape[0]
    left, right = np.zeros((M - 1, 4), np.uint64), np.zeros((M - 1, 4), np.uint64)
    ev = np.zeros(4, np.uint64)
    assert lib().po_circuit_layers(_p(_u(leaves)), ctypes.c_size_t(M), _p(left), _p(right), _p(ev)) == 0
    ls, rs, o, h = [], [], 0, M // 2
    while h >= 1:
        ls.append(left[o:o + h])
        rs.append(right[o:o + h])
        o += h
        h //= 2
    return ls, rs, ev


def cubic_batched(label, claim, num_rounds, Apar, Bpar, Cpar, Aseq, Bseq, Cseq, coeffs):
    """Apar, Bpar: [n_par, len, 4]; Cpar: [len, 4]; Aseq, Bseq, Cseq: [n_seq, len, 4]. Returns polys [rounds, 3, 4],
    r [rounds, 4], the bound vectors as a dict (Apar, Bpar: [n_par, m, 4]; Cpar: [m, 4]; Aseq ..: [n_seq, m, 4], m =
    len >> rounds) and the 64-byte transcript check."""
    n_par, n_seq, ln = len(Apar), len(Aseq), Cpar.shape[0]
    m = ln >> num_rounds
    z = np.zeros((1, 4), np.uint64)
    arrs = [_u(x) if len(x) else z for x in (Apar, Bpar)] + [_u(Cpar)] + [_u(x) if len(x) else z for x in (Aseq, Bseq, Cseq)]
    polys = np.zeros((max(num_rounds, 1), 3, 4), np.uint64)
    r = np.zeros((max(num_rounds, 1), 4), np.uint64)
    bound = np.zeros((2 * n_par + 1 + 3 * n_seq, m, 4), np.uint64)
    check = np.zeros(64, np.uint8)
    rc = lib().po_cubic_batched(ctypes.c_char_p(label), _p(_u(claim)), ctypes.c_size_t(num_rounds), _p(arrs[0]),
                                _p(arrs[1]), ctypes.c_size_t(n_par), _p(arrs[2]), _p(arrs[3]), _p(arrs[4]), _p(arrs[5]),
                                ctypes.c_size_t(n_seq), ctypes.c_size_t(ln), _p(_u(coeffs)), _p(polys), _p(r), _p(bound),
                                _p(check))
    assert rc == 0
    o = 2 * n_par + 1
    out = {"Apar": bound[:n_par], "Bpar": bound[n_par:2 * n_par], "Cpar": bound[2 * n_par], "Aseq": bound[o:o + n_seq],
           "Bseq": bound[o + n_seq:o + 2 * n_seq], "Cseq": bound[o + 2 * n_seq:]}
    return polys[:num_rounds], r[:num_rounds], out, check.tobytes()


def prove_batched(label, leaves, dotp, tamper=False):
    """leaves: [nc, M, 4]; dotp: [nd, 3, M/2, 4] (may be empty). Returns (proof bytes, rand [log2 M, 4], 64-byte
    transcript check, whether the oracle's verifier accepted the (tampered, if asked) proof)."""
    lv = _u(leaves)
    nc, M = lv.shape[0], lv.shape[1]
    nd = len(dotp)
    dp = _u(dotp) if nd else np.zeros((1, 4), np.uint64)
    cap = 1 << 20
    proof = np.zeros(cap, np.uint8)
    n = ctypes.c_size_t(0)
    rand = np.zeros((max(M.bit_length() - 1, 1), 4), np.uint64)
    check = np.zeros(64, np.uint8)
    ok = ctypes.c_int(-1)
    rc = lib().po_prove_batched(ctypes.c_char_p(label), _p(lv), ctypes.c_size_t(nc), ctypes.c_size_t(M), _p(dp),
                                ctypes.c_size_t(nd), ctypes.c_int(1 if tamper else 0), _p(proof), ctypes.c_size_t(cap),
                                ctypes.byref(n), _p(rand), _p(check), ctypes.byref(ok))
    assert rc == 0
    return proof[:n.value].tobytes(), rand[:M.bit_length() - 1].copy(), check.tobytes(), bool(ok.value)
