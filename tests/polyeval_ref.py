"""TEST HELPER loader: ctypes bindings over tests/polyeval_oracle/build/libpolyeval_oracle.so, the oracle's dense
polynomial commitment entries (tests/polyeval_oracle/polyeval_oracle.cpp, built from oracle/*.hpp as they stand) that
pyoracle does not expose. Scalars are Montgomery [u64; 4] rows, as everywhere in the tests.

Every prove wrapper returns a Proved: the bincode bytes, the 64 challenge bytes and the tape scalar drawn after the
prover (the positions it left transcript and tape in), and whether the oracle's own verifier accepted the proof."""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "polyeval_oracle")
_LIB_PATH = os.path.join(_HERE, "build", "libpolyeval_oracle.so")
_lib = None

TAPE = b"proof"
CAP = 1 << 20

Proved = collections.namedtuple("Proved", "proof check tape_next verified nproofs C_Zr")


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE], stdout=subprocess.DEVNULL)


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(_LIB_PATH)
        _lib.pe_groups.restype = ctypes.c_long
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _u(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)


def _sz(v):
    return (ctypes.c_size_t * max(len(v), 1))(*v)


def _cat(rows):
    rows = [_u(r) for r in rows if len(r)]
    return np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((1, 4), np.uint64)


def commit(label, gens_nv, Z, nv, blinds=None):
    """DensePolynomial::commit / commit_with_blind: [2^(nv/2), 32] rows"""
    rows = np.zeros((1 << (nv // 2), 32), np.uint8)
    assert lib().pe_commit(ctypes.c_char_p(label), ctypes.c_size_t(gens_nv), _p(_u(Z)), ctypes.c_size_t(nv),
                           _p(_u(blinds)), _p(rows)) == 0
    return rows


def bound(Z, r, blinds=None):
    """(L.Z [2^(nv - nv/2), 4], sum_i blinds[i] L[i]) of PolyEvalProof::prove"""
    nv = len(r)
    LZ, b = np.zeros((1 << (nv - nv // 2), 4), np.uint64), np.zeros(4, np.uint64)
    assert lib().pe_bound(_p(_u(Z)), ctypes.c_size_t(nv), _p(_u(r)), _p(_u(blinds)), _p(LZ), _p(b)) == 0
    return LZ, b


class _Out:
    def __init__(self):
        self.proof = np.zeros(CAP, np.uint8)
        self.n = ctypes.c_size_t(0)
        self.k = ctypes.c_size_t(1)
        self.check = np.zeros(64, np.uint8)
        self.tape_next = np.zeros(4, np.uint64)
        self.ok = ctypes.c_int(-1)
        self.czr = np.zeros(32, np.uint8)

    def result(self, rc, single=False):
        assert rc == 0, rc
        return Proved(self.proof[:self.n.value].tobytes(), self.check.tobytes(), self.tape_next.copy(),
                      bool(self.ok.value), 1 if single else int(self.k.value), self.czr.tobytes() if single else None)


def prove(label, gens_nv, tlabel, seed, Z, r, Zr, blinds=None, blind_Zr=None, tamper=False):
    """PolyEvalProof::prove with optional blinds at the point r (len(r) variables)"""
    o = _Out()
    rc = lib().pe_prove(ctypes.c_char_p(label), ctypes.c_size_t(gens_nv), ctypes.c_char_p(tlabel),
                        ctypes.c_char_p(TAPE), _p(_u(seed)), _p(_u(Z)), ctypes.c_size_t(len(r)), _p(_u(r)), _p(_u(Zr)),
                        _p(_u(blinds)), _p(_u(blind_Zr)), ctypes.c_int(1 if tamper else 0), _p(o.proof),
                        ctypes.c_size_t(CAP), ctypes.byref(o.n), _p(o.czr), _p(o.check), _p(o.tape_next),
                        ctypes.byref(o.ok))
    return o.result(rc, single=True)


def prove_points(label, gens_nv, tlabel, seed, Z, nv, r_list, Zr_list, tamper=False):
    """PolyEvalProof::prove_batched_points: r_list [K, nv, 4]"""
    o = _Out()
    K = len(r_list)
    rc = lib().pe_prove_points(ctypes.c_char_p(label), ctypes.c_size_t(gens_nv), ctypes.c_char_p(tlabel),
                               ctypes.c_char_p(TAPE), _p(_u(seed)), _p(_u(Z)), ctypes.c_size_t(nv), _p(_cat(r_list)),
                               ctypes.c_size_t(K), _p(_u(Zr_list)), ctypes.c_int(1 if tamper else 0), _p(o.proof),
                               ctypes.c_size_t(CAP), ctypes.byref(o.n), ctypes.byref(o.k), _p(o.check),
                               _p(o.tape_next), ctypes.byref(o.ok))
    return o.result(rc)


def prove_instances(label, gens_nv, tlabel, seed, Zs, nv_list, r_list, Zr_list, tamper=False):
    """PolyEvalProof::prove_batched_instances: Zs[i] [2^nv_list[i], 4], r_list[i] [len_i, 4]"""
    o = _Out()
    n = len(Zs)
    rc = lib().pe_prove_instances(ctypes.c_char_p(label), ctypes.c_size_t(gens_nv), ctypes.c_char_p(tlabel),
                                  ctypes.c_char_p(TAPE), _p(_u(seed)), _p(_cat(Zs)), _sz(nv_list), ctypes.c_size_t(n),
                                  _p(_cat(r_list)), _sz([len(r) for r in r_list]), _p(_u(Zr_list)),
                                  ctypes.c_int(1 if tamper else 0), _p(o.proof), ctypes.c_size_t(CAP),
                                  ctypes.byref(o.n), ctypes.byref(o.k), _p(o.check), _p(o.tape_next),
                                  ctypes.byref(o.ok))
    return o.result(rc)


def groups(nv_list, r_list, instances):
    """(group [n], exponent [n], fitted points [sum nv_i, 4], number of groups) as the oracle's provers derive them;
    points form: nv_list = [nv]"""
    n = len(r_list)
    nvs = list(nv_list) if instances else [nv_list[0]] * n
    g, e = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    fitted = np.zeros((max(sum(nvs), 1), 4), np.uint64)
    k = lib().pe_groups(ctypes.c_int(1 if instances else 0), ctypes.c_size_t(n), _sz(nv_list), _p(_cat(r_list)),
                        _sz([len(r) for r in r_list]), g, e, _p(fitted))
    return list(g), list(e), fitted[:sum(nvs)], int(k)
