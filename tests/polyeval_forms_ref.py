"""TEST HELPER loader: ctypes bindings over tests/polyeval_forms_oracle/build/libpolyeval_forms_oracle.so, the oracle's
disjoint-rounds and univariate PolyEvalProof forms (tests/polyeval_forms_oracle/polyeval_forms_oracle.cpp, built from
oracle/*.hpp as they stand). Scalars are Montgomery [u64; 4] rows, as everywhere in the tests.

Both prove wrappers return a Proved: the bincode bytes, the 64 challenge bytes and the tape scalar drawn after the
prover (the positions it left transcript and tape in), whether the oracle's own verifier accepted the proof, the number
of proofs, the prover's C_Zr_prime (univariate form) and the commitments C_Zr_i = Zr_i G_n to the evaluations."""
import collections
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "polyeval_forms_oracle")
_LIB_PATH = os.path.join(_HERE, "build", "libpolyeval_forms_oracle.so")
_lib = None

TAPE = b"proof"
CAP = 1 << 20

Proved = collections.namedtuple("Proved", "proof check tape_next verified nproofs C_Zr C_Zr_list")


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


def _u(x):
    a = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)
    return a if len(a) else np.zeros((1, 4), np.uint64)


def _sz(v):
    return (ctypes.c_size_t * max(len(v), 1))(*v)


def _cat(rows):
    return np.ascontiguousarray(np.concatenate([_u(r) for r in rows]))


class _Out:
    def __init__(self, n):
        self.proof = np.zeros(CAP, np.uint8)
        self.n = ctypes.c_size_t(0)
        self.k = ctypes.c_size_t(1)
        self.check = np.zeros(64, np.uint8)
        self.tape_next = np.zeros(4, np.uint64)
        self.ok = ctypes.c_int(-1)
        self.czr = np.zeros(32, np.uint8)
        self.czl = np.zeros((n, 32), np.uint8)

    def result(self, rc, single):
        assert rc == 0, rc
        return Proved(self.proof[:self.n.value].tobytes(), self.check.tobytes(), self.tape_next.copy(),
                      bool(self.ok.value), 1 if single else int(self.k.value), self.czr.tobytes() if single else None,
                      [row.tobytes() for row in self.czl])


def prove_disjoint(label, gens_nv, tlabel, seed, Zs, shapes, rq, ry, Zr_list):
    """prove_batched_instances_disjoint_rounds: Zs[i] [num_proofs_i * num_inputs_i, 4], shapes[i] = (num_proofs,
    num_inputs)"""
    n = len(Zs)
    o = _Out(n)
    rc = lib().pf_prove_disjoint(ctypes.c_char_p(label), ctypes.c_size_t(gens_nv), ctypes.c_char_p(tlabel),
                                 ctypes.c_char_p(TAPE), _p(_u(seed)), _p(_cat(Zs)), _sz([s[0] for s in shapes]),
                                 _sz([s[1] for s in shapes]), ctypes.c_size_t(n), _p(_u(rq)), ctypes.c_size_t(len(rq)),
                                 _p(_u(ry)), ctypes.c_size_t(len(ry)), _p(_u(Zr_list)), _p(o.proof),
                                 ctypes.c_size_t(CAP), ctypes.byref(o.n), ctypes.byref(o.k), _p(o.check),
                                 _p(o.tape_next), ctypes.byref(o.ok), _p(o.czl))
    return o.result(rc, single=False)


def prove_uni(label, gens_nv, tlabel, seed, Zs, nv_list, r, Zr_list):
    """prove_uni_batched_instances: Zs[i] [2^nv_list[i], 4], r one scalar"""
    n = len(Zs)
    o = _Out(n)
    rc = lib().pf_prove_uni(ctypes.c_char_p(label), ctypes.c_size_t(gens_nv), ctypes.c_char_p(tlabel),
                            ctypes.c_char_p(TAPE), _p(_u(seed)), _p(_cat(Zs)), _sz(nv_list), ctypes.c_size_t(n),
                            _p(_u(r)), _p(_u(Zr_list)), _p(o.proof), ctypes.c_size_t(CAP), ctypes.byref(o.n),
                            _p(o.czr), _p(o.check), _p(o.tape_next), ctypes.byref(o.ok), _p(o.czl))
    return o.result(rc, single=True)


def uni_evals(Zs, nv_list, r):
    """[n, 4]: sum_k Z_i[k] r^k"""
    out = np.zeros((len(Zs), 4), np.uint64)
    assert lib().pf_uni_evals(_p(_cat(Zs)), _sz(nv_list), ctypes.c_size_t(len(Zs)), _p(_u(r)), _p(out)) == 0
    return out
