"""TEST HELPER loader: ctypes bindings over tests/r1cs_seams_oracle/build/libr1cs_seams_oracle.so, the pieces of the
oracle's R1CSProof::prove (tests/r1cs_seams_oracle/r1cs_seams_oracle.cpp, built from oracle/*.hpp as they stand) that
pyoracle does not expose one by one. Scalars are Montgomery [u64; 4] rows; a DensePolynomialPqx crosses flat in its
allocation layout (instance p's num_proofs[p] x nws x num_inputs[p] scalars row-major, instances concatenated)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "r1cs_seams_oracle")
_LIB_PATH = os.path.join(_HERE, "build", "libr1cs_seams_oracle.so")
_lib = None

GENS_LABEL = b"gens_r1cs_sat"
GENS_NV = 1 << 10  # R1CSGens(label, num_vars): gens_1 is the generator after gens_pc's 2^5, gens_4 the label's first 4


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


def _sz(v):
    return np.asarray(list(v), dtype=np.uint64)


def _c(n):
    return ctypes.c_size_t(n)


def zk_len(rounds):
    """bytes of bincode(ZKSumcheckInstanceProof) of `rounds` cubic rounds: three Vec lengths; per round two points and
    a DotProductProof (two points, a Vec of 4 scalars, two scalars)"""
    return 24 + rounds * (64 + 64 + 8 + 4 * 32 + 64)


def _sizes(s, P):
    s = [int(x) for x in s]
    return tuple(s[:4]), s[4:4 + P], s[4 + P:4 + 2 * P]


def new_rev(z, num_proofs, max_np, nws, num_inputs, max_ni):
    """Pqx::new_rev of z in (p, q, w, x) order -> (flat table, (dims, num_proofs, num_inputs))"""
    P = len(num_proofs)
    zz = _u(z, -1, 4)
    out = np.zeros_like(zz)
    sizes = np.zeros(4 + 2 * P, np.uint64)
    assert lib().rs_new_rev(_p(zz), _c(P), _p(_sz(num_proofs)), _c(max_np), _c(nws), _p(_sz(num_inputs)), _c(max_ni),
                            _p(out), _p(sizes)) == 0
    return out, _sizes(sizes, P)


def eval_tables(cinst, nws, max_ni, num_inputs, evals_rx):
    """the three per-matrix eval tables, each flat [p][w][i] over the instance's own matrices; None where the
    reference would index past its vector"""
    Pm = int(cinst.num_instances)
    n = sum(nws * int(x) for x in num_inputs[:Pm])
    rx = _u(evals_rx, -1, 4)
    outs = [np.zeros((n, 4), np.uint64) for _ in range(3)]
    rc = lib().rs_eval_tables(ctypes.byref(cinst), _c(nws), _c(max_ni), _p(_sz(num_inputs)), _p(rx), _c(rx.shape[0]),
                              *[_p(o) for o in outs])
    return outs if rc == 0 else None


def abc_poly(cinst, num_instances, nws, max_ni, num_inputs, evals_rx, rA, rB, rC):
    """(r_A A + r_B B + r_C C) of the eval tables through new_rev -> (flat table, sizes)"""
    Pm = int(cinst.num_instances)
    n = sum(nws * int(x) for x in num_inputs[:Pm])
    rx = _u(evals_rx, -1, 4)
    out = np.zeros((n, 4), np.uint64)
    sizes = np.zeros(4 + 2 * Pm, np.uint64)
    rc = lib().rs_abc_poly(ctypes.byref(cinst), _c(num_instances), _c(nws), _c(max_ni), _p(_sz(num_inputs)), _p(rx),
                           _c(rx.shape[0]), _p(_u(rA)), _p(_u(rB)), _p(_u(rC)), _p(out), _p(sizes))
    assert rc == 0, rc
    return out, _sizes(sizes, Pm)


def commit1(x, blind):
    out = np.zeros(32, np.uint8)
    assert lib().rs_commit1(ctypes.c_char_p(GENS_LABEL), _c(GENS_NV), _p(_u(x)), _p(_u(blind)), _p(out)) == 0
    return out.tobytes()


def phase1_round(mode, Ap, Aq, Ax, tabs, alloc_np, alloc_ni, cur):
    """the oracle's phase1_round_evals on the tables' current state; cur = (dims, num_proofs, num_inputs) as
    Pqx.shape() returns them. The round's lengths and local sizes are halved here as the reference's loop does."""
    dims, npf, nin = cur
    P = len(alloc_np)
    Ap, Aq, Ax = (_u(a, -1, 4) for a in (Ap, Aq, Ax))
    il, pl, cl = Ap.shape[0], Aq.shape[0], Ax.shape[0]
    if mode == 4:
        cl //= 2
    elif mode == 2:
        pl //= 2
    else:
        il //= 2
    lnp, lnc = list(npf), list(nin)
    for p in range(min(il, P)):
        if mode == 4 and lnc[p] > 1:
            lnc[p] //= 2
        if mode == 2 and lnp[p] > 1:
            lnp[p] //= 2
    out = np.zeros((3, 4), np.uint64)
    B, C, D = (_u(t, -1, 4) for t in tabs)
    assert lib().rs_phase1_round(ctypes.c_int(mode), _c(il), _c(pl), _c(cl), _c(P), _p(_sz(alloc_np)),
                                 _p(_sz(alloc_ni)), _p(_sz([dims[0]] + list(npf) + list(nin))), _p(_sz(lnp)),
                                 _p(_sz(lnc)), _p(Ap), _c(Ap.shape[0]), _p(Aq), _c(Aq.shape[0]), _p(Ax),
                                 _c(Ax.shape[0]), _p(B), _p(C), _p(D), _p(out)) == 0
    return out


def _zk_bufs(rounds, n_claims):
    cap = zk_len(rounds) + 64
    return dict(proof=np.zeros(cap, np.uint8), cap=cap, n=ctypes.c_size_t(0), r=np.zeros((rounds, 4), np.uint64),
                claims=np.zeros((n_claims, 4), np.uint64), blind=np.zeros(4, np.uint64), check=np.zeros(64, np.uint8),
                nxt=np.zeros(4, np.uint64))


def phase1(label, seed, nx, nq, np_, Ap, Aq, Ax, num_proofs, num_cons, B, C, D):
    """prove_phase1 on Transcript(label), RandomTape("proof", seed). Returns a dict: proof, r, claims (4), blind,
    B / C / D (bound, flat), sizes (of B), eq3 (Ap[0], Aq[0], Ax[0]), check (64 bytes), tape_next."""
    P = len(num_proofs)
    o = _zk_bufs(nx + nq + np_, 4)
    Bs = [_u(t, -1, 4) for t in (B, C, D)]
    outs = [np.zeros_like(t) for t in Bs]
    sizes = np.zeros(4 + 2 * P, np.uint64)
    eq3 = np.zeros((3, 4), np.uint64)
    rc = lib().rs_phase1(ctypes.c_char_p(GENS_LABEL), _c(GENS_NV), ctypes.c_char_p(label), _p(_u(seed)), _c(nx), _c(nq),
                         _c(np_), _p(_u(Ap, -1, 4)), _p(_u(Aq, -1, 4)), _p(_u(Ax, -1, 4)), _c(P), _p(_sz(num_proofs)),
                         _p(_sz(num_cons)), *[_p(t) for t in Bs], _p(o["proof"]), _c(o["cap"]), ctypes.byref(o["n"]),
                         _p(o["r"]), _p(o["claims"]), _p(o["blind"]), *[_p(t) for t in outs], _p(sizes), _p(eq3),
                         _p(o["check"]), _p(o["nxt"]))
    assert rc == 0, rc
    return dict(proof=o["proof"][:o["n"].value].tobytes(), r=o["r"], claims=o["claims"], blind=o["blind"], B=outs[0],
                C=outs[1], D=outs[2], sizes=_sizes(sizes, P), eq3=eq3, check=o["check"].tobytes(), tape_next=o["nxt"])


def phase2(label, seed, claim, blind_claim, ny, nw, np_, single, nws, eq, num_inputs_abc, ABC, num_proofs, max_np,
           num_inputs, z, rq):
    """prove_phase2 on Transcript(label), RandomTape("proof", seed), over eq, ABC (flat, new_rev order, one proof row)
    and Z = new_rev(z) bound at rq. Returns a dict: proof, r, claims (3), blind, ABC / Z (bound, flat), sizes_abc,
    sizes_z, eq0, check, tape_next."""
    P, Pa = len(num_proofs), len(num_inputs_abc)
    o = _zk_bufs(ny + nw + np_, 3)
    ABC, z = _u(ABC, -1, 4), _u(z, -1, 4)
    n_rq = len(rq)
    rq = _u(rq, -1, 4) if n_rq else np.zeros((1, 4), np.uint64)
    Ao, Zo = np.zeros_like(ABC), np.zeros_like(z)
    sa, sz = np.zeros(4 + 2 * Pa, np.uint64), np.zeros(4 + 2 * P, np.uint64)
    eq0 = np.zeros(4, np.uint64)
    rc = lib().rs_phase2(ctypes.c_char_p(GENS_LABEL), _c(GENS_NV), ctypes.c_char_p(label), _p(_u(seed)), _p(_u(claim)),
                         _p(_u(blind_claim)), _c(ny), _c(nw), _c(np_), ctypes.c_int(1 if single else 0), _c(nws),
                         _p(_u(eq, -1, 4)), _c(Pa), _p(_sz(num_inputs_abc)), _p(ABC), _c(P), _p(_sz(num_proofs)),
                         _c(max_np), _p(_sz(num_inputs)), _p(z), _p(rq), _c(n_rq), _p(o["proof"]), _c(o["cap"]),
                         ctypes.byref(o["n"]), _p(o["r"]), _p(o["claims"]), _p(o["blind"]), _p(Ao), _p(sa), _p(Zo),
                         _p(sz), _p(eq0), _p(o["check"]), _p(o["nxt"]))
    assert rc == 0, rc
    return dict(proof=o["proof"][:o["n"].value].tobytes(), r=o["r"], claims=o["claims"], blind=o["blind"], ABC=Ao, Z=Zo,
                sizes_abc=_sizes(sa, Pa), sizes_z=_sizes(sz, P), eq0=eq0, check=o["check"].tobytes(),
                tape_next=o["nxt"])


def verify(label, comm_claim, rounds, proof):
    """ZKSumcheckProof::verify on Transcript(label): (accepted, comm_claim_post, r, 64-byte transcript check)"""
    pb = np.frombuffer(bytes(proof), np.uint8).copy() if len(proof) else np.zeros(1, np.uint8)
    cc = np.frombuffer(bytes(comm_claim), np.uint8).copy()
    post, check = np.zeros(32, np.uint8), np.zeros(64, np.uint8)
    r = np.zeros((max(rounds, 1), 4), np.uint64)
    ok = lib().rs_verify(ctypes.c_char_p(GENS_LABEL), _c(GENS_NV), ctypes.c_char_p(label), _p(cc), _c(rounds), _p(pb),
                         _c(len(proof)), _p(post), _p(r), _p(check))
    return bool(ok), post.tobytes(), r[:rounds], check.tobytes()


def chain(cinst, wl, z, label, seed):
    """R1CSProof::prove's body from multiply_vec_block to the end of phase 2 (no sigma proofs between the phases; the
    phase-2 claim's blind is zero) -> (phase-1 proof, phase-2 proof, claims2 [3, 4], check, tape_next)"""
    lx, lq = (wl.max_num_cons - 1).bit_length(), (wl.max_num_proofs - 1).bit_length()
    lp, lw, ly = (wl.P - 1).bit_length(), (wl.nws - 1).bit_length(), (wl.max_num_inputs - 1).bit_length()
    c1, c2 = zk_len(lx + lq + lp) + 64, zk_len(ly + lw + lp) + 64
    p1, p2 = np.zeros(c1, np.uint8), np.zeros(c2, np.uint8)
    n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    claims2, check, nxt = np.zeros((3, 4), np.uint64), np.zeros(64, np.uint8), np.zeros(4, np.uint64)
    rc = lib().rs_chain(ctypes.byref(cinst), _c(wl.P), _p(_sz(wl.num_proofs)), _c(wl.max_num_proofs),
                        _p(_sz(wl.num_inputs)), _c(wl.max_num_inputs), _c(wl.nws), _p(_u(z, -1, 4)),
                        ctypes.c_char_p(GENS_LABEL), _c(GENS_NV), ctypes.c_char_p(label), _p(_u(seed)), _p(p1), _c(c1),
                        ctypes.byref(n1), _p(p2), _c(c2), ctypes.byref(n2), _p(claims2), _p(check), _p(nxt))
    assert rc == 0, rc
    return p1[:n1.value].tobytes(), p2[:n2.value].tobytes(), claims2, check.tobytes(), nxt
