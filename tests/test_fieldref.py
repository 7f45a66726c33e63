"""tests/fieldref.py (the Python-integer reference of tests/test_gpu_primitives.py) pinned on the CPU: against the
oracle's Fq and group operations and the libsodium ristretto255 vectors; then libspg_hostcheck (the product's
headers compiled for the host) on the full edge-pair lists against it, and the three Ristretto decoders (big-int,
oracle, the product's 8 x u32 and radix-2^51 forms) on the decode candidates."""
import ctypes
import json
import os

import numpy as np
import pytest

import fieldref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HC = os.environ.get("SPG_HOSTCHECK_LIB") or os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg_hostcheck.so")


@pytest.fixture(scope="module")
def hc():
    import subprocess

    # make decides whether the library is current (spgh_hext_roundtrip is newer than some built copies)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "spartan-parallel_amd"), "lib/libspg_hostcheck.so"])
    return ctypes.CDLL(HC)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def fq_pairs():
    a, b = fr.edge_pairs(fr.fq_edges(), np.random.default_rng(101), 3000, fr.Q)
    return a, b, fr.arr_u64(a), fr.arr_u64(b)


@pytest.fixture(scope="module")
def fp_pairs():
    a, b = fr.edge_pairs(fr.fp_edges(), np.random.default_rng(102), 3000, 2**256)
    return a, b, fr.arr_u32(a), fr.arr_u32(b)


@pytest.mark.parametrize("op", ["add", "sub", "mul", "neg", "square", "invert"])
def test_reference_fq_matches_oracle(oracle, fq_pairs, op):
    a, b, A, B = fq_pairs
    code = fr.FQ_OPS[op]
    ref = oracle.fq_op(op, A, B) if op in ("add", "sub", "mul") else oracle.fq_op(op, A)
    assert fr.ints(ref) == [fr.fq_op(code, x, y) for x, y in zip(a, b)]


def test_reference_fq_montgomery_form(oracle):
    for x in (0, 1, 2, 2**64 - 1):
        assert fr.ints(oracle.fq_from_u64(x)) == [fr.to_mont(x)]
    vals = fr.fq_edges()
    by = oracle.fq_to_bytes(fr.arr_u64([fr.to_mont(v) for v in vals]))
    assert fr.ints(by) == vals
    assert all(fr.from_mont(fr.to_mont(v)) == v for v in vals)
    assert fr.fq_op(5, 0) == 0 and all(fr.fq_op(2, fr.fq_op(5, v), v) == fr.to_mont(1) for v in vals if v)


def test_reference_curve_matches_sodium_vectors():
    f = json.load(open(os.path.join(ROOT, "tests", "golden", "ristretto_sodium.json")))
    pts = {}
    for h, enc in f["from_hash"]:
        pt = fr.from_uniform_bytes(bytes.fromhex(h))
        assert fr.on_curve(pt) and fr.encode(pt).hex() == enc
        dec = fr.decode(bytes.fromhex(enc))
        assert dec is not None and fr.on_curve(dec) and fr.encode(dec).hex() == enc
        pts[enc] = dec
    for a, b, c in f["add"]:
        assert fr.encode(fr.pt_add(fr.decode(bytes.fromhex(a)), fr.decode(bytes.fromhex(b)))).hex() == c
    for p, k, out in f["scalarmult"][:8]:
        kk = int.from_bytes(bytes.fromhex(k), "little")
        assert fr.encode(fr.pt_mul(kk, fr.decode(bytes.fromhex(p)))).hex() == out


def test_reference_curve_matches_oracle(oracle):
    c = [int.from_bytes(x, "little") for x in oracle.ristretto_consts()]
    assert c == [fr.D, fr.SQRT_M1, fr.SQRT_AD_MINUS_ONE, fr.INVSQRT_A_MINUS_D, fr.ONE_MINUS_D_SQ, fr.D_MINUS_ONE_SQ]
    rng = np.random.default_rng(7)
    n = 48
    uni = rng.integers(0, 256, 64 * n, dtype=np.uint8)
    uni[:64] = 0          # both map inputs 0
    uni[64:128] = 0xFF    # top bits set: masked, then >= p before reduction
    ref = oracle.ge_from_uniform_bytes(uni.tobytes())
    pts = [fr.from_uniform_bytes(uni[64 * i:64 * i + 64].tobytes()) for i in range(n)]
    assert [fr.encode(p) for p in pts] == ref
    for i in range(n - 1):
        assert fr.encode(fr.pt_add(pts[i], pts[i + 1])) == oracle.ge_add(ref[i], ref[i + 1])
        assert fr.encode(fr.pt_add(pts[i], pts[i])) == oracle.ge_add(ref[i], ref[i])
    # every representative of the coset encodes alike, and P - P is the identity's all-zero string
    for p in pts[:8]:
        assert {fr.encode(fr.pt_add(p, t)) for t in fr.TORSION} == {fr.encode(p)}
        assert fr.encode(fr.pt_add(p, fr.pt_neg(p))) == bytes(32) == fr.encode(fr.IDENTITY)
    k = (fr.Q - 1).to_bytes(32, "little")
    assert fr.encode(fr.pt_neg(pts[3])) == oracle.ge_scalarmul(ref[3], k)


@pytest.mark.parametrize("C", [8, 9, 10, 12, 13, 14])
def test_reference_recode(C):
    NB, W = 1 << (C - 1), 253 // C + 1
    rng = np.random.default_rng(C)
    ks = fr.recode_patterns(C) + [int.from_bytes(rng.bytes(40), "little") % fr.Q for _ in range(200)]
    seen = set()
    for k in ks:
        d = fr.recode(k, C)  # asserts the sum and the final carry itself
        assert len(d) == W and all(-NB < x <= NB for x in d)
        seen.update(abs(x) for x in d)
    assert {0, 1, NB - 1, NB} <= seen
    api = fr.api_carry_scalars()
    assert len(set(api)) == len(api) and all(0 < v < fr.Q for v in api)


@pytest.mark.parametrize("code", range(10))
def test_hostcheck_fq_edge_pairs(hc, fq_pairs, code):
    """every Fq op of the host build on all ordered pairs of the edge list and 3000 random pairs: bit-identical to
    the integers, results canonical"""
    a, b, A, B = fq_pairs
    out = np.zeros_like(A)
    hc.spgh_fq_op(code, _p(A), _p(B), _p(out), ctypes.c_size_t(len(a)))
    got = fr.ints(out)
    assert all(v < fr.Q for v in got)
    bad = [(i, hex(a[i]), hex(b[i])) for i in range(len(a)) if got[i] != fr.fq_op(code, a[i], b[i])]
    assert not bad, bad[:3]


@pytest.mark.parametrize("code", range(13))
def test_hostcheck_fp_edge_pairs(hc, fp_pairs, code):
    """every Fp op of the host build on all ordered pairs of the loose edge list and 3000 random pairs: the value mod p
    for all, the canonical integer for the canonicalised ops, and fp_addsub's limbs equal to fp_add's / fp_sub's"""
    a, b, A, B = fp_pairs
    n = len(a)
    out = np.zeros_like(A)
    hc.spgh_fp_op(code, _p(A), _p(B), _p(out), ctypes.c_size_t(n))
    got = fr.ints(out)
    raw = code in (8, 9, 10, 11)
    bad = [(i, hex(a[i]), hex(b[i])) for i in range(n)
           if (got[i] % fr.P if raw else got[i]) != fr.fp_op(code, a[i], b[i])]
    assert not bad, bad[:3]
    if code in (8, 9):
        other = np.zeros_like(out)
        hc.spgh_fp_op(code + 2, _p(A), _p(B), _p(other), ctypes.c_size_t(n))
        assert np.array_equal(out, other)


def test_decoders_agree(oracle, hc):
    """which 32-byte strings decode: the big-int RFC 9496 decoder, the oracle, the product's device-form decoder
    (ext_decompress, host build) and the radix-2^51 decoder the verifier uses accept the same set and re-encode the
    accepted ones to the same bytes"""
    cand = fr.decode_candidates(np.random.default_rng(31))
    why = [fr.decode_why(c) for c in cand]
    valid = [w[0] is not None for w in why]
    assert sum(valid) >= 50 and len(valid) - sum(valid) >= 300
    assert {w[1] for w in why if w[0] is None} == set(fr.REJECT_REASONS)
    o = np.zeros(32, np.uint8)
    for c, (pt, _) in zip(cand, why):
        exp = None if pt is None else fr.encode(pt)
        assert exp in (None, c), c.hex()  # a valid encoding is the canonical one of its element
        assert oracle.ge_roundtrip(c) == exp, c.hex()
        buf = np.frombuffer(c, np.uint8).copy()
        for name in ("spgh_roundtrip", "spgh_hext_roundtrip"):
            ok = getattr(hc, name)(_p(buf), _p(o))
            assert (o.tobytes() if ok else None) == exp, (name, c.hex())
