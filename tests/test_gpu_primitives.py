"""The device forms of the field, curve, quad, recode and block-sum primitives, each behind a trivial kernel of
lib/libspg_devcheck.so (tests/devcheck/devcheck.hip: the product's headers, unchanged), on the operands where carry
chains go wrong: loose Fp values >= p and next to 2^256, sums that wrap twice, q - 1, the Montgomery constants,
digits on the recode's d > NB boundary in every window, non-canonical and torsion-shifted point representatives.
Inside whole MSMs and proofs these reach the device with probability ~2^-32 per operation. The reference is
tests/fieldref.py (Python integers, pinned on the CPU by tests/test_fieldref.py); every assertion is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fieldref as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spartan-parallel_amd")
# (C, G) of bullet_round_comb / comb_msm_parts in csrc/msm.hip (window width, window groups: SPG_BCOMB_G) and the workgroup sizes
# quad_block_sum / row_block_sum are launched with (k_layer_round_q, k_layer_pair, k_layer_triple in csrc/layers.hip,
# quad_grid_post<256>, k_phase1_pair<256>, k_phase2_pair<256> in csrc/sumcheck.hip): extend with the launch tables
RECODE_SHAPES = [(13, 4), (13, 10), (12, 4), (12, 8), (12, 11)]
BLOCK_SIZES = [64, 256]


def _load(name, env):
    path = os.environ.get(env)
    if path:
        return ctypes.CDLL(path)
    path = os.path.join(PKG, "lib", name)
    if not os.path.exists(path):
        try:
            subprocess.check_output(["make", "-s", "-C", PKG, "lib/" + name], stderr=subprocess.STDOUT)
        except (OSError, subprocess.CalledProcessError) as e:
            pytest.fail("%s is missing and `make lib/%s` failed: %s\n%s" % (
                path, name, e, getattr(e, "output", b"").decode(errors="replace")[-2000:]))
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def dc():
    return _load("libspg_devcheck.so", "SPG_DEVCHECK_LIB")


@pytest.fixture(scope="module")
def hc():
    return _load("libspg_hostcheck.so", "SPG_HOSTCHECK_LIB")


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _sz(n):
    return ctypes.c_size_t(n)


def dev(rc):
    assert rc == 0, "HIP error %d from libspg_devcheck" % rc


@pytest.fixture(scope="module")
def fq_pairs():
    a, b = fr.edge_pairs(fr.fq_edges(), np.random.default_rng(201), 3000, fr.Q)
    return a, b, fr.arr_u64(a), fr.arr_u64(b)


@pytest.fixture(scope="module")
def fp_pairs():
    a, b = fr.edge_pairs(fr.fp_edges(), np.random.default_rng(202), 3000, 2**256)
    return a, b, fr.arr_u32(a), fr.arr_u32(b)


# ---------------------------------------------------------------- Fq
@pytest.mark.parametrize("code", range(10))
def test_fq_ops(dc, hc, fq_pairs, code):
    """add, sub, mul (fq_mul_ps through mac / mac_flush), neg, sqr, inv (the Fermat chain, run nowhere on the host),
    from_mont, to_mont, mul_ps, mul32 on every ordered pair of the edge list and 3000 random pairs: bit-identical to
    the integers and to the host build, canonical"""
    a, b, A, B = fq_pairs
    n = len(a)
    out, host = np.zeros_like(A), np.zeros_like(A)
    dev(dc.spgd_fq_op(code, _p(A), _p(B), _p(out), _sz(n)))
    hc.spgh_fq_op(code, _p(A), _p(B), _p(host), _sz(n))
    got = fr.ints(out)
    bad = [(i, hex(a[i]), hex(b[i]), hex(got[i])) for i in range(n) if got[i] != fr.fq_op(code, a[i], b[i])]
    assert not bad, bad[:3]
    assert all(v < fr.Q for v in got)
    assert np.array_equal(out, host)
    if code == 5:
        prod = np.zeros_like(A)
        dev(dc.spgd_fq_op(2, _p(A), _p(out), _p(prod), _sz(n)))
        one = fr.to_mont(1)
        assert fr.ints(prod) == [one if v else 0 for v in a]
        assert all(g == 0 for g, v in zip(got, a) if v == 0) and a.count(0) > 0


# ---------------------------------------------------------------- Fp
@pytest.mark.parametrize("code", range(13))
def test_fp_ops(dc, hc, fp_pairs, code):
    """every Fp op on loose operands (all ordered pairs of the edge list, 3000 random pairs): the value mod p is the
    integers', and the limbs -- the representative of the raw ops 8 .. 11 included -- are the host build's"""
    a, b, A, B = fp_pairs
    n = len(a)
    out, host = np.zeros_like(A), np.zeros_like(A)
    dev(dc.spgd_fp_op(code, _p(A), _p(B), _p(out), _sz(n)))
    hc.spgh_fp_op(code, _p(A), _p(B), _p(host), _sz(n))
    got = fr.ints(out)
    raw = code in (8, 9, 10, 11)
    bad = [(i, hex(a[i]), hex(b[i]), hex(got[i])) for i in range(n)
           if (got[i] % fr.P if raw else got[i]) != fr.fp_op(code, a[i], b[i])]
    assert not bad, bad[:3]
    assert np.array_equal(out, host)
    if code in (8, 9):  # fp_addsub's representative is fp_add's / fp_sub's, limb for limb
        other = np.zeros_like(A)
        dev(dc.spgd_fp_op(code + 2, _p(A), _p(B), _p(other), _sz(n)))
        assert np.array_equal(out, other)


# ---------------------------------------------------------------- curve and quads
class Points:
    """pairs (P_i, Q_i) of affine points with the representative each is handed over in, and cached encodings"""

    def __init__(self):
        rng = np.random.default_rng(203)
        base = [fr.from_uniform_bytes(rng.bytes(64)) for _ in range(61)]
        pairs = []
        for i in range(60):
            p, q = base[i], base[i + 1]
            pairs += [(p, q), (fr.IDENTITY, q), (p, fr.IDENTITY), (p, fr.pt_neg(p)), (p, p)]
            pairs += [(fr.pt_add(p, fr.TORSION[j]), fr.pt_add(q, fr.TORSION[(i + j) % 4])) for j in range(1, 4)]
            pairs += [(fr.TORSION[1 + i % 3], q), (p, fr.TORSION[1 + i % 3])]
        pairs += [(fr.IDENTITY, fr.IDENTITY), (fr.TORSION[1], fr.TORSION[2]), (fr.TORSION[3], fr.TORSION[3])]
        while len(pairs) % 16 == 0 or len(pairs) % 64 < 5:
            pairs.pop()
        self.pairs = pairs
        self.n = len(pairs)
        # representatives by position: affine, affine with every coordinate + p, a random projective factor, and the
        # factor with X and T (or Y and Z) + p
        lifts = [(), ("X", "Y", "Z", "T"), (), ("X", "T"), (), ("Y", "Z")]
        ra, rb = [], []
        for i, (p, q) in enumerate(pairs):
            k = i % 6
            za = 1 if k < 2 else 2 + int.from_bytes(rng.bytes(32), "little") % (fr.P - 2)
            zb = 1 if k < 2 else 2 + int.from_bytes(rng.bytes(32), "little") % (fr.P - 2)
            ra.append(fr.ext_raw(p, za, lifts[k]))
            rb.append(fr.ext_raw(q, zb, lifts[(k + 1) % 6] if k >= 2 else lifts[k]))
        self.A = np.array(ra, dtype=np.uint32)
        self.B = np.array(rb, dtype=np.uint32)
        self._enc = {}
        self.want = {
            0: [self.enc(fr.pt_add(p, q)) for p, q in pairs],
            1: [self.enc(fr.pt_add(p, p)) for p, _ in pairs],
            3: [self.enc(fr.pt_add(p, fr.pt_neg(q))) for p, q in pairs],
            5: [self.enc(p) for p, _ in pairs],
        }
        self.want[2] = self.want[0]
        self.want[4] = self.want[5]

    def enc(self, pt):
        if pt not in self._enc:
            self._enc[pt] = fr.encode(pt)
        return self._enc[pt]


@pytest.fixture(scope="module")
def points():
    return Points()


def _rows(buf, n):
    return [buf[32 * i:32 * i + 32].tobytes() for i in range(n)]


@pytest.mark.parametrize("op", range(6))
def test_curve_ops_raw(dc, points, op):
    """ext_add, ext_dbl, ext_madd + / - (through ext_to_niels), the Niels round trip and ext_compress, one thread per
    point, on raw extended representatives: hash-to-group points, the identity, P + (-P), P + P through the addition
    formula, torsion-shifted points and the torsion points, coordinates + p, random projective factors"""
    n = points.n
    out, ok = np.zeros(32 * n, np.uint8), np.zeros(n, np.int32)
    dev(dc.spgd_point_op(op, _p(points.A), _p(points.B), _p(out), _p(ok), _sz(n), 1))
    assert ok.all()
    got = _rows(out, n)
    bad = [i for i in range(n) if got[i] != points.want[op][i]]
    assert not bad, (op, bad[:5])


def test_curve_ops_encoded(dc, hc, oracle, points):
    """the same ops from 32-byte encodings (ext_decompress first) and the one-way map, against the reference and the
    host build"""
    rng = np.random.default_rng(204)
    n = 200
    uni = rng.integers(0, 256, 64 * n, dtype=np.uint8)
    uni[:64] = 0
    uni[64:128] = 0xFF
    enc, ok = np.zeros(32 * n, np.uint8), np.zeros(n, np.int32)
    dev(dc.spgd_point_op(6, _p(uni), None, _p(enc), _p(ok), _sz(n), 0))
    pts = [fr.from_uniform_bytes(uni[64 * i:64 * i + 64].tobytes()) for i in range(n)]
    assert _rows(enc, n) == [points.enc(p) for p in pts]
    host = np.zeros(32 * n, np.uint8)
    hc.spgh_from_uniform(_p(uni), _p(host), _sz(n))
    assert np.array_equal(enc, host)
    assert _rows(enc, 16) == oracle.ge_from_uniform_bytes(uni[:64 * 16].tobytes())
    enc_b = np.roll(enc.reshape(n, 32), 1, axis=0).copy()
    qs = pts[-1:] + pts[:-1]
    want = {0: [fr.pt_add(p, q) for p, q in zip(pts, qs)], 1: [fr.pt_add(p, p) for p in pts],
            3: [fr.pt_add(p, fr.pt_neg(q)) for p, q in zip(pts, qs)], 4: pts, 5: pts}
    want[2] = want[0]
    for op in range(6):
        out = np.zeros(32 * n, np.uint8)
        dev(dc.spgd_point_op(op, _p(enc), _p(enc_b), _p(out), _p(ok), _sz(n), 0))
        assert ok.all() and _rows(out, n) == [points.enc(p) for p in want[op]], op
    o = np.zeros(32, np.uint8)
    for i in range(8):
        for op in range(4):
            assert hc.spgh_point_op(op, _p(enc[32 * i:]), _p(enc_b[i]), _p(o)) == 1
            assert o.tobytes() == points.enc(want[op][i])


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("op", range(6))
def test_quad_ops(dc, points, op, bs):
    """quad_add, quad_dbl, quad_madd + / - (niels_coord), quad_add_op with the operand handed over in LDS by another
    quad (quad_put_op / quad_get_op), quad_put: a different point in every quad over several waves and workgroups, the
    last wave with whole quads switched off, and every one of the four lanes must hold ext_add's / ext_dbl's /
    ext_madd's element"""
    n, S = points.n, bs // 4
    assert n % 16 != 0 and n > 2 * S
    out = np.zeros(128 * n, np.uint8)
    dev(dc.spgd_quad_op(op, _p(points.A), _p(points.B), _p(out), _sz(n), bs))
    if op == 4:  # quad p adds the second operand of its workgroup's mirrored quad (the identity past the end)
        want = []
        for p in range(n):
            m = (p // S) * S + S - 1 - p % S
            want.append(points.enc(fr.pt_add(points.pairs[p][0], points.pairs[m][1] if m < n else fr.IDENTITY)))
    else:
        want = points.want[op]
    got = _rows(out, 4 * n)
    bad = [(p, q) for p in range(n) for q in range(4) if got[4 * p + q] != want[p]]
    assert not bad, (op, bs, bad[:8])


# ---------------------------------------------------------------- recode
@pytest.mark.parametrize("C,G", RECODE_SHAPES)
def test_recode(dc, C, G):
    """comb_window_entries<C, ceil(W / G)>: 0, 1, q - 1, 2^252, 2^252 - 1, a single digit in each window, every
    window at NB, NB + 1, NB - 1, 2^C - 1 and NB + 1 / NB - 1 alternating, and random scalars. The entries decode to
    digits with sum d_w 2^(C w) = k and |d_w| <= NB, all ones exactly for d_w = 0, and the index is
    (w NS + s) NB + |d_w| - 1 with the sign in bit 31"""
    W, NB = 253 // C + 1, 1 << (C - 1)
    WG = (W + G - 1) // G
    NS = 16385
    rng = np.random.default_rng(C * 100 + G)
    ks = fr.recode_patterns(C) + [int.from_bytes(rng.bytes(40), "little") % fr.Q for _ in range(1000)]
    n = len(ks)
    slot = rng.integers(0, NS, n, dtype=np.uint64).astype(np.uint32)
    slot[:3] = [0, NS - 1, 1]
    K = fr.arr_u32(ks)
    out = np.zeros((n, G * WG), np.uint32)
    dev(dc.spgd_recode(C, G, _p(K), _p(slot), NS, _p(out), _sz(n)))
    seen = set()
    for i, k in enumerate(ks):
        ent = [int(x) for x in out[i]]
        assert all(e == 0xFFFFFFFF for e in ent[W:]), (i, hex(k))
        digits = []
        for w in range(W):
            e = ent[w]
            if e == 0xFFFFFFFF:
                digits.append(0)
                continue
            mag = (e & 0x7FFFFFFF) - (w * NS + int(slot[i])) * NB + 1
            assert 1 <= mag <= NB, (i, hex(k), w, hex(e))
            digits.append(-mag if e >> 31 else mag)
        assert sum(d << (C * w) for w, d in enumerate(digits)) == k, (i, hex(k), digits)
        assert digits == fr.recode(k, C), (i, hex(k))
        seen.update(digits)
    assert {0, 1, -1, NB, NB - 1, -(NB - 1)} <= seen


# ---------------------------------------------------------------- block sums and lane-argument helpers
@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("op,res", [(0, 3), (1, 16)])
def test_block_sums(dc, op, res, bs):
    """quad_block_sum (op 0: lanes with equal thread & 3, sums for 0 .. 2) and row_block_sum (op 1: thread & 15) over
    three workgroups: a distinct random value in every thread, then q - 1 everywhere"""
    nb = 3
    n = nb * bs
    rng = np.random.default_rng(300 + bs + op)
    rnd = [int.from_bytes(rng.bytes(40), "little") % fr.Q for _ in range(n)]
    assert len(set(rnd)) == n
    mod = 4 if op == 0 else 16
    for vals in (rnd, [fr.Q - 1] * n):
        A = fr.arr_u64(vals)
        out = np.zeros((nb * res, 4), np.uint64)
        dev(dc.spgd_block_sum(op, bs, _p(A), None, None, None, None, _p(out), _sz(n)))
        want = [sum(vals[b * bs + t] for t in range(bs) if t % mod == r) % fr.Q for b in range(nb) for r in range(res)]
        assert fr.ints(out) == want


def test_lane_helpers(dc):
    """line_at (p in 0 .. 2), fq_small (n in 0 .. 3) and cube_at (t, s in 0 .. 3) for every lane argument, on the
    edge list and random values"""
    rng = np.random.default_rng(310)
    e = fr.fq_edges()
    n = 16 * 40
    v = [[e[(i * (3 + 2 * j) + j) % len(e)] if i < n // 2 else int.from_bytes(rng.bytes(40), "little") % fr.Q
          for i in range(n)] for j in range(4)]
    arrs = [fr.arr_u64(x) for x in v]
    for op, nargs, f in [
        (2, 3, lambda a, b, c, d, g: (a, 2 * b - a, 3 * b - 2 * a)[g] % fr.Q),
        (3, 4, lambda a, b, c, d, g: g * a % fr.Q),
        (4, 16, lambda a, b, c, d, g: (a + (g & 3) * (b - a) + (g >> 2) * ((c - a) + (g & 3) * (d - c - b + a))) % fr.Q),
    ]:
        arg = np.array([(i + i // 16) % nargs for i in range(n)], dtype=np.int32)
        assert set(arg.tolist()) == set(range(nargs))
        out = np.zeros((n, 4), np.uint64)
        dev(dc.spgd_block_sum(op, 0, _p(arrs[0]), _p(arrs[1]), _p(arrs[2]), _p(arrs[3]), _p(arg), _p(out), _sz(n)))
        want = [f(v[0][i], v[1][i], v[2][i], v[3][i], int(arg[i])) for i in range(n)]
        assert fr.ints(out) == want, op


# ---------------------------------------------------------------- decoders
@pytest.fixture(scope="module")
def candidates():
    cand = fr.decode_candidates(np.random.default_rng(31))
    why = [fr.decode_why(c) for c in cand]
    return cand, why


def test_decode_candidates_cover_every_rejection(candidates):
    cand, why = candidates
    valid = sum(w[0] is not None for w in why)
    assert valid >= 50 and len(cand) - valid >= 300
    assert {w[1] for w in why if w[0] is None} == set(fr.REJECT_REASONS)


def test_device_decoder_accepts_the_reference_set(dc, candidates):
    """ext_decompress on the device accepts exactly the strings the big-int RFC 9496 decoder accepts and re-encodes
    them byte for byte"""
    cand, why = candidates
    n = len(cand)
    buf = np.frombuffer(b"".join(cand), np.uint8).copy()
    out, ok = np.zeros(32 * n, np.uint8), np.zeros(n, np.int32)
    dev(dc.spgd_point_op(5, _p(buf), None, _p(out), _p(ok), _sz(n), 0))
    got = _rows(out, n)
    bad = [(cand[i].hex(), why[i][1], int(ok[i])) for i in range(n) if bool(ok[i]) != (why[i][0] is not None)]
    assert not bad, bad[:5]
    assert all(got[i] == cand[i] for i in range(n) if ok[i])


def test_gens_upload_accepts_the_reference_set(ctx, candidates):
    """spg_gens_upload (k_decompress): all valid candidates upload, and their sum through the uploaded table is the
    reference's; one invalid candidate at any position of a batch fails the upload"""
    import spg

    cand, why = candidates
    valid = [(c, w[0]) for c, w in zip(cand, why) if w[0] is not None]
    comp = np.frombuffer(b"".join(c for c, _ in valid), np.uint8).reshape(-1, 32).copy()
    m = len(valid) - 1
    g = spg.Gens(ctx, m, compressed=comp)
    assert np.array_equal(g.compressed(), comp)
    acc = fr.IDENTITY
    for _, pt in valid[:m]:
        acc = fr.pt_add(acc, pt)
    ones = np.tile(np.array(fr.to_u64(fr.to_mont(1)), dtype=np.uint64), (m, 1))
    assert g.msm(ones) == fr.encode(acc)
    good = comp[:33].copy()
    pos = 0
    for c, w in zip(cand, why):
        if w[0] is not None:
            continue
        batch = good.copy()
        batch[pos] = np.frombuffer(c, np.uint8)
        with pytest.raises(spg.SpgError):
            spg.Gens(ctx, 32, compressed=batch)
        pos = (pos + 1) % 33
    assert np.array_equal(spg.Gens(ctx, 32, compressed=good).compressed(), good)
