"""Plain Python-integer reference for the arithmetic the kernels compute exactly: the scalar field Fq in
Montgomery form (R = 2^256), GF(2^255 - 19), the twisted Edwards curve on affine rationals, the RFC 9496
ristretto255 encode / decode / one-way map, and the signed-window recode of the comb and bucket MSMs.
Also the edge operand lists shared by tests/test_fieldref.py (CPU: pins this module against the oracle and
the libsodium vectors, then libspg_hostcheck against it) and tests/test_gpu_primitives.py (the device forms).
Nothing here imports the product."""
import numpy as np

Q = 2**252 + 27742317777372353535851937790883648493
P = 2**255 - 19
R = 2**256
RINV = pow(R, -1, Q)
M256 = 2**256 - 1

# ---------------------------------------------------------------- limbs
def to_u32(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def to_u64(x):
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def arr_u32(vals):
    return np.array([to_u32(v) for v in vals], dtype=np.uint32).reshape(-1, 8)


def arr_u64(vals):
    return np.array([to_u64(v) for v in vals], dtype=np.uint64).reshape(-1, 4)


def ints(a):
    """rows of little-endian limbs (any unsigned dtype) -> Python integers"""
    a = np.ascontiguousarray(a)
    a = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(1, -1)
    return [int.from_bytes(row.tobytes(), "little") for row in a]


# ---------------------------------------------------------------- Fq (operands and results in Montgomery form)
def to_mont(x):
    return x * R % Q


def from_mont(m):
    return m * RINV % Q


# op codes of spgh_fq_op / spgd_fq_op
FQ_OPS = {"add": 0, "sub": 1, "mul": 2, "neg": 3, "square": 4, "invert": 5, "from_mont": 6, "to_mont": 7,
          "mul_ps": 8, "mul32": 9}


def fq_op(code, a, b=0):
    """the Montgomery-form result of op `code` on Montgomery-form a, b in [0, q)"""
    if code == 0:
        return (a + b) % Q
    if code == 1:
        return (a - b) % Q
    if code in (2, 8, 9):
        return a * b * RINV % Q
    if code == 3:
        return -a % Q
    if code == 4:
        return a * a * RINV % Q
    if code == 5:  # (a / R)^-1 R, and 0 -> 0
        return pow(a, Q - 2, Q) * R * R % Q
    if code == 6:
        return a * RINV % Q
    if code == 7:
        return a * R % Q
    raise ValueError(code)


def fq_edges():
    """canonical values in [0, q): the ends of the range, the carries of every limb boundary, the Montgomery
    constants, and values next to 2^252 (q's top limb)"""
    e = [0, 1, 2, Q - 1, Q - 2, (Q + 1) // 2, (Q - 1) // 2, 2**252, 2**252 + 1, 2**252 - 1, Q - 2**32, Q - 2**64,
         R % Q, R * R % Q, -R % Q, RINV, -RINV % Q]
    for k in range(1, 8):
        e += [2**(32 * k), 2**(32 * k) - 1]
    e.append((2**252 - 1) >> 128 << 128)
    assert all(0 <= v < Q for v in e) and len(set(e)) == len(e)
    return e


def edge_pairs(edges, rng, nrand, bound):
    """every ordered pair of edges, then nrand uniformly random pairs below bound"""
    a = [x for x in edges for _ in edges]
    b = [y for _ in edges for y in edges]
    nb = (bound.bit_length() + 7) // 8 + 8
    for _ in range(nrand):
        a.append(int.from_bytes(rng.bytes(nb), "little") % bound)
        b.append(int.from_bytes(rng.bytes(nb), "little") % bound)
    return a, b


# ---------------------------------------------------------------- Fp (loose operands in [0, 2^256))
def fp_op(code, a, b=0):
    """the value mod p of op `code` (spgh_fp_op / spgd_fp_op) on loose a, b"""
    if code in (0, 8, 10):
        return (a + b) % P
    if code in (1, 9, 11):
        return (a - b) % P
    if code in (2, 6):
        return a * b % P
    if code in (3, 7):
        return a * a % P
    if code == 4:
        return pow(a % P, P - 2, P)
    if code == 5:
        return a % P
    if code == 12:
        return a * (b & 0x3FFFF) % P
    raise ValueError(code)


def fp_edges():
    """loose values in [0, 2^256): around 0, 19, 38, 76 (the wrap constants), p, 2p, 2^256, and limb patterns"""
    e = [0, 1, 19, 37, 38, 39, 75, 76, P - 1, P, P + 1, 2 * P, 2 * P + 37,
         2**256 - 1, 2**256 - 38, 2**256 - 39, 2**256 - 75, 2**256 - 76, 2**255, 2**128 + 1, 2**128 - 1,
         2**256 - 2**128, M256,
         2**256 - 2, 2**256 - 19, 2**256 - 37]  # more pairs whose sum wraps twice (a + b >= 2^257 - 38)
    out = []
    for v in e:
        if v not in out:
            out.append(v)
    assert all(0 <= v < 2**256 for v in out)
    return out


# ---------------------------------------------------------------- curve: -x^2 + y^2 = 1 + d x^2 y^2 over Fp
D = -121665 * pow(121666, -1, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
assert SQRT_M1 * SQRT_M1 % P == P - 1


def is_neg(x):
    return (x % P) & 1


def fabs(x):
    x %= P
    return P - x if x & 1 else x


def sqrt_ratio_m1(u, v):
    """RFC 9496 4.2: (was_square, non-negative root of u/v, or of sqrt(-1) u/v)"""
    u %= P
    v %= P
    r = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    check = v * r * r % P
    correct = check == u
    flipped = check == -u % P
    flipped_i = check == -u * SQRT_M1 % P
    if flipped or flipped_i:
        r = r * SQRT_M1 % P
    return correct or flipped, fabs(r)


# 1 / sqrt(a - d) and sqrt(a d - 1) for a = -1, with the signs RFC 9496 4.1 fixes (the libsodium vectors in
# tests/golden/ristretto_sodium.json and the oracle's constants pin them, tests/test_fieldref.py)
INVSQRT_A_MINUS_D = 54469307008909316920995813868745141605393597292927456921205312896311721017578
SQRT_AD_MINUS_ONE = 25063068953384623474111414158702152701244531502492656460079210482610430750235
ONE_MINUS_D_SQ = (1 - D * D) % P
D_MINUS_ONE_SQ = (D - 1) * (D - 1) % P
assert INVSQRT_A_MINUS_D**2 * (-1 - D) % P == 1 and SQRT_AD_MINUS_ONE**2 % P == (-D - 1) % P

IDENTITY = (0, 1)
# the 4-torsion subgroup: a ristretto255 element is a coset of it
TORSION = [(0, 1), (0, P - 1), (SQRT_M1, 0), (P - SQRT_M1, 0)]


def on_curve(pt):
    x, y = pt
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def pt_add(p1, p2):
    """affine twisted Edwards addition, a = -1 (complete on this curve)"""
    x1, y1 = p1
    x2, y2 = p2
    k = D * x1 * x2 * y1 * y2 % P
    x3 = (x1 * y2 + x2 * y1) * pow(1 + k, P - 2, P) % P
    y3 = (y1 * y2 + x1 * x2) * pow(1 - k, P - 2, P) % P
    return x3, y3


def pt_neg(p1):
    return (-p1[0] % P, p1[1])


def pt_mul(k, p1):
    acc = IDENTITY
    for bit in bin(k)[2:] if k else "":
        acc = pt_add(acc, acc)
        if bit == "1":
            acc = pt_add(acc, p1)
    return acc


def encode_ext(X, Y, Z, T):
    """RFC 9496 4.3.2 on extended coordinates"""
    u1 = (Z + Y) * (Z - Y) % P
    u2 = X * Y % P
    _, invsqrt = sqrt_ratio_m1(1, u1 * u2 * u2)
    den1 = invsqrt * u1 % P
    den2 = invsqrt * u2 % P
    z_inv = den1 * den2 * T % P
    if is_neg(T * z_inv):
        x, y, den_inv = Y * SQRT_M1 % P, X * SQRT_M1 % P, den1 * INVSQRT_A_MINUS_D % P
    else:
        x, y, den_inv = X, Y, den2
    if is_neg(x * z_inv):
        y = -y % P
    return fabs(den_inv * (Z - y)).to_bytes(32, "little")


def encode(pt):
    x, y = pt
    return encode_ext(x % P, y % P, 1, x * y % P)


REJECT_REASONS = ("non-canonical", "odd", "non-square", "negative t", "y = 0")


def decode_why(b):
    """RFC 9496 4.3.1: ((x, y), None) for a valid encoding, else (None, reason)"""
    s = int.from_bytes(bytes(b), "little")
    if s >= P:
        return None, "non-canonical"
    if s & 1:
        return None, "odd"
    ss = s * s % P
    u1 = (1 - ss) % P
    u2 = (1 + ss) % P
    u2s = u2 * u2 % P
    v = (-D * u1 * u1 - u2s) % P
    was_square, invsqrt = sqrt_ratio_m1(1, v * u2s)
    den_x = invsqrt * u2 % P
    den_y = invsqrt * den_x * v % P
    x = fabs(2 * s * den_x)
    y = u1 * den_y % P
    if not was_square:
        return None, "non-square"
    if is_neg(x * y):
        return None, "negative t"
    if y == 0:
        return None, "y = 0"
    return (x, y), None


def decode(b):
    return decode_why(b)[0]


def ristretto_map(t):
    """RFC 9496 4.3.4 MAP, as an affine point"""
    r = SQRT_M1 * t * t % P
    u = (r + 1) * ONE_MINUS_D_SQ % P
    v = (-1 - r * D) * (r + D) % P
    was_square, s = sqrt_ratio_m1(u, v)
    c = P - 1
    if not was_square:
        s = -fabs(s * t) % P
        c = r
    N = (c * (r - 1) * D_MINUS_ONE_SQ - v) % P
    w0 = 2 * s * v % P
    w1 = N * SQRT_AD_MINUS_ONE % P
    w2 = (1 - s * s) % P
    w3 = (1 + s * s) % P
    zi = pow(w1 * w3, P - 2, P)
    return w0 * w3 * zi % P, w2 * w1 * zi % P


def from_uniform_bytes(b64):
    b64 = bytes(b64)
    t0 = (int.from_bytes(b64[:32], "little") & (2**255 - 1)) % P
    t1 = (int.from_bytes(b64[32:], "little") & (2**255 - 1)) % P
    return pt_add(ristretto_map(t0), ristretto_map(t1))


def ext_raw(pt, z=1, lift=()):
    """an extended representative (X, Y, Z, T) of the affine point scaled by z, as 32 u32 words in the Ext layout;
    the coordinates named in `lift` ('X', 'Y', 'Z', 'T') get + p where that stays below 2^256"""
    x, y = pt
    c = {"X": x * z % P, "Y": y * z % P, "Z": z % P, "T": x * y * z % P}
    for name in lift:
        if c[name] + P < 2**256:
            c[name] += P
    return to_u32(c["X"]) + to_u32(c["Y"]) + to_u32(c["Z"]) + to_u32(c["T"])


def decode_candidates(rng):
    """32-byte strings around every edge of DECODE: small s, s next to p (both sides), next to 2^255 and 2^256,
    random even canonical s and random strings"""
    c = list(range(40)) + [P - 1 - i for i in range(40)] + [P + i for i in range(19)]
    c += [2**255 + i for i in range(20)] + [2**256 - 1 - i for i in range(20)]
    for _ in range(400):
        c.append((int.from_bytes(rng.bytes(40), "little") % P) & ~1)
    out = [v.to_bytes(32, "little") for v in c]
    out += [rng.bytes(32) for _ in range(50)]
    return out


# ---------------------------------------------------------------- signed-window recode
def recode(k, C):
    """the W = 253 // C + 1 signed C-bit digits of k < 2^253: sum d_w 2^(C w) = k, -2^(C-1) < d_w <= 2^(C-1);
    a window above 2^(C-1) borrows from the next (msm.hip, msm_big.hip, comb.hip, bullet.hpp)"""
    W, NB = 253 // C + 1, 1 << (C - 1)
    d, carry = [], 0
    for w in range(W):
        v = ((k >> (C * w)) & ((1 << C) - 1)) + carry
        carry = 1 if v > NB else 0
        d.append(v - (carry << C))
    assert carry == 0 and sum(x << (C * w) for w, x in enumerate(d)) == k
    return d


def recode_patterns(C):
    """canonical scalars whose windows sit on the recode's decisions: every window equal to NB, NB + 1, NB - 1 or
    2^C - 1, NB + 1 / NB - 1 alternating (each cut below 2^252 < q), and a single lowest / NB digit in each window"""
    W, NB = 253 // C + 1, 1 << (C - 1)
    cut = 2**252 - 1
    out = [0, 1, Q - 1, 2**252, 2**252 - 1]
    for v in (NB, NB + 1, NB - 1, (1 << C) - 1):
        out.append(sum(v << (C * w) for w in range(W)) & cut)
    out.append(sum((NB + 1 if w % 2 == 0 else NB - 1) << (C * w) for w in range(W)) & cut)
    out.append(sum((NB - 1 if w % 2 == 0 else NB + 1) << (C * w) for w in range(W)) & cut)
    for w in range(W):
        for v in (1, NB, NB + 1):
            if (v << (C * w)) < Q:
                out.append(v << (C * w))
    return out


def api_carry_scalars(cs=(8, 9, 10, 12, 13, 14)):
    """the all-window patterns of recode_patterns for the window widths the MSM paths use, as canonical integers"""
    out = []
    for C in cs:
        for v in recode_patterns(C)[5:11]:
            if v not in out:
                out.append(v)
    return out
