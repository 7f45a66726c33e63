"""Shared inputs of the variable-base MSM tests (tests/test_gpu_msm_var.py on the device, tests/test_msm_var_host.py
through the host emulation): points from gens_stream(b"vmsm_test", 4096), the size list, the edge scalars of
test_gpu_msm.py's test_msm_edge_scalars, and edge points. The reference is always the oracle's orc_msm
(pyoracle.msm), computed once per case and kept (ref)."""
import numpy as np

import fieldref

SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4096]
CHILD_SIZES = [1, 5, 65, 1000]
Q = fieldref.Q

_PTS = None
_REF = {}


def points(oracle):
    global _PTS
    if _PTS is None:
        _PTS = oracle.gens_stream(b"vmsm_test", 4096)
    return _PTS


def rand_fq(oracle, rng, n):
    return oracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * n, dtype=np.uint8).tobytes())


def carry_scalars():
    """Montgomery scalars whose every c-bit window sits on the signed recode's d > NB decision"""
    return fieldref.arr_u64([fieldref.to_mont(v) for v in fieldref.api_carry_scalars()])


def neg_point(oracle, P):
    return oracle.ge_scalarmul(bytes(P), (Q - 1).to_bytes(32, "little"))


def size_case(oracle, n):
    return points(oracle)[:n], rand_fq(oracle, np.random.default_rng(n), n)


def edge_scalar_cases(oracle):
    """name -> (points, scalars) at n = 256"""
    n = 256
    pts = points(oracle)[:n]
    one = oracle.fq_from_u64(1)
    zero = np.zeros(4, np.uint64)
    neg1 = oracle.fq_op("neg", one)[0]
    cases = {
        "zeros": np.tile(zero, (n, 1)),
        "ones": np.tile(one, (n, 1)),
        "neg_ones": np.tile(neg1, (n, 1)),
        "same_random": np.tile(rand_fq(oracle, np.random.default_rng(1), 1)[0], (n, 1)),
        "pow2_252": np.tile(oracle.fq_from_raw([0, 0, 0, 1 << 60]), (n, 1)),
    }
    cs = carry_scalars()
    cases["carry_patterns"] = np.concatenate([cs] * (n // len(cs) + 1))[:n]
    for i in range(0, len(cs), 6):  # six patterns at a time, alone among zeros
        lone = np.zeros((n, 4), np.uint64)
        lone[7:13] = cs[i:i + 6]
        cases["carry_patterns_%d" % i] = lone
    return {k: (pts, v) for k, v in cases.items()}


def edge_point_cases(oracle):
    """name -> (points, scalars) at n <= 64: the identity encoding among others; one point 64 times with equal
    scalars (every addition in its bucket, the tree and the group reduce doubles); P next to -P with equal scalars
    (the identity); and all three in one bucket"""
    P = points(oracle)
    rng = np.random.default_rng(77)
    same = np.tile(rand_fq(oracle, rng, 1)[0], (64, 1))
    ident = P[:64].copy()
    ident[5] = 0
    ident[63] = 0
    rep = np.tile(P[7], (64, 1))
    pm = P[:64].copy()
    for i in range(32):
        pm[2 * i] = P[i]
        pm[2 * i + 1] = np.frombuffer(neg_point(oracle, P[i]), dtype=np.uint8)
    mixed = np.zeros((64, 32), np.uint8)
    negP = np.frombuffer(neg_point(oracle, P[9]), dtype=np.uint8)
    for i in range(64):
        mixed[i] = (P[9], P[9], negP, np.zeros(32, np.uint8), P[9])[i % 5]
    return {
        "identity_among": (ident, rand_fq(oracle, rng, 64)),
        "repeated_point": (rep, same),
        "p_and_minus_p": (pm, same),
        "one_bucket_mixed": (mixed, same),
    }


def ref(oracle, name, pts, s):
    """the oracle's MSM of a case, computed once per process"""
    if name not in _REF:
        _REF[name] = oracle.msm(pts, s) if len(pts) else bytes(32)
    return _REF[name]


def child_cases(oracle):
    """the cases one child process per forced window runs through the kernels (SPG_VMSM_HOST_MAX=0)"""
    out = {"n%d" % n: size_case(oracle, n) for n in CHILD_SIZES}
    out["same_random"] = edge_scalar_cases(oracle)["same_random"]
    out["p_and_minus_p"] = edge_point_cases(oracle)["p_and_minus_p"]
    # 4096 entries in one bucket of every window: the bucket splits into several chunks
    out["same_random_4096"] = (points(oracle), np.tile(rand_fq(oracle, np.random.default_rng(3), 1)[0], (4096, 1)))
    return out


def child_main():
    """prints `name hex` per child case (run in a fresh process that reads the SPG_VMSM_* knobs)"""
    import pyoracle
    import spg

    ctx = spg.Context(0)
    for name, (pts, s) in child_cases(pyoracle).items():
        P = spg.Points(ctx, pts)
        print(name, P.msm(s).hex())
        P.free()
    print("ok")
