"""Shared inputs of tests/test_polyeval_forms_oracle.py (CPU: the plans against the reference's rules) and
tests/test_gpu_polyeval_forms.py (the same cases with real data on the device): the shape lists of the disjoint-rounds
form and the num_vars lists of the univariate form of PolyEvalProof.

Rs = 32 is the host Bullet at the default crossover, Rs = 64 uses device Bullet rounds, Rs = 512 gives two column
blocks and split row ranges."""
import numpy as np

import fieldref as fr
import polyeval_cases as pc

ZERO = np.zeros(4, np.uint64)
ONE = fr.arr_u64([fr.to_mont(1)])[0]

CYCLE = [(4, 4), (2, 8), (8, 2), (1, 16), (2, 2)]

# name -> (rq_len, ry_len, [(num_proofs, num_inputs)], expected number of proofs)
DISJOINT_CASES = {
    # (1, 16) takes no rq entry and a zero-padded ry; (4, 4) trims both
    "abacba": (3, 3, [(8, 8), (4, 4), (8, 8), (1, 16), (4, 4), (8, 8)], 3),
    # four shapes of 16 entries each under different keys; (16, 1) has an empty ry part
    "same_nv": (4, 3, [(2, 8), (4, 4), (1, 16), (16, 1)], 4),
    # Rs = 64 twice and 32 once
    "bullet": (5, 6, [(32, 64), (32, 64), (16, 64)], 2),
    # past any fixed job count: five keys, exponents 1 .. 35
    "forty": (3, 4, [CYCLE[i % 5] for i in range(40)], 5),
    "wide": (8, 9, [(256, 512)], 1),
}
ABACBA_GROUPS, ABACBA_EXPS = [0, 1, 0, 2, 1, 0], [0, 0, 1, 0, 2, 3]

# name -> (num_vars list, r): r None = a random scalar
UNI_CASES = {
    "single_1": ([1], None),
    "single_4": ([4], None),
    # the widest polynomial is not first; Rs = 4, 4, 8, 64, 64, 4, 2; num_vars 3 and 4 share Rs 4 with different Ls
    "ragged": ([3, 4, 5, 11, 12, 4, 1], None),
    "ragged_r0": ([3, 4, 5, 11, 12, 4, 1], ZERO),  # L = R = (1, 0, ..): the fold starts at one
    "ragged_r1": ([3, 4, 5, 11, 12, 4, 1], ONE),   # all ones
    "host_bullet": ([10, 3, 9], None),
    "forty": ([[3, 4, 5, 6][i % 4] for i in range(40)], None),
    "wide": ([11, 17, 4], None),
}


def lg(x):
    return x.bit_length() - 1


def disjoint_inputs(name):
    """(shapes, rq, ry, polynomials): seeded by the case's position"""
    k = list(DISJOINT_CASES).index(name)
    rq_len, ry_len, shapes, _ = DISJOINT_CASES[name]
    rq, ry = pc.scalars(900 + k, rq_len), pc.scalars(920 + k, ry_len)
    Zs = [pc.scalars(1000 + 100 * k + i, p * q) for i, (p, q) in enumerate(shapes)]
    return shapes, rq, ry, Zs


def disjoint_point(shape, rq, ry):
    """the reference's point of a polynomial keyed (num_proofs, num_inputs) (dense_mlpoly.rs:905-921): the last
    lg num_proofs entries of rq, then ry padded with zeros at the front or trimmed to its last lg num_inputs entries"""
    nq, ny = lg(shape[0]), lg(shape[1])
    rq, ry = np.asarray(rq, np.uint64).reshape(-1, 4), np.asarray(ry, np.uint64).reshape(-1, 4)
    return np.concatenate([rq[len(rq) - nq:], pc.fit(ry, ny)])


def disjoint_evals(shapes, rq, ry, Zs):
    """the true evaluations Z_i(point_i), [n, 4]"""
    import pyoracle

    return np.array([pyoracle.dense_eval(Z, disjoint_point(s, rq, ry))[0] for s, Z in zip(shapes, Zs)], np.uint64)


def uni_inputs(name):
    """(num_vars list, r [4], polynomials)"""
    k = list(UNI_CASES).index(name)
    nvs, r = UNI_CASES[name]
    if r is None:
        r = pc.scalars(940 + k, 1)[0]
    return nvs, np.asarray(r, np.uint64), [pc.scalars(2000 + 100 * k + i, 1 << nv) for i, nv in enumerate(nvs)]


def gens_nv(max_nv):
    return 4 if max_nv <= 4 else (12 if max_nv <= 12 else max_nv)


def proof_bytes(Rs):
    return 2 * (8 + 32 * lg(Rs)) + 128
