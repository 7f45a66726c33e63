"""Shared inputs of tests/test_polyeval_oracle.py (CPU: the plan against the checker) and tests/test_gpu_polyeval.py
(the same cases with real data on the device): random Montgomery scalars, point lists with a chosen pattern of equal
left halves, and the instance lists of the batched-instances form."""
import numpy as np

import pyoracle


def scalars(seed, n):
    """n Montgomery scalars [n, 4], uniform (from_bytes_wide of seeded bytes)"""
    rng = np.random.default_rng(seed)
    return pyoracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * max(n, 1), dtype=np.uint8).tobytes())[:n]


def fit(r, nv):
    """the reference's fitted point: zeros at the front, or the last nv entries"""
    r = np.asarray(r, dtype=np.uint64).reshape(-1, 4)
    if nv >= len(r):
        return np.concatenate([np.zeros((nv - len(r), 4), np.uint64), r])
    return r[len(r) - nv:]


def evaluate(Z, r, nv):
    """Z(fit(r, nv)) as a Montgomery scalar"""
    return pyoracle.dense_eval(Z, fit(r, nv))[0]


def points(seed, nv, pattern):
    """one point per letter of `pattern`: equal letters share the left half (the first nv // 2 scalars), every point
    has a right half of its own. Returns [K, nv, 4]."""
    ln = nv // 2
    left = {}
    out = []
    for i, ch in enumerate(pattern):
        if ch not in left:
            left[ch] = scalars(seed * 1000 + ord(ch), ln)
        out.append(np.concatenate([left[ch].reshape(-1, 4), scalars(seed * 1000 + 500 + i, nv - ln)]))
    return np.array(out, dtype=np.uint64).reshape(len(pattern), nv, 4)


# left halves a, b, a, c, b, a: the repeats' exponents must count 1, 2, 3 in encounter order across groups
ABACBA = "abacba"
ABACBA_GROUPS, ABACBA_EXPS = [0, 1, 0, 2, 1, 0], [0, 0, 1, 0, 2, 3]


def instance_cases():
    """name -> (num_vars_list, r_list): the instance lists of prove_batched_instances"""
    long_r = scalars(11, 12)
    cases = {}
    # every size twice with one long point: four groups, then each repeats (exponents 1 .. 4 across the groups)
    cases["mixed"] = ([3, 4, 11, 12, 3, 4, 11, 12], [long_r] * 8)
    # num_vars 4 with points shorter (padded at the front) and longer (trimmed at the front); the last two scalars
    # are shared, so R is equal and the three L vectors differ: one group
    tail = scalars(12, 2)
    cases["padtrim"] = ([4, 4, 4], [tail, np.concatenate([scalars(13, 2), tail]), np.concatenate([scalars(14, 5), tail])])
    # two polynomials with equal (num_vars, R) and different L, then one with another R
    right = scalars(15, 6)
    cases["same_R"] = ([11, 11, 11], [np.concatenate([scalars(16, 5), right]), np.concatenate([scalars(17, 5), right]),
                                     scalars(18, 11)])
    # 40 polynomials in one call (past the 32-job cap of the R1CS witness opening), five distinct right halves
    rights = [scalars(20 + k, 2) for k in range(5)]
    cases["forty"] = ([4] * 40, [np.concatenate([scalars(40 + i, 2), rights[i % 5]]) for i in range(40)])
    return cases


def instance_polys(seed, nv_list):
    return [scalars(seed + i, 1 << nv) for i, nv in enumerate(nv_list)]
