"""R1CS satisfiability on Python integers (the reference's R1CSInstance::is_sat, src/r1csinstance.rs:322-357, over
every execution of every instance of a workload.R1CSWorkload): A z, B z, C z by a sparse product the way
sparse_cases.satisfiable computes A z, then (A z)[row] (B z)[row] == (C z)[row] row by row. The expected
spg_sat_report of spg_r1cs_sat_check / spg_pqx_sat_check.

Column c of a matrix reads section c // max_num_inputs, entry c % max_num_inputs of the execution's witness; a
column past the sections or past the instance's width contributes nothing (include/spg.h, multiply_vec_block)."""
import collections

import workload
from sparse_cases import _ints

Q = workload.Q
Report = collections.namedtuple("Report", "rows violations p q row az bz cz")


def _products(wl, p, mats, z):
    """[(Az, Bz, Cz)] per execution of instance p: three lists of num_cons[p] integers each"""
    X, Y, M = wl.num_cons[p], wl.num_inputs[p], wl.max_num_inputs
    out = []
    for q in range(wl.num_proofs[p]):
        abc = []
        for rows, cols, vals in mats:
            acc = [0] * X
            for r, c, v in zip(rows, cols, vals):
                w, i = c // M, c % M
                if w < wl.nws and i < Y:
                    acc[r] += v * z[w][q if len(z[w]) > 1 else 0][i]
            abc.append([a % Q for a in acc])
        out.append(abc)
    return out


def report(wl):
    """the spg_sat_report of the workload: rows, violations and the lowest violating (p, q, row) with its three values
    (None when every row holds)"""
    rows = violations = 0
    first = None
    mats_of = {}
    for p in range(wl.P):
        pi = 0 if wl.shared else p
        if pi not in mats_of:
            mats_of[pi] = [([int(r) for r in m[:, 0]], [int(c) for c in m[:, 1]], _ints(m[:, 2:])) for m in wl.entries[pi]]
        Y = wl.num_inputs[p]
        z = []
        for w in range(wl.nws):
            sec = wl.sections[w][p]
            flat = _ints(sec)
            z.append([flat[q * Y:(q + 1) * Y] for q in range(sec.shape[0])])
        for q, (az, bz, cz) in enumerate(_products(wl, p, mats_of[pi], z)):
            for r in range(wl.num_cons[p]):
                rows += 1
                if az[r] * bz[r] % Q != cz[r]:
                    violations += 1
                    if first is None:
                        first = (p, q, r, az[r], bz[r], cz[r])
    if first is None:
        return Report(rows, 0, None, None, None, None, None, None)
    return Report(rows, violations, *first)


def tamper(wl, p, q, col, value=12345, section=0):
    """one witness scalar of (instance p, execution q) replaced, in place; returns wl"""
    wl.sections[section][p][q, col] = workload.to_mont_limbs([value])[0]
    return wl
