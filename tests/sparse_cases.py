"""Structured sparse matrices for the stand-alone entries (spg_r1cs_prove, spg_r1cs_multi_evaluate, spg_spark_*,
multiply_vec_block). workload.R1CSWorkload gives A, B and C exactly one entry per row, every value 1, no duplicate
(row, col) and nnz == num_cons (a power of two, never zero); workload.SparkWorkload permutes the columns, so every
column-side read timestamp is 0 and N == cells. Here the matrices of a R1CSWorkload (whose witness sections stay) are
replaced, from a seed, by matrices whose per-matrix nnz is ragged across A / B / C and across instances: 0, 1, 37,
more than num_cons, and more than 2^max(num_vars_x, num_vars_y) = the SPARK memory's cells, so there are more
operations than cells. Every matrix of 8 entries or more has
  * one row holding a third of its entries and one column holding another third (beyond 256 where nnz >= 770: read
    timestamps and one CSR row outgrow a workgroup),
  * one exact duplicate (row, col),
  * values cycling through 0, 1, q-1 and random scalars,
  * its entries in shuffled order.
Columns stay inside each instance's witness width (section w < num_sections, index < num_inputs[p]).

A new per-matrix or per-instance field of the R1CS or SPARK prover needs a case here in which it differs between the
matrices of one instance and between instances."""
import numpy as np

import workload

Q = workload.Q

# (num_cons, num_proofs, witness sections, shared instance, nnz of [A_0, B_0, C_0, A_1, ...])
CASES = {
    # N = 1024 operations over 512 cells; an empty matrix, a single entry, 37
    "ragged_p2_x64": ([64, 32], [4, 2], 3, False, [800, 37, 0, 1, 300, 64]),
    # 256-row instances: the tiled SpMV (k_spmv<true>) meets multi-entry rows; N = 1024 over 512 cells
    "tiled_p2_x256": ([256, 256], [4, 4], 1, False, [900, 513, 300, 0, 1, 777]),
    # one shared matrix triple under three witnesses; N = 128 over 64 cells
    "shared_p3_x32": ([32, 32, 32], [4, 2, 1], 1, True, [100, 37, 5]),
    # fewer operations than cells (N = 128, 512 cells), as every R1CSWorkload case has
    "below_cells_x256": ([256], [2], 1, False, [37, 100, 0]),
}
SATISFIABLE = ([64, 16], [4, 2], 2, False)


def _vals(rng, n):
    v = [(0, 1, Q - 1)[i % 4] if i % 4 < 3 else int.from_bytes(rng.bytes(40), "little") % Q for i in range(n)]
    return workload.to_mont_limbs(v) if n else np.zeros((0, 4), np.uint64)


def _matrix(rng, nnz, num_rows, cols):
    """(nnz, 6) uint64 entries over rows < num_rows and the allowed columns `cols`"""
    cols = np.asarray(cols, dtype=np.uint64)
    row = rng.integers(0, num_rows, nnz).astype(np.uint64)
    col = cols[rng.integers(0, len(cols), nnz)]
    if nnz >= 8:
        third = nnz // 3
        pick = lambda pool, n: rng.permutation(pool)[:n] if n <= len(pool) else rng.choice(pool, n)
        row[:third] = rng.integers(0, num_rows)  # the hot row, over distinct columns while they last
        col[:third] = pick(cols, third)
        col[third:2 * third] = cols[rng.integers(0, len(cols))]  # the hot column
        row[third:2 * third] = pick(np.arange(num_rows, dtype=np.uint64), third)
        row[nnz - 1], col[nnz - 1] = row[nnz - 2], col[nnz - 2]  # an exact duplicate
    arr = np.zeros((nnz, 6), dtype=np.uint64)
    arr[:, 0], arr[:, 1] = row, col
    arr[:, 2:] = _vals(rng, nnz)
    return arr[rng.permutation(nnz)]


def _columns(wl, p):
    return [w * wl.max_num_inputs + i for w in range(wl.nws) for i in range(wl.num_inputs[p])]


def structured(case, seed=7):
    """the case's R1CSWorkload with its matrices replaced (the witness sections are R1CSWorkload's)"""
    nc, npf, nws, shared, nnz = CASES[case]
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    rng = np.random.default_rng(seed)
    assert len(nnz) == 3 * len(wl.entries)
    wl.entries = [[_matrix(rng, nnz[3 * p + m], wl.num_cons[p], _columns(wl, p)) for m in range(3)]
                  for p in range(len(wl.entries))]
    return wl


def sorted_entries(wl):
    """the same matrices with every entry list sorted by (row, col) (stable: duplicates keep their order)"""
    import copy

    out = copy.copy(wl)
    out.entries = [[m[np.lexsort((m[:, 1], m[:, 0]))] for m in mats] for mats in wl.entries]
    return out


def _ints(limbs):
    Rinv = pow(workload.R, -1, Q)
    flat = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(r[i]) << (64 * i) for i in range(4)) * Rinv % Q for r in flat]


def satisfiable(seed=11):
    """A rows: linear combinations of 1 to 24 terms over random witness columns of every section (duplicates and the
    values 0, 1, q-1 among them); B = [(row, 0, 1)] (z[0] = 1); C: one entry of value 1 on a fresh column of section 0
    whose witness value is set to (A z)[row], computed on Python integers. So (A z) * (B z) = C z in every execution."""
    nc, npf, nws, shared = SATISFIABLE
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    rng = np.random.default_rng(seed)
    one = workload.to_mont_limbs([1])[0]
    entries = []
    for p in range(wl.P):
        X, Y = wl.num_cons[p], wl.num_inputs[p]
        assert Y >= 2 * X, "columns X .. 2X-1 of section 0 are the fresh ones"
        free = [w * wl.max_num_inputs + i for w in range(nws) for i in range(X if w == 0 else Y)]
        A = []
        for r in range(X):
            n = int(rng.integers(1, 25))
            cs = rng.choice(free, n)
            vals = _vals(rng, n)
            for c, v in zip(cs, vals):
                A.append((r, int(c), v))
        Aarr = np.zeros((len(A), 6), dtype=np.uint64)
        Aarr[:, 0] = [r for r, _, _ in A]
        Aarr[:, 1] = [c for _, c, _ in A]
        Aarr[:, 2:] = np.stack([v for _, _, v in A])
        Barr = np.zeros((X, 6), dtype=np.uint64)
        Barr[:, 0] = np.arange(X)
        Barr[:, 2:] = one
        Carr = Barr.copy()
        Carr[:, 1] = X + np.arange(X)
        # the witness: z[q][X + r] = sum_e A[r, c_e] z[q][c_e]
        Aval = _ints(Aarr[:, 2:])
        z = [np.array(_ints(wl.sections[w][p]), dtype=object).reshape(wl.num_proofs[p], Y) for w in range(nws)]
        for q in range(wl.num_proofs[p]):
            acc = [0] * X
            for (r, c, _), v in zip(A, Aval):
                acc[r] += v * int(z[c // wl.max_num_inputs][q][c % wl.max_num_inputs])
            for r in range(X):
                z[0][q][X + r] = acc[r] % Q
        wl.sections[0][p] = workload.to_mont_limbs(z[0].reshape(-1)).reshape(wl.num_proofs[p], Y, 4)
        perm = rng.permutation(len(A))
        entries.append([Aarr[perm], Barr[rng.permutation(X)], Carr[rng.permutation(X)]])
    wl.entries = entries
    return wl


def eval_point(oracle, wl, seed=3):
    """random (rx, ry) for multi_evaluate / SPARK, as tests/test_oracle_spark.py draws them"""
    nx = (wl.max_num_cons - 1).bit_length()
    ny = (wl.num_vars - 1).bit_length()
    rng = np.random.default_rng(seed)
    r = oracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * (nx + ny), dtype=np.uint8).tobytes())
    return r[:nx], r[nx:]
