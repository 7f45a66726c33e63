"""The shape SNARK::prove and SNARK::verify share (csrc/snark_shape.hpp) without a GPU, through libspg_hostcheck.so:
merge_order (the witness-section merge both sides run) and SnarkShape (block sort, padding, pairwise order, sizes)
against short restatements of the reference's rules (src/lib.rs:546-604, 1155-1296)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def hc():
    import spg

    lib = spg.hostcheck()
    assert hasattr(lib, "spgh_merge_order") and hasattr(lib, "spgh_snark_shape")
    lib.spgh_merge_order.restype = ctypes.c_long
    lib.spgh_snark_shape.restype = ctypes.c_long
    return lib


def _sz(v):
    return np.ascontiguousarray(v, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def merge_ref(comps):
    """instances interleaved by decreasing num_proofs, ties to the earlier component; None without an order"""
    ptr, out = [0] * len(comps), []
    while len(out) < sum(map(len, comps)):
        best, neg_c = max((comps[c][ptr[c]], -c) for c in range(len(comps)) if ptr[c] < len(comps[c]))
        if best == 0:
            return None
        out.append(-neg_c)
        ptr[-neg_c] += 1
    return out


def merge_lib(hc, comps):
    GUARD = 0xDEADBEEF
    total = sum(map(len, comps))
    sizes, lens = _sz([x for c in comps for x in c] + [0]), _sz([len(c) for c in comps] + [0])
    out = np.full(total + 4, GUARD, np.uint64)
    n = hc.spgh_merge_order(_p(sizes), _p(lens), ctypes.c_size_t(len(comps)), _p(out))
    assert all(out[total:] == GUARD), "wrote past the merged instances"
    return None if n < 0 else [int(x) for x in out[:n]]


MERGE_CASES = {
    "ties_earlier_component_wins": ([[4, 2], [4, 2]], [0, 1, 0, 1]),
    "three_way_tie": ([[2], [2], [2]], [0, 1, 2]),
    "empty_component": ([[], [2, 1], []], [1, 1]),
    "all_empty": ([[], []], []),
    "component_exhausted_early": ([[8], [4, 2, 1]], [0, 1, 1, 1]),
    "later_component_larger": ([[2, 1], [8, 1]], [1, 0, 0, 1]),
    "all_equal": ([[2, 2], [2, 2], [2]], [0, 0, 1, 1, 2]),
    "one_component": ([[4, 4, 1]], [0, 0, 0]),
    "same_component_twice_and_thrice": ([[8], [4, 2], [4, 2], [4, 2]], [0, 1, 2, 3, 1, 2, 3]),
    # inconsistent sizes: an instance without proofs has no place in the order
    "zero_inside": ([[4, 0], [2]], None),
    "zero_only": ([[0]], None),
    "zero_last_after_others_ran_out": ([[2], [1, 0]], None),
}


@pytest.mark.parametrize("case", sorted(MERGE_CASES))
def test_merge_order_cases(hc, case):
    comps, want = MERGE_CASES[case]
    assert merge_ref(comps) == want, "the restatement itself"
    assert merge_lib(hc, comps) == want


def test_merge_order_random(hc):
    rng = np.random.default_rng(7)
    for _ in range(300):
        comps = []
        for _c in range(int(rng.integers(1, 7))):
            n = int(rng.integers(0, 5))
            comps.append(sorted((1 << int(e) for e in rng.integers(0, 4, n)), reverse=True))
            if n and rng.integers(0, 12) == 0:
                comps[-1][int(rng.integers(0, n))] = 0
        assert merge_lib(hc, comps) == merge_ref(comps), comps


def npow2(x):
    return 1 << max(x - 1, 0).bit_length()


def shape_ref(nproofs, nvars, phy, vir, niu, bmax, consis, totals, ts_bits):
    order = sorted((b for b in range(len(nproofs)) if nproofs[b]), key=lambda b: -nproofs[b])  # (stable)
    t = [npow2(x) if x else 0 for x in totals]
    pw_sizes = [npow2(consis), t[2], t[3]]
    pw_order = sorted((i for i in range(3) if pw_sizes[i]), key=lambda i: -pw_sizes[i])
    head = [len(order), npow2(bmax), npow2(consis)] + t + [max(pw_sizes), max(pw_sizes + t[:2]), max(8, ts_bits),
                                                          len(pw_order)] + pw_order + [0] * (3 - len(pw_order))
    rows = [order, [nproofs[b] for b in order], [npow2(nproofs[b]) for b in order], [nvars[b] for b in order],
            [phy[b] for b in order], [vir[b] for b in order],
            [npow2(2 * niu + 2 * phy[b] + 4 * vir[b]) for b in order]]
    return head, rows


def shape_lib(hc, nproofs, nvars, phy, vir, niu, bmax, consis, totals, ts_bits):
    Bb = len(nproofs)
    head, per = np.zeros(14, np.uint64), np.zeros((7, Bb), np.uint64)
    scal = _sz([niu, bmax, consis] + list(totals) + [ts_bits])
    P = hc.spgh_snark_shape(ctypes.c_size_t(Bb), _p(_sz(nproofs)), _p(_sz(nvars)), _p(_sz(phy)), _p(_sz(vir)), _p(scal),
                            _p(head), _p(per))
    assert P == int(head[0]) and all((per[:, P:] == 0).ravel())
    return [int(x) for x in head], [[int(x) for x in r[:P]] for r in per]


# (block_num_proofs, block_num_vars, phy ops, vir ops, niu, block_max_num_proofs, consis_num_proofs,
#  (init phy, init vir, phy, vir) totals, mem_addr_ts_bits_size)
SHAPE_CASES = {
    "two_even_blocks_no_memory": ([512, 512], [1024, 1024], [0, 0], [0, 0], 4, 512, 1024, (0, 0, 0, 0), 4),
    "unsorted_with_a_block_that_never_runs": ([2, 4, 0], [32, 64, 32], [0, 1, 0], [0, 0, 2], 4, 4, 6, (0, 0, 0, 0), 4),
    "only_zero_proof_blocks_but_one": ([0, 0, 3, 0], [16, 16, 32, 16], [1, 1, 2, 1], [0, 0, 0, 0], 5, 3, 3, (3, 0, 6, 0), 4),
    "ties_keep_block_order": ([4, 1, 4, 1, 4], [8, 16, 32, 64, 128], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0], 5, 4, 14,
                              (0, 0, 0, 0), 4),
    "phy_only_larger_than_consis": ([2, 2], [64, 64], [2, 2], [0, 0], 4, 2, 4, (5, 0, 8, 0), 4),
    "vir_only": ([2, 2], [64, 64], [0, 0], [2, 2], 5, 2, 4, (0, 3, 0, 8), 16),
    "phy_and_vir_vir_largest": ([3, 1], [64, 64], [1, 1], [2, 2], 5, 3, 4, (3, 5, 4, 9), 8),
    "phy_and_vir_all_equal_sizes": ([4, 4], [64, 64], [1, 1], [2, 2], 5, 4, 8, (1, 1, 8, 8), 8),
    "consis_not_a_power_of_two": ([5, 7, 3], [64, 64, 64], [0, 0, 0], [0, 0, 0], 4, 7, 15, (0, 0, 0, 0), 4),
    "totals_not_powers_of_two": ([1], [32], [3], [2], 6, 1, 1, (20, 7, 3, 2), 4),
}


@pytest.mark.parametrize("case", sorted(SHAPE_CASES))
def test_snark_shape_cases(hc, case):
    args = SHAPE_CASES[case]
    assert shape_lib(hc, *args) == shape_ref(*args)


def test_snark_shape_orders_by_case():
    """what the named cases are there for, on the restatement: P < Bb, and pw_order of every length"""
    head, rows = shape_ref(*SHAPE_CASES["unsorted_with_a_block_that_never_runs"])
    assert head[0] == 2 and rows[0] == [1, 0]
    assert shape_ref(*SHAPE_CASES["ties_keep_block_order"])[1][0] == [0, 2, 4, 1, 3]
    pw = {c: shape_ref(*SHAPE_CASES[c])[0][10:] for c in SHAPE_CASES}
    assert pw["two_even_blocks_no_memory"] == [1, 0, 0, 0]
    assert pw["phy_only_larger_than_consis"] == [2, 1, 0, 0]
    assert pw["vir_only"] == [2, 2, 0, 0]
    assert pw["phy_and_vir_vir_largest"] == [3, 2, 0, 1]
    assert pw["phy_and_vir_all_equal_sizes"] == [3, 0, 1, 2]


def width_violation(hc, prog):
    """block_width_violation on the C views spg_snark_encode / spg_snark_witness_new are given"""
    import workload

    v = workload.SnarkViews(prog)
    a, ci = v.inputs, v.block.inst
    hc.spgh_block_width_violation.restype = ctypes.c_long
    return hc.spgh_block_width_violation(
        ctypes.c_size_t(a.block_num_instances_bound), a.block_num_proofs, a.block_num_vars, a.block_num_phy_ops,
        a.block_num_vir_ops, ctypes.c_size_t(a.num_inputs_unpadded), ctypes.c_size_t(a.num_vars), ci.entries, ci.nnz)


def test_block_width_check(hc):
    """what spg_snark_prove refuses with SPG_E_ARG before any launch: an executed block whose matrices name a column
    at or beyond its block_num_vars, or whose rows are too short for its io and memory-operation variables (the
    host's w2 recurrences would read past them). Honest programs pass, and a block that never runs is not read."""
    import hetero_program
    import workload
    from r1cs_cases import SNARK_CASES
    from test_circ import out_of_width_program

    for case in hetero_program.CASES:
        assert width_violation(hc, hetero_program.program(case)) == -1
    for case in ("widths_b3_x64", "mem_uneven_b3_x64", "uneven_b3_x32"):
        assert width_violation(hc, workload.SnarkWorkload(**SNARK_CASES[case])) == -1
    assert width_violation(hc, out_of_width_program(executed=True)[2]) == 1
    assert width_violation(hc, out_of_width_program(executed=False)[2]) == -1
    prog = hetero_program.program("hetero_mem_b3")
    prog._num_vars_per_block = [32, 64, 32]  # block 2: 10 io + 2 + 16 memory-operation variables, then the chain
    assert width_violation(hc, prog) == 2
    prog._num_vars_per_block = [32, 64, 16]
    assert width_violation(hc, prog) == 2
    prog._num_vars_per_block = [32, 128, 64]  # wider than num_vars, the section stride of the matrices
    assert width_violation(hc, prog) == 1


def test_snark_shape_random(hc):
    rng = np.random.default_rng(11)
    for _ in range(200):
        Bb = int(rng.integers(1, 9))
        nproofs = [int(x) for x in rng.integers(0, 9, Bb)]
        if not any(nproofs):
            nproofs[0] = 1
        nvars = [1 << int(e) for e in rng.integers(3, 8, Bb)]
        phy, vir = [int(x) for x in rng.integers(0, 4, Bb)], [int(x) for x in rng.integers(0, 3, Bb)]
        totals = [int(x) * int(k) for x, k in zip(rng.integers(0, 20, 4), rng.integers(0, 2, 4))]
        args = (nproofs, nvars, phy, vir, int(rng.integers(3, 7)), max(nproofs), sum(nproofs), totals,
                1 << int(rng.integers(2, 5)))
        assert shape_lib(hc, *args) == shape_ref(*args), args
