"""Broken witnesses for the satisfiability checks (tests/test_gpu_sat_check.py), each built from an honest
workload by changing values the prover reads: R1CS workloads for spg_r1cs_sat_check, whole programs of
tests/hetero_program.py for spg_snark_check.

What a change to a program reaches (spg_snark_report):
  * a block witness value (hetero_program.tampered)       sat[block]
  * an exec-inputs value the block witness does not share  sat[pairwise] (execution consistency: exec k's outputs are
    exec k + 1's inputs) and perm_products[exec / blocks] (the two sides are products over the exec rows and over the
    block rows)
  * a value of the address-sorted physical / virtual list  perm_products[physical] / [virtual] (the list against the
    init list and the blocks' operations)
  * the public output                                      io_point
sat[perm_root] stays clean under every change to the caller's inputs: that instance constrains w2 / w3 of the
permutation arguments, which the prover derives itself from whatever inputs it is given, so only a fault in the
library's own witness generation could break it; no caller-side tamper can."""
import numpy as np

import hetero_program
import sat_ref
import sparse_cases
import workload

# more instances than one launch's kernel arguments hold (kMaxP = 32): 36 instances of 2 constraints, 1 or 2 executions
MANY = ([2] * 36, [1 + (p % 2) for p in range(36)], 1, False)


def many_instances():
    nc, npf, nws, shared = MANY
    return workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)


def every_row_broken(seed=5):
    """R1CSWorkload's squaring chains over a witness of random values: no row holds"""
    wl = workload.R1CSWorkload([16, 8], [2, 4])
    rng = np.random.default_rng(seed)
    for p in range(wl.P):
        n = wl.num_proofs[p] * wl.num_inputs[p]
        vals = [int.from_bytes(rng.bytes(40), "little") % workload.Q for _ in range(n)]
        wl.sections[0][p] = workload.to_mont_limbs(vals).reshape(wl.num_proofs[p], wl.num_inputs[p], 4)
    return wl


def one_change():
    """sparse_cases.satisfiable() with the fresh column X + 15 of (instance 1, execution 1) changed: exactly row
    (1, 1, 15), the last row of the domain, breaks"""
    return sat_ref.tamper(sparse_cases.satisfiable(), 1, 1, 16 + 15)


def two_changes():
    """.. and the fresh column X + 40 of (instance 0, execution 2): two rows, the lower one in instance 0"""
    return sat_ref.tamper(one_change(), 0, 2, 64 + 40, value=777)


def _set(arr, idx, value):
    arr[idx] = workload.to_mont_limbs([value % workload.Q])[0]


def exec_input_changed(case, k=1):
    """execution k's first input (exec_inputs[k][3]; the block's own copy of the row keeps the honest value)"""
    prog = hetero_program.program(case)
    _set(prog.exec_inputs, (k, 3), 424242)
    return prog


def phy_list_changed(case):
    """the data of one entry of the address-sorted physical memory list"""
    prog = hetero_program.program(case)
    _set(prog.addr_phy_mems, (1, 3), 515151)
    return prog


def vir_list_changed(case):
    """the data of one entry of the address-sorted virtual memory list"""
    prog = hetero_program.program(case)
    _set(prog.addr_vir_mems, (1, 3), 616161)
    return prog
