"""Heterogeneous programs (tests/hetero_program.py) on the CPU: the cases really differ between blocks in every respect
the prover indexes per block, the oracle proves and verifies them (bytes frozen in tests/golden/snark_proofs.json),
rejects them after one witness value is changed, and a case that goes through .ctk / .rtk files proves alike."""
import hashlib
import json
import os

import numpy as np
import pytest

import hetero_program
from hetero_program import CASES

G = os.path.join(os.path.dirname(__file__), "golden")


def _golden(case):
    return json.load(open(os.path.join(G, "snark_proofs.json")))[case]


def _row_lengths(mat):
    return np.bincount(mat[:, 0].astype(np.int64)) if len(mat) else np.zeros(1, np.int64)


def _has_duplicate(mat):
    return len({(int(r), int(c)) for r, c in mat[:, :2]}) < len(mat)


@pytest.mark.parametrize("case", sorted(CASES))
def test_cases_are_heterogeneous(case):
    """what each case is there for, so that a later edit cannot make the blocks uniform unnoticed"""
    import circ

    ctk, rtk = hetero_program.build(**CASES[case])
    prog = circ.CircProgram(ctk, rtk)
    mats, _, ncons, _ = prog.block_inst
    B, nproofs = prog.num_blocks, prog.block_num_proofs
    # in every case: ragged padded constraint counts and widths, executions neither equal nor sorted, a row of at
    # least 40 terms, a duplicate (row, col) inside one matrix, an empty user row
    assert len(set(ncons)) >= 2 and len(set(prog.num_vars_per_block)) >= 2
    assert len(set(nproofs)) >= 2 and nproofs != sorted(nproofs) and nproofs != sorted(nproofs, reverse=True)
    assert max(int(_row_lengths(m).max()) for m3 in mats for m in m3) >= 40
    assert any(_has_duplicate(m) for m3 in mats for m in m3)
    assert any(row == ([], [], []) for block in ctk.args for row in block)
    assert any(len({c for c, _ in row[0]}) < len(row[0]) for block in ctk.args for row in block), "a column twice in a row"
    # the prover's sort really permutes the blocks
    order = sorted(range(B), key=lambda b: -nproofs[b])
    assert order[:sum(1 for n in nproofs if n)] != list(range(sum(1 for n in nproofs if n)))
    if case == "hetero_mem_b3":
        assert len(set(ncons)) == 3, ncons
        assert len(set(zip(prog.block_num_phy_ops, prog.block_num_vir_ops))) == 3
        assert len(set(prog.block_num_phy_ops)) == 3 and len(set(prog.block_num_vir_ops)) == 3
        most = max(range(B), key=lambda b: ncons[b])
        assert nproofs[most] == min(nproofs) and nproofs[most] > 0
        # the maxima are not taken by one block: max ops, max constraints and max executions sit on different blocks
        assert max(range(B), key=lambda b: prog.block_num_vir_ops[b]) != most
        assert len(prog.addr_phy_mems) > 0 and len(prog.addr_vir_mems) > 0
    if case == "hetero_nomem_b4":
        assert B == 4 and not any(prog.block_num_phy_ops) and not any(prog.block_num_vir_ops)
        assert 0 in nproofs and 1 in nproofs and len(set(ncons)) >= 3
    if case == "hetero_b33":
        assert B > 32 and 0 in nproofs
        assert len(set(prog.block_num_phy_ops)) == 3, "physical reads differ between blocks beyond kMaxP too"
        executed = [b for b in order if nproofs[b]]
        assert [prog.block_num_phy_ops[b] for b in executed] != prog.block_num_phy_ops[:len(executed)]
        assert all(ncons[b] == ncons[b % 2] for b in range(B)) and ncons[0] != ncons[1]
        w = prog.num_vars_per_block
        assert all(w[b] == w[b % 2] for b in range(B)) and w[0] != w[1]


@pytest.fixture(scope="module")
def proofs(oracle):
    import workload

    out = {}
    for case in CASES:
        out[case] = oracle.snark_prove(hetero_program.program(case), workload.tape_seed())
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_proves_and_verifies(proofs, case):
    proof, rc = proofs[case]
    assert rc == 0, f"oracle verifier rejected at stage {rc}"
    assert _golden(case) == {"proof_sha256": hashlib.sha256(proof).hexdigest(), "proof_len": len(proof)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_rejects_changed_witness(oracle, case):
    """one chain value of one execution changed: a column that block's chain rows and its multi-term rows name"""
    import workload

    prog, bad = hetero_program.program(case), hetero_program.tampered(case)
    diff = [int((a != b).any(axis=-1).sum()) for a, b in zip(prog.block_vars_sorted, bad.block_vars_sorted)]
    assert sum(diff) == 1, "exactly one scalar differs"
    b = max(range(prog.num_blocks), key=lambda i: prog.block_num_proofs[i])
    col = hetero_program.chain_column(case, b)
    A = prog.block_inst[0][b][0]
    rows_with_col = {int(r) for r in A[A[:, 1] == col][:, 0]}
    assert any(int(_row_lengths(A)[r]) >= 20 for r in rows_with_col), "the column sits under a multi-term row"
    _, rc = oracle.snark_prove(bad, workload.tape_seed())
    assert rc != 0


def test_hetero_program_through_files_proves_alike(oracle, proofs, tmp_path):
    import circ
    import workload

    case = "hetero_mem_b3"
    ctk, rtk = hetero_program.build(**CASES[case])
    cp, rp = tmp_path / "h_bin.ctk", tmp_path / "h_bin.rtk"
    cp.write_bytes(ctk.to_bytes())
    rp.write_bytes(rtk.to_bytes())
    prog = circ.CircProgram.load(str(cp), str(rp))
    assert prog.block_num_proofs == [4, 1, 4] and prog.num_vars_per_block == CASES[case]["widths"]
    proof, rc = oracle.snark_prove(prog, workload.tape_seed())
    assert rc == 0 and proof == proofs[case][0]


def test_generator_rejects_a_column_beyond_the_block_width():
    spec = dict(CASES["hetero_nomem_b4"])
    spec["widths"] = [64, 8, 32, 64]  # block 1's chain ends at column 9
    with pytest.raises(AssertionError, match="widths"):
        hetero_program.build(**spec)
