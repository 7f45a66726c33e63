"""The stand-alone entries on structured sparse matrices (tests/sparse_cases.py): ragged per-matrix nnz (0, 1, 37,
more than num_cons, more operations than SPARK memory cells), hot rows and columns beyond a workgroup, duplicate
(row, col) entries, the values 0, 1 and q-1, shuffled entry lists. spg_r1cs_multi_evaluate, spg_spark_commit / prove /
verify and spg_r1cs_prove against the CPU oracle byte for byte (hashes frozen in tests/golden/spark_proofs.json and
r1cs_proofs.json under structured_<case>; on a mismatch the oracle's own bytes name the first differing field)."""
import hashlib
import json
import os

import numpy as np
import pytest

import sparse_cases
from sparse_cases import CASES
from test_gpu_r1cs import GENS_LABEL, GENS_NV, _eq_table, _int, gpu_prove
from test_gpu_spark import GENS_LABEL as SPARK_GENS_LABEL

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def r1cs_gens(ctx):
    import spg

    return spg.R1CSGens(ctx, GENS_LABEL, GENS_NV)


def _golden(name, case):
    return json.load(open(os.path.join(G, name)))["structured_" + case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_spark_on_structured_matrices(ctx, oracle, case):
    """multi_evaluate, the commitment and the evaluation proof equal the oracle's; the verifier accepts them and
    rejects another label, other evaluations and altered fields"""
    import spg
    import workload
    from proof_layout import first_diff_spark, spark_proof_fields

    wl = sparse_cases.structured(case)
    rx, ry = sparse_cases.eval_point(oracle, wl)
    v = workload.CViews(wl)
    gens_nnz = len(wl.entries) * max(max(int(m.shape[0]) for m in mats) for mats in wl.entries)
    comm = spg.SparkCommitment(ctx, v.inst, SPARK_GENS_LABEL, gens_nnz, 3)
    evals = spg.r1cs_multi_evaluate(ctx, spg.R1CSInst(ctx, v.inst), len(wl.entries), rx, ry)
    assert np.array_equal(evals, oracle.r1cs_multi_evaluate(wl, rx, ry))
    proof = comm.prove(rx, ry, evals, spg.Transcript(b"spark_test"), spg.RandomTape(b"proof", workload.tape_seed()))
    golden = _golden("spark_proofs.json", case)
    if (hashlib.sha256(comm.bytes).hexdigest(), hashlib.sha256(proof).hexdigest()) != (golden["comm_sha256"],
                                                                                     golden["proof_sha256"]):
        rcomm, ref, ok = oracle.spark_prove(wl, rx, ry, workload.tape_seed())
        assert ok and hashlib.sha256(ref).hexdigest() == golden["proof_sha256"], "the oracle left its golden bytes"
        assert comm.bytes == rcomm, "commitment bytes differ"
        where = first_diff_spark(proof, ref) if len(proof) == len(ref) else f"length {len(proof)} vs {len(ref)}"
        pytest.fail(f"SPARK proof bytes differ first at {where}")
    ok, why = comm.verify(rx, ry, evals, spg.Transcript(b"spark_test"), proof)
    assert ok, why
    ok, _ = comm.verify(rx, ry, evals, spg.Transcript(b"spark_other"), proof)
    assert not ok
    for k in (0, len(evals) - 1):
        bad_evals = evals.copy()
        bad_evals[k] = workload.to_mont_limbs([1 if _int(evals[k]) != 1 else 2])[0]
        ok, _ = comm.verify(rx, ry, bad_evals, spg.Transcript(b"spark_test"), proof)
        assert not ok, f"accepted with evaluation {k} changed"
    fields = spark_proof_fields(proof)
    for name, s, e in fields[:: max(1, len(fields) // 24)]:
        bad = bytearray(proof)
        bad[s + (e - s) // 2] ^= 0x04
        ok, _ = comm.verify(rx, ry, evals, spg.Transcript(b"spark_test"), bytes(bad))
        assert not ok, f"accepted with {name} altered"


@pytest.mark.parametrize("case", sorted(CASES))
def test_r1cs_proof_on_structured_matrices(ctx, oracle, r1cs_gens, case):
    """R1CSProof::prove: the oracle's bytes and challenges, and the same proof from the same matrices with every
    entry list sorted by (row, col): the order of a matrix's entries (so the CSR build's) must not matter"""
    import workload
    from proof_layout import first_diff

    wl = sparse_cases.structured(case)
    seed = workload.tape_seed()
    ref, ref_ch = oracle.r1cs_prove(wl, seed, gens_label=GENS_LABEL, gens_num_vars=GENS_NV)
    assert hashlib.sha256(ref).hexdigest() == _golden("r1cs_proofs.json", case)["sha256"]
    got, got_ch = gpu_prove(ctx, r1cs_gens, wl, seed)
    assert len(got_ch) == len(ref_ch)
    for a, b in zip(got_ch, ref_ch):
        assert np.array_equal(a, b), "challenges differ"
    assert len(got) == len(ref)
    if got != ref:
        pytest.fail(f"proof bytes differ first at field {first_diff(got, ref)}")
    again, _ = gpu_prove(ctx, r1cs_gens, sparse_cases.sorted_entries(wl), seed)
    if again != got:
        pytest.fail(f"sorted entry lists give another proof, first at field {first_diff(again, got)}")


def test_r1cs_verify_on_satisfiable_matrices(ctx, oracle, r1cs_gens):
    """spg_r1cs_verify accepts the GPU proof (the oracle's bytes) of the satisfiable structured case with the
    rp-bound evaluations, returns the prover's challenges, and rejects each altered claim"""
    import spg
    import workload

    wl = sparse_cases.satisfiable()
    seed = workload.tape_seed()
    proof, ch = gpu_prove(ctx, r1cs_gens, wl, seed)
    ref, ref_ch = oracle.r1cs_prove(wl, seed, gens_label=GENS_LABEL, gens_num_vars=GENS_NV)
    assert proof == ref and hashlib.sha256(ref).hexdigest() == _golden("r1cs_proofs.json", "satisfiable")["sha256"]
    for a, b in zip(ch, ref_ch):
        assert np.array_equal(a, b)
    rp, rx, rwry = ch[0], ch[2], ch[3]
    v = workload.CViews(wl)
    ev = spg.r1cs_multi_evaluate(ctx, spg.R1CSInst(ctx, v.inst), len(wl.entries), rx, rwry)
    assert np.array_equal(ev, oracle.r1cs_multi_evaluate(wl, rx, rwry))
    eq = _eq_table([_int(x) for x in rp])
    bound = [sum(eq[p] * _int(ev[3 * p + k]) for p in range(wl.P)) % workload.Q for k in range(3)]
    sections = []
    for w in range(wl.nws):
        mats = wl.sections[w]
        sections.append(([m.shape[0] for m in mats], [m.shape[1] for m in mats],
                         [spg.r1cs_gens_commit(ctx, r1cs_gens, m.reshape(-1, 4)) for m in mats]))
    args = (ctx, r1cs_gens, wl.P, wl.max_num_proofs, wl.num_proofs, wl.max_num_inputs, sections, wl.max_num_cons)
    ok, why, vch = spg.r1cs_verify(*args, workload.to_mont_limbs(bound), spg.Transcript(b"r1cs_test"), proof)
    assert ok, why
    for a, b in zip(vch, ch):
        assert np.array_equal(a, b)
    for k in range(3):
        bad = list(bound)
        bad[k] = (bad[k] + 1) % workload.Q
        ok, _, _ = spg.r1cs_verify(*args, workload.to_mont_limbs(bad), spg.Transcript(b"r1cs_test"), proof)
        assert not ok, f"accepted with claim {k} altered"
