"""SNARK::prove and SNARK::verify on the GPU for heterogeneous programs (tests/hetero_program.py): block types that
differ in constraint count, witness width, memory operations, row length and executions, so an index taken in the
wrong order (sort position against block number, a maximum against the per-block value) changes the bytes. Everything
is compared byte for byte with the CPU oracle (tests/golden/snark_proofs.json holds its proofs' hashes, frozen after
its verifier accepted; on a mismatch the oracle runs live to name the first differing field)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hetero_program
from hetero_program import CASES

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
GENS_LABEL = b"gens_r1cs_sat"
GENS_NV = 1 << 24


@pytest.fixture(scope="module")
def vars_gens(ctx):
    import spg

    return spg.R1CSGens(ctx, GENS_LABEL, GENS_NV)


class Program:
    def __init__(self, ctx, vars_gens, case):
        import spg
        import workload

        self.ctx, self.gens = ctx, vars_gens
        self.prog = hetero_program.program(case)
        self.v = workload.SnarkViews(self.prog)
        self.block = spg.SnarkComp(ctx, self.v.block, multi=True)
        self.pairwise = spg.SnarkComp(ctx, self.v.pairwise)
        self.perm_root = spg.SnarkComp(ctx, self.v.perm_root)
        self.wit = spg.SnarkWitness(ctx, self.v.inputs)

    def prove(self, label=b"snark_test"):
        import spg
        import workload

        return spg.snark_prove(self.ctx, self.block, self.pairwise, self.perm_root, self.wit, self.gens,
                               spg.Transcript(label), spg.RandomTape(b"proof", workload.tape_seed()))

    def verify(self, proof, label=b"snark_test"):
        import spg

        return spg.snark_verify(self.ctx, self.block, self.pairwise, self.perm_root, self.v.inputs, self.gens,
                                spg.Transcript(label), proof)


def _check(got, case, oracle):
    golden = json.load(open(os.path.join(G, "snark_proofs.json")))[case]
    if hashlib.sha256(got).hexdigest() == golden["proof_sha256"]:
        return
    import workload
    from proof_layout import first_diff_snark

    ref, rc = oracle.snark_prove(hetero_program.program(case), workload.tape_seed())
    assert rc == 0 and hashlib.sha256(ref).hexdigest() == golden["proof_sha256"], "the oracle left its golden bytes"
    where = first_diff_snark(got, ref) if len(got) == len(ref) else f"length {len(got)} vs {len(ref)}"
    pytest.fail(f"SNARK bytes differ first at {where}")


@pytest.mark.parametrize("case", sorted(CASES))
def test_hetero_proof_matches_oracle(ctx, oracle, vars_gens, case):
    p = Program(ctx, vars_gens, case)
    a = p.prove()
    _check(a, case, oracle)
    assert p.prove() == a, "proof not repeatable"
    ok, why = p.verify(a)
    assert ok, why


@pytest.fixture(scope="module")
def mem_b3(ctx, vars_gens):
    p = Program(ctx, vars_gens, "hetero_mem_b3")
    p.proof = p.prove()
    return p


def test_hetero_verify_rejects_altered_fields(mem_b3):
    """one bit flipped in each of at least 48 fields spread over the whole proof and in the first 8 vector lengths"""
    from proof_layout import snark_proof_fields

    fields = snark_proof_fields(mem_b3.proof)
    spread, lens = fields[::max(1, len(fields) // 48)], [f for f in fields if f[0].endswith(".len")][:8]
    assert len(spread) >= 48 and len(lens) == 8
    picked = spread + lens
    for name, s, e in picked:
        bad = bytearray(mem_b3.proof)
        bad[s + (e - s) // 2] ^= 0x04
        ok, _ = mem_b3.verify(bytes(bad))
        assert not ok, f"accepted with {name} altered"


def test_hetero_verify_rejects_other_output(mem_b3):
    import workload

    ok, why = mem_b3.verify(mem_b3.proof)
    assert ok, why
    keep = mem_b3.v.inputs.output
    out = np.ascontiguousarray(workload.to_mont_limbs([(mem_b3.prog.output + 1) % workload.Q])[0])
    mem_b3.v.inputs.output = out.ctypes.data_as(ctypes.c_void_p).value
    try:
        ok, _ = mem_b3.verify(mem_b3.proof)
    finally:
        mem_b3.v.inputs.output = keep
    assert not ok, "accepted a wrong output"


PRE = [(b"app-domain", b"verifier session"), (b"app-nonce", bytes(range(24)))]


def _pre_transcript(oracle, label):
    t = oracle.OracleTranscript(label)
    for lbl, msg in PRE:
        t.append_message(lbl, msg)
    return t


def test_hetero_verify_public_from_commitment_bytes(ctx, oracle, vars_gens):
    """spg_snark_verify_public, holding only the exported commitment bytes, block_comm_map and the public values,
    accepts the proof made on a caller transcript and leaves that transcript in the oracle verifier's state"""
    import spg
    import workload

    prog = hetero_program.program("hetero_mem_b3")
    v = workload.SnarkViews(prog)
    pub = workload.SnarkPublic(prog)
    seed = workload.tape_seed()
    block = spg.SnarkComp(ctx, v.block, multi=True)
    pairwise = spg.SnarkComp(ctx, v.pairwise)
    perm_root = spg.SnarkComp(ctx, v.perm_root)
    cb, cmap = block.comm_bytes(True), block.comm_map()
    cp, cr = pairwise.comm_bytes(False), perm_root.comm_bytes(False)
    tp = _pre_transcript(oracle, b"snark_pub")
    proof = spg.snark_prove(ctx, block, pairwise, perm_root, spg.SnarkWitness(ctx, v.inputs), vars_gens,
                            spg.Transcript.from_callbacks(tp.append_message, tp.challenge_bytes),
                            spg.RandomTape(b"proof", seed))
    del block, pairwise, perm_root
    ovt = _pre_transcript(oracle, b"snark_pub")
    ref, verdict = oracle.snark_prove_verify_on(prog, seed, _pre_transcript(oracle, b"snark_pub"), ovt)
    assert proof == ref and verdict == 0
    c = pub.c
    vb = spg.SnarkComp.load(ctx, cb, True, cmap, c.block_num_cons, pub.block_gens)
    vp = spg.SnarkComp.load(ctx, cp, False, None, c.pairwise_check_num_cons, pub.pairwise_gens)
    vr = spg.SnarkComp.load(ctx, cr, False, None, c.perm_root_num_cons, pub.perm_root_gens)
    t = _pre_transcript(oracle, b"snark_pub")
    ok, why = spg.snark_verify_public(ctx, vb, vp, vr, c, vars_gens,
                                      spg.Transcript.from_callbacks(t.append_message, t.challenge_bytes), proof)
    assert ok, why
    assert t.challenge_bytes(b"after", 32) == ovt.challenge_bytes(b"after", 32), "verifier transcripts diverge"


# the switches under which per-block shape matters (a fresh process reads them)
FORMS = {
    "eval_one_thread": {"SPG_SC_QUAD_MAX": "0"},
    "eval_one_thread_per_point": {"SPG_SC_QUAD_MAX": "0", "SPG_P1_ROWS": "0"},
    "fold_launches": {"SPG_SC_FUSE": "0"},
    "spmv_and_z_fill_untiled": {"SPG_SPMV_TILED": "0", "SPG_Z_TILED": "0"},
    "q_folds_one_per_challenge": {"SPG_Q_BOUND_ALL": "0"},
    "witness_parts_copied": {"SPG_WIT_IN_PLACE": "0"},
    "phase1_single_rounds": {"SPG_P1_PAIR": "0"},
    "phase2_single_rounds": {"SPG_P2_PAIR": "0"},
    "rounds_commit_their_own_points": {"SPG_TAPE_AHEAD": "0"},
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_hetero_round_forms(form):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    case = "hetero_mem_b3"
    code = (
        "import sys, hashlib; sys.path[:0] = [%r, %r]\n"
        "import spg\n"
        "from test_gpu_hetero import Program, GENS_LABEL, GENS_NV\n"
        "ctx = spg.Context(0)\n"
        "p = Program(ctx, spg.R1CSGens(ctx, GENS_LABEL, GENS_NV), %r).prove()\n"
        "print(hashlib.sha256(p).hexdigest())\n"
    ) % (os.path.join(root, "spartan-parallel_amd"), os.path.join(root, "tests"), case)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **FORMS[form]), capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    golden = json.load(open(os.path.join(G, "snark_proofs.json")))[case]
    assert out.stdout.split()[-1] == golden["proof_sha256"]
