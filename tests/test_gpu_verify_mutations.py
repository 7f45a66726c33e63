"""spg_snark_verify against the CPU oracle's verdicts on every well-formed alteration of a whole proof
(tests/proof_mutations.py): each pt / sc field replaced by another valid point / canonical scalar, so the bytes parse
and decompress and only a check of the verifier can refuse them. The oracle's verdicts are those frozen in
tests/golden/snark_mutations.json (tests/test_oracle_snark_mutations.py recomputes them on the CPU); no oracle
verification runs here. The proof is the GPU prover's, whose sha256 must be the fixture's.

  * verdict parity: the product verifier rejects exactly when the oracle did, never as "malformed", and the deferred
    mode (spg_set_verify_device) returns the eager mode's (verdict, text);
  * each equation is load-bearing: the response scalars of the sigma protocols never reach the transcript, so one
    check alone can refuse them, and the rejection names it (proof_mutations.SIGMA_ROWS), for both mutation kinds in
    both modes;
  * the deferred launch still carries the whole proof's equations when the last scalar of the last R1CSProof is the
    one altered.

All comparisons are exact."""
import hashlib
import json
import os
import time

import pytest

import proof_mutations as pm
from test_gpu_verify import Program, vars_gens  # noqa: F401  (the module's generator fixture)

pytestmark = pytest.mark.gpu

FX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "snark_mutations.json")))
CHUNKS = {case: pm.chunks(FX[case]["stages"]) for case in sorted(pm.SWEEP)}
ITEMS = [(case, part) for case in sorted(pm.SWEEP) for part in CHUNKS[case]]
# the fields the reference's verifier does not bind (accepted by both verifiers)
from test_oracle_snark_mutations import UNBOUND  # noqa: E402


class Mutated:
    """one case: the GPU prover's proof and its (field, mutation) table"""

    def __init__(self, ctx, gens, case):
        from proof_layout import snark_dotlog_names

        self.prog = Program(ctx, gens, case)
        proof = self.prog.proof
        assert hashlib.sha256(proof).hexdigest() == FX[case]["proof_sha256"], "the prover's bytes are not the fixture's"
        self.dotlogs = set(snark_dotlog_names(proof))
        self.table = {key: (name, how, start, new) for key, name, how, start, new in pm.mutations(proof, pm.SWEEP[case])}
        assert list(self.table) == list(FX[case]["stages"]), "the fixture's (field, mutation) pairs differ from the sweep's"

    def bytes_of(self, key):
        _, _, start, new = self.table[key]
        return pm.apply(self.prog.proof, start, new)


@pytest.fixture(scope="module")
def mutated(ctx, vars_gens):  # noqa: F811
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Mutated(ctx, vars_gens, case)
        return cache[case]

    return get


def named(why, row):
    """the rejection text is that of the row's check and of no other (DotProductProof is a prefix of
    DotProductProofLog)"""
    return why.endswith(": " + pm.SIGMA_ROWS[row][1])


@pytest.mark.parametrize("case,part", ITEMS)
def test_verdict_parity_and_texts(ctx, mutated, case, part):
    m = mutated(case)
    keys = CHUNKS[case][part]
    variants = [m.bytes_of(k) for k in keys]
    got, secs = {}, {}
    try:
        for deferred in (False, True):
            ctx.set_verify_device(deferred)
            t0 = time.perf_counter()
            got[deferred] = [m.prog.verify(b) for b in variants]
            secs[deferred] = time.perf_counter() - t0
    finally:
        ctx.set_verify_device(False)
    print(f"\n{case} {part}: {len(keys)} proofs, eager {secs[False]:.2f} s, deferred {secs[True]:.2f} s")
    for key, eager, deferred in zip(keys, got[False], got[True]):
        name = m.table[key][0]
        stage = FX[case]["stages"][key]
        assert (stage == 0) == (name in UNBOUND), key
        assert eager[0] == (stage == 0), f"{key}: oracle stage {stage}, product {eager}"
        assert deferred == eager, f"{key}: eager {eager}, deferred {deferred}"
        if eager[0]:
            continue
        assert "malformed" not in eager[1], (key, eager)
        row = pm.sigma_row(name, m.dotlogs)
        if row:
            assert named(eager[1], row), f"{key}: expected the {row} check, got {eager[1]!r}"


@pytest.mark.parametrize("case", sorted(pm.SWEEP))
def test_every_sigma_row_is_swept(mutated, case):
    """the patterns of SIGMA_ROWS select something in every row, in both kinds unless an honest response is zero, and
    the DotProductProofLog instances found by their response scalars are the _dotlog records of the typed map (all of
    them in the small case, those under the memory case's prefixes there)"""
    m = mutated(case)
    rows = {}
    for key, (name, how, _, _) in m.table.items():
        row = pm.sigma_row(name, m.dotlogs)
        if row:
            rows.setdefault(row, {}).setdefault(how, set()).add(name)
    assert set(rows) == set(pm.SIGMA_ROWS), rows.keys()
    for row, kinds in rows.items():
        assert kinds["inc"] and kinds.get("zero"), row
        assert kinds["zero"] <= kinds["inc"]
    sel = pm.SWEEP[case]
    want = {d for d in m.dotlogs if sel is None or d.startswith(sel)}
    assert want
    found = {n[:-3] for n in rows["DotProductProofLog"]["inc"]}
    assert len(found) == len(want) and found == want
    for d in want:
        assert {d + ".z1", d + ".z2"} <= rows["DotProductProofLog"]["inc"]
    # every round of both ZK sumchecks, every coefficient: z[j] for each j of the round's length, z_delta and z_beta
    from proof_layout import snark_proof_fields_typed

    for name, s, e, kind in snark_proof_fields_typed(m.prog.proof):
        if kind == "len" and name.endswith(".z.len") and ".proofs[" in name and (sel is None or name.startswith(sel)):
            n = int.from_bytes(m.prog.proof[s:e], "little")
            head = name[:-len(".z.len")]
            assert n > 0
            assert {f"{head}.z[{j}]" for j in range(n)} | {head + ".z_delta", head + ".z_beta"} <= rows["DotProductProof"]["inc"]


def test_deferred_launch_carries_the_whole_proof(ctx, mutated):
    """the last scalar of the last R1CSProof altered: every earlier equation holds, the deferred verifier still
    reaches its one launch, and that launch holds the accepted proof's equations and terms"""
    m = mutated(pm.SMALL)
    key = "perm_root_r1cs_sat_proof.proof_eq_sc_phase2.z|inc"
    bad = m.bytes_of(key)
    ctx.prof_enable(True)
    try:
        ctx.set_verify_device(True)
        ctx.prof_read()
        ok, why = m.prog.verify()
        assert ok, why
        assert ctx.prof_read()["eqs_check"][0] == 1
        counts = ctx.eqs_last_counts()
        ok, why = m.prog.verify(bad)
        assert not ok and named(why, "EqualityProof"), why
        assert ctx.prof_read()["eqs_check"][0] == 1
        assert ctx.eqs_last_counts() == counts
    finally:
        ctx.set_verify_device(False)
        ctx.prof_enable(False)
