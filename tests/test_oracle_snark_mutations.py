"""The CPU oracle's verdict on every well-formed alteration of a whole SNARK proof (tests/proof_mutations.py): its
verifier, reading the bytes through the bincode reader De (oracle/nizk.hpp), rejects each one at a stage 1..16, and
the stages are frozen in tests/golden/snark_mutations.json, which the product verifier's parity tests read
(tests/test_gpu_verify_mutations.py).

Swept: every pt / sc field of the smallest program's proof (b2_x32_q2: 2 332 fields, 2 997 (field, mutation) pairs),
and of the memory program's proof (mem_both_b3_x64_q2) the parts that are empty or shorter in the small one, by the
name prefixes proof_mutations.MEM_PREFIXES: the memory commitment lists addr_comm_* and {init_,}{phy,vir}_mem*_comm_*,
everything under pairwise_check_*, perm_poly_poly_list, proof_eval_perm_poly_prod_list and shift_proof.* (1 210
fields, 1 567 pairs). No field of either selection is left out: the counts are pinned below.

UNBOUND lists the fields whose alteration the oracle accepts, i.e. that the reference verifier does not bind. An
accepted alteration outside the table fails, and so does a table entry that is rejected."""
import hashlib
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import proof_mutations as pm
from r1cs_cases import SNARK_CASES

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(G, "snark_mutations.json")

# {field: "src/...rs:line, why"}: alterations of these fields are accepted by the reference's verifier
UNBOUND = {}

PAIRS = {pm.SMALL: 2997, pm.MEM: 1567}  # (field, mutation) pairs per case


def oracle_sweep(O, case):
    """(proof, {key: stage}) of the oracle over every (field, mutation) of the case, on at most 16 threads"""
    import workload

    wl = workload.SnarkWorkload(**SNARK_CASES[case])
    proof, rc = O.snark_prove(wl, workload.tape_seed())
    assert rc == 0, (case, rc)
    verifier = O.SnarkVerifier(wl)
    assert verifier.verify(proof) == 0
    muts = pm.mutations(proof, pm.SWEEP[case])
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        stages = list(pool.map(lambda m: verifier.verify(pm.apply(proof, m[3], m[4])), muts))
    return proof, {m[0]: st for m, st in zip(muts, stages)}


def _fixture():
    return json.load(open(FIXTURE))


_ITEMS = [(case, part) for case in sorted(pm.SWEEP) for part in pm.chunks(_fixture()[case]["stages"])]


@pytest.fixture(scope="module")
def sweeps(oracle):
    out = {}
    for case in sorted(pm.SWEEP):
        t0 = time.time()
        out[case] = oracle_sweep(oracle, case)
        print(f"oracle sweep {case}: {len(out[case][1])} verdicts in {time.time() - t0:.1f} s")
    return out


@pytest.mark.parametrize("case", sorted(pm.SWEEP))
def test_sweep_covers_every_field(sweeps, case):
    """the proof is the frozen one, and the sweep and the fixture hold exactly the (field, mutation) pairs of the
    typed map's selection: nothing sampled, nothing left over"""
    from proof_layout import snark_proof_fields_typed

    proof, stages = sweeps[case]
    fx = _fixture()[case]
    assert hashlib.sha256(proof).hexdigest() == fx["proof_sha256"]
    assert fx["proof_sha256"] == json.load(open(os.path.join(G, "snark_proofs.json")))[case]["proof_sha256"]
    sel = pm.SWEEP[case]
    fields = [n for n, _, _, k in snark_proof_fields_typed(proof) if k != "len" and (sel is None or n.startswith(sel))]
    assert len(fields) == pm.SWEEP_FIELDS[case]
    assert {k.split("|")[0] for k in stages if k.endswith("|inc")} == set(fields)
    assert len(stages) == PAIRS[case]
    assert list(stages) == list(fx["stages"]), "the fixture's keys differ from the sweep's (regenerate: make_golden.py mutations)"
    if sel is not None:  # every prefix of the subset selects something
        for p in sel:
            assert any(n.startswith(p) for n in fields), p


@pytest.mark.parametrize("case,part", _ITEMS)
def test_oracle_rejects_every_mutation(sweeps, case, part):
    _, stages = sweeps[case]
    fx = _fixture()[case]["stages"]
    for key in pm.chunks(fx)[part]:
        st = stages[key]
        assert st != 0 or key.split("|")[0] in UNBOUND, f"the oracle accepts {key}: an unbound field outside UNBOUND"
        assert st == 0 or key.split("|")[0] not in UNBOUND, f"{key} is in UNBOUND but rejected at stage {st}"
        assert st >= 0, f"{key}: a well-formed alteration read as malformed / not decompressing ({st})"
        assert st == fx[key], f"{key}: stage {st}, fixture {fx[key]}"


def test_unbound_entries_are_fields_of_the_sweep():
    fx = _fixture()
    names = {k.split("|")[0] for case in fx for k in fx[case]["stages"]}
    assert set(UNBOUND) <= names


@pytest.mark.parametrize("case", sorted(SNARK_CASES))
def test_reserialize_round_trip(oracle, case):
    """De then Ser gives back the bytes of every frozen proof; truncated and extended bytes are malformed"""
    import workload

    wl = workload.SnarkWorkload(**SNARK_CASES[case])
    proof, rc = oracle.snark_prove(wl, workload.tape_seed())
    assert rc == 0
    assert hashlib.sha256(proof).hexdigest() == json.load(open(os.path.join(G, "snark_proofs.json")))[case]["proof_sha256"]
    assert oracle.snark_proof_reserialize(proof) == proof
    assert oracle.snark_proof_reserialize(proof[:-1]) is None
    assert oracle.snark_proof_reserialize(proof + b"\0") is None


@pytest.mark.parametrize("case", sorted(pm.SWEEP))
def test_typed_map_self_checks(oracle, case):
    """on the honest proof every pt field decodes, every sc field is canonical, and the spans tile the bytes"""
    import fieldref
    import workload
    from proof_layout import snark_dotlog_names, snark_proof_fields, snark_proof_fields_typed

    proof, _ = oracle.snark_prove(workload.SnarkWorkload(**SNARK_CASES[case]), workload.tape_seed())
    typed = snark_proof_fields_typed(proof)
    assert [t[:3] for t in typed] == snark_proof_fields(proof)
    at = 0
    for name, s, e, kind in typed:
        assert s == at and e - s == (8 if kind == "len" else 32), name
        at = e
        if kind == "pt":
            assert fieldref.decode(proof[s:e]) is not None, name
        elif kind == "sc":
            assert int.from_bytes(proof[s:e], "little") < fieldref.Q, name
        else:
            assert kind == "len", name
    assert at == len(proof)
    assert len({t[0] for t in typed}) == len(typed), "field names repeat"
    names = {t[0] for t in typed}
    for d in snark_dotlog_names(proof):
        assert {d + ".L.len", d + ".R.len", d + ".delta", d + ".beta", d + ".z1", d + ".z2"} <= names


def test_verify_bytes_verdicts_and_threads(oracle):
    """orc_snark_verify_bytes: accept, malformed, a point that does not decompress, and the same verdicts when
    called from several threads at once"""
    import workload
    from proof_layout import snark_proof_fields_typed

    wl = workload.SnarkWorkload(**SNARK_CASES[pm.SMALL])
    proof, _ = oracle.snark_prove(wl, workload.tape_seed())
    views = workload.SnarkViews(wl)
    assert oracle.snark_verify_bytes(views, proof) == 0
    assert oracle.snark_verify_bytes(views, proof[:-1]) == oracle.MALFORMED
    assert oracle.snark_verify_bytes(views, proof + b"\0") == oracle.MALFORMED
    assert oracle.snark_verify_bytes(views, proof, label=b"snark_other") > 0
    # the first point the verifier decompresses: round 0 of the block R1CSProof's first ZK sumcheck (sumcheck.rs:141)
    name, s, e, _ = next(t for t in snark_proof_fields_typed(proof)
                         if t[0] == "block_r1cs_sat_proof.sc_proof_phase1.comm_evals[0]")
    bad = pm.apply(proof, s, (1).to_bytes(32, "little"))  # odd: no ristretto255 encoding (RFC 9496 4.3.1)
    assert oracle.snark_verify_bytes(views, bad) == oracle.DECOMPRESSION, name
    variants = [proof, bad, proof[:-1], pm.apply(proof, len(proof) - 32, bytes(32))] * 2
    with ThreadPoolExecutor(max_workers=8) as pool:
        got = list(pool.map(lambda b: oracle.snark_verify_bytes(views, b), variants))
    assert got[:4] == got[4:] and got[:3] == [0, oracle.DECOMPRESSION, oracle.MALFORMED] and got[3] > 0, got
