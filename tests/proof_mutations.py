"""Well-formed alterations of bincode(SNARK): every `pt` / `sc` field of the typed map (tests/proof_layout.py)
replaced by another valid value, so that the altered proof parses, every point decompresses and every scalar is
canonical, and only a check of the verifier can tell it from the honest one. Deterministic, no RNG.

  inc    sc: the stored 256-bit integer v -> (v + 1) mod q (the Montgomery limbs of another residue, still < q)
         pt: encode(decode(P) + B), B the ristretto255 basepoint (a valid encoding of another point)
  zero   sigma-protocol fields only (SIGMA_ROWS and the commitments of the same protocols): sc -> 0, pt -> the
         identity's encoding (32 zero bytes); left out where the honest value already is that

Shared by the oracle sweep (tests/test_oracle_snark_mutations.py, tests/golden/make_golden.py mutations) and the
product verifier's parity tests (tests/test_gpu_verify_mutations.py). Nothing here imports the product."""
import re

import fieldref
from proof_layout import snark_dotlog_names, snark_proof_fields_typed

BASEPOINT = fieldref.decode(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"))
assert BASEPOINT is not None and fieldref.on_curve(BASEPOINT)

# The two programs of the sweep (tests/r1cs_cases.py SNARK_CASES). The small one has every field swept; the memory
# program only the parts that are empty or shorter in the small one, by these name prefixes (1 210 pt / sc fields
# of its 3 630: 56 addr_comm_*, 104 {init_,}{phy,vir}_mem*_comm_*, 880 pairwise_check_*, 14 + 60 of the permutation
# product and 96 shift_proof.*; tests/test_oracle_snark_mutations.py pins the counts).
SMALL, MEM = "b2_x32_q2", "mem_both_b3_x64_q2"
MEM_PREFIXES = ("addr_comm_", "init_phy_mem_comm_", "init_vir_mem_comm_", "phy_mem_addr_comm_", "vir_mem_addr_comm_",
                "pairwise_check_", "perm_poly_poly_list", "proof_eval_perm_poly_prod_list", "shift_proof.")
SWEEP_FIELDS = {SMALL: 2332, MEM: 1210}  # pt / sc fields swept per case
SWEEP = {SMALL: None, MEM: MEM_PREFIXES}

# response scalars of the sigma protocols: never appended to the transcript, so exactly one check of the verifier
# binds each, and its rejection must name that check (row name -> (field pattern, the text))
_R1CS = r"(block|pairwise_check|perm_root)_r1cs_sat_proof\."
SIGMA_ROWS = {
    "KnowledgeProof": (re.compile(_R1CS + r"pok_Cz_claim\.z[12]$"), "KnowledgeProof"),
    "ProductProof": (re.compile(_R1CS + r"proof_prod\.z[0-4]$"), "ProductProof"),
    "EqualityProof": (re.compile(_R1CS + r"proof_eq_sc_phase[12]\.z$"), "EqualityProof"),
    "DotProductProof": (re.compile(_R1CS + r"sc_proof_phase[12]\.proofs\[\d+\]\.(z\[\d+\]|z_delta|z_beta)$"),
                        "DotProductProof"),
    # .z1 / .z2 of a DotProductProofLog record; the records are those of the typed map (sigma_row)
    "DotProductProofLog": (re.compile(r"\.z[12]$"), "DotProductProofLog"),
}
# the commitment side of the same protocols goes through the transcript: the `zero` kind is applied, only the verdict
# is compared
_SIGMA_COMMIT = re.compile(_R1CS + r"(pok_Cz_claim\.alpha|proof_prod\.(alpha|beta|delta)|proof_eq_sc_phase[12]\.alpha|"
                           r"sc_proof_phase[12]\.(comm_polys\[\d+\]|comm_evals\[\d+\]|proofs\[\d+\]\.(delta|beta)))$")


def part_of(name):
    """the top-level field of bincode(SNARK) a field belongs to"""
    return re.split(r"[.\[]", name, maxsplit=1)[0]


def sigma_row(name, dotlogs):
    """the SIGMA_ROWS key whose check alone binds this field, or None"""
    for row in ("KnowledgeProof", "ProductProof", "EqualityProof", "DotProductProof"):
        if SIGMA_ROWS[row][0].match(name):
            return row
    if name[-3:] in (".z1", ".z2") and name[:-3] in dotlogs:
        return "DotProductProofLog"
    return None


def _is_sigma(name, dotlogs):
    if sigma_row(name, dotlogs) or _SIGMA_COMMIT.match(name):
        return True
    head, _, leaf = name.rpartition(".")
    if leaf in ("delta", "beta"):
        return head in dotlogs
    m = re.match(r"(.*)\.[LR]\[\d+\]$", name)
    return bool(m and m.group(1) in dotlogs)


def mutate_value(raw, kind, how):
    """the replacement of one field's 32 bytes, or None where the `zero` kind would not change it"""
    if how == "zero":
        return None if raw == bytes(32) else bytes(32)
    assert how == "inc"
    if kind == "sc":
        v = int.from_bytes(raw, "little")
        assert v < fieldref.Q
        return ((v + 1) % fieldref.Q).to_bytes(32, "little")
    p = fieldref.decode(raw)
    assert p is not None
    out = fieldref.encode(fieldref.pt_add(p, BASEPOINT))
    assert out != raw
    return out


def mutations(proof, prefixes=None):
    """[(key, name, how, start, replacement)] of every (field, mutation) of the sweep over `proof`, in field order;
    key = "<field>|<how>". prefixes: only the fields whose name starts with one of them."""
    dotlogs = set(snark_dotlog_names(proof))
    out = []
    for name, s, e, kind in snark_proof_fields_typed(proof):
        if kind == "len" or (prefixes is not None and not name.startswith(prefixes)):
            continue
        for how in ("inc", "zero") if _is_sigma(name, dotlogs) else ("inc",):
            new = mutate_value(proof[s:e], kind, how)
            if new is not None:
                out.append((f"{name}|{how}", name, how, s, new))
    return out


def apply(proof, start, replacement):
    return proof[:start] + replacement + proof[start + len(replacement):]


def chunks(keys, size=64):
    """{"<part>#<k>": [keys]}: the keys of one case by top-level proof part, parts of more than `size` keys split in
    runs of `size`, so that one test item stays short whatever the proof's shape"""
    by_part = {}
    for k in keys:
        by_part.setdefault(part_of(k.split("|")[0]), []).append(k)
    out = {}
    for part, ks in by_part.items():
        for i in range(0, len(ks), size):
            out[f"{part}#{i // size}"] = ks[i:i + size]
    return out
