"""The verifiers' deferred mode (spg_set_verify_device): the sigma-protocol group equations collected and checked in
one spg_eqs_check launch at the end of the call. On one context and the same proof bytes the verdict and the text of
spg_last_error are those of the default (eager) mode for every input: accepted proofs, one flipped bit per field pick
(the selection of tests/test_gpu_verify.py::test_verify_rejects_altered_fields), truncated and extended bytes, parts
exchanged (test_verify_rejects_swapped_parts), and one proof each through spg_r1cs_verify and spg_poly_eval_verify. The
profile scope of the launch pins "one launch": none in eager mode, exactly one for an accepted proof in deferred mode."""
import pytest

from test_gpu_verify import Program, vars_gens  # noqa: F401  (the module's generator fixture)

pytestmark = pytest.mark.gpu

SWAPS = [("io_proof.proofs[0]", "io_proof.proofs[1]"),
         ("shift_proof.C_orig_evals[0]", "shift_proof.C_orig_evals[1]"),
         ("block_r1cs_eval_proof_list[0].dotp_left[0]", "block_r1cs_eval_proof_list[0].dotp_right[0]")]


def both_modes(ctx, verify):
    """(eager result, deferred result) of one verification, the context left in eager mode"""
    try:
        ctx.set_verify_device(False)
        eager = verify()
        ctx.set_verify_device(True)
        deferred = verify()
    finally:
        ctx.set_verify_device(False)
    return eager, deferred


def swapped(proof, a, b):
    from proof_layout import snark_proof_fields

    spans = {}
    for name, s, e in snark_proof_fields(proof):
        for want in (a, b):
            if name == want or name.startswith(want + "."):
                lo, hi = spans.get(want, (s, e))
                spans[want] = (min(lo, s), max(hi, e))
    (sa, ea), (sb, eb) = spans[a], spans[b]
    assert ea - sa == eb - sb and ea <= sb
    return proof[:sa] + proof[sb:eb] + proof[ea:sb] + proof[sa:ea] + proof[eb:]


@pytest.mark.parametrize("case", ["b2_x32_q2", "mem_both_b3_x64_q2"])
def test_snark_verdicts_and_texts_equal_eager(ctx, vars_gens, case):  # noqa: F811
    from proof_layout import snark_proof_fields

    prog = Program(ctx, vars_gens, case)
    eager, deferred = both_modes(ctx, prog.verify)
    assert eager[0] and deferred[0], (eager, deferred)
    fields = snark_proof_fields(prog.proof)
    step = max(1, len(fields) // 48)
    picked = fields[::step] + [f for f in fields if f[0].endswith(".len")][:8]
    variants = []
    for name, s, e in picked:
        bad = bytearray(prog.proof)
        bad[s + (e - s) // 2] ^= 0x04
        variants.append((name, bytes(bad)))
    variants += [("truncated", prog.proof[:-1]), ("extended", prog.proof + b"\x00")]
    variants += [("swap %s" % a, swapped(prog.proof, a, b)) for a, b in SWAPS]
    texts = set()
    for name, proof in variants:
        eager, deferred = both_modes(ctx, lambda: prog.verify(proof))
        assert not eager[0], name
        assert deferred == eager, (name, eager, deferred)
        texts.add(eager[1])
    assert len(texts) >= 4, texts  # the picks reach several different checks


def test_one_launch_per_accepted_proof(ctx, vars_gens):  # noqa: F811
    """eager mode never reaches the launch; deferred mode reaches it once per accepted proof, with the equations and
    terms of the whole proof in it"""
    prog = Program(ctx, vars_gens, "b2_x32_q2")
    ctx.prof_enable(True)
    try:
        ctx.prof_read()
        ctx.set_verify_device(False)
        assert prog.verify()[0]
        assert "eqs_check" not in ctx.prof_read()
        ctx.set_verify_device(True)
        assert prog.verify()[0]
        assert ctx.prof_read()["eqs_check"][0] == 1
        E, T = ctx.eqs_last_counts()
        assert E > 50 and T > 4 * E, (E, T)
    finally:
        ctx.set_verify_device(False)
        ctx.prof_enable(False)


def test_r1cs_verify_equals_eager(ctx):
    import spg
    import workload
    from r1cs_cases import CASES
    from test_gpu_r1cs import GENS_LABEL, GENS_NV, _eq_table, _int, gpu_prove

    gens = spg.R1CSGens(ctx, GENS_LABEL, GENS_NV)
    nc, npf, nws, shared = CASES[sorted(CASES)[0]]
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    proof, ch = gpu_prove(ctx, gens, wl, workload.tape_seed())
    rp, rx, rwry = ch[0], ch[2], ch[3]
    v = workload.CViews(wl)
    ev = spg.r1cs_multi_evaluate(ctx, spg.R1CSInst(ctx, v.inst), len(wl.entries), rx, rwry)
    eq = _eq_table([_int(x) for x in rp])
    if len(wl.entries) == 1:
        bound = [_int(ev[k]) for k in range(3)]
    else:
        bound = [sum(eq[p] * _int(ev[3 * p + k]) for p in range(wl.P)) % workload.Q for k in range(3)]
    sections = []
    for w in range(wl.nws):
        mats = wl.sections[w]
        sections.append(([m.shape[0] for m in mats], [m.shape[1] for m in mats],
                         [spg.r1cs_gens_commit(ctx, gens, m.reshape(-1, 4)) for m in mats]))
    args = (ctx, gens, wl.P, wl.max_num_proofs, wl.num_proofs, wl.max_num_inputs, sections, wl.max_num_cons,
            workload.to_mont_limbs(bound))

    def verify(p):
        ok, why, _ = spg.r1cs_verify(*args, spg.Transcript(b"r1cs_test"), p)
        return ok, why

    eager, deferred = both_modes(ctx, lambda: verify(proof))
    assert eager[0] and deferred[0], (eager, deferred)
    for at in (len(proof) // 3, len(proof) // 2, len(proof) - 40):
        bad = bytearray(proof)
        bad[at] ^= 0x04
        eager, deferred = both_modes(ctx, lambda: verify(bytes(bad)))
        assert not eager[0] and deferred == eager, (at, eager, deferred)


def test_poly_eval_verify_equals_eager(ctx):
    import spg
    import workload

    import polyeval_cases as pc

    LABEL, TLABEL = b"gens_polyeval_test", b"polyeval_test"  # those of tests/test_gpu_polyeval.py
    nv = 10
    g = spg.PolyGens(ctx, LABEL, 12)
    Z, r = pc.scalars(100 + nv, 1 << nv), pc.scalars(200 + nv, nv)
    Zr = pc.evaluate(Z, r, nv)
    buf = spg.Buf(ctx, Z)
    proof, czr = spg.poly_eval_prove(ctx, g, buf, r, Zr, spg.Transcript(TLABEL),
                                     spg.RandomTape(b"proof", workload.tape_seed()))
    comm = spg.poly_commit(ctx, g, buf, nv)
    buf.free()

    def verify(p):
        return tuple(spg.poly_eval_verify(ctx, g, r, czr, comm, spg.Transcript(TLABEL), p))

    eager, deferred = both_modes(ctx, lambda: verify(proof))
    assert eager[0] and deferred[0], (eager, deferred)
    for at in (20, len(proof) // 2, len(proof) - 20):
        bad = bytearray(proof)
        bad[at] ^= 0x04
        eager, deferred = both_modes(ctx, lambda: verify(bytes(bad)))
        assert not eager[0] and deferred == eager, (at, eager, deferred)
    g.free()
