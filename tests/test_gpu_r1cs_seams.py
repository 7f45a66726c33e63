"""The seams that carry R1CSProof::prove (src/r1csproof.rs:210-685) from z_mat to the polynomial openings on caller
tables, bit-exact against the oracle's own pieces of that prove (tests/r1cs_seams_ref.py): DensePolynomialPqx::new_rev
and bound_poly_vars_rq, the eval tables and prove_abc_gen, the p rounds of the phase-1 round seam, the two ZK sumcheck
provers with their verifier, and all of them chained with every intermediate left on the device."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import r1cs_cases
import r1cs_seams_ref as ref

pytestmark = pytest.mark.gpu

CASE_IDS = sorted(r1cs_cases.CASES) + ["p40_ragged_2secs", "p36_shared"]
ZERO = np.zeros(4, np.uint64)


def rand_fq(oracle, rng, n):
    if n == 0:
        return np.zeros((0, 4), np.uint64)
    return oracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * n, dtype=np.uint8).tobytes()).reshape(n, 4)


def workload_of(oracle, case, seed=1):
    """the case's R1CSWorkload with random matrix values instead of the synthetic circuit's ones, and its z_mat flat
    in (p, q, w, x) order"""
    import workload

    nc, npf, nws, shared = r1cs_cases.ALL_R1CS[case]
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    rng = np.random.default_rng(seed + len(case))
    for mats in wl.entries:
        for m in mats:
            m[:, 2:] = rand_fq(oracle, rng, m.shape[0])
    return wl, z_of(wl)


def z_of(wl):
    return np.concatenate([np.stack([wl.sections[w][p][q] for w in range(wl.nws)]).reshape(-1, 4)
                           for p in range(wl.P) for q in range(wl.num_proofs[p])])


def lgs(wl):
    """(lx, lq, lp, lw, ly): the variables of x (constraints), q, p, w (sections), y (inputs)"""
    return tuple((n - 1).bit_length() for n in (wl.max_num_cons, wl.max_num_proofs, wl.P, wl.nws, wl.max_num_inputs))


def cons_of(wl):
    return [wl.num_cons[0 if wl.shared else p] for p in range(wl.P)]


def npow2(n):
    return 1 << (n - 1).bit_length()


@pytest.fixture(scope="module")
def gens(ctx):
    import spg

    return spg.R1CSGens(ctx, ref.GENS_LABEL, ref.GENS_NV)


# ---- DensePolynomialPqx::new_rev, bound_poly_vars_rq

@pytest.mark.parametrize("case", CASE_IDS)
def test_new_rev_and_bound_rq(ctx, oracle, case):
    """new_rev from host scalars and from a device buffer at an offset, entry by entry with shape(); bound_rq of
    every prefix length equals repeated bound(.., 2) and the oracle's binds; one challenge too many is refused"""
    import spg

    wl, z = workload_of(oracle, case)
    shape = (wl.num_proofs, wl.max_num_proofs, wl.nws, wl.num_inputs, wl.max_num_inputs)
    want, sizes = ref.new_rev(z, *shape)
    assert want.any()
    pad = rand_fq(oracle, np.random.default_rng(2), 3)
    zbuf = spg.Buf(ctx, np.concatenate([pad, z, pad]))
    for T in (spg.Pqx.new_rev(ctx, z, *shape), spg.Pqx.new_rev(ctx, zbuf, *shape, offset=3)):
        assert np.array_equal(T.download(), want)
        assert T.shape() == sizes
    with pytest.raises(spg.SpgError):  # the shape's total reaches past the buffer
        spg.Pqx.new_rev(ctx, zbuf, *shape, offset=7)
    lq = lgs(wl)[1]
    rq = rand_fq(oracle, np.random.default_rng(3), lq + 1)
    for n in range(lq + 1):
        T = spg.Pqx.new_rev(ctx, zbuf, *shape, offset=3)
        T.bound_rq(rq[:n])
        S = spg.Pqx.new_rev(ctx, z, *shape)
        for k in range(n):
            S.bound(rq[k], 2)
        exp = oracle.pqx_bind(want, *shape, [2] * n, rq[:n])
        assert exp[0].any()
        assert np.array_equal(S.download(), exp[0])
        # (the one-pass forms rewrite the live rows alone: the rows past them, which nothing reads, keep their entries)
        live = live_mask(wl, exp[2])
        assert np.array_equal(T.download()[live], exp[0][live])
        assert T.shape() == S.shape() == tuple(exp[1:])
    T = spg.Pqx.new_rev(ctx, z, *shape)
    with pytest.raises(spg.SpgError):
        T.bound_rq(rq)
    assert np.array_equal(T.download(), want) and T.shape() == sizes


def live_mask(wl, num_proofs_now):
    """the allocated entries of a (p, q, w, x) table that lie in its live rows q < num_proofs_now[p]"""
    m = []
    for p in range(wl.P):
        row = wl.nws * wl.num_inputs[p]
        m += [True] * (num_proofs_now[p] * row) + [False] * ((wl.num_proofs[p] - num_proofs_now[p]) * row)
    return np.asarray(m)


# ---- compute_eval_table_sparse_disjoint_rounds, prove_abc_gen

def check_eval_tables(ctx, oracle, wl, seed):
    import spg
    import workload

    v = workload.CViews(wl)
    inst = spg.R1CSInst(ctx, v.inst)
    Pm, Y = len(wl.entries), wl.max_num_inputs
    rng = np.random.default_rng(seed)
    rx = rand_fq(oracle, rng, wl.max_num_cons)
    rs = rand_fq(oracle, rng, 3)
    erx = spg.Buf(ctx, rx)
    want = ref.eval_tables(v.inst, wl.nws, Y, wl.num_inputs, rx)
    assert want is not None and any(w.any() for w in want)
    got = spg.r1cs_eval_tables(ctx, inst, wl.P, wl.nws, Y, wl.num_inputs, erx)
    dims = (npow2(Pm), 1, npow2(wl.nws), Y)
    for T, W in zip(got, want):
        assert np.array_equal(T.download(), W)
        assert T.shape() == (dims, [1] * Pm, list(wl.num_inputs[:Pm]))
    want_abc, sizes = ref.abc_poly(v.inst, wl.P, wl.nws, Y, wl.num_inputs, rx, *rs)
    abc = spg.r1cs_abc_poly(ctx, inst, wl.P, wl.nws, Y, wl.num_inputs, erx, *rs)
    assert want_abc.any() and np.array_equal(abc.download(), want_abc) and abc.shape() == sizes
    # .. and on the device results alone: (r_A A + r_B B + r_C C) of the three tables put through new_rev
    comb = None
    for r, T in zip(rs, got):
        term = oracle.fq_op("mul", np.repeat(r.reshape(1, 4), T.n, axis=0), T.download())
        comb = term if comb is None else oracle.fq_op("add", comb, term)
    rev = spg.Pqx.new_rev(ctx, comb, [1] * Pm, 1, wl.nws, wl.num_inputs[:Pm], Y)
    assert np.array_equal(rev.download(), abc.download())


@pytest.mark.parametrize("case", CASE_IDS)
def test_eval_tables_match_oracle(ctx, oracle, case):
    wl, _ = workload_of(oracle, case)
    check_eval_tables(ctx, oracle, wl, 11)


def column_split(seed=13):
    """matrices whose column distributions differ between A, B and C of one instance and between instances: A_0 in
    section 0 only, B_0 in the last section only, C_0 on odd columns; instance 1 the other way round with A_1 empty"""
    import sparse_cases
    import workload

    wl = workload.R1CSWorkload([32, 16], [2, 2], num_sections=3)
    rng = np.random.default_rng(seed)
    Y = wl.max_num_inputs

    def cols(p, kind):
        allc = [w * Y + i for w in range(wl.nws) for i in range(wl.num_inputs[p])]
        return {"first": [c for c in allc if c // Y == 0], "last": [c for c in allc if c // Y == wl.nws - 1],
                "odd": [c for c in allc if c % 2]}[kind]

    plan = [[("first", 90), ("last", 41), ("odd", 64)], [("odd", 0), ("first", 70), ("last", 9)]]
    wl.entries = [[sparse_cases._matrix(rng, n, wl.num_cons[p], cols(p, kind)) for kind, n in plan[p]]
                  for p in range(wl.P)]
    return wl


@pytest.mark.parametrize("case", ["ragged_p2_x64", "tiled_p2_x256", "shared_p3_x32", "below_cells_x256", "column_split"])
def test_eval_tables_on_structured_matrices(ctx, oracle, case):
    """nnz 0 and 1, hot rows and columns, duplicate (row, col) entries, shuffled entry lists (tests/sparse_cases.py),
    and column distributions that differ between the matrices of one instance and between instances"""
    import sparse_cases

    wl = column_split() if case == "column_split" else sparse_cases.structured(case)
    check_eval_tables(ctx, oracle, wl, 17)


def test_eval_tables_reject_bad_arguments(ctx, oracle):
    import spg
    import workload

    wl, _ = workload_of(oracle, "p3_ragged_3secs")
    inst = spg.R1CSInst(ctx, workload.CViews(wl).inst)
    Y = wl.max_num_inputs
    erx = spg.Buf(ctx, rand_fq(oracle, np.random.default_rng(1), wl.max_num_cons))
    short = spg.Buf(ctx, rand_fq(oracle, np.random.default_rng(1), wl.max_num_cons - 1))
    r = rand_fq(oracle, np.random.default_rng(2), 3)
    bad = [
        dict(num_instances=2),                    # 2 instances against a 3-instance matrix list
        dict(max_num_inputs=Y // 2),              # next_pow2(nws) max_num_inputs != num_vars
        dict(num_witness_secs=1),                 # likewise
        dict(evals_rx=short),                     # |evals_rx| < max_num_cons
        dict(num_witness_secs=9),                 # 9 sections
        dict(num_inputs=[Y, 3, 4]),               # not a power of two
    ]
    for b in bad:
        a = dict(num_instances=wl.P, num_witness_secs=wl.nws, max_num_inputs=Y, num_inputs=wl.num_inputs, evals_rx=erx)
        a.update(b)
        args = (ctx, inst, a["num_instances"], a["num_witness_secs"], a["max_num_inputs"], a["num_inputs"], a["evals_rx"])
        with pytest.raises(spg.SpgError):
            spg.r1cs_eval_tables(*args)
        with pytest.raises(spg.SpgError):
            spg.r1cs_abc_poly(*args, *r)


# ---- the p rounds of spg_phase1_round_evals

@pytest.mark.parametrize("case", CASE_IDS)
def test_phase1_round_walk_with_p_rounds(ctx, oracle, case):
    """every x round, every q round, then every p round on Az, Bz, Cz from the SpMV seam: (e0, e2, e3) against the
    oracle's phase1_round_evals, the eq vectors and tables bound through the seams between rounds; mode 1 before x
    and q are bound is refused"""
    import spg
    import workload

    wl, z = workload_of(oracle, case)
    inst = spg.R1CSInst(ctx, workload.CViews(wl).inst)
    tabs = spg.r1cs_multiply_vec_block(ctx, inst, wl.num_proofs, wl.max_num_proofs, wl.num_inputs, wl.max_num_inputs,
                                       wl.nws, z)
    lx, lq, lp, _, _ = lgs(wl)
    rng = np.random.default_rng(77)
    Ap, Aq, Ax = (spg.Buf(ctx, rand_fq(oracle, rng, 1 << n)) for n in (lp, lq, lx))
    modes = [4] * lx + [2] * lq + [1] * lp
    seen = False
    for j, mode in enumerate(modes):
        if mode != 1 and lp:
            with pytest.raises(spg.SpgError):
                spg.phase1_round_evals(Ap, Aq, Ax, *tabs, 1)
        got = spg.phase1_round_evals(Ap, Aq, Ax, *tabs, mode)
        want = ref.phase1_round(mode, Ap.download(), Aq.download(), Ax.download(), [T.download() for T in tabs],
                                wl.num_proofs, cons_of(wl), tabs[0].shape())
        seen = seen or want.any()
        assert np.array_equal(got, want), (j, mode)
        r = rand_fq(oracle, rng, 1)[0]
        {4: Ax, 2: Aq, 1: Ap}[mode].bound_top(r)
        for T in tabs:
            T.bound(r, mode)
    assert seen
    assert (Ap.n, Aq.n, Ax.n) == (1, 1, 1)
    with pytest.raises(spg.SpgError):  # no p variable left
        spg.phase1_round_evals(Ap, Aq, Ax, *tabs, 1)


# ---- the two ZK sumcheck provers

def run_provers(ctx, gens, oracle, case, small_cap=False):
    """zk_phase1_prove on the SpMV seam's tables (random eq vectors), then zk_phase2_prove on abc_poly and new_rev(z)
    bound at random rq, each on a fresh transcript and tape. Returns (device results, oracle results) per phase."""
    import spg
    import workload

    wl, z = workload_of(oracle, case)
    v = workload.CViews(wl)
    inst = spg.R1CSInst(ctx, v.inst)
    seed = workload.tape_seed()
    lx, lq, lp, lw, ly = lgs(wl)
    Y = wl.max_num_inputs
    single = len(wl.entries) == 1
    rng = np.random.default_rng(31)
    out = []

    # phase 1
    eqs = [rand_fq(oracle, rng, 1 << n) for n in (lp, lq, lx)]
    tabs = spg.r1cs_multiply_vec_block(ctx, inst, wl.num_proofs, wl.max_num_proofs, wl.num_inputs, Y, wl.nws, z)
    before = [T.download() for T in tabs]
    want = ref.phase1(b"seam_p1", seed, lx, lq, lp, *eqs, wl.num_proofs, cons_of(wl), *before)
    bufs = [spg.Buf(ctx, e) for e in eqs]
    t, tape = spg.Transcript(b"seam_p1"), spg.RandomTape(b"proof", seed)
    if small_cap:
        with pytest.raises(spg.SpgError):
            spg.zk_phase1_prove(ctx, gens, lx, lq, lp, *bufs, *tabs, t, tape, cap=ref.zk_len(lx + lq + lp) - 1)
        assert ctx.last_len == ref.zk_len(lx + lq + lp)
        for b, e in zip(bufs, eqs):
            b.n = e.shape[0]  # (the wrapper's own lengths; the native vectors did not move)
        assert all(np.array_equal(T.download(), b) for T, b in zip(tabs, before))
        assert all(np.array_equal(b.download(), e) for b, e in zip(bufs, eqs))
        probe = spg.Transcript(b"seam_p1")
        assert np.array_equal(spg.Transcript(b"seam_p1").challenge_scalar(b"probe"), probe.challenge_scalar(b"probe"))
    proof, r, claims, blind = spg.zk_phase1_prove(ctx, gens, lx, lq, lp, *bufs, *tabs, t, tape)
    got = dict(proof=proof, r=r, claims=claims, blind=blind, tabs=[T.download() for T in tabs],
               shapes=[T.shape() for T in tabs], eq=[b.download() for b in bufs],
               check=t.challenge_bytes(b"seam_check", 64), tape_next=tape.random_scalar(b"seam_next"))
    out.append((got, want))

    # phase 2
    rx = rand_fq(oracle, rng, wl.max_num_cons)
    rs = rand_fq(oracle, rng, 3)
    claim, bl = rand_fq(oracle, rng, 2)
    rq = rand_fq(oracle, rng, lq)
    eq = rand_fq(oracle, rng, 1 << lp)
    abc_flat, (_, _, abc_ni) = ref.abc_poly(v.inst, wl.P, wl.nws, Y, wl.num_inputs, rx, *rs)
    want = ref.phase2(b"seam_p2", seed, claim, bl, ly, lw, lp, single, wl.nws, eq, abc_ni, abc_flat, wl.num_proofs,
                      wl.max_num_proofs, wl.num_inputs, z, rq)
    ABC = spg.r1cs_abc_poly(ctx, inst, wl.P, wl.nws, Y, wl.num_inputs, spg.Buf(ctx, rx), *rs)
    Z = spg.Pqx.new_rev(ctx, z, wl.num_proofs, wl.max_num_proofs, wl.nws, wl.num_inputs, Y)
    Z.bound_rq(rq)
    eqb = spg.Buf(ctx, eq)
    t, tape = spg.Transcript(b"seam_p2"), spg.RandomTape(b"proof", seed)
    if small_cap:
        za = Z.download(), ABC.download()
        with pytest.raises(spg.SpgError):
            spg.zk_phase2_prove(ctx, gens, ly, lw, lp, single, wl.nws, eqb, ABC, Z, t, tape, claim=claim, blind_claim=bl,
                                cap=0)
        assert ctx.last_len == ref.zk_len(ly + lw + lp)
        eqb.n = eq.shape[0]
        assert np.array_equal(Z.download(), za[0]) and np.array_equal(ABC.download(), za[1])
        assert np.array_equal(eqb.download(), eq)
    proof, r, claims, blind = spg.zk_phase2_prove(ctx, gens, ly, lw, lp, single, wl.nws, eqb, ABC, Z, t, tape,
                                                  claim=claim, blind_claim=bl)
    got = dict(proof=proof, r=r, claims=claims, blind=blind, tabs=[ABC.download(), Z.download()],
               shapes=[ABC.shape(), Z.shape()], eq=[eqb.download()], check=t.challenge_bytes(b"seam_check", 64),
               tape_next=tape.random_scalar(b"seam_next"), live=live_mask(wl, [1] * wl.P), claim=claim, blind_claim=bl)
    out.append((got, want))
    return out


def digest(got):
    h = hashlib.sha256()
    for k in ("proof", "check"):
        h.update(got[k])
    for k in ("r", "claims", "blind", "tape_next"):
        h.update(np.ascontiguousarray(got[k]).tobytes())
    return h.hexdigest()


def compare_provers(res):
    (g1, w1), (g2, w2) = res
    assert w1["claims"].any() and w2["claims"].any() and len(w1["proof"]) > 24
    for g, w in ((g1, w1), (g2, w2)):
        assert g["proof"] == w["proof"]
        assert np.array_equal(g["r"], w["r"]) and np.array_equal(g["claims"], w["claims"])
        assert np.array_equal(g["blind"], w["blind"])
        assert g["check"] == w["check"] and np.array_equal(g["tape_next"], w["tape_next"])
        assert all(e.shape[0] == 1 for e in g["eq"])
    for T, W, s in zip(g1["tabs"], (w1["B"], w1["C"], w1["D"]), g1["shapes"]):
        assert np.array_equal(T, W) and s == w1["sizes"]
    assert np.array_equal(g1["claims"][0], ref_product(w1["eq3"])) and all(
        np.array_equal(e[0], x) for e, x in zip(g1["eq"], w1["eq3"]))
    assert np.array_equal(g2["tabs"][0], w2["ABC"]) and g2["shapes"][0] == w2["sizes_abc"]
    live = g2["live"]  # (Z's rows past the first keep whatever the q folds left there)
    assert np.array_equal(g2["tabs"][1][live], w2["Z"][live]) and g2["shapes"][1] == w2["sizes_z"]
    assert np.array_equal(g2["eq"][0][0], w2["eq0"])


def ref_product(eq3):
    import pyoracle

    return pyoracle.fq_op("mul", pyoracle.fq_op("mul", eq3[0].reshape(1, 4), eq3[1].reshape(1, 4)),
                          eq3[2].reshape(1, 4))[0]


@pytest.mark.parametrize("case", CASE_IDS)
def test_zk_provers_match_oracle(ctx, gens, oracle, case):
    """proof bytes, r, claims, blind, the bound tables and eq vectors, the transcript check and the next tape scalar;
    a cap one byte short sets *len and moves nothing (the run that follows reuses the same transcript, tape, tables)"""
    compare_provers(run_provers(ctx, gens, oracle, case, small_cap=True))


@pytest.mark.parametrize("case", ["p3_ragged_3secs", "p5_q1"])
def test_zk_provers_without_tape_ahead(oracle, case):
    """SPG_TAPE_AHEAD=0 in a fresh process (every round draws d_vec, r_delta, r_beta itself and commits its own
    points): the same bytes, challenges, claims, transcript state and tape position as the oracle's"""
    import pyoracle  # noqa: F401  (the oracle is built)

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys; sys.path[:0] = [%r, %r, %r]\n"
        "import spg, pyoracle\n"
        "import r1cs_seams_ref as ref\n"
        "import test_gpu_r1cs_seams as m\n"
        "ctx = spg.Context(0)\n"
        "res = m.run_provers(ctx, spg.R1CSGens(ctx, ref.GENS_LABEL, ref.GENS_NV), pyoracle, %r)\n"
        "m.compare_provers(res)\n"
        "print('ok', m.digest(res[0][0]), m.digest(res[1][0]))\n"
    ) % (os.path.join(root, "spartan-parallel_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests"), case)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPG_TAPE_AHEAD="0"), capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-3] == "ok"


def test_zk_provers_reject_bad_arguments(ctx, gens, oracle):
    """zero rounds, bound tables, eq vectors of the wrong length: refused before anything moves"""
    import spg

    rng = np.random.default_rng(5)
    one = [spg.Buf(ctx, rand_fq(oracle, rng, 1)) for _ in range(3)]
    tabs = [spg.Pqx(ctx, rand_fq(oracle, rng, 1), [1], 1, 1, [1], 1) for _ in range(3)]
    t, tape = spg.Transcript(b"x"), spg.RandomTape(b"proof", ZERO)
    with pytest.raises(spg.SpgError):  # no round: the reference would index blinds_evals[-1]
        spg.zk_phase1_prove(ctx, gens, 0, 0, 0, *one, *tabs, t, tape)
    with pytest.raises(spg.SpgError):
        spg.zk_phase2_prove(ctx, gens, 0, 0, 0, True, 1, one[0], tabs[0], tabs[1], t, tape)
    z = rand_fq(oracle, rng, 2 * 4 * 8)
    tabs = [spg.Pqx(ctx, z, [4, 4], 4, 1, [8, 8], 8) for _ in range(3)]
    eqs = [spg.Buf(ctx, rand_fq(oracle, rng, n)) for n in (2, 4, 8)]
    with pytest.raises(spg.SpgError):  # |Ax| != 2^nx
        spg.zk_phase1_prove(ctx, gens, 2, 2, 1, *eqs, *tabs, t, tape)
    tabs[1].bound(z[0], 4)
    with pytest.raises(spg.SpgError):  # C already bound once
        spg.zk_phase1_prove(ctx, gens, 3, 2, 1, *eqs, *tabs, t, tape)
    assert np.array_equal(t.challenge_scalar(b"probe"), spg.Transcript(b"x").challenge_scalar(b"probe"))
    assert np.array_equal(tape.random_scalar(b"probe"), spg.RandomTape(b"proof", ZERO).random_scalar(b"probe"))


# ---- ZKSumcheckInstanceProof::verify

def tampered(proof, rounds):
    """(name, bytes, round count): one flipped bit in each field class, wrong round counts, cut and padded bytes"""
    dp = 24 + 64 * rounds  # the first DotProductProof: delta, beta, len(z), z[4], z_delta, z_beta
    spots = {"comm_polys": 8 + 32 * (rounds - 1), "comm_evals": 16 + 32 * rounds, "dp_delta": dp, "dp_beta": dp + 32,
             "dp_z": dp + 72 + 64, "dp_z_delta": dp + 200, "dp_z_beta": dp + 232,
             "last_dp_z_beta": len(proof) - 32}
    out = []
    for name, o in spots.items():
        b = bytearray(proof)
        b[o] ^= 1
        out.append((name, bytes(b), rounds))
    b = bytearray(proof)
    b[dp + 64] ^= 1  # the Vec length of z: 5
    out += [("dp_z_len", bytes(b), rounds), ("rounds+1", proof, rounds + 1), ("cut", proof[:-1], rounds),
            ("cut_round", proof[:-264], rounds), ("trailing", proof + b"\0", rounds), ("empty", b"", rounds)]
    if rounds > 1:
        out.append(("rounds-1", proof, rounds - 1))
    return out


@pytest.mark.parametrize("case", ["p3_ragged_3secs", "p1_x32", "p5_q1"])
def test_zk_sumcheck_verify(ctx, gens, oracle, case):
    """accepts the provers' bytes with the helper's comm_claim_post and r and ends in the prover's transcript state;
    every tampering gets the helper's verdict (rejected)"""
    import spg

    res = run_provers(ctx, gens, oracle, case)
    for (got, want), label, cc in ((res[0], b"seam_p1", ref.commit1(ZERO, ZERO)), (res[1], b"seam_p2", None)):
        rounds = got["r"].shape[0]
        if cc is None:
            cc = ref.commit1(got["claim"], got["blind_claim"])
        w_ok, w_post, w_r, w_check = ref.verify(label, cc, rounds, got["proof"])
        t = spg.Transcript(label)
        ok, post, r, why = spg.zk_sumcheck_verify(ctx, gens, cc, rounds, t, got["proof"])
        assert ok and w_ok, why
        assert post == w_post and np.array_equal(r, w_r) and np.array_equal(r, got["r"])
        assert t.challenge_bytes(b"seam_check", 64) == w_check == got["check"]
        for name, bad, n in tampered(got["proof"], rounds):
            ok, _, _, _ = spg.zk_sumcheck_verify(ctx, gens, cc, n, spg.Transcript(label), bad)
            assert ok == ref.verify(label, cc, n, bad)[0] and not ok, name
        wrong = ref.commit1(np.array([1, 0, 0, 0], np.uint64), ZERO)
        ok, _, _, _ = spg.zk_sumcheck_verify(ctx, gens, wrong, rounds, spg.Transcript(label), got["proof"])
        assert ok == ref.verify(label, wrong, rounds, got["proof"])[0] and not ok
        with pytest.raises(spg.SpgError):  # both call sites pass 3; gens_4 has 4 points
            spg.zk_sumcheck_verify(ctx, gens, cc, rounds, spg.Transcript(label), got["proof"], degree_bound=2)


# ---- the chain

@pytest.mark.parametrize("case", CASE_IDS)
def test_chain_matches_oracle(ctx, gens, oracle, case):
    """multiply_vec_block, phase 1, r_A r_B r_C from the same transcript, eq(rx), abc_poly, new_rev(z), bound_rq,
    eq(rp), phase 2, every table left on the device between the calls: both proofs, the phase-2 claims, the final
    transcript check and the tape position equal the oracle's same walk. Fails if two seams disagree about a layout."""
    import spg
    import workload

    wl, z = workload_of(oracle, case)
    v = workload.CViews(wl)
    seed = workload.tape_seed()
    w_p1, w_p2, w_claims, w_check, w_next = ref.chain(v.inst, wl, z, b"seam_chain", seed)
    assert w_claims.any()
    lx, lq, lp, lw, ly = lgs(wl)
    Y = wl.max_num_inputs
    inst = spg.R1CSInst(ctx, v.inst)
    t, tape = spg.Transcript(b"seam_chain"), spg.RandomTape(b"proof", seed)
    taus = [[t.challenge_scalar(lab) for _ in range(n)]
            for lab, n in ((b"challenge_tau_p", lp), (b"challenge_tau_q", lq), (b"challenge_tau_x", lx))]
    Ap, Aq, Ax = (spg.Buf.eq_evals(ctx, tau) for tau in taus)
    zbuf = spg.Buf(ctx, z)
    tabs = spg.r1cs_multiply_vec_block(ctx, inst, wl.num_proofs, wl.max_num_proofs, wl.num_inputs, Y, wl.nws, z)
    p1, r1, claims1, _ = spg.zk_phase1_prove(ctx, gens, lx, lq, lp, Ap, Aq, Ax, *tabs, t, tape)
    rA, rB, rC = (t.challenge_scalar(lab) for lab in (b"challenge_Az", b"challenge_Bz", b"challenge_Cz"))
    claim2 = None
    for r, c in zip((rA, rB, rC), claims1[1:]):
        term = oracle.fq_op("mul", r.reshape(1, 4), c.reshape(1, 4))
        claim2 = term if claim2 is None else oracle.fq_op("add", claim2, term)
    rx, rq_rev, rp = r1[:lx][::-1], r1[lx:lx + lq], r1[lx + lq:]
    ABC = spg.r1cs_abc_poly(ctx, inst, wl.P, wl.nws, Y, wl.num_inputs, spg.Buf.eq_evals(ctx, rx), rA, rB, rC)
    Z = spg.Pqx.new_rev(ctx, zbuf, wl.num_proofs, wl.max_num_proofs, wl.nws, wl.num_inputs, Y)
    Z.bound_rq(rq_rev)
    eq_p = spg.Buf.eq_evals(ctx, rp)
    p2, _, claims2, _ = spg.zk_phase2_prove(ctx, gens, ly, lw, lp, len(wl.entries) == 1, wl.nws, eq_p, ABC, Z, t, tape,
                                            claim=claim2[0])
    assert p1 == w_p1 and p2 == w_p2
    assert np.array_equal(claims2, w_claims)
    assert t.challenge_bytes(b"seam_check", 64) == w_check
    assert np.array_equal(tape.random_scalar(b"seam_next"), w_next)
