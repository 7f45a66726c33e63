"""The dense polynomial commitment seam on the device (include/spg.h spg_poly_*, csrc/polyeval.hip): generators,
Hyrax row commitments, single and batched evaluation proofs of polynomials resident in HBM, bytes against the tests'
checker (tests/polyeval_ref.py over the oracle's headers) under the same labels and tape seed, with the positions the
prover leaves transcript and tape in; the verifiers on those proofs and on damaged ones; the argument errors.

Sizes: num_vars 1, 3, 4 are the smallest odd and even splits (L = 1 at 1); 10 gives Rs = 32 (the host Bullet at the
default crossover) and 11 Rs = 64 (device Bullet rounds); 17 gives Rs = 512: two column blocks and a split row range."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import polyeval_cases as pc
import polyeval_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL, TLABEL = b"gens_polyeval_test", b"polyeval_test"
CHECK = b"seam_check"


@pytest.fixture(scope="module")
def spg(oracle):
    import spg as m

    return m


@pytest.fixture(scope="module")
def seed(oracle):
    import workload

    return workload.tape_seed()


@pytest.fixture(scope="module")
def gens(spg, ctx):
    """PolyGens per num_vars, made once"""
    made = {}

    def get(nv):
        if nv not in made:
            made[nv] = spg.PolyGens(ctx, LABEL, nv)
        return made[nv]

    yield get
    for g in made.values():
        g.free()


def fresh(spg, seed):
    return spg.Transcript(TLABEL), spg.RandomTape(ref.TAPE, seed)


def positions(t, tape):
    return t.challenge_bytes(CHECK, 64), tape.random_scalar(CHECK)


def assert_matches(got, t, tape, want):
    """the proof bytes are the checker's, and transcript and tape were left where the checker's prover left them"""
    assert got == want.proof
    check, nxt = positions(t, tape)
    assert check == want.check and np.array_equal(nxt, want.tape_next)


def gens_nv_for(nv):
    return 4 if nv <= 4 else (12 if nv <= 12 else nv)


@pytest.mark.parametrize("nv", [1, 4, 11])
def test_gens_points(spg, ctx, oracle, gens, nv):
    g = gens(nv)
    n = 1 << (nv - nv // 2)
    assert g.n == n
    # gens_n = points 0 .. n-1 with h = point n + 1, gens_1 = point n: the first n + 2 points of the label's stream
    assert np.array_equal(g.compressed(), oracle.gens_stream(LABEL, n + 2))


@pytest.mark.parametrize("nv", [1, 3, 4, 11])
def test_commit(spg, ctx, gens, nv):
    gnv = gens_nv_for(nv)
    Z = pc.scalars(500 + nv, 1 << nv)
    pad = pc.scalars(1, 5)
    buf = spg.Buf(ctx, np.concatenate([pad, Z, pad]))  # a non-zero offset into a longer buffer
    bl = pc.scalars(600 + nv, 1 << (nv // 2))
    assert np.array_equal(spg.poly_commit(ctx, gens(gnv), buf, nv, offset=5), ref.commit(LABEL, gnv, Z, nv))
    assert np.array_equal(spg.poly_commit(ctx, gens(gnv), buf, nv, offset=5, blinds=bl), ref.commit(LABEL, gnv, Z, nv, bl))
    buf.free()


@pytest.mark.parametrize("nv,blinded", [(1, False), (3, False), (4, False), (4, True), (10, False), (11, False),
                                        (11, True), (17, False)])
def test_single_prove_and_verify(spg, ctx, seed, gens, nv, blinded):
    gnv = gens_nv_for(nv)
    g = gens(gnv)
    Z, r = pc.scalars(100 + nv, 1 << nv), pc.scalars(200 + nv, nv)
    Zr = pc.evaluate(Z, r, nv)
    bl = pc.scalars(300 + nv, 1 << (nv // 2)) if blinded else None
    bz = pc.scalars(400 + nv, 1)[0] if blinded else None
    want = ref.prove(LABEL, gnv, TLABEL, seed, Z, r, Zr, bl, bz)
    assert want.verified
    buf = spg.Buf(ctx, np.concatenate([pc.scalars(2, 3), Z]))
    t, tape = fresh(spg, seed)
    got, czr = spg.poly_eval_prove(ctx, g, buf, r, Zr, t, tape, offset=3, blinds=bl, blind_Zr=bz)
    assert czr == want.C_Zr
    assert_matches(got, t, tape, want)
    comm = spg.poly_commit(ctx, g, buf, nv, offset=3, blinds=bl)
    buf.free()
    tv = spg.Transcript(TLABEL)
    ok, why = spg.poly_eval_verify(ctx, g, r, czr, comm, tv, got)
    assert ok, why
    assert tv.challenge_bytes(CHECK, 64) == want.check
    if not blinded:
        tv = spg.Transcript(TLABEL)
        ok, why = spg.poly_eval_verify_plain(ctx, g, r, Zr, comm, tv, got)
        assert ok, why
        assert tv.challenge_bytes(CHECK, 64) == want.check


POINT_CASES = {"one_4": (4, "a"), "one_11": (11, "a"), "abacba_11": (11, pc.ABACBA),
               "tile_plus_one_11": (11, "abcdea")}  # kPeKT + 1 distinct left halves and one repeat


@pytest.fixture(scope="module")
def point_runs(spg, ctx, seed, gens):
    """every points case proved once on the device: name -> (nv, r_list, Zr, comm, proof, checker result)"""
    runs = {}
    for name, (nv, pattern) in POINT_CASES.items():
        gnv = gens_nv_for(nv)
        Z, rl = pc.scalars(110 + nv, 1 << nv), pc.points(5, nv, pattern)
        Zr = np.array([pc.evaluate(Z, r, nv) for r in rl])
        want = ref.prove_points(LABEL, gnv, TLABEL, seed, Z, nv, rl, Zr)
        buf = spg.Buf(ctx, np.concatenate([pc.scalars(3, 7), Z]))
        t, tape = fresh(spg, seed)
        got = spg.poly_eval_prove_batched_points(ctx, gens(gnv), buf, nv, rl, Zr, t, tape, offset=7)
        comm = spg.poly_commit(ctx, gens(gnv), buf, nv, offset=7)
        buf.free()
        runs[name] = (nv, rl, Zr, comm, got, want, positions(t, tape))
    return runs


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_batched_points(spg, ctx, gens, point_runs, name):
    nv, rl, Zr, comm, got, want, (check, nxt) = point_runs[name]
    assert want.verified and want.nproofs == len(set(POINT_CASES[name][1]))
    assert got == want.proof
    assert check == want.check and np.array_equal(nxt, want.tape_next)
    tv = spg.Transcript(TLABEL)
    ok, why = spg.poly_eval_verify_plain_batched_points(ctx, gens(gens_nv_for(nv)), nv, rl, Zr, comm, tv, got)
    assert ok, why
    assert tv.challenge_bytes(CHECK, 64) == want.check


@pytest.fixture(scope="module")
def instance_runs(spg, ctx, seed, gens):
    """every instance list proved once on the device, the polynomials spread over two buffers at different offsets"""
    runs = {}
    for name, (nvs, rl) in pc.instance_cases().items():
        gnv = gens_nv_for(max(nvs))
        Zs = pc.instance_polys(700, nvs)
        Zr = np.array([pc.evaluate(Z, r, nv) for Z, r, nv in zip(Zs, rl, nvs)])
        want = ref.prove_instances(LABEL, gnv, TLABEL, seed, Zs, nvs, rl, Zr)
        parts, offs, where = [[pc.scalars(4, 3)], [pc.scalars(5, 1)]], [3, 1], []
        for i, Z in enumerate(Zs):
            where.append((i % 2, offs[i % 2]))
            parts[i % 2].append(Z)
            offs[i % 2] += len(Z)
        bufs = [spg.Buf(ctx, np.concatenate(p)) for p in parts]
        t, tape = fresh(spg, seed)
        got = spg.poly_eval_prove_batched_instances(ctx, gens(gnv), [bufs[b] for b, _ in where], nvs, rl, Zr, t, tape,
                                                    offsets=[o for _, o in where])
        comms = [spg.poly_commit(ctx, gens(gnv), bufs[b], nv, offset=o) for (b, o), nv in zip(where, nvs)]
        for b in bufs:
            b.free()
        runs[name] = (gnv, nvs, rl, Zr, comms, got, want, positions(t, tape))
    return runs


@pytest.mark.parametrize("name", ["mixed", "padtrim", "same_R", "forty"])
def test_batched_instances(spg, ctx, gens, instance_runs, name):
    gnv, nvs, rl, Zr, comms, got, want, (check, nxt) = instance_runs[name]
    assert want.verified and want.nproofs == {"mixed": 4, "padtrim": 1, "same_R": 2, "forty": 5}[name]
    assert got == want.proof
    assert check == want.check and np.array_equal(nxt, want.tape_next)
    tv = spg.Transcript(TLABEL)
    ok, why = spg.poly_eval_verify_plain_batched_instances(ctx, gens(gnv), rl, Zr, comms, nvs, tv, got)
    assert ok, why
    assert tv.challenge_bytes(CHECK, 64) == want.check


# ---------------------------------------------------------------- damaged proofs: SPG_E_VERIFY, never an exception
def flipped(proof):
    b = bytearray(proof)
    b[-64] ^= 1  # the lowest byte of the last proof's z1
    return bytes(b)


def one_short(proof, nv):
    """a proof list without its last entry (every proof of one num_vars has the same size)"""
    size = 2 * (8 + 32 * (nv - nv // 2)) + 128
    n = int.from_bytes(proof[:8], "little")
    return (n - 1).to_bytes(8, "little") + proof[8:len(proof) - size]


def bad_rows(comm, other_point):
    """(one row replaced by another valid point, one row that is no valid encoding)"""
    a, b = np.array(comm, copy=True), np.array(comm, copy=True)
    a[0] = np.frombuffer(other_point, dtype=np.uint8)
    b[-1] = 0xFF
    return a, b


def rejected(res):
    ok, why = res
    return (not ok) and bool(why)


def test_verify_rejects_single(spg, ctx, seed, gens):
    nv, g = 4, gens(4)
    Z, r = pc.scalars(104, 1 << nv), pc.scalars(204, nv)
    Zr = pc.evaluate(Z, r, nv)
    buf = spg.Buf(ctx, Z)
    t, tape = fresh(spg, seed)
    proof, czr = spg.poly_eval_prove(ctx, g, buf, r, Zr, t, tape)
    comm = spg.poly_commit(ctx, g, buf, nv)
    buf.free()
    other = g.compressed()[0].tobytes()

    def plain(p=proof, zr=Zr, c=comm):
        return spg.poly_eval_verify_plain(ctx, g, r, zr, c, spg.Transcript(TLABEL), p)

    def committed(p=proof, cz=czr, c=comm):
        return spg.poly_eval_verify(ctx, g, r, cz, c, spg.Transcript(TLABEL), p)

    assert plain()[0] and committed()[0]
    swapped, invalid = bad_rows(comm, other)
    for run in (plain, committed):
        assert rejected(run(p=flipped(proof)))
        assert rejected(run(p=proof[:-1]))
        assert rejected(run(p=proof + b"\0"))
        assert rejected(run(c=swapped))
        assert rejected(run(c=invalid))
        assert rejected(run(c=comm[:-1]))  # a commitment of the wrong row count
    assert rejected(plain(zr=pc.scalars(9, 1)[0]))
    assert rejected(committed(cz=other))
    assert rejected(committed(cz=b"\xff" * 32))


def test_verify_rejects_batched_points(spg, ctx, gens, point_runs):
    nv, rl, Zr, comm, proof, want, _ = point_runs["abacba_11"]
    g = gens(gens_nv_for(nv))
    other = g.compressed()[0].tobytes()

    def run(p=proof, zr=Zr, c=comm):
        return spg.poly_eval_verify_plain_batched_points(ctx, g, nv, rl, zr, c, spg.Transcript(TLABEL), p)

    assert run()[0]
    wrong = Zr.copy()
    wrong[4] = pc.scalars(9, 1)[0]
    swapped, invalid = bad_rows(comm, other)
    for res in (run(p=flipped(proof)), run(zr=wrong), run(c=swapped), run(c=invalid), run(c=comm[:-1]),
                run(p=one_short(proof, nv)), run(p=proof[:-1])):
        assert rejected(res)


def test_verify_rejects_batched_instances(spg, ctx, gens, instance_runs):
    gnv, nvs, rl, Zr, comms, proof, want, _ = instance_runs["same_R"]
    g = gens(gnv)
    other = g.compressed()[0].tobytes()

    def run(p=proof, zr=Zr, c=comms):
        return spg.poly_eval_verify_plain_batched_instances(ctx, g, rl, zr, c, nvs, spg.Transcript(TLABEL), p)

    assert run()[0]
    wrong = Zr.copy()
    wrong[1] = pc.scalars(9, 1)[0]
    swapped, invalid = bad_rows(comms[1], other)
    for res in (run(p=flipped(proof)), run(zr=wrong), run(c=[comms[0], swapped, comms[2]]),
                run(c=[comms[0], invalid, comms[2]]), run(c=[comms[0], comms[1][:-1], comms[2]]),
                run(p=one_short(proof, 11)), run(p=proof[:-1])):
        assert rejected(res)


# ---------------------------------------------------------------- argument errors
def arg_error(spg, fn):
    with pytest.raises(spg.SpgError, match="SPG_E_ARG"):
        fn()


def test_cap_too_small_leaves_transcript_and_tape(spg, ctx, seed, gens):
    untouched = positions(*fresh(spg, seed))

    def same_positions(t, tape):
        check, nxt = positions(t, tape)
        return check == untouched[0] and np.array_equal(nxt, untouched[1])

    nv, g = 4, gens(4)
    Z, r = pc.scalars(104, 1 << nv), pc.scalars(204, nv)
    buf = spg.Buf(ctx, Z)
    size = 2 * (8 + 32 * 2) + 128
    t, tape = fresh(spg, seed)
    arg_error(spg, lambda: spg.poly_eval_prove(ctx, g, buf, r, Z[0], t, tape, cap=size - 1))
    assert ctx.last_len == size and same_positions(t, tape)
    rl = pc.points(5, nv, "aba")
    t, tape = fresh(spg, seed)
    arg_error(spg, lambda: spg.poly_eval_prove_batched_points(ctx, g, buf, nv, rl, Z[:3], t, tape, cap=8 + 2 * size - 1))
    assert ctx.last_len == 8 + 2 * size and same_positions(t, tape)
    nvs, pts = pc.instance_cases()["padtrim"]
    t, tape = fresh(spg, seed)
    arg_error(spg, lambda: spg.poly_eval_prove_batched_instances(ctx, g, [buf] * 3, nvs, pts, Z[:3], t, tape, cap=8))
    assert ctx.last_len == 8 + size and same_positions(t, tape)
    # with the exact size the same calls go through
    t, tape = fresh(spg, seed)
    assert len(spg.poly_eval_prove(ctx, g, buf, r, Z[0], t, tape, cap=size)[0]) == size
    buf.free()


def test_argument_errors(spg, ctx, seed, gens):
    g4 = gens(4)
    Z11 = pc.scalars(111, 1 << 11)
    buf = spg.Buf(ctx, Z11)
    r11, r4 = pc.scalars(211, 11), pc.scalars(204, 4)
    t, tape = fresh(spg, seed)
    untouched = positions(*fresh(spg, seed))
    # Rs = 64 beyond the handle's n = 4
    arg_error(spg, lambda: spg.poly_commit(ctx, g4, buf, 11))
    arg_error(spg, lambda: spg.poly_eval_prove(ctx, g4, buf, r11, Z11[0], t, tape))
    arg_error(spg, lambda: spg.poly_eval_prove_batched_points(ctx, g4, buf, 11, [r11], Z11[:1], t, tape))
    arg_error(spg, lambda: spg.poly_eval_prove_batched_instances(ctx, g4, [buf], [11], [r11], Z11[:1], t, tape))
    arg_error(spg, lambda: spg.poly_eval_verify_plain(ctx, g4, r11, Z11[0], np.zeros((32, 32), np.uint8), t, b"\0" * 8))
    # offset + 2^num_vars past the buffer
    arg_error(spg, lambda: spg.poly_commit(ctx, g4, buf, 4, offset=(1 << 11) - 15))
    arg_error(spg, lambda: spg.poly_eval_prove(ctx, g4, buf, r4, Z11[0], t, tape, offset=(1 << 11) - 15))
    arg_error(spg, lambda: spg.poly_eval_prove_batched_points(ctx, g4, buf, 4, [r4], Z11[:1], t, tape, offset=1 << 11))
    arg_error(spg, lambda: spg.poly_eval_prove_batched_instances(ctx, g4, [buf, buf], [4, 4], [r4, r4], Z11[:2], t, tape,
                                                                offsets=[0, (1 << 11) - 15]))
    # num_vars 0
    none = np.zeros((0, 4), np.uint64)
    arg_error(spg, lambda: spg.PolyGens(ctx, LABEL, 0))
    arg_error(spg, lambda: spg.poly_commit(ctx, g4, buf, 0))
    arg_error(spg, lambda: spg.poly_eval_prove(ctx, g4, buf, none, Z11[0], t, tape))
    arg_error(spg, lambda: spg.poly_eval_prove_batched_points(ctx, g4, buf, 0, none.reshape(1, 0, 4), Z11[:1], t, tape))
    arg_error(spg, lambda: spg.poly_eval_prove_batched_instances(ctx, g4, [buf], [0], [r4], Z11[:1], t, tape))
    # K = 0 and n = 0
    arg_error(spg, lambda: spg.poly_eval_prove_batched_points(ctx, g4, buf, 4, none.reshape(0, 4, 4), none, t, tape))
    arg_error(spg, lambda: spg.poly_eval_prove_batched_instances(ctx, g4, [], [], [], none, t, tape))
    # nothing was appended or drawn by any of them
    check, nxt = positions(t, tape)
    assert check == untouched[0] and np.array_equal(nxt, untouched[1])
    buf.free()


# ---------------------------------------------------------------- the checked build
CHECKED_LIB = os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg_checked.so")
CHECKED_SCRIPT = """
import hashlib, sys
sys.path[:0] = {paths!r}
import numpy as np
import spg, workload
import polyeval_cases as pc
ctx = spg.Context(0)
seed = workload.tape_seed()
g = spg.PolyGens(ctx, {label!r}, 17)
Z, r = pc.scalars(117, 1 << 17), pc.scalars(217, 17)
buf = spg.Buf(ctx, Z)
pf, _ = spg.poly_eval_prove(ctx, g, buf, r, Z[0], spg.Transcript({tlabel!r}), spg.RandomTape(b"proof", seed))
print(hashlib.sha256(pf).hexdigest(), flush=True)
nvs, rl = pc.instance_cases()["forty"]
Zs = pc.instance_polys(700, nvs)
bufs = [spg.Buf(ctx, z) for z in Zs]
pf = spg.poly_eval_prove_batched_instances(ctx, g, bufs, nvs, rl, Z[:40], spg.Transcript({tlabel!r}),
                                           spg.RandomTape(b"proof", seed))
print(hashlib.sha256(pf).hexdigest(), flush=True)
"""


def test_checked_build(oracle, seed):
    """the num_vars 17 single proof and the 40-polynomial call under the bounds- and ownership-checked library: the
    checker's bytes, and none of its checks fires (the bound's kernels print theirs as k_pe_*)"""
    assert os.path.exists(CHECKED_LIB), "libspg_checked.so not built"
    Z, r = pc.scalars(117, 1 << 17), pc.scalars(217, 17)
    want = [hashlib.sha256(ref.prove(LABEL, 17, TLABEL, seed, Z, r, Z[0]).proof).hexdigest()]
    nvs, rl = pc.instance_cases()["forty"]
    want.append(hashlib.sha256(ref.prove_instances(LABEL, 17, TLABEL, seed, pc.instance_polys(700, nvs), nvs, rl,
                                                   Z[:40]).proof).hexdigest())
    paths = [os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    r = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT.format(paths=paths, label=LABEL, tlabel=TLABEL)],
                       env=dict(os.environ, SPG_LIB=CHECKED_LIB), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "[spg checked]" not in r.stderr and "k_pe_" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.split() == want
