"""The disjoint-rounds and univariate forms of PolyEvalProof on the device (include/spg.h spg_pe_*,
csrc/polyeval.hip): proof bytes against the tests' checker (tests/polyeval_forms_ref.py over the oracle's headers)
under the labels and tape seed of tests/test_gpu_polyeval.py, with the positions the prover leaves transcript and tape
in; the univariate evaluations bit for bit; the verifiers on those proofs and on damaged ones; the argument errors; the
ragged column sum under the checked build.

Cases: tests/polyeval_forms_cases.py. Every case is proved once (module fixtures), its polynomials spread over two
buffers at non-zero offsets."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import polyeval_cases as pc
import polyeval_forms_cases as fc
import polyeval_forms_ref as ref

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


def spread(spg, ctx, Zs):
    """the polynomials over two buffers at non-zero offsets: (bufs, [buffer of polynomial i], [its offset])"""
    parts, offs, where = [[pc.scalars(4, 3)], [pc.scalars(5, 1)]], [3, 1], []
    for i, Z in enumerate(Zs):
        where.append((i % 2, offs[i % 2]))
        parts[i % 2].append(Z)
        offs[i % 2] += len(Z)
    bufs = [spg.Buf(ctx, np.concatenate(p)) for p in parts]
    return bufs, [bufs[b] for b, _ in where], [o for _, o in where]


@pytest.fixture(scope="module")
def disjoint_runs(spg, ctx, seed, gens):
    runs = {}
    for name in fc.DISJOINT_CASES:
        shapes, rq, ry, Zs = fc.disjoint_inputs(name)
        nps, nis = [s[0] for s in shapes], [s[1] for s in shapes]
        gnv = fc.gens_nv(max(fc.lg(p * q) for p, q in shapes))
        Zr = fc.disjoint_evals(shapes, rq, ry, Zs)
        want = ref.prove_disjoint(LABEL, gnv, TLABEL, seed, Zs, shapes, rq, ry, Zr)
        bufs, polys, offsets = spread(spg, ctx, Zs)
        t, tape = fresh(spg, seed)
        got = spg.pe_prove_disjoint(ctx, gens(gnv), polys, nps, nis, rq, ry, Zr, t, tape, offsets=offsets)
        comms = [spg.poly_commit(ctx, gens(gnv), b, fc.lg(p * q), offset=o)
                 for b, o, (p, q) in zip(polys, offsets, shapes)]
        for b in bufs:
            b.free()
        runs[name] = (gnv, nps, nis, rq, ry, comms, got, want, positions(t, tape))
    return runs


@pytest.fixture(scope="module")
def uni_runs(spg, ctx, seed, gens):
    runs = {}
    for name in fc.UNI_CASES:
        nvs, r, Zs = fc.uni_inputs(name)
        gnv = fc.gens_nv(max(nvs))
        Zr = ref.uni_evals(Zs, nvs, r)
        want = ref.prove_uni(LABEL, gnv, TLABEL, seed, Zs, nvs, r, Zr)
        bufs, polys, offsets = spread(spg, ctx, Zs)
        evals = spg.pe_uni_evals(ctx, polys, nvs, r, offsets=offsets)
        t, tape = fresh(spg, seed)
        got, czr = spg.pe_prove_uni(ctx, gens(gnv), polys, nvs, r, Zr, t, tape, offsets=offsets)
        comms = [spg.poly_commit(ctx, gens(gnv), b, nv, offset=o) for b, o, nv in zip(polys, offsets, nvs)]
        for b in bufs:
            b.free()
        runs[name] = (gnv, nvs, r, Zr, evals, comms, got, czr, want, positions(t, tape))
    return runs


@pytest.mark.parametrize("name", list(fc.UNI_CASES))
def test_uni_evals(uni_runs, name):
    _, _, _, Zr, evals, *_ = uni_runs[name]
    assert np.array_equal(evals, Zr)


@pytest.mark.parametrize("name", list(fc.DISJOINT_CASES))
def test_disjoint_prove_and_verify(spg, ctx, gens, disjoint_runs, name):
    gnv, nps, nis, rq, ry, comms, got, want, (check, nxt) = disjoint_runs[name]
    expected = fc.DISJOINT_CASES[name][3]
    assert want.verified and want.nproofs == expected
    assert got == want.proof and int.from_bytes(got[:8], "little") == expected
    assert check == want.check and np.array_equal(nxt, want.tape_next)
    tv = spg.Transcript(TLABEL)
    ok, why = spg.pe_verify_disjoint(ctx, gens(gnv), nps, nis, rq, ry, want.C_Zr_list, comms, tv, got)
    assert ok, why
    assert tv.challenge_bytes(CHECK, 64) == want.check


@pytest.mark.parametrize("name", list(fc.UNI_CASES))
def test_uni_prove_and_verify(spg, ctx, gens, uni_runs, name):
    gnv, nvs, r, Zr, _, comms, got, czr, want, (check, nxt) = uni_runs[name]
    assert want.verified
    assert got == want.proof and len(got) == fc.proof_bytes(1 << (max(nvs) - max(nvs) // 2))
    assert czr == want.C_Zr
    assert check == want.check and np.array_equal(nxt, want.tape_next)
    tv = spg.Transcript(TLABEL)
    ok, why = spg.pe_verify_uni(ctx, gens(gnv), r, want.C_Zr_list, comms, [1 << nv for nv in nvs], tv, got)
    assert ok, why
    assert tv.challenge_bytes(CHECK, 64) == want.check


# ---------------------------------------------------------------- damaged proofs: SPG_E_VERIFY, never an exception
def flipped(proof):
    b = bytearray(proof)
    b[-64] ^= 1  # the lowest byte of the last proof's z1
    return bytes(b)


def bad_rows(comm, other_point):
    """(one row replaced by another valid point, one row that is no valid encoding)"""
    a, b = np.array(comm, copy=True), np.array(comm, copy=True)
    a[0] = np.frombuffer(other_point, dtype=np.uint8)
    b[-1] = 0xFF
    return a, b


def rejected(res):
    ok, why = res
    return (not ok) and bool(why)


def with_item(lst, i, x):
    out = list(lst)
    out[i] = x
    return out


def test_verify_rejects_disjoint(spg, ctx, gens, disjoint_runs):
    gnv, nps, nis, rq, ry, comms, proof, want, _ = disjoint_runs["abacba"]
    g = gens(gnv)
    other = g.compressed()[0].tobytes()

    def run(p=proof, cz=want.C_Zr_list, c=comms, np_=nps, ni_=nis):
        return spg.pe_verify_disjoint(ctx, g, np_, ni_, rq, ry, cz, c, spg.Transcript(TLABEL), p)

    assert run()[0]
    swapped, invalid = bad_rows(comms[1], other)
    last = fc.proof_bytes(4)  # the last proof is the (1, 16) key's: Rs = 4
    one_short = (2).to_bytes(8, "little") + proof[8:len(proof) - last]
    for res in (run(p=flipped(proof)), run(cz=with_item(want.C_Zr_list, 4, other)),
                run(cz=with_item(want.C_Zr_list, 2, b"\xff" * 32)), run(c=with_item(comms, 1, swapped)),
                run(c=with_item(comms, 1, invalid)), run(c=with_item(comms, 1, comms[1][:-1])), run(p=proof[:-1]),
                run(p=proof + b"\0"), run(p=one_short),
                run(np_=with_item(with_item(nps, 0, nps[1]), 1, nps[0]),
                    ni_=with_item(with_item(nis, 0, nis[1]), 1, nis[0]))):
        assert rejected(res)


def test_verify_rejects_uni(spg, ctx, gens, uni_runs):
    gnv, nvs, r, Zr, _, comms, proof, czr, want, _ = uni_runs["ragged"]
    g = gens(gnv)
    other = g.compressed()[0].tobytes()
    sizes = [1 << nv for nv in nvs]

    def run(p=proof, cz=want.C_Zr_list, c=comms, sz=sizes):
        return spg.pe_verify_uni(ctx, g, r, cz, c, sz, spg.Transcript(TLABEL), p)

    assert run()[0]
    swapped, invalid = bad_rows(comms[3], other)
    for res in (run(p=flipped(proof)), run(cz=with_item(want.C_Zr_list, 5, other)),
                run(cz=with_item(want.C_Zr_list, 3, b"\xff" * 32)), run(c=with_item(comms, 3, swapped)),
                run(c=with_item(comms, 3, invalid)), run(c=with_item(comms, 3, comms[3][:-1])), run(p=proof[:-1]),
                run(p=proof + b"\0"), run(sz=with_item(sizes, 0, 2 * sizes[0]))):
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

    g = gens(12)
    Z = pc.scalars(104, 1 << 6)
    buf = spg.Buf(ctx, Z)
    rq, ry = pc.scalars(1, 3), pc.scalars(2, 3)
    # (8, 8) twice and (4, 4): Rs = 8 and 4, two proofs
    nps, nis = [8, 4, 8], [8, 4, 8]
    size = 8 + fc.proof_bytes(8) + fc.proof_bytes(4)
    t, tape = fresh(spg, seed)
    arg_error(spg, lambda: spg.pe_prove_disjoint(ctx, g, [buf] * 3, nps, nis, rq, ry, Z[:3], t, tape, cap=size - 1))
    assert ctx.last_len == size and same_positions(t, tape)
    assert len(spg.pe_prove_disjoint(ctx, g, [buf] * 3, nps, nis, rq, ry, Z[:3], t, tape, cap=size)) == size
    # num_vars 3, 6, 4: R_size = 8
    size = fc.proof_bytes(8)
    t, tape = fresh(spg, seed)
    arg_error(spg, lambda: spg.pe_prove_uni(ctx, g, [buf] * 3, [3, 6, 4], Z[0], Z[:3], t, tape, cap=size - 1))
    assert ctx.last_len == size and same_positions(t, tape)
    assert len(spg.pe_prove_uni(ctx, g, [buf] * 3, [3, 6, 4], Z[0], Z[:3], t, tape, cap=size)[0]) == size
    buf.free()


def test_argument_errors(spg, ctx, seed, gens):
    g4 = gens(4)
    Z = pc.scalars(111, 1 << 11)
    buf = spg.Buf(ctx, Z)
    rq, ry, r = pc.scalars(1, 3), pc.scalars(2, 8), Z[0]
    none = np.zeros((0, 4), np.uint64)
    t, tape = fresh(spg, seed)
    untouched = positions(*fresh(spg, seed))
    rows = np.zeros((4, 32), np.uint8)

    def prove_d(shapes, q=rq, bufs=None, offsets=None):
        n = len(shapes)
        return lambda: spg.pe_prove_disjoint(ctx, g4, bufs if bufs is not None else [buf] * n, [s[0] for s in shapes],
                                             [s[1] for s in shapes], q, ry, Z[:n], t, tape, offsets=offsets)

    def verify_d(shapes, q=rq):
        n = len(shapes)
        return lambda: spg.pe_verify_disjoint(ctx, g4, [s[0] for s in shapes], [s[1] for s in shapes], q, ry,
                                              [b"\0" * 32] * n, [rows] * n, t, b"\0" * 8)

    for shapes, q in (([], rq),                  # n = 0
                      ([(3, 4)], rq), ([(4, 3)], rq), ([(0, 4)], rq),  # not powers of two
                      ([(1, 1)], rq),            # num_vars 0
                      ([(1 << 3, 1 << 28)], rq),  # num_vars 31
                      ([(4, 4)], rq[:1]),        # lg num_proofs beyond rq
                      ([(4, 4), (8, 256)], rq)):  # Rs = 64 beyond the handle's n = 4
        arg_error(spg, prove_d(shapes, q))
        arg_error(spg, verify_d(shapes, q))
    arg_error(spg, prove_d([(4, 4), (4, 4)], offsets=[0, (1 << 11) - 15]))  # offset + 2^num_vars past the buffer

    def prove_u(nvs, gens_=g4, offsets=None):
        n = len(nvs)
        return lambda: spg.pe_prove_uni(ctx, gens_, [buf] * n, nvs, r, Z[:n], t, tape, offsets=offsets)

    def evals_u(nvs, offsets=None):
        return lambda: spg.pe_uni_evals(ctx, [buf] * len(nvs), nvs, r, offsets=offsets)

    def verify_u(sizes):
        n = len(sizes)
        return lambda: spg.pe_verify_uni(ctx, g4, r, [b"\0" * 32] * n, [rows] * n, sizes, t, b"\0" * 8)

    for nvs in ([], [0], [3, 31]):
        arg_error(spg, prove_u(nvs))
        arg_error(spg, evals_u(nvs))
        arg_error(spg, verify_u([1 << nv for nv in nvs]))
    arg_error(spg, prove_u([3, 11]))  # the widest polynomial's Rs = 64 beyond the handle's n = 4
    arg_error(spg, verify_u([8, 1 << 11]))
    arg_error(spg, verify_u([8, (1 << 10) + 1]))  # next_pow2: num_vars 11
    arg_error(spg, prove_u([4, 4], offsets=[0, (1 << 11) - 15]))
    arg_error(spg, evals_u([4, 4], offsets=[0, (1 << 11) - 15]))
    # null pointers, straight at the C-ABI
    lib, sz, one = spg.lib(), ctypes.c_size_t, (ctypes.c_size_t * 1)(4)
    arr = (ctypes.c_void_p * 1)(buf.handle.value)
    out = np.zeros(4, np.uint64)
    rp, op = r.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    assert lib.spg_pe_uni_evals(ctx.handle, None, one, one, sz(1), rp, op) == spg.SPG_E_ARG
    assert lib.spg_pe_uni_evals(ctx.handle, arr, one, one, sz(1), None, op) == spg.SPG_E_ARG
    assert lib.spg_pe_uni_evals(ctx.handle, arr, one, one, sz(1), rp, None) == spg.SPG_E_ARG
    n = sz(0)
    assert lib.spg_pe_prove_uni(ctx.handle, None, arr, one, one, sz(1), rp, rp, t.handle, tape.handle, op, sz(0),
                                ctypes.byref(n), None) == spg.SPG_E_ARG
    assert lib.spg_pe_prove_uni(ctx.handle, g4.handle, arr, one, one, sz(1), rp, None, t.handle, tape.handle, op, sz(0),
                                ctypes.byref(n), None) == spg.SPG_E_ARG
    assert lib.spg_pe_prove_disjoint(ctx.handle, g4.handle, arr, one, one, None, sz(1), rp, sz(1), rp, sz(1), rp,
                                     t.handle, tape.handle, op, sz(0), ctypes.byref(n)) == spg.SPG_E_ARG
    assert lib.spg_pe_verify_disjoint(ctx.handle, g4.handle, one, one, sz(1), rp, sz(1), rp, sz(1), None, op, one,
                                      t.handle, op, sz(8)) == spg.SPG_E_ARG
    assert lib.spg_pe_verify_uni(ctx.handle, g4.handle, rp, op, None, one, one, sz(1), t.handle, op,
                                 sz(8)) == spg.SPG_E_ARG
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
import polyeval_forms_cases as fc
ctx = spg.Context(0)
seed = workload.tape_seed()
g = spg.PolyGens(ctx, {label!r}, 17)
for name in ("wide", "forty"):
    nvs, r, Zs = fc.uni_inputs(name)
    bufs = [spg.Buf(ctx, z) for z in Zs]
    Zr = spg.pe_uni_evals(ctx, bufs, nvs, r)
    pf, _ = spg.pe_prove_uni(ctx, g, bufs, nvs, r, Zr, spg.Transcript({tlabel!r}), spg.RandomTape(b"proof", seed))
    print(hashlib.sha256(pf).hexdigest(), flush=True)
shapes, rq, ry, Zs = fc.disjoint_inputs("forty")
bufs = [spg.Buf(ctx, z) for z in Zs]
pf = spg.pe_prove_disjoint(ctx, g, bufs, [s[0] for s in shapes], [s[1] for s in shapes], rq, ry,
                           fc.disjoint_evals(shapes, rq, ry, Zs), spg.Transcript({tlabel!r}),
                           spg.RandomTape(b"proof", seed))
print(hashlib.sha256(pf).hexdigest(), flush=True)
"""


def test_checked_build(oracle, seed):
    """the univariate wide and forty cases and the disjoint forty case under the bounds- and ownership-checked
    library: the checker's bytes, and none of its checks fires (the bound's kernels print theirs as k_pe_*)"""
    assert os.path.exists(CHECKED_LIB), "libspg_checked.so not built"
    want = []
    for name in ("wide", "forty"):
        nvs, r, Zs = fc.uni_inputs(name)
        want.append(hashlib.sha256(ref.prove_uni(LABEL, 17, TLABEL, seed, Zs, nvs, r,
                                                 ref.uni_evals(Zs, nvs, r)).proof).hexdigest())
    shapes, rq, ry, Zs = fc.disjoint_inputs("forty")
    want.append(hashlib.sha256(ref.prove_disjoint(LABEL, 17, TLABEL, seed, Zs, shapes, rq, ry,
                                                  fc.disjoint_evals(shapes, rq, ry, Zs)).proof).hexdigest())
    paths = [os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    r = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT.format(paths=paths, label=LABEL, tlabel=TLABEL)],
                       env=dict(os.environ, SPG_LIB=CHECKED_LIB), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "[spg checked]" not in r.stderr and "k_pe_" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.split() == want
