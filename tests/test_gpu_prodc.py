"""The memory-checking and grand-product seams (csrc/prodc.hip; include/spg.h spg_hash_layer, spg_prodc_*,
spg_prove_cubic_batched, spg_prodc_prove_batched) on the device against the oracle (tests/prodc_oracle through
prodc_ref), bit-exact: hashes, tree layers, sumcheck polynomials, challenges, bound vectors, proof bytes and the
transcript state afterwards."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import prodc_ref
from test_gpu_seams import Q, mont, rand_fq

pytestmark = pytest.mark.gpu

SPG_E_ARG = -1
CHECK = b"seam_check"


def fq_prod(oracle, v):
    v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
    while v.shape[0] > 1:
        if v.shape[0] & 1:
            v = np.concatenate([v, mont(1).reshape(1, 4)])
        h = v.shape[0] // 2
        v = oracle.fq_op("mul", v[:h], v[h:])
    return v[0]


# ------------------------------------------------------------------------------------------------ hash layer
def hash_inputs(oracle, cells, ops, n, seed):
    rng = np.random.default_rng(seed)
    table, audit_ts = rand_fq(oracle, rng, cells), rand_fq(oracle, rng, cells)
    addrs, derefs, rts = (rand_fq(oracle, rng, n * ops).reshape(n, ops, 4) for _ in range(3))
    # an address >= 2^32, timestamps 0 and q - 1 (the write's ts + 1 wraps to 0)
    addrs[0, 0] = mont(2**32 + 5)
    rts[0, 0] = mont(0)
    rts[n - 1, ops - 1] = mont(Q - 1)
    audit_ts[0] = mont(0)
    audit_ts[cells - 1] = mont(Q - 1)
    return table, audit_ts, addrs, derefs, rts, rng


def run_hash_layer(ctx, table, audit_ts, addrs, derefs, rts, rh, rms):
    import spg

    n = addrs.shape[0]
    bt, ba = spg.Buf(ctx, table), spg.Buf(ctx, audit_ts)
    la, ld, lt = ([spg.Buf(ctx, x[k]) for k in range(n)] for x in (addrs, derefs, rts))
    init, reads, writes, audit = spg.hash_layer(ctx, bt, la, ld, lt, ba, rh, rms)
    # the operands are left unchanged
    assert np.array_equal(bt.download(), table) and np.array_equal(la[0].download(), addrs[0])
    return init, reads, writes, audit


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ops", [1, 64, 4096])
@pytest.mark.parametrize("cells", [1, 2, 256, 1024])
def test_hash_layer(ctx, oracle, cells, ops, n):
    table, audit_ts, addrs, derefs, rts, rng = hash_inputs(oracle, cells, ops, n, 1000 * cells + 10 * ops + n)
    rh, rms = rand_fq(oracle, rng, 2)
    init, reads, writes, audit = run_hash_layer(ctx, table, audit_ts, addrs, derefs, rts, rh, rms)
    e_init, e_reads, e_writes, e_audit = prodc_ref.hash_layer(table, audit_ts, addrs, derefs, rts, rh, rms)
    assert init.n == cells and audit.n == cells and all(b.n == ops for b in reads + writes)
    assert np.array_equal(init.download(), e_init)
    assert np.array_equal(audit.download(), e_audit)
    for k in range(n):
        assert np.array_equal(reads[k].download(), e_reads[k])
        assert np.array_equal(writes[k].download(), e_writes[k])


def test_hash_layer_r_hash_zero(ctx, oracle):
    table, audit_ts, addrs, derefs, rts, rng = hash_inputs(oracle, 256, 64, 3, 77)
    rh, rms = mont(0), rand_fq(oracle, rng, 1)[0]
    init, reads, writes, audit = run_hash_layer(ctx, table, audit_ts, addrs, derefs, rts, rh, rms)
    e_init, e_reads, e_writes, e_audit = prodc_ref.hash_layer(table, audit_ts, addrs, derefs, rts, rh, rms)
    assert np.array_equal(init.download(), e_init) and np.array_equal(audit.download(), e_audit)
    assert np.array_equal(init.download(), audit.download())  # hash = addr - r_multiset whatever the timestamp
    for k in range(3):
        assert np.array_equal(reads[k].download(), e_reads[k])
        assert np.array_equal(writes[k].download(), e_writes[k])


# ------------------------------------------------------------------------------------------------ trees
# 2048 / 4096: the largest M whose levels all come from k_tree_top, and the smallest with a k_tree_level launch
# (layers.hip tree_build: levels of more than kTopHalf = 1024 products per circuit take one grid-wide launch each)
@pytest.mark.parametrize("nc", [1, 4, 8])
@pytest.mark.parametrize("M", [2, 4, 64, 1024, 2048, 4096, 1 << 14])
def test_prodc_new(ctx, oracle, M, nc):
    import spg

    rng = np.random.default_rng(31 * M + nc)
    leaves = rand_fq(oracle, rng, nc * M).reshape(nc, M, 4)
    bufs = [spg.Buf(ctx, leaves[c]) for c in range(nc)]
    pc = spg.ProductCircuits(ctx, bufs)
    assert pc.shape == (nc, M)
    ev = pc.evaluate()
    for c in range(nc):
        ls, rs, e = prodc_ref.circuit_layers(leaves[c])
        assert np.array_equal(ev[c], e)
        for k in range(len(ls)):
            left, right = pc.layer(c, k)
            assert np.array_equal(left, ls[k]) and np.array_equal(right, rs[k]), (c, k)
        assert np.array_equal(bufs[c].download(), leaves[c])  # ProductCircuit::new borrows its input


def test_prodc_zero_leaf(ctx, oracle):
    import spg

    rng = np.random.default_rng(9)
    leaves = rand_fq(oracle, rng, 2 * 64).reshape(2, 64, 4)
    leaves[1, 37] = 0
    pc = spg.ProductCircuits(ctx, [spg.Buf(ctx, leaves[c]) for c in range(2)])
    ev = pc.evaluate()
    assert np.array_equal(ev[0], fq_prod(oracle, leaves[0])) and ev[0].any()
    assert not ev[1].any()


# ------------------------------------------------------------------------------------------------ prove_cubic_batched
def cubic_inputs(oracle, n_par, n_seq, k, seed):
    rng = np.random.default_rng(seed)
    ln = 1 << k
    Ap, Bp = (rand_fq(oracle, rng, n_par * ln).reshape(n_par, ln, 4) for _ in range(2))
    Cp = rand_fq(oracle, rng, ln)
    As, Bs, Cs = (rand_fq(oracle, rng, n_seq * ln).reshape(n_seq, ln, 4) for _ in range(3))
    coeffs = rand_fq(oracle, rng, n_par + n_seq)
    claim = rand_fq(oracle, rng, 1)[0]
    return Ap, Bp, Cp, As, Bs, Cs, coeffs, claim


@pytest.mark.parametrize("short", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 7, 11])
@pytest.mark.parametrize("n_par,n_seq", [(1, 0), (0, 1), (4, 2), (8, 6)])
def test_prove_cubic_batched(ctx, oracle, n_par, n_seq, k, short):
    import spg

    rounds = k - short
    Ap, Bp, Cp, As, Bs, Cs, coeffs, claim = cubic_inputs(oracle, n_par, n_seq, k, 100 * k + 10 * n_par + n_seq)
    e_polys, e_r, e_bound, e_check = prodc_ref.cubic_batched(b"cubic_batched", claim, rounds, Ap, Bp, Cp, As, Bs, Cs,
                                                             coeffs)
    up = lambda X: [spg.Buf(ctx, X[i]) for i in range(X.shape[0])]  # noqa: E731
    bAp, bBp, bAs, bBs, bCs = up(Ap), up(Bp), up(As), up(Bs), up(Cs)
    bCp = spg.Buf(ctx, Cp)
    tr = spg.Transcript(b"cubic_batched")
    polys, r, cpar, cseq = spg.prove_cubic_batched(ctx, claim, rounds, bAp, bBp, bCp, bAs, bBs, bCs, coeffs, tr)
    assert np.array_equal(polys, e_polys)
    assert np.array_equal(r, e_r)
    m = (1 << k) >> rounds
    for name, bufs in (("Apar", bAp), ("Bpar", bBp), ("Aseq", bAs), ("Bseq", bBs), ("Cseq", bCs)):
        for i, b in enumerate(bufs):
            assert b.n == m and np.array_equal(b.download(), e_bound[name][i]), (name, i)
    assert bCp.n == m and np.array_equal(bCp.download(), e_bound["Cpar"])
    # final entries: A finals, B finals, C_par[0]; A, B, C finals of the triples
    assert np.array_equal(cpar[:n_par], e_bound["Apar"][:, 0]) and np.array_equal(cpar[n_par:2 * n_par], e_bound["Bpar"][:, 0])
    assert np.array_equal(cpar[2 * n_par], e_bound["Cpar"][0])
    for v, name in enumerate(("Aseq", "Bseq", "Cseq")):
        assert np.array_equal(cseq[v], e_bound[name][:, 0])
    assert tr.challenge_bytes(CHECK, 64) == e_check


# ------------------------------------------------------------------------------------------------ prove_batched
def batched_inputs(oracle, M, nc, nd, seed):
    rng = np.random.default_rng(seed)
    leaves = rand_fq(oracle, rng, nc * M).reshape(nc, M, 4)
    dotp = rand_fq(oracle, rng, max(nd, 1) * 3 * (M // 2)).reshape(max(nd, 1), 3, M // 2, 4)[:nd]
    return leaves, dotp


def gpu_prove_batched(ctx, leaves, dotp, label=b"prodc_batched", cap=None):
    import spg

    pc = spg.ProductCircuits(ctx, [spg.Buf(ctx, leaves[c]) for c in range(leaves.shape[0])])
    bd = [tuple(spg.Buf(ctx, dotp[k, v]) for v in range(3)) for k in range(dotp.shape[0])]
    tr = spg.Transcript(label)
    proof, rand = pc.prove_batched(bd, tr, cap=cap)
    return proof, rand, tr.challenge_bytes(CHECK, 64), bd


@pytest.mark.parametrize("nc,nd", [(1, 0), (4, 0), (4, 2), (8, 6)])  # (8, 6): the SPARK row layer of a batch of 3
@pytest.mark.parametrize("M", [2, 4, 8, 64, 1024])
def test_prodc_prove_batched(ctx, oracle, M, nc, nd):
    leaves, dotp = batched_inputs(oracle, M, nc, nd, 7 * M + 10 * nc + nd)
    e_proof, e_rand, e_check, ok = prodc_ref.prove_batched(b"prodc_batched", leaves, dotp)
    assert ok  # the oracle's verifier accepts the bytes compared against
    proof, rand, check, bd = gpu_prove_batched(ctx, leaves, dotp)
    assert proof == e_proof
    assert np.array_equal(rand, e_rand)
    assert check == e_check
    # the dot-product vectors were bound in place: one entry each, the claims_dotp of the proof (its last 3 vectors)
    tail = np.frombuffer(proof[len(proof) - 3 * (8 + 32 * nd):], dtype=np.uint8)
    for k, tr3 in enumerate(bd):
        for v, b in enumerate(tr3):
            want = tail[v * (8 + 32 * nd) + 8 + 32 * k:][:32].view(np.uint64)
            assert b.n == 1 and np.array_equal(b.download()[0], want)


def test_prodc_prove_batched_cap_one_short(ctx, oracle):
    import spg

    leaves, dotp = batched_inputs(oracle, 8, 4, 2, 3)
    e_proof, _, _, _ = prodc_ref.prove_batched(b"prodc_batched", leaves, dotp)
    pc = spg.ProductCircuits(ctx, [spg.Buf(ctx, leaves[c]) for c in range(4)])
    assert pc.proof_size(2) == len(e_proof)
    bd = [tuple(spg.Buf(ctx, dotp[k, v]) for v in range(3)) for k in range(2)]
    flat = (ctypes.c_void_p * 6)(*[b.handle.value for t3 in bd for b in t3])
    out = np.zeros(len(e_proof), dtype=np.uint8)
    n, rl = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rand = np.zeros((3, 4), dtype=np.uint64)
    tr = spg.Transcript(b"prodc_batched")
    rc = spg.lib().spg_prodc_prove_batched(ctx.handle, pc.handle, flat, ctypes.c_size_t(2), tr.handle,
                                           out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(e_proof) - 1),
                                           ctypes.byref(n), rand.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rl))
    assert rc == SPG_E_ARG and n.value == len(e_proof)
    # nothing ran: the same handles then prove with the right capacity
    proof, _ = pc.prove_batched(bd, tr)
    assert proof == e_proof


def test_memory_check_end_to_end(ctx, oracle):
    """hash_layer -> ProductCircuits -> evaluate on a consistent memory trace: init * prod(writes) = prod(reads) * audit
    (the multiset identity ProductLayerProof::verify checks, src/sparse_mlpoly.rs:1300-1312)"""
    import spg

    rng = np.random.default_rng(2024)
    cells, ops, n = 16, 64, 2
    table = rand_fq(oracle, rng, cells)
    addr = rng.integers(0, cells, size=(n, ops))
    # AddrTimestamps::new (src/sparse_mlpoly.rs:212-271): a read returns the cell's counter, the write stores it + 1;
    # the counters run on across the instances and end as audit_ts
    audit = np.zeros(cells, dtype=np.int64)
    read_ts = np.zeros((n, ops), dtype=np.int64)
    for k in range(n):
        for i in range(ops):
            read_ts[k, i] = audit[addr[k, i]]
            audit[addr[k, i]] += 1
    to_fq = lambda a: np.stack([mont(int(x)) for x in a.reshape(-1)]).reshape(a.shape + (4,))  # noqa: E731
    addrs, rts, audit_ts = to_fq(addr), to_fq(read_ts), to_fq(audit)
    derefs = table[addr]
    rh, rms = rand_fq(oracle, rng, 2)
    b = lambda X: [spg.Buf(ctx, X[k]) for k in range(n)]  # noqa: E731
    init, reads, writes, aud = spg.hash_layer(ctx, spg.Buf(ctx, table), b(addrs), b(derefs), b(rts),
                                              spg.Buf(ctx, audit_ts), rh, rms)
    mem = spg.ProductCircuits(ctx, [init, aud]).evaluate()
    opsc = spg.ProductCircuits(ctx, reads + writes).evaluate()
    lhs = fq_prod(oracle, np.concatenate([mem[0:1], opsc[n:]]))
    rhs = fq_prod(oracle, np.concatenate([opsc[:n], mem[1:2]]))
    assert np.array_equal(lhs, rhs) and lhs.any()
    # and the identity fails for a trace with one timestamp off
    rts[1, 5] = mont(int(read_ts[1, 5]) + 1)
    _, reads2, writes2, _ = spg.hash_layer(ctx, spg.Buf(ctx, table), b(addrs), b(derefs), b(rts), spg.Buf(ctx, audit_ts),
                                           rh, rms)
    ops2 = spg.ProductCircuits(ctx, reads2 + writes2).evaluate()
    assert not np.array_equal(fq_prod(oracle, np.concatenate([mem[0:1], ops2[n:]])),
                              fq_prod(oracle, np.concatenate([ops2[:n], mem[1:2]])))


# ------------------------------------------------------------------------------------------------ launch forms
FORMS = [{"SPG_WIDE_MIN": "1"}, {"SPG_LAYER_PAIR": "0", "SPG_LAYER_TRIPLE": "0"},
         {"SPG_TRIPLE_MAX": "1536", "SPG_WIDE_MIN": "1000000000000", "SPG_STEP_COSTS": "18,25,1"}]


def test_prodc_prove_batched_launch_forms(ctx, oracle):
    """the (4, 2), M = 1024 proof with every round through the throughput form, through single rounds only, and
    tripled wherever it fits: the bytes of the default form (the knobs are read once per process: one fresh child
    per setting, each under its own timeout; the first failing child ends the test)"""
    import hashlib

    leaves, dotp = batched_inputs(oracle, 1024, 4, 2, 7 * 1024 + 10 * 4 + 2)
    proof, rand, check, _ = gpu_prove_batched(ctx, leaves, dotp)
    want = hashlib.sha256(proof + rand.tobytes() + check).hexdigest()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, hashlib; sys.path[:0] = [%r, %r, %r]\n"
        "import pyoracle, spg\n"
        "from test_gpu_prodc import batched_inputs, gpu_prove_batched\n"
        "leaves, dotp = batched_inputs(pyoracle, 1024, 4, 2, 7 * 1024 + 10 * 4 + 2)\n"
        "ctx = spg.Context(0)\n"
        "proof, rand, check, _ = gpu_prove_batched(ctx, leaves, dotp)\n"
        "print(hashlib.sha256(proof + rand.tobytes() + check).hexdigest())\n"
    ) % (os.path.join(root, "tests"), os.path.join(root, "oracle"), os.path.join(root, "spartan-parallel_amd"))
    for env in FORMS:
        res = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True,
                             timeout=120)
        assert res.returncode == 0, (env, res.stderr[-2000:])
        assert res.stdout.strip().splitlines()[-1] == want, env


# the lane form's grid (layers.hip layer_grid; only rounds that are neither wide nor in the quad form take it, and only
# single rounds): every round ticketed over several workgroups, one workgroup looping over everything, and 1 or 8
# elements per thread of the wider grids
LANE = {"SPG_LAYER_QUAD": "0", "SPG_WIDE_MIN": "1000000000000", "SPG_LAYER_PAIR": "0", "SPG_LAYER_TRIPLE": "0"}
GRID_FORMS = [dict(LANE, SPG_LAYER_ONEWG="0"), dict(LANE, SPG_LAYER_ONEWG=str(1 << 20)),
              dict(LANE, SPG_LAYER_ONEWG="0", SPG_LAYER_EPT="1"), dict(LANE, SPG_LAYER_ONEWG="0", SPG_LAYER_EPT="8")]


def test_prodc_layer_grid_forms(oracle):
    """the (4, 2), M = 4096 proof with every round a single lane-form round on layer_grid's shapes, against the
    oracle's bytes. The top layer's first round runs over 6 x 1024 elements: 12 workgroups by default, 24 and 3 with
    1 and 8 elements per thread, one with SPG_LAYER_ONEWG past that size; with SPG_LAYER_ONEWG=0 every round of more
    than 64 elements takes the ticketed form. The profile's spark_layer_round count shows that every round of every
    layer was such a launch (no pair, triple or wide launch took one)."""
    import hashlib

    import msm_form_cases as fc

    M, nc, nd = 4096, 4, 2
    leaves, dotp = batched_inputs(oracle, M, nc, nd, 7 * M + 10 * nc + nd)
    e_proof, e_rand, e_check, ok = prodc_ref.prove_batched(b"prodc_batched", leaves, dotp)
    assert ok
    want = hashlib.sha256(e_proof + e_rand.tobytes() + e_check).hexdigest()
    W = (nc + nd) * (M // 4)
    assert [fc.layer_grid(W, env)[0] for env in GRID_FORMS] == [12, 1, 24, 3] and fc.layer_grid(W)[0] == 12
    assert fc.layer_grid(65, GRID_FORMS[0]) == (1, 256) and fc.layer_grid(1025, GRID_FORMS[0])[0] == 3
    rounds = sum(range(1, M.bit_length() - 1))  # layers of 2, 4, .., M / 2 entries per half: 1 + 2 + .. + 11 rounds
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, hashlib; sys.path[:0] = [%r, %r, %r]\n"
        "import pyoracle, spg\n"
        "from test_gpu_prodc import batched_inputs, gpu_prove_batched\n"
        "leaves, dotp = batched_inputs(pyoracle, %d, %d, %d, %d)\n"
        "ctx = spg.Context(0)\n"
        "ctx.prof_enable(True)\n"
        "ctx.prof_read(reset=True)\n"
        "proof, rand, check, _ = gpu_prove_batched(ctx, leaves, dotp)\n"
        "prof = ctx.prof_read()\n"
        "print(*(prof.get(k, (0,))[0] for k in ('spark_layer_round', 'spark_layer_pair', 'spark_layer_triple')))\n"
        "print(hashlib.sha256(proof + rand.tobytes() + check).hexdigest())\n"
    ) % (os.path.join(root, "tests"), os.path.join(root, "oracle"), os.path.join(root, "spartan-parallel_amd"), M, nc, nd,
         7 * M + 10 * nc + nd)
    for env in GRID_FORMS:
        res = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True,
                             timeout=240)
        assert res.returncode == 0, (env, res.stderr[-2000:])
        lines = res.stdout.strip().splitlines()
        assert lines[-1] == want, env
        assert lines[-2].split() == [str(rounds), "0", "0"], (env, lines[-2])


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(ctx, oracle):
    import spg

    L = spg.lib()
    rng = np.random.default_rng(1)
    P = ctypes.c_void_p
    arr = lambda bufs: (P * len(bufs))(*[b.handle.value for b in bufs])  # noqa: E731
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    b1, b2, b4, b6, b8 = (spg.Buf(ctx, rand_fq(oracle, rng, n)) for n in (1, 2, 4, 6, 8))
    b4b = spg.Buf(ctx, rand_fq(oracle, rng, 4))
    one = rand_fq(oracle, rng, 1)
    out = P()

    # spg_prodc_new: null pointers, unequal lengths, not a power of two, M < 2
    assert L.spg_prodc_new(ctx.handle, None, ctypes.c_size_t(1), ctypes.byref(out)) == SPG_E_ARG
    assert L.spg_prodc_new(ctx.handle, arr([b4]), ctypes.c_size_t(1), None) == SPG_E_ARG
    assert L.spg_prodc_new(ctx.handle, (P * 2)(b4.handle.value, None), ctypes.c_size_t(2), ctypes.byref(out)) == SPG_E_ARG
    assert L.spg_prodc_new(ctx.handle, arr([b4, b8]), ctypes.c_size_t(2), ctypes.byref(out)) == SPG_E_ARG
    assert L.spg_prodc_new(ctx.handle, arr([b6]), ctypes.c_size_t(1), ctypes.byref(out)) == SPG_E_ARG
    assert L.spg_prodc_new(ctx.handle, arr([b1]), ctypes.c_size_t(1), ctypes.byref(out)) == SPG_E_ARG
    assert b"power of two" in L.spg_last_error(ctx.handle)
    assert not out.value

    # spg_hash_layer: null pointers, unequal lengths, lengths that are no power of two
    init, audit = P(), P()
    reads, writes = (P * 1)(), (P * 1)()

    def hl(table, a, d, t, au):
        return L.spg_hash_layer(ctx.handle, table.handle if table else None, arr([a]), arr([d]), arr([t]),
                                ctypes.c_size_t(1), au.handle, ptr(one), ptr(one), ctypes.byref(init), reads, writes,
                                ctypes.byref(audit))

    assert hl(None, b4, b4, b4, b2) == SPG_E_ARG
    assert hl(b2, b4, b4, b4, b4) == SPG_E_ARG  # audit_ts of another length than eval_table
    assert hl(b2, b4, b8, b4, b2) == SPG_E_ARG  # derefs of another length than addrs
    assert hl(b6, b4, b4, b4, b6) == SPG_E_ARG
    assert hl(b2, b6, b6, b6, b2) == SPG_E_ARG
    assert not init.value and not audit.value and not reads[0] and not writes[0]

    # spg_prove_cubic_batched: null pointers, unequal lengths, not a power of two, more rounds than variables
    polys, r = np.zeros((4, 3, 4), np.uint64), np.zeros((4, 4), np.uint64)
    cpar, cseq = np.zeros((3, 4), np.uint64), np.zeros((3, 4), np.uint64)
    tr = spg.Transcript(b"args")

    def cb(rounds, A, B, C, t=tr, seq=False):
        par = ([arr([A]), arr([B]), ctypes.c_size_t(1), C.handle if C else None, None, None, None, ctypes.c_size_t(0)]
               if not seq else [None, None, ctypes.c_size_t(0), None, arr([A]), arr([B]), arr([C]), ctypes.c_size_t(1)])
        return L.spg_prove_cubic_batched(ctx.handle, ptr(one), ctypes.c_size_t(rounds), *par, ptr(one),
                                         t.handle if t else None, ptr(polys), ptr(r), ptr(cpar), ptr(cseq))

    assert cb(2, b4, b4b, None) == SPG_E_ARG
    assert cb(2, b4, b4b, b4, t=None) == SPG_E_ARG
    assert cb(2, b4, b8, b4) == SPG_E_ARG
    assert cb(2, b4, b4b, b8) == SPG_E_ARG
    assert cb(2, b6, b6, b6, seq=True) == SPG_E_ARG
    assert cb(3, b4, b4b, b4, seq=True) == SPG_E_ARG
    assert [b.n for b in (b4, b4b, b6, b8)] == [int(L.spg_buf_len(b.handle)) for b in (b4, b4b, b6, b8)] == [4, 4, 6, 8]

    # spg_prodc_prove_batched: dot-product vectors that do not hold M / 2 scalars, too many circuits for the mailbox
    n, rl = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rand = np.zeros((4, 4), np.uint64)
    buf = np.zeros(1 << 16, np.uint8)

    def pb(pc, dot, nd, cap=1 << 16):
        return L.spg_prodc_prove_batched(ctx.handle, pc.handle if pc else None, arr(dot) if dot else None,
                                         ctypes.c_size_t(nd), tr.handle, ptr(buf), ctypes.c_size_t(cap), ctypes.byref(n),
                                         ptr(rand), ctypes.byref(rl))

    pc = spg.ProductCircuits(ctx, [b8])
    assert pb(None, None, 0) == SPG_E_ARG
    assert pb(pc, [b4, b4b, b2], 1) == SPG_E_ARG
    assert b"M / 2" in L.spg_last_error(ctx.handle)
    many = spg.ProductCircuits(ctx, [b2] * 683)  # 3 * 683 + 1 = 2050 scalars > the mailbox's 2047
    assert pb(many, None, 0, cap=1 << 16) == SPG_E_ARG
    assert b"mailbox" in L.spg_last_error(ctx.handle)
    assert pb(pc, None, 0, cap=0) == SPG_E_ARG and n.value == pc.proof_size(0)
    # none of these consumed the circuits
    assert np.array_equal(pc.evaluate()[0], fq_prod(oracle, b8.download()))
