"""Multi-process path on the CPU (gloo, world_size 2): the allgather adapter that shards R1CSProof::prove
across ranks (spg.torch_allgather -> spg_set_comm) carries each rank's partial round sums to every rank, and
the product's exchange code (comm.hpp, which api.hip's comm_sum_fq and so Prover::sum_ranks run; exported by
libspg_hostcheck.so) adds them exactly mod q and fails every rank alike when one rank reports an error."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys

    sys.path[:0] = [os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "oracle")]
    import torch.distributed as dist

    import spg

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hc = ctypes.CDLL(os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg_hostcheck.so"))
        fn = spg.torch_allgather(dist)
        rng = np.random.default_rng(100 + rank)
        mine = rng.integers(0, 2**63, (3, 4), dtype=np.uint64)
        mine[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
        out = np.zeros((3, 4), dtype=np.uint64)
        rc = hc.spgh_comm_sum(fn, None, world, 0, mine.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(3),
                              out.ctypes.data_as(ctypes.c_void_p))
        # an error on the last rank only (a local HIP failure, -3): every rank's exchange returns it
        junk = np.zeros((3, 4), dtype=np.uint64)
        rc_fail = hc.spgh_comm_sum(fn, None, world, -3 if rank == world - 1 else 0,
                                   mine.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(3),
                                   junk.ctypes.data_as(ctypes.c_void_p))
        # raw gather through the same adapter: rank-ordered concatenation
        raw = (ctypes.c_uint8 * (8 * world))()
        send = (ctypes.c_uint8 * 8)(*([rank + 1] * 8))
        rc2 = fn(None, ctypes.addressof(send), 8, ctypes.addressof(raw))
        q.put((rank, rc, rc2, mine.tolist(), out.tolist(), list(raw), rc_fail))
    finally:
        dist.destroy_process_group()


def test_allgather_sum_two_ranks(oracle):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in ps:
        p.join(timeout=60)
    res.sort()
    parts = [np.array(r[3], dtype=np.uint64) for r in res]
    expect = oracle.fq_op("add", parts[0], parts[1])
    for rank, rc, rc2, _, out, raw, rc_fail in res:
        assert rc == 0 and rc2 == 0 and rc_fail == -3
        assert np.array_equal(np.array(out, dtype=np.uint64), expect)
        assert raw == [1] * 8 + [2] * 8


def _msm_worker(rank, world, port, q):
    import sys

    sys.path[:0] = [os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "oracle")]
    import torch.distributed as dist

    import pyoracle
    import shard

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n = 37  # ragged split over the ranks
        pts = pyoracle.gens_stream(b"spg_bench_msm", n + 1)[:n]
        rng = np.random.default_rng(7)
        Z = pyoracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * n, dtype=np.uint8).tobytes())
        got, _ = shard.sharded_msm(dist, lambda lo, hi: pyoracle.msm_partial(pts[lo:hi], Z[lo:hi]), n)
        q.put((rank, got, pyoracle.msm(pts, Z)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_msm_matches_single(oracle, world):
    """contiguous shards, one allgather of uncompressed partials, exact host sum == the
    unsharded MSM (partials from the CPU oracle; tests/test_gpu_dist.py runs the device partials)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_msm_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in ps:
        p.join(timeout=60)
    for rank, got, ref in res:
        assert got == ref, rank


def test_shard_chunks_cover():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "spartan-parallel_amd"))
    import shard

    for n in (0, 1, 7, 64, 65537):
        for w in (1, 2, 3, 8):
            cs = [shard.chunk(n, r, w) for r in range(w)]
            assert cs[0][0] == 0 and cs[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(cs, cs[1:]))
            assert max(h - l for l, h in cs) - min(h - l for l, h in cs) <= 1


# ---- sharded SPARK layout (spark.hip "sharded proof"), restated with Python integers mod q on gloo ranks -----
Qmod = 2**252 + 27742317777372353535851937790883648493


def _eq(r, n):
    """EqPolynomial::evals (src/dense_mlpoly.rs:76-92), r[0] the most significant bit"""
    out = []
    for b in range(1 << n):
        acc = 1
        for j in range(n):
            acc = acc * (r[j] if (b >> (n - 1 - j)) & 1 else 1 - r[j]) % Qmod
        out.append(acc)
    return out


def _layer_rounds(A, B, C, rs, W=1, sum_fn=None):
    """prove_cubic_batched rounds (src/sumcheck.rs:264-434) of one (A, B, C) triple, binding the top variable;
    returns [(e0, e2, e3)] per round (summed over ranks by sum_fn) and the folded vectors"""
    evs = []
    for r in rs:
        ln = len(A) // 2
        e = [0, 0, 0]
        for i in range(ln):
            for k, x in enumerate((0, 2, 3)):
                a = A[i] + x * (A[i + ln] - A[i])
                b = B[i] + x * (B[i + ln] - B[i])
                c = C[i] + x * (C[i + ln] - C[i])
                e[k] = (e[k] + a * b * c) % Qmod
        if sum_fn:
            e = sum_fn(e)
        evs.append(tuple(e))
        A = [(A[i] + r * (A[i + ln] - A[i])) % Qmod for i in range(ln)]
        B = [(B[i] + r * (B[i + ln] - B[i])) % Qmod for i in range(ln)]
        C = [(C[i] + r * (C[i + ln] - C[i])) % Qmod for i in range(ln)]
    return evs, (A, B, C)


def _tree_worker(rank, world, port, q):
    import random

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rnd = random.Random(11)
        M = 32
        leaves = [rnd.randrange(Qmod) for _ in range(M)]
        # local product tree over leaves i = W i' + r (ProductCircuit::compute_layer keeps the low bits)
        v = leaves[rank::world]
        while len(v) > 1:
            h = len(v) // 2
            v = [v[i] * v[i + h] % Qmod for i in range(h)]
        level = [None] * world
        dist.all_gather_object(level, v[0])  # the global level of W entries, index = rank

        def allsum(e):
            parts = [None] * world
            dist.all_gather_object(parts, e)
            return [sum(p[k] for p in parts) % Qmod for k in range(3)]

        # layer 0 of the circuit: left / right halves of the leaves, eq over lg(M/2) variables
        half = M // 2
        lgh, lgw = half.bit_length() - 1, world.bit_length() - 1
        rand = [rnd.randrange(Qmod) for _ in range(lgh)]
        rs = [rnd.randrange(Qmod) for _ in range(lgh)]
        left, right = leaves[:half], leaves[half:]
        # local shares: left/right keep i = W i' + r; eq share = eq(rand_hi) * eq(rand_lo)[r]
        sc = _eq(rand[lgh - lgw:], lgw)[rank]
        Cl = [x * sc % Qmod for x in _eq(rand[:lgh - lgw], lgh - lgw)]
        nloc = lgh - lgw
        ev_loc, (Af, Bf, Cf) = _layer_rounds(left[rank::world], right[rank::world], Cl, rs[:nloc], sum_fn=allsum)
        g = [None] * world
        dist.all_gather_object(g, (Af[0], Bf[0], Cf[0]))  # the gather: one entry per rank, index = rank
        ev_rep, fin = _layer_rounds([x[0] for x in g], [x[1] for x in g], [x[2] for x in g], rs[nloc:])
        q.put((rank, level, ev_loc + ev_rep, [f[0] for f in fin]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_interleaved_product_tree_shards(world):
    """the sharded SPARK layout (spark.hip spark_prove_core / batched_prove): interleaved local product
    trees meet the global tree's W-entry level, and local layer rounds summed over gloo ranks + gathered tail
    rounds give the unsharded round polynomials and final claims"""
    import random

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_tree_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in ps:
        p.join(timeout=60)
    rnd = random.Random(11)
    M = 32
    leaves = [rnd.randrange(Qmod) for _ in range(M)]
    v = leaves
    while len(v) > world:
        h = len(v) // 2
        v = [v[i] * v[i + h] % Qmod for i in range(h)]
    half = M // 2
    lgh = half.bit_length() - 1
    rand = [rnd.randrange(Qmod) for _ in range(lgh)]
    rs = [rnd.randrange(Qmod) for _ in range(lgh)]
    ev, fin = _layer_rounds(leaves[:half], leaves[half:], _eq(rand, lgh), rs)
    for rank, level, evs, f in res:
        assert level == v, rank
        assert evs == ev, rank
        assert f == [x[0] for x in fin], rank
