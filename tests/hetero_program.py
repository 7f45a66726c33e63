"""Heterogeneous programs for the whole-proof tests: block types that differ in everything the prover indexes per
block. workload.SnarkWorkload gives every block type the same squaring chain (one term per row, every coefficient 1,
the same constraint count and the same memory operations), so an index taken from the wrong order (sort position
against block number, the maximum against the per-block value) still yields the oracle's bytes. Here every block b has
its own phy[b] / vir[b] memory operations, chain[b] squarings, witness width widths[b] and extra_rows[b], and the
schedule gives unsorted, unequal block_num_proofs.

The generator emits what CirC would write, a (circ.CompileTimeKnowledge, circ.RunTimeKnowledge) pair, so the program
reaches the prover through circ.CircProgram, workload.gen_block_inst and workload.SnarkViews like any CirC file. The
trace follows SnarkWorkload.__init__ with per-block lists: block b's chain starts at column
base[b] = 2 niu + 2 phy[b] + 4 vir[b]; the memory counters run over the whole trace (physical reads cycle through the
input stack; virtual cell vc mod init_vir is stored then loaded at timestamp vc // init_vir + 1); the address-sorted
lists, D and the timestamp bit rows are built the same way.

extra_rows are constraints that hold for any witness, so the trace stays honest without a solver:
  ("lin", n)  (T, [(0, 1)], T) for n terms T with coefficients 3^i, q-1-i, 2^i      (a long linear combination)
  ("dup",)    ([(c, 3), (c, 4)], [(0, 1)], [(c, 7)])                                (a duplicate column in one row)
  ("empty",)  ([], [], [])
  ("neg",)    ([(c, q-1)], [(0, 2)], [(c, q-2)])
Columns beyond a block's chain hold random values, so these rows evaluate to something.

A new per-block field of the prover (anything read as X[b] or X[sorted position]) needs a case here in which that
field differs between blocks and block_num_proofs is not sorted."""
import types

import numpy as np

import circ
import workload

Q = workload.Q


def _row(kind, b, k, width, anchor, rng):
    """one extra row of block b (k: its index among the block's extra rows); `anchor` is a chain column every
    ("lin", n) row names, so a changed chain value sits under multi-term rows"""
    if kind[0] == "lin":
        n = kind[1]
        cols = [int(c) for c in (rng.permutation(width)[:n] if n <= width else rng.integers(0, width, n))]
        if anchor not in cols:
            cols[0] = anchor
        coef = lambda i: (pow(3, i + 5 * k + b, Q), Q - 1 - i, pow(2, i + 3 * k))[i % 3]
        T = [(c, coef(i)) for i, c in enumerate(cols)]
        return (T, [(0, 1)], list(T))
    c = int(rng.integers(2, width))
    if kind[0] == "dup":
        return ([(c, 3), (c, 4)], [(0, 1)], [(c, 7)])
    if kind[0] == "empty":
        return ([], [], [])
    assert kind[0] == "neg", kind
    return ([(c, Q - 1)], [(0, 2)], [(c, Q - 2)])


def build(num_vars, phy, vir, chain, widths, extra_rows, schedule, niu=4, max_ts_width=2, init_phy=0, init_vir=0,
          seed=0x4845544552303031):
    """-> (CompileTimeKnowledge, RunTimeKnowledge) of the program described by the per-block lists"""
    B = len(phy)
    assert all(len(v) == B for v in (vir, chain, widths, extra_rows))
    assert all(v % 2 == 0 for v in vir), "virtual operations come as store/load pairs"
    assert niu >= 5 or not any(vir), "a VIR entry's timestamp must fall on an input slot (SnarkWorkload)"
    assert not any(phy) or init_phy > 0
    assert not any(vir) or init_vir > 0
    assert schedule and all(0 <= b < B for b in schedule)
    io_width = 2 * niu
    num_ios = 1 << (io_width - 1).bit_length()
    base = [io_width + 2 * phy[b] + 4 * vir[b] for b in range(B)]
    V_in, V_out = (lambda i: 2 + i), (lambda i: 2 + (niu - 1) + i)
    rng = np.random.default_rng(seed & 0xFFFFFFFF)
    args = []
    for b in range(B):
        m, w = chain[b], widths[b]
        assert m >= 1 and not w & (w - 1) and base[b] + m + 1 <= w <= num_vars, "widths[b] must hold the chain"
        rows = [([(V_in(1), 1)], [(0, 1)], [(base[b], 1)])]
        rows += [([(base[b] + j - 1, 1)], [(base[b] + j - 1, 1)], [(base[b] + j, 1)]) for j in range(1, m + 1)]
        rows += [([(base[b] + m, 1)], [(0, 1)], [(V_out(1), 1)]), ([(V_in(2), 1)], [(0, 1)], [(V_out(2), 1)])]
        rows += [_row(kind, b, k, w, base[b] + 1, rng) for k, kind in enumerate(extra_rows[b])]
        for row in rows:
            assert all(0 <= c < w for terms in row for c, _ in terms), "a row names a column beyond widths[b]"
        args.append(rows)
    # ---- execution trace (workload.SnarkWorkload.__init__ with per-block phy / vir / chain / width)
    E = len(schedule)
    seeds, st = workload.random_fq(2, seed)
    x, y = int(seeds[0]), int(seeds[1])
    x0 = x
    stack, st = workload.random_fq(max(init_phy, 1), st)
    imem, st = workload.random_fq(max(init_vir, 1), st)
    n_pairs = sum(vir[b] // 2 for b in schedule)
    vir_data, st = workload.random_fq(max(n_pairs, 1), st)
    input_stack = [int(v) for v in stack[:init_phy]]
    input_mem = [int(v) for v in imem[:init_vir]]
    phy_acc = [(a, input_stack[a]) for a in range(init_phy)]
    vir_acc = [(a, input_mem[a], 0, 0) for a in range(init_vir)]
    per_block = [[] for _ in range(B)]
    exec_rows = []
    pc = vc = 0
    for k in range(E):
        b = schedule[k]
        nb = schedule[k + 1] if k + 1 < E else B
        ch = [x]
        for _ in range(chain[b]):
            ch.append(ch[-1] * ch[-1] % Q)
        xo = ch[-1]
        io = [1, 0, b, x, y] + [0] * (niu - 4) + [nb, xo, y] + [0] * (niu - 4)
        exec_rows.append(io + [0] * (num_ios - len(io)))
        memv = []
        for _ in range(phy[b]):
            a = pc % init_phy
            pc += 1
            memv += [a, input_stack[a]]
            phy_acc.append((a, input_stack[a]))
        for _ in range(vir[b] // 2):
            a, d, ts = vc % init_vir, int(vir_data[vc]), vc // init_vir + 1
            vc += 1
            memv += [a, d, 0, ts, a, d, 1, ts]
            vir_acc += [(a, d, 0, ts), (a, d, 1, ts)]
        fill, st = workload.random_fq(widths[b], st)
        row = io + memv + ch
        per_block[b].append(row + [int(v) for v in fill[len(row):]])
        x = xo

    def mems(acc, width):  # D = v_next * (v + addr - addr_next) (gen_pairwise_check_inst)
        out = []
        for j, e in enumerate(acc):
            D = 0 if j + 1 == len(acc) else (1 + e[0] - acc[j + 1][0]) % Q
            out.append([1, D] + list(e) + [0] * (width - 2 - len(e)))
        return out

    phy_acc.sort(key=lambda e: e[0])  # stable: the init entry of a cell precedes its reads
    vir_acc.sort(key=lambda e: (e[0], e[3], e[2]))
    ts_size = 1 << (2 + max_ts_width - 1).bit_length()
    addr_vir = mems(vir_acc, 8) if any(vir) else []
    ts_bits = []
    for j, e in enumerate(addr_vir):
        nxt = addr_vir[j + 1] if j + 1 < len(addr_vir) else [0] * 8
        diff = (nxt[5] - e[5]) % Q if e[1] else 0
        assert diff < (1 << max_ts_width)
        r = [e[1] * nxt[4] % Q, 0] + [(diff >> i) & 1 for i in range(max_ts_width)]
        ts_bits.append(r + [0] * (ts_size - len(r)))
    block_vars = [workload.to_mont_limbs(np.array(r, dtype=object).reshape(-1)).reshape(len(r), w, 4)
                  for r, w in zip(per_block, widths)]
    nproofs = [len(r) for r in per_block]
    order = sorted(range(B), key=lambda b: -nproofs[b])
    t = types.SimpleNamespace(
        num_blocks=B, num_vars=num_vars, num_inputs_unpadded=niu, num_vars_per_block=list(widths),
        block_num_phy_ops=list(phy), block_num_vir_ops=list(vir), max_ts_width=max_ts_width, args=args,
        input_liveness=[False, False, True], func_input_width=1, input_offset=1, input_block_num=schedule[0],
        output_offset=2, output_block_num=B, block_max_num_proofs=max(nproofs), block_num_proofs=nproofs,
        consis_num_proofs=E, block_vars_sorted=[block_vars[b] for b in order],
        exec_inputs=workload.to_mont_limbs(np.array(exec_rows, dtype=object).reshape(-1)).reshape(E, num_ios, 4),
        init_phy_mems=[[1, 0, a, v] for a, v in enumerate(input_stack)],
        init_vir_mems=[[1, 0, a, v] for a, v in enumerate(input_mem)],
        addr_phy_mems=mems(phy_acc, 4) if any(phy) else [], addr_vir_mems=addr_vir, addr_ts_bits=ts_bits,
        input=workload.to_mont_limbs([0, 0, x0]), input_stack=input_stack, input_mem=input_mem,
        output_mont=workload.to_mont_limbs([x])[0], output_exec_num=E - 1)
    return circ.export_workload(t)


def _lin(*ns):
    return [("lin", n) for n in ns]


CASES = {
    # padded constraint counts 32 / 128 / 64, all three blocks with their own memory operations; block 1 has the most
    # constraints (extra rows) and the fewest executions; block_num_proofs = [4, 1, 4]; power-of-two input stack and
    # memory (what SNARK::verify's public arguments need)
    "hetero_mem_b3": dict(
        num_vars=64, niu=5, phy=[0, 2, 1], vir=[2, 0, 4], chain=[2, 3, 10], widths=[32, 64, 64],
        extra_rows=[[("lin", 20), ("empty",)],
                    _lin(48, 33, 20, 41) * 9 + [("dup",), ("empty",), ("neg",), ("dup",)],
                    [("lin", 45), ("dup",), ("neg",), ("empty",), ("lin", 24), ("lin", 31)]],
        schedule=[2, 0, 2, 2, 0, 2, 1, 0, 0], init_phy=4, init_vir=8),
    # no memory: block 2 never runs, block 1 runs once, block_num_proofs = [3, 1, 0, 2]; padded counts 32 / 32 / 64 / 128
    "hetero_nomem_b4": dict(
        num_vars=64, niu=4, phy=[0] * 4, vir=[0] * 4, chain=[5, 1, 20, 9], widths=[64, 16, 32, 64],
        extra_rows=[[("lin", 44), ("dup",), ("empty",)], [], _lin(20, 32, 27) * 4 + [("neg",), ("empty",), ("dup",)],
                    _lin(21, 30) * 20 + [("neg",)]],
        schedule=[3, 0, 1, 0, 3, 0]),
    # more block types than one launch's kernel arguments hold (kMaxP = 32): constraint counts 32 / 64 and widths
    # 32 / 64 alternating, executions 2 / 1 / 1 / 0 by block number mod 4, physical reads 0 / 1 / 2 by block number mod 3
    "hetero_b33": dict(
        num_vars=64, niu=4, phy=[b % 3 for b in range(33)], vir=[0] * 33, init_phy=4,
        chain=[3 if b % 2 == 0 else 12 for b in range(33)],
        widths=[32 if b % 2 == 0 else 64 for b in range(33)],
        extra_rows=[[("lin", 20), ("empty",)] if b % 2 == 0 else _lin(40, 22) * 6 + [("dup",), ("empty",), ("neg",)]
                    for b in range(33)],
        schedule=[b for b in range(33) if b % 4 != 3] + [b for b in range(0, 33, 4)]),
}


def program(case):
    """the case as a circ.CircProgram, with the public values workload.SnarkPublic reads (SnarkWorkload's names)"""
    ctk, rtk = build(**CASES[case])
    return with_public(circ.CircProgram(ctk, rtk), rtk)


def with_public(prog, rtk):
    as_int = lambda b: int.from_bytes(b, "little")
    prog.x0 = as_int(rtk.input[-1])
    prog.output = as_int(rtk.output)
    prog.input_stack = [as_int(b) for b in rtk.input_stack]
    prog.input_mem = [as_int(b) for b in rtk.input_mem]
    return prog


def chain_column(case, b):
    """a chain column of block b that its ("lin", n) rows name too"""
    c = CASES[case]
    return 2 * c.get("niu", 4) + 2 * c["phy"][b] + 4 * c["vir"][b] + 1


def tampered(case):
    """the program with one witness value changed: a chain value of the first execution of the block with the most
    executions, a column its chain rows and its multi-term rows name"""
    prog = program(case)
    b = max(range(prog.num_blocks), key=lambda i: prog.block_num_proofs[i])  # sort position 0 (stable)
    v = prog.block_vars_sorted[0]
    v[0, chain_column(case, b)] = workload.to_mont_limbs([12345])[0]
    return prog
