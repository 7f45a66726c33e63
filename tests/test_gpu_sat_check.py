"""Witness satisfiability on the device: spg_pqx_sat_check, spg_r1cs_sat_check, spg_snark_check and the provers'
check mode (spg_set_check_sat), against the Python-integer reference of tests/sat_ref.py.

Shapes: sparse_cases.satisfiable() has 4 * 64 + 2 * 16 = 288 rows, two workgroups of k_sat_check with the second one
partial, and its last row is (1, 1, 15). The structured cases add a shared matrix triple with a one-execution
instance (lg_q = 0), 8 workgroups over tables the tiled SpMV wrote, and 36 instances, whose descriptors go through
device memory.

spg_snark_report fields no case here sets, and why: sat[perm_root] (tests/sat_cases.py: the instance constrains what
the prover derives itself); every other field is set by some case below."""
import ctypes
import os
import socket

import numpy as np
import pytest

import hetero_program
import sat_cases
import sat_ref
import sparse_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENS_LABEL = b"gens_r1cs_sat"
GENS_NV = 1 << 24


@pytest.fixture(scope="module")
def gens(ctx):
    import spg

    return spg.R1CSGens(ctx, GENS_LABEL, GENS_NV)


class Loaded:
    """a workload on the device, with its reference report"""

    def __init__(self, ctx, wl):
        import spg
        import workload

        self.ctx, self.wl = ctx, wl
        self.v = workload.CViews(wl)
        self.inst = spg.R1CSInst(ctx, self.v.inst)
        self.wit = spg.R1CSWitness(ctx, self.v.secs, wl.nws)
        self.ref = sat_ref.report(wl)

    def shape(self):
        wl = self.wl
        return wl.P, wl.max_num_proofs, wl.num_proofs, wl.max_num_inputs, wl.num_inputs

    def r1cs_check(self):
        import spg

        return spg.r1cs_sat_check(self.ctx, self.inst, self.wit, *self.shape())

    def z(self):
        """z_mat (p, q, w, x) of multiply_vec_block"""
        wl = self.wl
        return np.concatenate([np.stack([wl.sections[w][p] for w in range(wl.nws)], axis=1).reshape(-1, 4)
                               for p in range(wl.P)])

    def tables(self):
        import spg

        wl = self.wl
        return spg.r1cs_multiply_vec_block(self.ctx, self.inst, wl.num_proofs, wl.max_num_proofs, wl.num_inputs,
                                           wl.max_num_inputs, wl.nws, self.z())

    def pqx_check(self):
        import spg

        return spg.pqx_sat_check(self.ctx, *self.tables())

    def prove(self, gens, label=b"sat_test"):
        """(return code, proof bytes, proof_len, spg_last_error) of spg_r1cs_prove, whatever it returns"""
        import spg
        import workload

        P, mnp, npf, mni, nin = self.shape()
        cap = 1 << 22
        buf = self.ctx.out_buf(cap)
        ln = ctypes.c_size_t(123)
        tr, tape = spg.Transcript(label), spg.RandomTape(b"proof", workload.tape_seed())
        rc = spg.lib().spg_r1cs_prove(self.ctx.handle, gens.handle, self.inst.handle, P, mnp,
                                      (ctypes.c_size_t * P)(*npf), mni, (ctypes.c_size_t * P)(*nin), self.wit.handle,
                                      tr.handle, tape.handle, spg._p(buf), cap, ctypes.byref(ln), None, None)
        err = spg.lib().spg_last_error(self.ctx.handle).decode(errors="replace") if rc else ""
        return rc, buf[: ln.value].tobytes(), ln.value, err


def _same(got, ref):
    assert tuple(got) == tuple(ref), (got, ref)


@pytest.fixture(scope="module")
def honest(ctx):
    return Loaded(ctx, sparse_cases.satisfiable())


def test_satisfiable_has_no_violation(honest):
    assert honest.ref.violations == 0 and honest.ref.rows == 288
    _same(honest.r1cs_check(), honest.ref)
    _same(honest.pqx_check(), honest.ref)


def test_check_mode_leaves_an_honest_proof_alone(honest, gens, ctx):
    """the same bytes with the mode on and off; one sat_check launch with it on, none with it off"""
    rc, _, _, err = honest.prove(gens)  # (what only a context's first prove launches stays out of the counts)
    assert rc == 0, err
    ctx.prof_enable(True)
    try:
        ctx.prof_read()
        rc, off, _, err = honest.prove(gens)
        assert rc == 0, err
        prof_off = ctx.prof_read()
        ctx.set_check_sat(True)
        rc, on, _, err = honest.prove(gens)
        assert rc == 0, err
        prof_on = ctx.prof_read()
    finally:
        ctx.set_check_sat(False)
        ctx.prof_enable(False)
    assert on == off and len(on) > 0
    assert "sat_check" not in prof_off and prof_off["spmv_block"][0] == 1
    assert prof_on["sat_check"][0] == 1 and prof_on["sat_check"][2] == 96.0 * 288
    assert {k: v[0] for k, v in prof_on.items() if k != "sat_check"} == {k: v[0] for k, v in prof_off.items()}


def test_one_changed_scalar_is_named(ctx, gens):
    import spg

    w = Loaded(ctx, sat_cases.one_change())
    assert (w.ref.violations, w.ref.p, w.ref.q, w.ref.row) == (1, 1, 1, 15)  # the last row of the domain
    _same(w.r1cs_check(), w.ref)
    _same(w.pqx_check(), w.ref)
    rc, proof, _, _ = w.prove(gens)  # mode off: the prover still writes a proof
    assert rc == 0 and len(proof) > 0
    ctx.set_check_sat(True)
    try:
        rc, _, proof_len, err = w.prove(gens)
    finally:
        ctx.set_check_sat(False)
    assert rc == spg.SPG_E_UNSAT and proof_len == 0
    assert "R1CS unsatisfied: instance 1 execution 1 constraint 15 (1 of 288 rows)" in err, err


def test_two_changes_report_the_lower_row(ctx):
    w = Loaded(ctx, sat_cases.two_changes())
    assert (w.ref.violations, w.ref.p, w.ref.q, w.ref.row) == (2, 0, 2, 40)
    _same(w.r1cs_check(), w.ref)
    _same(w.pqx_check(), w.ref)


@pytest.mark.parametrize("case", sorted(sparse_cases.CASES))
def test_structured_cases_match_the_reference(ctx, case):
    w = Loaded(ctx, sparse_cases.structured(case))
    assert w.ref.rows == sum(x * q for x, q in zip(*sparse_cases.CASES[case][:2]))
    _same(w.r1cs_check(), w.ref)
    _same(w.pqx_check(), w.ref)  # (multiply_vec_block serves a shared triple too)


def test_every_row_broken(ctx):
    w = Loaded(ctx, sat_cases.every_row_broken())
    assert w.ref.violations == w.ref.rows == 64 and (w.ref.p, w.ref.q, w.ref.row) == (0, 0, 0)
    _same(w.r1cs_check(), w.ref)
    _same(w.pqx_check(), w.ref)


def test_more_instances_than_kernel_arguments_hold(ctx):
    """36 instances: the descriptors go through device memory. R1CSWorkload's own witness holds; z[2] of (instance 33,
    execution 1) changed breaks z[1]^2 = z[2] and z[2]^2 = z[3] there, and one more row in instance 35"""
    w = Loaded(ctx, sat_cases.many_instances())
    assert w.ref.rows == 108 and w.ref.violations == 0
    _same(w.r1cs_check(), w.ref)
    _same(w.pqx_check(), w.ref)
    wl = sat_ref.tamper(sat_ref.tamper(sat_cases.many_instances(), 33, 1, 2), 35, 0, 3)
    w = Loaded(ctx, wl)
    assert (w.ref.violations, w.ref.p, w.ref.q, w.ref.row) == (3, 33, 1, 0)
    _same(w.r1cs_check(), w.ref)
    _same(w.pqx_check(), w.ref)


def test_pqx_check_refuses_other_tables(ctx, honest):
    import spg

    Az, Bz, Cz = honest.tables()
    assert spg.pqx_sat_check(ctx, Az, Bz, Cz).violations == 0
    other = Loaded(ctx, sat_cases.every_row_broken()).tables()
    rep = spg.CSatReport()
    rc = spg.lib().spg_pqx_sat_check(ctx.handle, Az.handle, other[1].handle, Cz.handle, ctypes.byref(rep))
    assert rc == spg.SPG_E_ARG  # mismatched shapes
    r = np.asarray([5, 0, 0, 0], dtype=np.uint64)
    Cz.bound(r, 4)  # one x variable bound: the current sizes leave the allocation sizes
    rc = spg.lib().spg_pqx_sat_check(ctx.handle, Az.handle, Bz.handle, Cz.handle, ctypes.byref(rep))
    assert rc == spg.SPG_E_ARG
    Az.bound(r, 4)
    Bz.bound(r, 4)
    rc = spg.lib().spg_pqx_sat_check(ctx.handle, Az.handle, Bz.handle, Cz.handle, ctypes.byref(rep))
    assert rc == spg.SPG_E_ARG  # all three bound alike: still not the tables multiply_vec_block returns


# ---- whole programs -------------------------------------------------------------------------------------------------
class Program:
    def __init__(self, ctx, gens, prog):
        import spg
        import workload

        self.ctx, self.gens, self.prog = ctx, gens, prog
        self.v = workload.SnarkViews(prog)
        self.block = spg.SnarkComp(ctx, self.v.block, multi=True)
        self.pairwise = spg.SnarkComp(ctx, self.v.pairwise)
        self.perm_root = spg.SnarkComp(ctx, self.v.perm_root)
        self.wit = spg.SnarkWitness(ctx, self.v.inputs)

    def check(self, label=b"snark_test"):
        import spg

        return spg.snark_check(self.ctx, self.block, self.pairwise, self.perm_root, self.wit, self.gens,
                               spg.Transcript(label))

    def prove(self, label=b"snark_test"):
        import spg
        import workload

        return spg.snark_prove(self.ctx, self.block, self.pairwise, self.perm_root, self.wit, self.gens,
                               spg.Transcript(label), spg.RandomTape(b"proof", workload.tape_seed()))

    def verify(self, proof, label=b"snark_test"):
        import spg

        return spg.snark_verify(self.ctx, self.block, self.pairwise, self.perm_root, self.v.inputs, self.gens,
                                spg.Transcript(label), proof)


def _clean(rep):
    import spg

    assert rep.first == spg.FIRST_NONE and rep.io_point == -1 and rep.perm_products == (0, 0, 0), rep
    assert all(s.violations == 0 and s.rows > 0 for s in rep.sat), rep


SNARK_CASES = ("hetero_mem_b3", "hetero_nomem_b4")


@pytest.mark.parametrize("case", SNARK_CASES + ("hetero_b33",))
def test_snark_check_passes_an_honest_program(ctx, gens, case):
    rep, err = Program(ctx, gens, hetero_program.program(case)).check()
    _clean(rep)
    assert err == ""


@pytest.mark.parametrize("case", SNARK_CASES)
def test_snark_check_names_a_tampered_block(ctx, gens, case):
    import spg

    prog = hetero_program.tampered(case)
    b = max(range(prog.num_blocks), key=lambda i: prog.block_num_proofs[i])
    p = Program(ctx, gens, prog)
    rep, err = p.check()
    assert rep.first == spg.SAT_BLOCK and rep.component[spg.SAT_BLOCK] == b, rep
    s = rep.sat[spg.SAT_BLOCK]
    assert s.violations > 0 and s.p == 0 and s.q == 0 and (s.az * s.bz - s.cz) % sat_ref.Q != 0
    assert err.startswith("block: R1CS unsatisfied: instance 0 execution 0 constraint %d " % s.row), err
    assert err.endswith("block %d" % b), err
    # mode off: the prover still writes a proof, which the verifier rejects
    proof = p.prove()
    ok, why = p.verify(proof)
    assert not ok and why
    ctx.set_check_sat(True)
    try:
        with pytest.raises(spg.SpgError) as e:
            p.prove()
    finally:
        ctx.set_check_sat(False)
    msg = str(e.value)
    assert "SPG_E_UNSAT" in msg and "block: R1CS unsatisfied: instance 0 execution 0" in msg, msg
    assert msg.endswith("block %d" % b), msg


@pytest.mark.parametrize("case", SNARK_CASES)
def test_check_mode_leaves_an_honest_snark_alone(ctx, gens, case):
    p = Program(ctx, gens, hetero_program.program(case))
    off = p.prove()
    ctx.set_check_sat(True)
    try:
        on = p.prove()
    finally:
        ctx.set_check_sat(False)
    assert on == off
    ok, why = p.verify(on)
    assert ok, why


@pytest.mark.parametrize("case", SNARK_CASES)
def test_snark_check_sees_another_public_output(ctx, gens, case):
    """the public output changed as test_gpu_hetero.test_hetero_verify_rejects_other_output changes it"""
    import spg
    import workload

    prog = hetero_program.program(case)
    prog.output_mont = np.ascontiguousarray(workload.to_mont_limbs([(prog.output + 1) % workload.Q])[0])
    rep, err = Program(ctx, gens, prog).check()
    assert rep.io_point >= 0 and rep.first == spg.FIRST_IO, rep
    assert all(s.violations == 0 for s in rep.sat) and rep.perm_products == (0, 0, 0)
    assert "IO proof" in err


@pytest.mark.parametrize("case", SNARK_CASES)
def test_snark_check_sees_a_changed_exec_input(ctx, gens, case):
    """execution 1's input no longer equals execution 0's output, and the product over the exec rows leaves the
    product over the block rows; the block instances themselves still hold"""
    import spg

    rep, err = Program(ctx, gens, sat_cases.exec_input_changed(case)).check()
    assert rep.sat[spg.SAT_BLOCK].violations == 0
    s = rep.sat[spg.SAT_PAIRWISE]
    assert s.violations > 0 and rep.component[spg.SAT_PAIRWISE] == spg.PAIRWISE_CONSIS, rep
    assert rep.perm_products[spg.PERM_EXEC] == 1
    assert rep.first == spg.SAT_PAIRWISE and err.startswith("pairwise: R1CS unsatisfied"), (rep, err)
    assert rep.sat[spg.SAT_PERM_ROOT].violations == 0 and rep.io_point == -1


def test_snark_check_sees_changed_memory_lists(ctx, gens):
    import spg

    rep, _ = Program(ctx, gens, sat_cases.phy_list_changed("hetero_mem_b3")).check()
    assert rep.perm_products[spg.PERM_PHY] == 1 and rep.perm_products[spg.PERM_EXEC] == 0, rep
    assert rep.sat[spg.SAT_BLOCK].violations == 0 and rep.first in (spg.SAT_PAIRWISE, spg.FIRST_PERM_PHY)
    if rep.sat[spg.SAT_PAIRWISE].violations:
        assert rep.component[spg.SAT_PAIRWISE] == spg.PAIRWISE_PHY
    rep, _ = Program(ctx, gens, sat_cases.vir_list_changed("hetero_mem_b3")).check()
    assert rep.perm_products[spg.PERM_VIR] == 1 and rep.perm_products[spg.PERM_EXEC] == 0, rep
    assert rep.sat[spg.SAT_BLOCK].violations == 0 and rep.first in (spg.SAT_PAIRWISE, spg.FIRST_PERM_VIR)
    if rep.sat[spg.SAT_PAIRWISE].violations:
        assert rep.component[spg.SAT_PAIRWISE] == spg.PAIRWISE_VIR


# ---- two ranks on one GPU (gloo), launched as tests/test_gpu_dist.py launches its ranks ------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys

    sys.path[:0] = [os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "tests")]
    import torch.distributed as dist

    import sat_cases
    import spg
    import workload

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["SPG_PIN"] = "0"  # the ranks share the test box's GPU
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        wl = sat_cases.one_change()  # the violation lies in instance 1: rank 0's shard is clean
        ctx = spg.Context(0)
        ctx.set_comm(rank, world, spg.torch_allgather(dist))
        v = workload.CViews(wl)
        inst = spg.R1CSInst(ctx, v.inst)
        wit = spg.R1CSWitness(ctx, v.secs, wl.nws, shard=spg.shard_range(wl.P, rank, world))
        shape = (wl.P, wl.max_num_proofs, wl.num_proofs, wl.max_num_inputs, wl.num_inputs)
        rep = spg.r1cs_sat_check(ctx, inst, wit, *shape)
        ctx.set_check_sat(True)
        gens = spg.R1CSGens(ctx, b"gens_r1cs_sat", 1 << 24)
        err = None
        try:
            spg.r1cs_prove(ctx, gens, inst, wit, *shape, spg.Transcript(b"sat_test"),
                           spg.RandomTape(b"proof", workload.tape_seed()))
        except spg.SpgError as e:
            err = str(e)
        q.put((rank, tuple(rep), err))
    except Exception as e:  # noqa: BLE001
        q.put((rank, None, repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_share_the_report_and_the_verdict():
    import queue

    import torch.multiprocessing as mp

    ref = sat_ref.report(sat_cases.one_change())
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    ps = [mpc.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = []
    try:
        for _ in range(2):
            res.append(q.get(timeout=120))
    except queue.Empty:
        pass
    for p in ps:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    assert len(res) == 2, f"only ranks {sorted(r[0] for r in res)} returned: a rank is blocked"
    for rank, rep, err in sorted(res):
        assert rep is not None, err
        assert rep == tuple(ref), f"rank {rank}: {rep}"
        assert err and "SPG_E_UNSAT" in err and "instance 1 execution 1 constraint 15 (1 of 288 rows)" in err, (rank, err)
