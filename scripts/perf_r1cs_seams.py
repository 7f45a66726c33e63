"""What the seam boundary costs over the fused R1CS prover, one GPU command, at SURVEY 8d config 4's shape with five
witness sections (P = 8 instances x Q = 2^9 proofs x X = 2^10 constraints; --instances / --log-proofs / --log-cons /
--sections for other shapes):

  1. the seams of R1CSProof::prove on caller tables: spg_pqx_new_rev_buf, spg_pqx_bound_rq against the same binds one
     call each, spg_r1cs_eval_tables, spg_r1cs_abc_poly, spg_zk_phase1_prove, spg_zk_phase2_prove -- the device-event
     time of each call (spg_last_kernel_us; for the two provers it spans the whole round loop, host work between the
     launches included) with the host clock around the call beside it, median of --reps;
  2. spg_r1cs_prove on the same matrices and witness with spg_prof on: the per-kernel records of the fused prover
     (eval_table_abc, z_fill, the phase-1 / phase-2 evaluations and folds) to set beside them.

The matrices are workload.R1CSWorkload's; the witness is uniform random scalars (the costs do not depend on values).
Writes profiles/r1cs_seams.json (--out). The run ends at the first GPU call that raises: nothing more is started on
the GPU after that, what was measured up to there is written with a "stopped" entry, and the exit status is 1."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "oracle")]
import spg  # noqa: E402
import workload  # noqa: E402

T0 = time.perf_counter()


def log(*a):
    print("[%6.1fs]" % (time.perf_counter() - T0), *a, flush=True)


def rand_limbs(rng, n):
    """n uniform values below 2^252 taken as Montgomery representations"""
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4),
                                                                                            dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8)
    ap.add_argument("--log-proofs", type=int, default=9)
    ap.add_argument("--log-cons", type=int, default=10)
    ap.add_argument("--sections", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_seams.json"))
    a = ap.parse_args()
    P, Q, X, nws = a.instances, 1 << a.log_proofs, 1 << a.log_cons, a.sections
    wl = workload.R1CSWorkload([X] * P, [1] * P, num_sections=nws)  # the matrices; the witness comes below
    Y = wl.max_num_inputs
    wl.num_proofs, wl.max_num_proofs = [Q] * P, Q
    rng = np.random.default_rng(4)
    z = rand_limbs(rng, P * Q * nws * Y)
    log("shape", dict(P=P, Q=Q, X=X, nws=nws, Y=Y), "z: %.0f MB" % (z.nbytes / 1e6))
    res = {"shape": dict(instances=P, num_proofs=Q, num_cons=X, sections=nws, max_num_inputs=Y), "seams": {}}
    lx, lq, lp, lw, ly = ((n - 1).bit_length() for n in (X, Q, P, nws, Y))
    shape = (wl.num_proofs, Q, nws, wl.num_inputs, Y)
    try:
        ctx = spg.Context(0)
        gens = spg.R1CSGens(ctx, b"gens_r1cs_sat", 1 << 24)
        v = workload.CViews(wl)
        inst = spg.R1CSInst(ctx, v.inst)
        zbuf = spg.Buf(ctx, z)
        seed = workload.tape_seed()

        def timed(name, fn, reps=a.reps):
            wall, dev, out = [], [], None
            for _ in range(reps):
                out = None  # (the previous result's device memory goes before the next call allocates)
                t = time.perf_counter()
                out = fn()
                wall.append((time.perf_counter() - t) * 1e6)
                dev.append(ctx.last_kernel_us())
            res["seams"][name] = dict(device_us=med(dev), wall_us=med(wall))
            log(name, res["seams"][name])
            return out

        timed("pqx_new_rev_buf", lambda: spg.Pqx.new_rev(ctx, zbuf, *shape))
        rq = rand_limbs(rng, lq)
        one, each = [], []
        for _ in range(a.reps):
            Z = spg.Pqx.new_rev(ctx, zbuf, *shape)
            t = time.perf_counter()
            Z.bound_rq(rq)
            one.append(((time.perf_counter() - t) * 1e6, ctx.last_kernel_us()))
            Z = None
            Z = spg.Pqx.new_rev(ctx, zbuf, *shape)
            t = time.perf_counter()
            for k in range(lq):
                Z.bound(rq[k], 2)
            each.append((time.perf_counter() - t) * 1e6)
            Z = None
        res["seams"]["pqx_bound_rq"] = dict(device_us=med([d for _, d in one]), wall_us=med([w for w, _ in one]),
                                            single_binds_wall_us=med(each), binds=lq)
        log("pqx_bound_rq", res["seams"]["pqx_bound_rq"])
        erx = spg.Buf(ctx, rand_limbs(rng, X))
        rs = rand_limbs(rng, 3)
        timed("r1cs_eval_tables", lambda: spg.r1cs_eval_tables(ctx, inst, P, nws, Y, wl.num_inputs, erx))
        timed("r1cs_abc_poly", lambda: spg.r1cs_abc_poly(ctx, inst, P, nws, Y, wl.num_inputs, erx, *rs))

        # the two provers, with the per-kernel records of their launches
        ctx.prof_enable(True)
        for rep in range(a.reps):
            tabs = spg.r1cs_multiply_vec_block(ctx, inst, wl.num_proofs, Q, wl.num_inputs, Y, nws, z)
            eqs = [spg.Buf(ctx, rand_limbs(rng, 1 << n)) for n in (lp, lq, lx)]
            ctx.prof_read(reset=True)
            t = time.perf_counter()
            spg.zk_phase1_prove(ctx, gens, lx, lq, lp, *eqs, *tabs, spg.Transcript(b"perf"),
                                spg.RandomTape(b"proof", seed))
            w1, d1, k1 = (time.perf_counter() - t) * 1e6, ctx.last_kernel_us(), ctx.prof_read(reset=True)
            tabs = None
            ABC = spg.r1cs_abc_poly(ctx, inst, P, nws, Y, wl.num_inputs, erx, *rs)
            Z = spg.Pqx.new_rev(ctx, zbuf, *shape)
            Z.bound_rq(rq)
            eq = spg.Buf(ctx, rand_limbs(rng, 1 << lp))
            ctx.prof_read(reset=True)
            t = time.perf_counter()
            spg.zk_phase2_prove(ctx, gens, ly, lw, lp, False, nws, eq, ABC, Z, spg.Transcript(b"perf"),
                                spg.RandomTape(b"proof", seed))
            w2, d2, k2 = (time.perf_counter() - t) * 1e6, ctx.last_kernel_us(), ctx.prof_read(reset=True)
            ABC = Z = None
            res["seams"].setdefault("zk_phase1_prove", []).append(dict(device_us=d1, wall_us=w1, kernels=k1))
            res["seams"].setdefault("zk_phase2_prove", []).append(dict(device_us=d2, wall_us=w2, kernels=k2))
            log("zk_phase1_prove", dict(device_us=d1, wall_us=w1), "zk_phase2_prove", dict(device_us=d2, wall_us=w2))
        zbuf = None

        # the fused prover on the same matrices and witness
        z5 = z.reshape(P, Q, nws, Y, 4)
        wl.sections = [[np.ascontiguousarray(z5[p, :, w]) for p in range(P)] for w in range(nws)]
        v = workload.CViews(wl)
        wit = spg.R1CSWitness(ctx, v.secs, nws)
        fused = []
        for rep in range(a.reps + 1):  # (the first prove builds the generator tables)
            ctx.prof_read(reset=True)
            t = time.perf_counter()
            spg.r1cs_prove(ctx, gens, inst, wit, P, Q, wl.num_proofs, Y, wl.num_inputs, spg.Transcript(b"perf"),
                           spg.RandomTape(b"proof", seed))
            fused.append(dict(wall_us=(time.perf_counter() - t) * 1e6, kernels=ctx.prof_read(reset=True)))
            log("r1cs_prove", fused[-1]["wall_us"])
        res["r1cs_prove"] = fused[1:]
        keep = ("eval_table_abc", "z_fill", "sc_phase1_eval", "sc_phase1_fold_eval", "sc_phase2_eval",
                "sc_phase2_fold_eval", "sc_fold", "sc_fold_q_all", "spmv")
        log("fused kernels (launches, total us):",
            {k: (r[0], round(r[1], 1)) for k, r in fused[-1]["kernels"].items() if k in keep or k.startswith("sc_")})
    except Exception as e:  # noqa: BLE001  (a GPU call raised: stop here)
        res["stopped"] = repr(e)
        log("stopped:", repr(e))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    log("wrote", a.out)
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    sys.exit(main())
