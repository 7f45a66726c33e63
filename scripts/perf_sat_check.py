"""What the satisfiability check costs, one GPU command:

  1. device time of the `sat_check` launches beside `spmv_block` (spg_prof records, check mode on): the headline
     SNARK::prove (2 block types x 2^9 executions x 2^10 constraints; three launches per prove) and R1CSProof::prove at
     SURVEY 8d config 4's shape (8 instances x 2^9 x 2^10, one section), with the achieved fraction of the HBM peak;
  2. spg_snark_prove with the mode on against off: --pairs alternated pairs of --steps proves each (the order of a
     pair flips every pair), the median step of every run and the median over the runs; proof hashes must agree;
  3. spg_snark_check's wall time on the headline program, beside prove and verify.

Prints one JSON object and writes it to --out. The run ends at the first GPU call that raises."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "oracle")]
import spg  # noqa: E402
import workload  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X
GENS_LABEL, GENS_NV = b"gens_r1cs_sat", 1 << 24


def med(v):
    return float(np.median(v))


def kernels(prof, proves):
    out = {}
    for k in ("sat_check", "spmv_block"):
        n, us, nbytes = prof[k]
        out[k] = {"launches_per_prove": n / proves, "us_per_launch": round(us / n, 2),
                  "modelled_bytes_per_launch": nbytes / n, "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)}
    return out


def profiled(ctx, step, proves):
    ctx.set_check_sat(True)
    ctx.prof_enable(True)
    try:
        ctx.prof_read()
        for _ in range(proves):
            step()
        return kernels(ctx.prof_read(), proves)
    finally:
        ctx.prof_enable(False)
        ctx.set_check_sat(False)


def run(step, steps):
    laps = []
    for _ in range(steps):
        t = time.perf_counter()
        out = step()
        laps.append(time.perf_counter() - t)
    return med(laps) * 1e3, hashlib.sha256(out).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--log-cons", type=int, default=10)
    ap.add_argument("--log-proofs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "sat_check.json"))
    a = ap.parse_args()
    ctx = spg.Context(0)
    seed = workload.tape_seed()
    gens = spg.R1CSGens(ctx, GENS_LABEL, GENS_NV)
    res = {}

    # ---- the headline program
    wl = workload.SnarkWorkload(num_blocks=2, log_cons=a.log_cons, log_proofs=a.log_proofs, num_vars=1 << a.log_cons)
    views = workload.SnarkViews(wl)
    block = spg.SnarkComp(ctx, views.block, multi=True)
    pairwise = spg.SnarkComp(ctx, views.pairwise)
    perm_root = spg.SnarkComp(ctx, views.perm_root)
    wit = spg.SnarkWitness(ctx, views.inputs)

    def prove():
        return spg.snark_prove(ctx, block, pairwise, perm_root, wit, gens, spg.Transcript(b"snark_bench"),
                               spg.RandomTape(b"proof", seed))

    for _ in range(5):
        proof = prove()
    res["snark_kernels"] = profiled(ctx, prove, 10)

    on, off, hashes = [], [], set()
    for i in range(a.pairs):
        for mode in ((True, False) if i % 2 else (False, True)):
            ctx.set_check_sat(mode)
            ms, h = run(prove, a.steps)
            (on if mode else off).append(round(ms, 3))
            hashes.add(h)
    ctx.set_check_sat(False)
    assert len(hashes) == 1, hashes
    res["snark_prove_ms"] = {"steps_per_run": a.steps, "mode_off_runs": off, "mode_on_runs": on,
                             "mode_off_median": round(med(off), 3), "mode_on_median": round(med(on), 3),
                             "proof_sha256": hashes.pop()}

    def check():
        rep, _ = spg.snark_check(ctx, block, pairwise, perm_root, wit, gens, spg.Transcript(b"snark_bench"))
        assert rep.first == spg.FIRST_NONE, rep
        return b""

    def verify():
        ok, why = spg.snark_verify(ctx, block, pairwise, perm_root, views.inputs, gens, spg.Transcript(b"snark_bench"),
                                   proof)
        assert ok, why
        return b""

    check()
    verify()
    res["snark_wall_ms"] = {"snark_check": round(run(check, 20)[0], 3), "snark_prove": round(run(prove, 20)[0], 3),
                            "snark_verify": round(run(verify, 10)[0], 3)}
    del wit, block, pairwise, perm_root

    # ---- config 4
    rw = workload.R1CSWorkload([1024] * 8, [512] * 8, num_sections=1)
    v = workload.CViews(rw)
    inst = spg.R1CSInst(ctx, v.inst)
    rwit = spg.R1CSWitness(ctx, v.secs, rw.nws)
    shape = (rw.P, rw.max_num_proofs, rw.num_proofs, rw.max_num_inputs, rw.num_inputs)

    def r1cs():
        return spg.r1cs_prove(ctx, gens, inst, rwit, *shape, spg.Transcript(b"r1cs_bench"),
                              spg.RandomTape(b"proof", seed))[0]

    for _ in range(3):
        r1cs()
    res["config4_kernels"] = profiled(ctx, r1cs, 10)
    t = time.perf_counter()
    rep = spg.r1cs_sat_check(ctx, inst, rwit, *shape)
    res["config4_r1cs_sat_check_wall_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    assert rep.violations == 0 and rep.rows == 8 * 512 * 1024, rep

    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
