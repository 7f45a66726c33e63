"""Measurements of the verifiers' deferred mode (spg_set_verify_device, eqcheck.hip) on the headline shape of bench.py
(2 block types x 2^9 executions x 2^10 constraints), one GPU command:

  1. the number of equations and terms the deferred verifier collects for that proof (spg_eqs_last_counts);
  2. spg_snark_verify wall time with the mode off and on, alternated --rounds times (at least three) on one context after
     a warm-up of both; off is the eager verifier, the baseline;
  3. the device time of the one launch (the eqs_check profile scope and spg_last_kernel_us) and the host time that
     remains of a deferred verification (the verifier has no trace laps: that remainder is not broken down).

Every timing is a host clock around the (synchronising) call. Writes profiles/verify_eqs.json (--out). The run ends at
the first GPU call that raises: nothing more is started on the GPU after that, what was measured up to there is
written with a "stopped" entry and the exit status is 1."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-cons", type=int, default=10)
    ap.add_argument("--log-proofs", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3, help="off / on alternations")
    ap.add_argument("--calls", type=int, default=3, help="verifications per side of one alternation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_eqs.json"))
    a = ap.parse_args()
    out = {"shape": {"block_types": 2, "log_cons": a.log_cons, "log_proofs": a.log_proofs},
           "rounds": max(3, a.rounds), "calls_per_side": a.calls}
    rc = 0
    try:
        measure(a, out)
    except Exception as e:  # noqa: BLE001 - the first failing GPU call ends the run
        out["stopped"] = repr(e)
        rc = 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log("wrote", a.out)
    return rc


def measure(a, out):
    ctx = spg.Context(0)
    wl = workload.SnarkWorkload(num_blocks=2, log_cons=a.log_cons, log_proofs=a.log_proofs, num_vars=1 << a.log_cons,
                                seed=0x5350415254414E31)
    views = workload.SnarkViews(wl)
    gens = spg.R1CSGens(ctx, b"gens_r1cs_sat", 1 << 24)
    block = spg.SnarkComp(ctx, views.block, multi=True)
    pairwise = spg.SnarkComp(ctx, views.pairwise)
    perm_root = spg.SnarkComp(ctx, views.perm_root)
    wit = spg.SnarkWitness(ctx, views.inputs)
    proof = spg.snark_prove(ctx, block, pairwise, perm_root, wit, gens, spg.Transcript(b"snark_bench"),
                            spg.RandomTape(b"proof", workload.tape_seed()))
    log("proved,", len(proof), "bytes")

    def verify():
        t = time.perf_counter()
        ok, why = spg.snark_verify(ctx, block, pairwise, perm_root, views.inputs, gens, spg.Transcript(b"snark_bench"),
                                   proof)
        dt = time.perf_counter() - t
        if not ok:
            raise RuntimeError("verification rejected: %s" % why)
        return dt * 1e3

    for on in (False, True, False, True):  # warm-up of both sides (tables, workspace, page-locked staging)
        ctx.set_verify_device(on)
        verify()
    E, T = ctx.eqs_last_counts()
    out["equations"], out["terms"] = E, T
    log("deferred verifier: %d equations, %d terms" % (E, T))
    off, on_, kern = [], [], []
    for r in range(max(3, a.rounds)):
        ctx.set_verify_device(False)
        off.append([verify() for _ in range(a.calls)])
        ctx.set_verify_device(True)
        lap = []
        for _ in range(a.calls):
            lap.append(verify())
            kern.append(ctx.last_kernel_us() * 1e-3)
        on_.append(lap)
        log("round %d: off %s ms, on %s ms" % (r, ["%.2f" % x for x in off[-1]], ["%.2f" % x for x in on_[-1]]))
    out["verify_ms_off"] = [[round(x, 2) for x in lap] for lap in off]
    out["verify_ms_on"] = [[round(x, 2) for x in lap] for lap in on_]
    out["verify_ms_off_median"] = round(float(np.median(off)), 2)
    out["verify_ms_on_median"] = round(float(np.median(on_)), 2)
    out["flush_kernel_ms_last_kernel_us"] = [round(x, 3) for x in kern]
    # the launch's profile scope (both kernels between one event pair), one deferred verification
    ctx.prof_enable(True)
    ctx.prof_read()
    ctx.set_verify_device(True)
    t_on = verify()
    prof = ctx.prof_read()
    ctx.prof_enable(False)
    ctx.set_verify_device(False)
    launches, us, _ = prof.get("eqs_check", (0, 0.0, 0.0))
    out["flush_scope"] = {"launches": launches, "ms": round(us * 1e-3, 3)}
    out["deferred_host_ms_remaining"] = round(out["verify_ms_on_median"] - float(np.median(kern)), 2)
    out["profiled_verify_ms_on"] = round(t_on, 2)
    log("flush: %d launch, %.3f ms on the device; host remainder %.2f ms" %
        (launches, us * 1e-3, out["deferred_host_ms_remaining"]))
    ctx.close()


if __name__ == "__main__":
    sys.exit(main())
