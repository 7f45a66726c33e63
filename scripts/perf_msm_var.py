"""Measurements of the variable-base MSM (spg_points / spg_msm_var*, msm_var.hip), one GPU command:

  1. device path against host path for n = 2^4 .. 2^20, points and scalars resident, the two sides alternated in one
     process (spg_set_vmsm_host_max), and a sweep of SPG_VMSM_C at 2^10, 2^13 and 2^16 .. 2^20 (one child process per
     c: that knob is read once);
  2. the one-off cost at 2^12 and 2^16: spg_msm_points (upload included) against the parent commit's only route,
     spg_gens_upload + spg_msm with its table build (lib/libspg_base.so from scripts/build_base.sh when present), and
     the steady-state fixed-base spg_msm_buf at 2^16 for context;
  3. vmsm_accum's modelled mixed additions per second at 2^16 and 2^20 beside msm_big_accum's at 2^16 (spg_prof);
  4. bench.py --full's verify_ms with and without SPG_VERIFY_VMSM=1, three alternations.

Every timing is a host clock around the (synchronising) call, with the device-event time (spg_last_kernel_us) beside
it where the call has one. Writes profiles/vmsm_sizes.json (--out).

The run ends at the first GPU call that raises and at the first child process that returns non-zero, is killed by a
signal or runs into its time limit: nothing more is started on the GPU after that. What was measured up to there is
written with a "stopped" entry, the exit status is 1, and only parts that were never started read "not measured"."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "oracle")]
import pyoracle  # noqa: E402
import spg  # noqa: E402

SWEEP_SIZES = [10, 13, 16, 17, 18, 19, 20]
MADD_RATE = 3.0e10  # whole-chip one-lane mixed additions per second (scripts/micro/ext_throughput)
T0 = time.perf_counter()


def log(*a):
    print("[%6.1fs]" % (time.perf_counter() - T0), *a, flush=True)


def rand(rng, n):
    return pyoracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * n, dtype=np.uint8).tobytes())


def tiled_points(n):
    """n valid encodings: 4096 hash-to-group points repeated (the bucket loads depend on the scalars only)"""
    base = pyoracle.gens_stream(b"vmsm_test", min(n, 4096))
    return np.ascontiguousarray(np.tile(base, ((n + len(base) - 1) // len(base), 1))[:n])


def med(x):
    return float(np.median(x))


def timed_calls(fn, ctx, calls):
    wall, dev = [], []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(ctx.last_kernel_us() * 1e-3)
    return wall, dev


def run_child(cmd, env, timeout):
    """a child process on the GPU; any failure of it (non-zero or negative status, time limit) ends the whole run"""
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)  # TimeoutExpired propagates
    if r.returncode != 0:
        raise RuntimeError("child %s ended with status %d: %s" % (cmd[1:], r.returncode, r.stderr[-300:]))
    return r.stdout.split("\n")


def n_calls(ms):
    return 200 if ms < 5.0 else max(20, int(1000.0 / ms))


def part_sizes(out, ctx, rng, lo, hi, host_to):
    for k in range(lo, hi + 1):
        n = 1 << k
        P = spg.Points(ctx, tiled_points(n))
        buf = spg.Buf(ctx, rand(rng, n))

        def call():
            return P.msm_buf(buf)

        sides = ["device"] + (["host"] if k <= host_to else [])
        knob = {"device": 0, "host": 1 << 31}
        res, first = {}, {}
        for sd in sides:
            ctx.set_vmsm_host_max(knob[sd])
            for _ in range(3):
                res[sd] = call()
            t = time.perf_counter()
            call()
            first[sd] = (time.perf_counter() - t) * 1e3
        calls = n_calls(max(first.values()))
        rounds = 20
        per = max(1, calls // rounds)
        wall = {sd: [] for sd in sides}
        dev = []
        wins = []
        for _ in range(rounds):
            m = {}
            for sd in sides:
                ctx.set_vmsm_host_max(knob[sd])
                w, d = timed_calls(call, ctx, per)
                wall[sd] += w
                m[sd] = med(w)
                if sd == "device":
                    dev += d
            if "host" in m:
                wins.append(m["device"] < m["host"])
        rec = {"n": n, "calls_per_side": per * rounds, "device_ms_median": round(med(wall["device"]), 4),
               "device_ms_min": round(min(wall["device"]), 4), "device_event_ms_median": round(med(dev), 4)}
        if "host" in sides:
            rec.update({"host_ms_median": round(med(wall["host"]), 4), "host_ms_min": round(min(wall["host"]), 4),
                        "device_wins_alternations": "%d/%d" % (sum(wins), len(wins)),
                        "results_agree": res["device"] == res["host"]})
        else:
            rec["host_ms_median"] = "not measured"
        out["2^%d" % k] = rec
        log("size", k, rec)
        P.free()
        buf.free()
    ctx.set_vmsm_host_max(-1)


def sweep_child():
    """one forced window (SPG_VMSM_C, SPG_VMSM_HOST_MAX=0 set by the parent): median ms per size"""
    ctx = spg.Context(0)
    rng = np.random.default_rng(2)
    out = {}
    for k in SWEEP_SIZES:
        n = 1 << k
        P = spg.Points(ctx, tiled_points(n))
        buf = spg.Buf(ctx, rand(rng, n))
        for _ in range(2):
            P.msm_buf(buf)
        t = time.perf_counter()
        P.msm_buf(buf)
        calls = n_calls((time.perf_counter() - t) * 1e3)
        w, d = timed_calls(lambda: P.msm_buf(buf), ctx, calls)
        out["2^%d" % k] = {"calls": calls, "ms_median": round(med(w), 4), "device_event_ms_median": round(med(d), 4)}
        P.free()
        buf.free()
    print("SWEEP " + json.dumps(out), flush=True)


def part_sweep(out):
    for c in range(4, 15):
        env = dict(os.environ, SPG_VMSM_C=str(c), SPG_VMSM_HOST_MAX="0")
        lines = run_child([sys.executable, os.path.abspath(__file__), "--sweep-child"], env, 120)
        out["c=%d" % c] = json.loads([x for x in lines if x.startswith("SWEEP ")][-1][6:])
        log("sweep c", c, out["c=%d" % c])
    best = {}
    for k in SWEEP_SIZES:
        key = "2^%d" % k
        t = {c: v[key]["ms_median"] for c, v in out.items()}
        best[key] = min(t, key=t.get)
    out["best"] = best


class BaseLib:
    """the parent commit's libspg through raw ctypes (its own context)"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.ctx = ctypes.c_void_p()
        assert self.lib.spg_init(0, ctypes.byref(self.ctx)) == 0

    def gens_upload_msm(self, comp, s):
        n = comp.shape[0] - 1
        g = ctypes.c_void_p()
        out = np.zeros(32, np.uint8)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        assert self.lib.spg_gens_upload(self.ctx, p(comp), ctypes.c_size_t(n), ctypes.byref(g)) == 0
        assert self.lib.spg_msm(self.ctx, g, ctypes.c_size_t(0), p(s), ctypes.c_size_t(n), None, p(out)) == 0
        self.lib.spg_gens_free(self.ctx, g)
        return out.tobytes()


def part_oneoff(ctx, rng):
    out = {}
    path = os.path.join(ROOT, "spartan-parallel_amd", "lib", "libspg_base.so")
    if os.path.exists(path):
        base = BaseLib(path)
        old = base.gens_upload_msm
        out["parent_route"] = "lib/libspg_base.so (scripts/build_base.sh): spg_gens_upload + spg_msm + spg_gens_free"
    else:
        def old(comp, s):
            g = spg.Gens(ctx, comp.shape[0] - 1, compressed=comp)
            r = g.msm(s)
            g.free()
            return r
        out["parent_route"] = "this build's spg_gens_upload + spg_msm (unchanged entry points; no libspg_base.so)"
    for k in (12, 16):
        n = 1 << k
        comp = tiled_points(n + 1)  # n points and the h that spg_gens_upload wants
        s = rand(rng, n)
        spg.msm_points(ctx, comp[:n], s)  # warm both sides at this size (workspaces, staging, code objects)
        old(comp, s)
        new_ms, old_ms, agree = [], [], True
        for _ in range(3):
            t = time.perf_counter()
            a = spg.msm_points(ctx, comp[:n], s)
            new_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            b = old(comp, s)
            old_ms.append((time.perf_counter() - t) * 1e3)
            agree = agree and a == b
        out["2^%d" % k] = {"msm_points_ms": [round(x, 3) for x in new_ms], "gens_upload_msm_ms": [round(x, 3) for x in old_ms],
                           "results_agree": agree, "new_faster_every_time": all(x < y for x, y in zip(new_ms, old_ms))}
        log("one-off", k, out["2^%d" % k])
    n = 1 << 16
    g = spg.Gens(ctx, n, b"spg_bench_msm")
    buf = spg.Buf(ctx, rand(rng, n))
    for _ in range(5):
        g.msm_buf(buf)
    w, _ = timed_calls(lambda: g.msm_buf(buf), ctx, 200)
    # (spg_msm_buf records no device-event time)
    out["fixed_base_msm_buf_2^16"] = {"ms_median": round(med(w), 4), "device_event_ms_median": "not measured"}
    log("fixed base", out["fixed_base_msm_buf_2^16"])
    g.free()
    buf.free()
    return out


def oneoff_in_child(out):
    lines = run_child([sys.executable, os.path.abspath(__file__), "--oneoff-child"], dict(os.environ), 240)
    line = [x for x in lines if x.startswith("ONEOFF ")][-1]
    log("one-off", line)
    out.update(json.loads(line[7:]))


def part_share(out, rng):
    ctx = spg.Context(0)
    ctx.set_vmsm_host_max(0)
    ctx.set_comb(False)  # spg_msm_buf through msm_big.hip's buckets (msm_big_accum), not the comb
    for k in (16, 20):
        n = 1 << k
        P = spg.Points(ctx, tiled_points(n))
        buf = spg.Buf(ctx, rand(rng, n))
        P.msm_buf(buf)
        g = spg.Gens(ctx, n, b"spg_bench_msm") if k == 16 else None  # the fixed-base buckets beside it, same run
        for _ in range(2 if g else 0):
            g.msm_buf(buf)
        ctx.prof_enable(True)
        ctx.prof_read(reset=True)
        for _ in range(20):
            P.msm_buf(buf)
            if g:
                g.msm_buf(buf)
        prof = ctx.prof_read(reset=True, ops=True)
        ctx.prof_enable(False)
        if g:
            g.free()
        tab = {}
        for name, (launches, us, nbytes, ops, _fq) in sorted(prof.items()):
            if name.startswith("vmsm_") or name.startswith("msm_big"):
                tab[name] = {"launches": launches, "us_per_launch": round(us / launches, 2),
                             "modelled_GBps": round(nbytes / us * 1e-3, 1) if nbytes else None,
                             "madd_per_s": round(ops / us * 1e6, 1) if ops else None,
                             "share_of_madd_rate": round(ops / us * 1e6 / MADD_RATE, 4) if ops else None}
        out["2^%d" % k] = tab
        log("share", k, tab)
        P.free()
        buf.free()
    ctx.close()


def part_verify_ab(out):
    runs = {"0": [], "1": []}
    out.update({"bench": "bench.py --gpus 1 --steps 3 --warmup 2 --full --no-cpu-baseline --extras none, alternated",
                "verify_ms_unset": runs["0"], "verify_ms_SPG_VERIFY_VMSM=1": runs["1"]})
    for i in range(3):
        for knob in ("0", "1"):
            env = dict(os.environ, SPG_VERIFY_VMSM=knob)
            lines = run_child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup",
                               "2", "--full", "--no-cpu-baseline", "--extras", "none"], env, 200)
            d = json.loads([x for x in lines if x.startswith("{")][-1])
            if not d.get("verify_ok"):
                raise RuntimeError("bench.py: the proof did not verify with SPG_VERIFY_VMSM=" + knob)
            runs[knob].append(d["verify_ms"])
            log("verify A/B", i, knob, runs[knob][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vmsm_sizes.json"))
    ap.add_argument("--sweep-child", action="store_true")
    ap.add_argument("--oneoff-child", action="store_true")
    ap.add_argument("--max-log", type=int, default=20)
    ap.add_argument("--budget-s", type=float, default=540.0, help="later parts are skipped once this much has passed")
    ap.add_argument("--parts", default="sizes,oneoff,share,sweep,verify")
    a = ap.parse_args()
    if a.sweep_child:
        return sweep_child()
    if a.oneoff_child:  # (a process of its own: it loads the parent commit's library beside this one)
        print("ONEOFF " + json.dumps(part_oneoff(spg.Context(0), np.random.default_rng(3))), flush=True)  # raises on failure
        return
    ctx = spg.Context(0)
    rng = np.random.default_rng(1)
    out = {"note": "host clock around each synchronising call (ms); device_event = spg_last_kernel_us; points and "
                   "scalars resident for the size and sweep tables"}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    parts = [("sizes", lambda o: part_sizes(o, ctx, rng, 4, a.max_log, 12)), ("oneoff", oneoff_in_child),
             ("share", lambda o: part_share(o, rng)), ("sweep", part_sweep), ("verify", part_verify_ab)]
    parts = [p for p in parts if p[0] in a.parts.split(",")]
    for i, (name, fn) in enumerate(parts):
        if time.perf_counter() - T0 > a.budget_s:
            out[name] = "not measured (time budget of the run spent)"
            continue
        out[name] = {}
        try:
            fn(out[name])  # fills out[name] as it goes
        except BaseException as e:  # noqa: BLE001 - a failed GPU call or child: nothing more is started on the GPU
            out["stopped"] = "in part %r: %r" % (name, e)
            for later, _ in parts[i + 1:]:
                out[later] = "not measured (the run stopped before it)"
            write()
            log("stopped in", name, repr(e))
            sys.exit(1)
        write()
    log("wrote", a.out)


if __name__ == "__main__":
    main()
