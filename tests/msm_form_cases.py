"""Shared inputs of the fixed-base MSM form tests (tests/test_gpu_msm_forms.py on the device,
tests/test_msm_plan_host.py without one): the launch-shape functions of csrc/msm_plan.hpp through libspg_hostcheck.so's
spgh_* exports, the sizes the tests pick by them, the scalar rows every shape embeds, and the child process that reads
an environment. The reference is always the oracle (pyoracle.msm per distinct row, blinds added with its scalar
multiplication), computed once per case and kept."""
import ctypes
import os
import subprocess

import numpy as np

import fieldref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spartan-parallel_amd")
HC = os.environ.get("SPG_HOSTCHECK_LIB") or os.path.join(PKG, "lib", "libspg_hostcheck.so")
Q = fieldref.Q

# the KScope names of the fixed-base MSM pipelines (ctx.prof_read)
MSM_SCOPES = ["msm_comb", "msm_digits_rows", "msm_count", "msm_scatter", "msm_bucket_items", "msm_segments", "msm_final",
              "msm_small_bucket", "msm_small_final", "msm_big_sort", "msm_big_accum", "msm_comb_single", "msm_compress"]
LABEL = b"spg_form_rows"

_hc = None
_dflt = None


def hc():
    global _hc
    if _hc is None:
        if not os.path.exists(HC):
            subprocess.check_call(["make", "-s", "-C", PKG, "lib/libspg_hostcheck.so"])
        lib = ctypes.CDLL(HC)
        z, i, li, ip = ctypes.c_size_t, ctypes.c_int, ctypes.c_long, ctypes.POINTER(ctypes.c_int)
        lib.spgh_pick_window.argtypes = [z]
        lib.spgh_pick_small_window.argtypes = [z, i]
        lib.spgh_msm_comb_rule.argtypes = [i, z, z, z]
        lib.spgh_msm_batch_route.argtypes = [z, z, i, i, i, li, i, ip]
        lib.spgh_msm_batch_route.restype = None
        lib.spgh_comb_rows_shape.argtypes = [z, z, z, z, z, ctypes.POINTER(z)]
        lib.spgh_comb_rows_shape.restype = None
        lib.spgh_big_digit_blocks.argtypes = [i, i, ip]
        lib.spgh_big_digit_blocks.restype = None
        lib.spgh_bullet_comb_shape.argtypes = [i, i, i, i, i, ip]
        lib.spgh_bullet_comb_shape.restype = None
        lib.spgh_bullet_comb_launch.argtypes = [i, i, i, i, i, i, i, ip]
        lib.spgh_layer_grid.argtypes = [z, z, z, ctypes.POINTER(ctypes.c_uint)]
        lib.spgh_layer_grid.restype = None
        lib.spgh_grid_for.argtypes = [ctypes.c_uint32, i]
        lib.spgh_knob_table.restype = z
        lib.spgh_knob_table.argtypes = [ctypes.c_char_p, z]
        _hc = lib
    return _hc


def knob_defaults():
    """name -> (kind, default text, lo, hi) of csrc/knobs.hpp"""
    global _dflt
    if _dflt is None:
        n = hc().spgh_knob_table(None, 0)
        buf = ctypes.create_string_buffer(n)
        hc().spgh_knob_table(buf, n)
        rows = [line.split("\t") for line in buf.raw.decode().splitlines()]
        _dflt = {r[0]: (r[1], r[2], r[3], r[4]) for r in rows}
    return _dflt


def knob(name, env=None):
    """the integer a site reads for an ON / INT / LONG knob under env (a dict of texts), by the table's parse rules"""
    kind, dflt, lo, hi = knob_defaults()[name]
    text = (env or {}).get(name)
    if kind == "ON":
        return 1 if text is None else int(int(text) != 0)
    assert kind in ("INT", "LONG"), (name, kind)
    if text is None:
        return 0 if dflt == "unset" else int(dflt)
    v = int(text)
    if lo != "-":
        v = max(v, int(lo))
    if hi != "-":
        v = min(v, int(hi))
    return v


# ---- the shape functions
def pick_window(per):
    return hc().spgh_pick_window(per)


def pick_small_window(per, env=None):
    return hc().spgh_pick_small_window(per, knob("SPG_SMSM_C", env))


def comb_rule(B, n, blinds=False, has_idx=False):
    return bool(hc().spgh_msm_comb_rule(int(has_idx), B, n, B * (n + (1 if blinds else 0))))


ROUTE_FIELDS = ("c", "NB", "W", "rows", "m", "S", "log2m", "seg_quad", "quad", "regroup", "final_S", "final_sl")


def batch_route(B, per, env=None):
    """msm_batch_device's route for B MSMs of per scalars (blind included) under env"""
    out = (ctypes.c_int * 12)()
    hc().spgh_msm_batch_route(B, per, knob("SPG_SEG_M", env), knob("SPG_ROWS_CMAX", env), knob("SPG_SMSM_QUAD", env),
                              knob("SPG_SEG_QUAD_MAX", env), knob("SPG_FINAL_SL", env), out)
    return dict(zip(ROUTE_FIELDS, out))


def comb_rows_shape(B, per, env=None):
    out = (ctypes.c_size_t * 2)()
    u = lambda v: v & ((1 << 64) - 1)  # noqa: E731  (a negative long reaches its site as a huge size_t)
    hc().spgh_comb_rows_shape(B, per, u(knob("SPG_COMB_WGS", env)), u(knob("SPG_COMB_GMAX", env)),
                              u(knob("SPG_COMB_GMIN", env)), out)
    return int(out[0]), int(out[1])


def big_digit_blocks(per, env=None):
    out = (ctypes.c_int * 2)()
    hc().spgh_big_digit_blocks(per, knob("SPG_BIG_SPT", env), out)
    return out[0], out[1]


def bullet_comb_shape(P, env=None):
    """(G, BS, R) by MSM size alone, before the table's window width is known"""
    out = (ctypes.c_int * 3)()
    hc().spgh_bullet_comb_shape(P, knob("SPG_BCOMB_G", env), knob("SPG_BCOMB_BS", env), knob("SPG_BCOMB_R", env),
                                knob("SPG_BCOMB_NOTREE", env), out)
    return tuple(out)


def bullet_comb_launch(shape_P, P, c, env=None):
    """(runs, G, BS, R, wgs) of a comb Bullet round (shape_P = P = n / 2) or of comb_msm_parts (P = n scalars,
    shape_P = max(2, n)) over c-bit windows"""
    out = (ctypes.c_int * 4)()
    ok = hc().spgh_bullet_comb_launch(shape_P, P, c, knob("SPG_BCOMB_G", env), knob("SPG_BCOMB_BS", env),
                                      knob("SPG_BCOMB_R", env), knob("SPG_BCOMB_NOTREE", env), out)
    return (bool(ok),) + tuple(out)


def layer_grid(W, env=None):
    out = (ctypes.c_uint * 2)()
    hc().spgh_layer_grid(W, knob("SPG_LAYER_ONEWG", env) & ((1 << 64) - 1), knob("SPG_LAYER_EPT", env), out)
    return out[0], out[1]


def grid_for(total, env=None):
    return hc().spgh_grid_for(total, knob("SPG_SC_GRID", env))


def smallest_n(c):
    """the fewest scalars per MSM that pick_window gives window c for (bisection: the choice is monotone in n), or
    None for a width it never picks (one whose window count 253 / c + 1 saves nothing over a narrower width's)"""
    if pick_window(1) >= c:
        return 1 if pick_window(1) == c else None
    lo, hi = 1, 1 << 20  # pick_window(lo) < c <= pick_window(hi)
    assert pick_window(hi) >= c
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pick_window(mid) >= c:
            hi = mid
        else:
            lo = mid
    return hi if pick_window(hi) == c else None


# ---- scalars
def rand_fq(oracle, rng, n):
    return oracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * n, dtype=np.uint8).tobytes())


def edge_scalars(oracle):
    """the edge set of test_commit_rows_comb (-1, 2^252, q - 2^252, 1, 0), then every window on the signed recode's
    carry decision (fieldref.api_carry_scalars), as Montgomery scalars"""
    one = oracle.fq_from_u64(1)
    p252 = oracle.fq_from_raw([0, 0, 0, 1 << 60])
    edge = [oracle.fq_op("neg", one)[0], p252, oracle.fq_op("neg", p252)[0], one, np.zeros(4, np.uint64)]
    carry = fieldref.arr_u64([fieldref.to_mont(v) for v in fieldref.api_carry_scalars()])
    return np.concatenate([np.stack(edge), carry])


def distinct_rows(oracle, n, seed):
    """four rows of n scalars: mixed (the edge scalars in front, -1 at every 7th place after them, random elsewhere),
    hot (one scalar repeated: one bucket of every window holds the whole row), and two random ones with edge scalars
    at their ends"""
    rng = np.random.default_rng(seed)
    e = edge_scalars(oracle)
    D = [rand_fq(oracle, rng, n) for _ in range(4)]
    k = min(n, len(e))
    D[0][:k] = e[:k]
    D[0][k::7] = e[0]
    D[1][:] = rand_fq(oracle, rng, 1)[0]
    D[2][n - min(n, 5):] = e[:min(n, 5)]
    D[3][:min(n, 3)] = e[1:1 + min(n, 3)]
    return D


def row_order(B):
    """which of the five rows (0..3: distinct_rows, 4: the all-zero row) row i of a batch of B is: 0..4 for B = 5, and
    for larger batches an order in which neighbours always differ"""
    return [(3 * i + i // 5) % 5 for i in range(B)] if B > 5 else list(range(5))[:B]


def batch(oracle, B, n, seed):
    """(Z, order): B rows of n scalars built from distinct_rows and the zero row"""
    D = distinct_rows(oracle, n, seed) + [np.zeros((n, 4), np.uint64)]
    order = row_order(B)
    return np.concatenate([D[k] for k in order]), order


_REF = {}


def expected(oracle, pts, h, B, n, seed, blinds=None):
    """the oracle's commitments of batch(oracle, B, n, seed): its MSM of each distinct row once (kept per (n, seed)),
    and blinds[i] * h added per row with its scalar multiplication"""
    key = (n, seed)
    if key not in _REF:
        D = distinct_rows(oracle, n, seed)
        _REF[key] = [oracle.msm(pts[:n], d) for d in D] + [bytes(32)]
    rows = [_REF[key][k] for k in row_order(B)]
    if blinds is not None:
        kb = oracle.fq_to_bytes(blinds)
        rows = [oracle.ge_add(r, oracle.ge_scalarmul(bytes(h), bytes(kb[i]))) for i, r in enumerate(rows)]
    return np.stack([np.frombuffer(bytes(r), dtype=np.uint8) for r in rows])


def blinds_for(oracle, B, seed):
    bl = rand_fq(oracle, np.random.default_rng(seed + 99991), B)
    bl[0] = edge_scalars(oracle)[0]
    return bl


def profile_of(ctx, fn):
    """fn() under the kernel profile: (result, {scope: launches} over MSM_SCOPES)"""
    ctx.prof_enable(True)
    ctx.prof_read(reset=True)
    try:
        out = fn()
        prof = ctx.prof_read(reset=True)
    finally:
        ctx.prof_enable(False)
    return out, {k: int(prof[k][0]) if k in prof else 0 for k in MSM_SCOPES}


def scopes_of_route(rt):
    """the scopes a bucket-pipeline batch on route rt launches (every other MSM scope must stay at zero)"""
    s = {"msm_bucket_items", "msm_segments", "msm_final"}
    return s | ({"msm_digits_rows"} if rt["rows"] else {"msm_count", "msm_scatter"})


# ---- the cases. A rows case is (name, generator-set size, B, n, seed); its Z is batch(oracle, B, n, seed).
WINDOWS = [c for c in range(4, 17) if smallest_n(c) is not None]
NG = smallest_n(16)  # the generator set of the bucket-pipeline cases covers the widest window's rows
MID = ("mid_128x512", 1024, 128, 512, 11)  # the mid-size shape the forms run on (rows sort, c = 10, 64 segments)
MID_FEW = ("mid_5x2634", 4096, 5, smallest_n(13), 12)  # .. and one the count / scatter kernels sort
# .. and one of 64 buckets per MSM (c = 7): SPG_SEG_M = 64 is all of them in one segment (m = NB, S = 1)
NARROW = ("narrow_5x14", 1024, 5, smallest_n(7), 13)


def bucket_cases():
    """batches for the bucket pipeline with the comb off: the shapes the comb took over from the old direct tests, one
    of >= 256 rows below the comb's size rule (k_final_q<32>), few rows at the narrowest 15-bit size (k_regroup_q), and
    per window width pick_window ever picks, at the fewest scalars it picks it for, five rows (k_digits count and
    scatter) and 64 rows (k_digits_rows<C>; c = 16 is the 128 KiB LDS edge)"""
    cases = [("old_128x512", NG, 128, 512, 1), ("old_64x1024", NG, 64, 1024, 2), ("old_512x64", NG, 512, 64, 3),
             ("final32_256x32", NG, 256, 32, 4)]
    for c in WINDOWS:
        cases.append(("few_c%d" % c, NG, 5, smallest_n(c), 100 + c))
        if c <= knob("SPG_ROWS_CMAX"):
            cases.append(("rows_c%d" % c, NG, 64, smallest_n(c), 100 + c))
    return cases


LATENCY_SIZES = [1, 63, 64, 65, 128, 129, 300]
SMSM_WINDOWS = ["4", "5", "6", "9", "77"]  # 77: outside 4..9, ignored

# comb rows on 256-generator sets (a 13-bit table of 257 slots is 2.7 GB): (64, 256) has few enough scalars that the
# default takes 4 window groups per scalar, (512, 256) so many that it takes 1
COMB_SHAPES = [("comb_64x256", 256, 64, 256, 21), ("comb_512x256", 256, 512, 256, 22)]
COMB_ENVS = [
    {"SPG_COMB_C": "10", "SPG_COMB_GMAX": "1"},
    {"SPG_COMB_C": "11", "SPG_COMB_GMAX": "2"},
    {"SPG_COMB_C": "12", "SPG_COMB_GMIN": "2"},
    {"SPG_COMB_C": "13", "SPG_COMB_GMIN": "4"},
    {"SPG_COMB_WGS": "1"},
    {"SPG_COMB_WGS": "1048576", "SPG_COMB_PAD": "0"},
]


def comb_table_bytes(c, slots, padded):
    """comb.hip's table_bytes: windows x (slots + h) x 2^(c-1) multiples of 96 (packed) or 128 (padded) bytes"""
    return (253 // c + 1) * (slots + 1) * (1 << (c - 1)) * 32 * (4 if padded else 3)


# ---- the child process (one per environment; the knobs are read once per process)
def child_main(spec):
    """spec: a list of (name, kind, args) read from the command line as Python text. Prints, per case, `name hex...`
    and `prof name scope=launches ...`; `ok` last."""
    import pyoracle
    import spg

    ctx = spg.Context(0)
    gens = {}

    def g(n):
        if n not in gens:
            gens[n] = spg.Gens(ctx, n, LABEL)
        return gens[n]

    for name, kind, a in spec:
        if kind == "setenv":  # a knob that is re-read on every call, swept in one process: a = (name, text)
            os.environ[a[0]] = a[1]
            continue
        if kind == "skew":  # test_gpu_msm.py's checks of one large MSM over a = (gens size, label); asserts inside
            from test_gpu_msm import edge_and_skew_checks

            big = spg.Gens(ctx, a[0], a[1])
            _, prof = profile_of(ctx, lambda: edge_and_skew_checks(pyoracle, big))
            print(name, "passed")
        elif kind == "rows":  # a = (gens size, B, n, seed, with blinds)
            G, B, n, seed, wb = a
            Z, _ = batch(pyoracle, B, n, seed)
            bl = blinds_for(pyoracle, B, seed) if wb else None
            out, prof = profile_of(ctx, lambda: g(G).commit_rows(Z, B, n, bl))
            print(name, out.tobytes().hex())
        elif kind == "one":  # one MSM per distinct row: a = (gens size, n, seed, with blind)
            G, n, seed, wb = a
            Z, _ = batch(pyoracle, 5, n, seed)
            bl = blinds_for(pyoracle, 5, seed) if wb else None
            out, prof = profile_of(ctx, lambda: b"".join(
                g(G).msm(Z[i * n:(i + 1) * n], blind=None if bl is None else bl[i:i + 1]) for i in range(5)))
            print(name, out.hex())
        else:
            raise ValueError(kind)
        print("prof", name, *("%s=%d" % kv for kv in prof.items()))
    b, built, _, _ = spg.comb_stats()
    print("comb", b, built)
    print("ok")


def run_child(spec, env):
    import sys

    code = ("import sys; sys.path[:0] = [%r, %r, %r]\nimport msm_form_cases\nmsm_form_cases.child_main(%r)\n"
            % (PKG, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), spec))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert lines[-2] == "ok", out.stdout[-500:]
    res, prof, comb = {}, {}, None
    for line in lines[:-2]:
        w = line.split()
        if w[0] == "prof":
            prof[w[1]] = {k: int(v) for k, v in (x.split("=") for x in w[2:])}
        elif w[0] == "comb":
            comb = (int(w[1]), int(w[2]))
        else:
            res[w[0]] = w[1]
    return res, prof, comb
