"""Every launch form of the fixed-base MSM pipelines against the CPU oracle, byte for byte: the bucket pipeline
(msm_batch_device) that every row batch falls back to when the comb table does not apply, the latency path, the comb
rows at every window width and group count, and one large MSM through msm_big.hip, the batch pipeline and the wide
comb. Sizes come from csrc/msm_plan.hpp's shape functions (msm_form_cases), so a retuned threshold moves the cases with
it; every case also reads the kernel profile and asserts the scopes its form must and must not launch, so that a case
which never reaches the switched site fails instead of passing by the default form's result. Forms that a process reads
once run in a fresh child per environment, one at a time."""
import ctypes

import numpy as np
import pytest

import msm_form_cases as fc

pytestmark = pytest.mark.gpu

_PTS = {}


def gens_pts(oracle, G):
    """the oracle's generators of the cases' set of G (+ h)"""
    if G not in _PTS:
        _PTS[G] = oracle.gens_stream(fc.LABEL, G + 1)
    return _PTS[G]


def want_rows(oracle, case, blinds):
    _, G, B, n, seed = case
    pts = gens_pts(oracle, G)
    return fc.expected(oracle, pts, pts[G], B, n, seed, fc.blinds_for(oracle, B, seed) if blinds else None)


def first_diff(got, want):
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    return "rows %s of %d differ" % (bad[:8], len(want)) if bad else ""


def check_scopes(prof, must, name):
    for s in fc.MSM_SCOPES:
        if s in must:
            assert prof[s] > 0, (name, s, prof)
        elif s != "msm_compress":
            assert prof[s] == 0, (name, s, prof)


# ---------------------------------------------------------------- bucket pipeline, comb off in this process
@pytest.fixture(scope="module")
def gens_ng(ctx):
    import spg

    return spg.Gens(ctx, fc.NG, fc.LABEL)


@pytest.fixture()
def comb_off(ctx):
    ctx.set_comb(False)
    yield
    ctx.set_comb(True)


@pytest.mark.parametrize("case", fc.bucket_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("blinds", [False, True], ids=["plain", "blinds"])
def test_bucket_pipeline_comb_off(ctx, oracle, gens_ng, comb_off, case, blinds):
    """spg_set_comb(ctx, 0): the batch runs the bucket pipeline on the route msm_plan.hpp gives for its size"""
    name, G, B, n, seed = case
    assert np.array_equal(gens_ng.compressed(), gens_pts(oracle, G))
    per = n + (1 if blinds else 0)
    rt = fc.batch_route(B, per)
    if name.startswith(("few_c", "rows_c")):
        # (a blind is one more scalar: the one-scalar rows of window 4 are two-scalar rows of window 5 with it)
        assert rt["c"] == int(name.split("_c")[1]) or (blinds and n == 1), rt
        assert bool(rt["rows"]) == name.startswith("rows_c")
    if name.startswith("old_"):
        assert fc.comb_rule(B, n, blinds), "the comb took these shapes over"
    if name.startswith("final32"):
        assert rt["final_sl"] == 32 and not fc.comb_rule(B, n, blinds)
    Z, _ = fc.batch(oracle, B, n, seed)
    bl = fc.blinds_for(oracle, B, seed) if blinds else None
    got, prof = fc.profile_of(ctx, lambda: gens_ng.commit_rows(Z, B, n, bl))
    check_scopes(prof, fc.scopes_of_route(rt), name)
    want = want_rows(oracle, case, blinds)
    assert np.array_equal(got, want), (name, "window %d" % rt["c"], first_diff(got, want))


def test_regroup_route_is_reached():
    """few rows at the fewest scalars of a 15-bit window: more than 1024 segments per MSM, regrouped ahead of the final
    scan (k_regroup_q); the case above with that name runs it"""
    n = fc.smallest_n(15)
    for per in (n, n + 1):
        rt = fc.batch_route(5, per)
        assert rt["c"] == 15 and rt["regroup"] and rt["final_S"] * 8 == rt["S"], rt


def test_set_comb_on_again(ctx, oracle, gens_ng):
    """spg_set_comb(ctx, 1) after 0: the same batch comes from the comb table again, with the same bytes"""
    case = fc.bucket_cases()[0]
    _, G, B, n, seed = case
    Z, _ = fc.batch(oracle, B, n, seed)
    got, prof = fc.profile_of(ctx, lambda: gens_ng.commit_rows(Z, B, n))
    check_scopes(prof, {"msm_comb"}, case[0])
    assert np.array_equal(got, want_rows(oracle, case, False))


# ---------------------------------------------------------------- children
def run_rows_children(oracle, cases, env, must_of, blinds=(False, True)):
    spec = [("%s_%d" % (c[0], wb), "rows", (c[1], c[2], c[3], c[4], wb)) for c in cases for wb in blinds]
    res, prof, comb = fc.run_child(spec, env)
    assert sorted(res) == sorted(s[0] for s in spec)
    for c in cases:
        for wb in blinds:
            name = "%s_%d" % (c[0], wb)
            check_scopes(prof[name], must_of(c, wb), (name, env))
            want = want_rows(oracle, c, wb)
            got = np.frombuffer(bytes.fromhex(res[name]), dtype=np.uint8).reshape(-1, 32)
            assert np.array_equal(got, want), (name, env, first_diff(got, want))
    return comb


def bucket_scopes(env):
    return lambda c, wb: fc.scopes_of_route(fc.batch_route(c[2], c[3] + (1 if wb else 0), env))


def test_bucket_pipeline_comb_env_off(oracle):
    """SPG_COMB=0 in a child: no comb table is built and the old shapes run the bucket pipeline"""
    cases = fc.bucket_cases()[:4]
    cases = [(c[0], 1024) + c[2:] for c in cases]
    comb = run_rows_children(oracle, cases, {"SPG_COMB": "0"}, bucket_scopes({}))
    assert comb == (0, 0)


BUCKET_FORMS = [
    {"SPG_FINAL_SL": "32", "SPG_SEG_M": "1", "SPG_ITEM_K": "1"},
    {"SPG_FINAL_SL": "64", "SPG_SEG_M": "4", "SPG_ITEM_K": "3"},
    {"SPG_FINAL_SL": "128", "SPG_SEG_M": "64", "SPG_ITEM_K": "64"},
    {"SPG_ROWS_CMAX": "0"},
    {"SPG_SEG_QUAD_MAX": "0"},
    {"SPG_SMSM_QUAD": "0"},
]


@pytest.mark.parametrize("env", BUCKET_FORMS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_bucket_forms(oracle, env):
    """the A/B forms of the bucket pipeline on a mid-size batch of 128 rows (LDS row sort) and one of 5 rows (count,
    scan, scatter), comb off, and on 5 rows of 64 buckets each. SPG_SEG_M = 1 is one bucket per segment (S = NB), 64
    fewer segments than the default, and on the 64-bucket rows one segment of all of them (m = NB, S = 1);
    SPG_ROWS_CMAX = 0 takes the 128 rows through count and scatter; SPG_SEG_QUAD_MAX = 0 the lane k_segments;
    SPG_SMSM_QUAD = 0 k_final (and the lane kernels of the latency path, below)"""
    for c in (fc.MID, fc.MID_FEW):
        rt, rt0 = fc.batch_route(c[2], c[3], env), fc.batch_route(c[2], c[3])
        assert rt["c"] == rt0["c"]
        if "SPG_FINAL_SL" in env:
            assert rt["final_sl"] == int(env["SPG_FINAL_SL"])
            assert rt["m"] == int(env["SPG_SEG_M"]) and rt["S"] * rt["m"] == rt["NB"] and rt["S"] != rt0["S"]
        if "SPG_ROWS_CMAX" in env:
            assert not rt["rows"] and rt0["rows"] == (c[2] >= 64)
        if "SPG_SEG_QUAD_MAX" in env:
            assert not rt["seg_quad"] and rt0["seg_quad"]
        if "SPG_SMSM_QUAD" in env:
            assert not rt["quad"] and rt0["quad"]
    narrow = fc.batch_route(fc.NARROW[2], fc.NARROW[3], env)
    assert narrow["NB"] == 64
    if env.get("SPG_SEG_M") == "64":
        assert narrow["m"] == narrow["NB"] and narrow["S"] == 1  # one segment holds every bucket
    if env.get("SPG_SEG_M") == "1":
        assert narrow["S"] == narrow["NB"]
    run_rows_children(oracle, [fc.MID, fc.MID_FEW, fc.NARROW], dict(env, SPG_COMB="0"), bucket_scopes(env))


# ---------------------------------------------------------------- latency path (B <= 4, n <= 16384)
def latency_spec(tag):
    spec = []
    for n in fc.LATENCY_SIZES:
        for wb in (0, 1):
            spec.append(("%s_one_n%d_%d" % (tag, n, wb), "one", (1024, n, 300 + n, wb)))
            spec.append(("%s_four_n%d_%d" % (tag, n, wb), "rows", (1024, 4, n, 300 + n, wb)))
    return spec


def check_latency(oracle, res, prof, tag):
    pts = gens_pts(oracle, 1024)
    for n in fc.LATENCY_SIZES:
        for wb in (0, 1):
            for kind, B in (("one", 5), ("four", 4)):
                name = "%s_%s_n%d_%d" % (tag, kind, n, wb)
                check_scopes(prof[name], {"msm_small_bucket", "msm_small_final"}, name)
                bl = fc.blinds_for(oracle, B, 300 + n) if wb else None
                want = fc.expected(oracle, pts, pts[1024], B, n, 300 + n, bl)
                got = np.frombuffer(bytes.fromhex(res[name]), dtype=np.uint8).reshape(-1, 32)
                assert np.array_equal(got, want), (name, first_diff(got, want))


def test_latency_path_windows(oracle):
    """SPG_SMSM_C = 4, 5, 6, 9 (launch_small<4, 5, 6, 9>; the default picks 7 or 8) and a value outside 4..9, which
    is ignored, swept in one child (the knob is re-read on every call): one MSM and four, with and without a blind, at
    sizes on both sides of the 64-, 128- and 256-thread launches"""
    assert [fc.pick_small_window(300, {"SPG_SMSM_C": w}) for w in fc.SMSM_WINDOWS] == [4, 5, 6, 9, 7]
    assert fc.pick_small_window(1025, {"SPG_SMSM_C": "77"}) == 8
    spec = []
    for w in fc.SMSM_WINDOWS:
        spec.append(("", "setenv", ("SPG_SMSM_C", w)))
        spec += latency_spec("c" + w)
    res, prof, _ = fc.run_child(spec, {})
    for w in fc.SMSM_WINDOWS:
        check_latency(oracle, res, prof, "c" + w)


def test_latency_path_lane_form(oracle):
    """SPG_SMSM_QUAD=0: k_smsm_bucket and k_smsm_final, a lane per point"""
    res, prof, _ = fc.run_child(latency_spec("lane"), {"SPG_SMSM_QUAD": "0"})
    check_latency(oracle, res, prof, "lane")


# ---------------------------------------------------------------- comb rows
@pytest.mark.parametrize("env", fc.COMB_ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_comb_rows_forms(oracle, env):
    """msm_comb at every table width (SPG_COMB_C = 10 .. 13), with the window groups per scalar moved off the default
    (SPG_COMB_GMAX, SPG_COMB_GMIN) at the sizes where msm_plan.hpp says they change, one workgroup per row
    (SPG_COMB_WGS = 1: no k_comb_join) and as many as the row has scalar groups, packed entries (SPG_COMB_PAD = 0)"""
    few, many = fc.COMB_SHAPES
    assert fc.comb_rows_shape(few[2], few[3])[0] == 4 and fc.comb_rows_shape(many[2], many[3])[0] == 1
    if "SPG_COMB_GMAX" in env:
        assert fc.comb_rows_shape(few[2], few[3], env)[0] == int(env["SPG_COMB_GMAX"])
    if "SPG_COMB_GMIN" in env:
        assert fc.comb_rows_shape(many[2], many[3], env)[0] == int(env["SPG_COMB_GMIN"])
    if env.get("SPG_COMB_WGS") == "1":
        assert fc.comb_rows_shape(few[2], few[3], env)[1] == 1 and fc.comb_rows_shape(many[2], many[3], env)[1] == 1
    elif "SPG_COMB_WGS" in env:  # S limited by the scalars of a row: 256 / G scalars per workgroup
        assert fc.comb_rows_shape(few[2], few[3], env) == (4, 4) and fc.comb_rows_shape(many[2], many[3] + 1, env) == (1, 2)
    comb = run_rows_children(oracle, fc.COMB_SHAPES, env, lambda c, wb: {"msm_comb"})
    c = int(env.get("SPG_COMB_C", 13))
    assert comb == (fc.comb_table_bytes(c, 256, env.get("SPG_COMB_PAD") != "0"), 1), comb


@pytest.mark.parametrize("gb,want", [("1", "buckets"), ("2", "packed 13-bit table")])
def test_comb_memory_cap_fallback(oracle, gb, want):
    """SPG_COMB_GB on a 256-generator set, whose 13-bit table is 2.7 GB padded and 2.0 GB packed, its 12-bit table
    1.5 GB and 1.1 GB: under 1 GB no table fits and the rows take the bucket pipeline; under 2 GB the packed 13-bit
    table is built"""
    sizes = [fc.comb_table_bytes(c, 256, p) for c, p in ((13, True), (13, False), (12, True), (12, False))]
    fits = [s <= int(gb) << 30 for s in sizes]
    assert fits == ([False] * 4 if want == "buckets" else [False, True, True, True])
    few = fc.COMB_SHAPES[0]
    must = bucket_scopes({}) if want == "buckets" else (lambda c, wb: {"msm_comb"})
    comb = run_rows_children(oracle, [few], {"SPG_COMB_GB": gb}, must)
    assert comb == ((0, 0) if want == "buckets" else (sizes[1], 1))


def test_comb_table_grows(ctx, oracle):
    """one generator set's table rebuilt twice in a process (256, then 512, then 1024 generators): rows of every width
    are right before and after each rebuild, from the table that replaced theirs too"""
    import spg

    g = spg.Gens(ctx, 1024, fc.LABEL)
    built0 = spg.comb_stats()[1]
    for step, R in enumerate([256, 512, 256, 1024, 512, 256]):
        case = ("grow_%d" % R, 1024, 64, R, 40 + R)
        Z, _ = fc.batch(oracle, 64, R, case[4])
        for wb in (False, True):
            bl = fc.blinds_for(oracle, 64, case[4]) if wb else None
            got, prof = fc.profile_of(ctx, lambda: g.commit_rows(Z, 64, R, bl))
            check_scopes(prof, {"msm_comb"}, (case[0], step))
            want = want_rows(oracle, case, wb)
            assert np.array_equal(got, want), (case[0], step, wb, first_diff(got, want))
        assert spg.comb_stats()[1] - built0 == {0: 1, 1: 2, 2: 2}.get(step, 3), step


def test_comb_table_retired_under_another_context(ctx, oracle):
    """a second context grows the table of a generator set (256 -> 512 -> 1024 generators) while this one keeps
    committing 256-scalar rows on its own stream from another thread: a launch that took its copy of the table before
    a rebuild runs on the retired table, which comb_ensure keeps allocated (comb_retired) until the set is freed.
    Every result of both contexts, before, during and after the rebuilds, is the oracle's."""
    import threading

    import spg

    g = spg.Gens(ctx, 1024, fc.LABEL)
    ctx2 = spg.Context(0)
    built0 = spg.comb_stats()[1]
    cases = {R: ("grow_%d" % R, 1024, 64, R, 40 + R) for R in (256, 512, 1024)}
    Z = {R: fc.batch(oracle, 64, R, cases[R][4])[0] for R in cases}
    want = {R: want_rows(oracle, cases[R], False) for R in cases}

    def rows(c, R):
        out = np.zeros((64, 32), dtype=np.uint8)
        z = np.ascontiguousarray(Z[R], dtype=np.uint64)
        c.call("spg_commit_rows", g._h, z.ctypes.data_as(ctypes.c_void_p), 64, R, None, out.ctypes.data_as(ctypes.c_void_p))
        return out

    assert np.array_equal(rows(ctx, 256), want[256])  # the 256-generator table exists before the threads start
    bad, done, count = [], threading.Event(), [0]

    def keep_committing():
        try:
            while not done.is_set() or count[0] < 20:
                if not np.array_equal(rows(ctx, 256), want[256]):
                    bad.append(("first context", count[0]))
                count[0] += 1
        except Exception as e:  # noqa: BLE001 - reported by the assertion below
            bad.append(("first context", repr(e)))

    t = threading.Thread(target=keep_committing)
    t.start()
    try:
        for R in (512, 256, 1024, 512):
            if not np.array_equal(rows(ctx2, R), want[R]):
                bad.append(("second context", R))
    finally:
        done.set()
        t.join(120)
    assert not t.is_alive()
    ctx2.close()
    assert not bad, bad
    assert count[0] >= 20 and spg.comb_stats()[1] - built0 == 3
    assert np.array_equal(rows(ctx, 1024), want[1024])


# ---------------------------------------------------------------- one large MSM
BIG = ("skew", (20000, b"spg_big_msm"))
BIG_FORMS = [
    # several scalars per thread in msm_big's digit blocks: what production takes past 512 x 256 scalars
    ({"SPG_BIG_SPT": "2", "SPG_BIG_COMB": "0"}, {"msm_big_sort", "msm_big_accum"}),
    ({"SPG_BIG_SPT": "4", "SPG_BIG_COMB": "0"}, {"msm_big_sort", "msm_big_accum"}),
    # the batch pipeline with B = 1 (a 15-bit window, regrouped segments)
    ({"SPG_MSM_BIG": "0"},
     {"msm_count", "msm_scatter", "msm_bucket_items", "msm_segments", "msm_final"}),
    ({"SPG_COMB_C_WIDE": "10"}, {"msm_comb_single"}),
    # no mapped host memory for the comb's parts: msm_single_comb declines and msm_big's buckets run
    ({"SPG_MAPPED_BUCKETS": "0"}, {"msm_big_sort", "msm_big_accum"}),
]


@pytest.mark.parametrize("env,must", BIG_FORMS, ids=[",".join("%s=%s" % kv for kv in e.items()) for e, _ in BIG_FORMS])
def test_big_msm_forms(env, must):
    """test_gpu_msm.py's edge and skew checks of one 20000-point MSM (asserted against the oracle in the child)
    through each form, and the scopes the form launches"""
    if "SPG_BIG_SPT" in env:
        G1, spb1 = fc.big_digit_blocks(20000)
        G, spb = fc.big_digit_blocks(20000, env)
        assert spb1 <= 256 < spb <= 256 * int(env["SPG_BIG_SPT"]) and G < G1, (G, spb)
    res, prof, _ = fc.run_child([("big",) + BIG], env)
    assert res["big"] == "passed"
    check_scopes(prof["big"], must, env)


def test_comb_big_rule_other_branch(oracle):
    """a table of exactly 16384 generators at SPG_COMB_C_BIG=12 (22 windows, 70 GB packed) under single MSMs of 16384
    scalars and a blind (without the blind, 16384 scalars are still the latency path's). The default, 13, is not run
    here: its table is 129 GB, which a device shared with other work may not have free, and where it does not fit the
    library itself falls back to this 12-bit table."""
    n = 16384
    spec = [("big16k_%d" % wb, "one", (n, n, 500, wb)) for wb in (1,)]
    res, prof, comb = fc.run_child(spec, {"SPG_COMB_C_BIG": "12"})
    pts = gens_pts(oracle, n)
    for wb in (1,):
        name = "big16k_%d" % wb
        check_scopes(prof[name], {"msm_comb_single"}, name)
        bl = fc.blinds_for(oracle, 5, 500) if wb else None
        want = fc.expected(oracle, pts, pts[n], 5, n, 500, bl)
        got = np.frombuffer(bytes.fromhex(res[name]), dtype=np.uint8).reshape(-1, 32)
        assert np.array_equal(got, want), (name, first_diff(got, want))
    assert comb == (fc.comb_table_bytes(12, n, False), 1), comb
