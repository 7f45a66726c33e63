"""The launch-shape functions of csrc/msm_plan.hpp without a GPU, through libspg_hostcheck.so's spgh_* exports: for
every size the callers can pass, the chosen shape has a case in the dispatch switches of msm.hip / comb.hip (the
instantiation lists are pinned here), the part counts stay within the host staging or the function reports the
fallback, and the window thresholds are where the GPU form tests (tests/test_gpu_msm_forms.py) expect them. The last
tests confirm, from these functions alone, that every size those tests name selects the form it is meant to."""
import itertools

import pytest

import msm_form_cases as fc


def around_pow2(lo, hi):
    """powers of two in [lo, hi] and their neighbours"""
    out = set()
    k = 1
    while k <= hi:
        out |= {k - 1, k, k + 1}
        k *= 2
    return sorted(v for v in out if lo <= v <= hi)


# (C, G, BS) of k_bullet_comb and k_comb_msm_parts (the launch switches of msm.hip)
BULLET_COMB_INST = {(c, g, bs) for c, gs in ((12, (4, 8, 11)), (13, (4, 10))) for g in gs for bs in (64, 128, 256)}
# (C, G) of k_comb_accum (the two launch switches of comb.hip; (12, 4) is their default)
COMB_ACCUM_INST = {(c, g) for c in (9, 10, 11, 12, 13) for g in (1, 2, 4)}
DIGITS_INST = set(range(4, 17))  # k_digits<C>, k_digits_rows<C>
SMALL_INST = set(range(4, 10))  # launch_small<C>, launch_buckets<C>
FINAL_SL_INST = {32, 64, 128}  # k_final_q<SL>

# the fewest scalars per MSM that pick_window picks each width for; 14 is never picked (19 windows, where 15 has 17)
SMALLEST_N = {4: 1, 5: 2, 6: 6, 7: 14, 8: 33, 9: 110, 10: 220, 11: 659, 12: 1317, 13: 2634, 14: None, 15: 10533,
              16: 42131}


def test_instantiation_lists():
    assert len(BULLET_COMB_INST) == 15 and len(COMB_ACCUM_INST) == 15


def test_pick_window_thresholds():
    assert {c: fc.smallest_n(c) for c in range(4, 17)} == SMALLEST_N
    prev = 4
    for n in around_pow2(1, 1 << 24) + [v for v in SMALLEST_N.values() if v] + [v - 1 for v in SMALLEST_N.values() if v and v > 1]:
        c = fc.pick_window(n)
        assert c in DIGITS_INST, (n, c)
    for n in sorted(v for v in SMALLEST_N.values() if v):
        c = fc.pick_window(n)
        assert c > prev or n == 1
        assert n == 1 or fc.pick_window(n - 1) < c
        prev = c
    assert fc.pick_window(16384) == 15  # rows of 2^14 scalars (the SPARK derefs commitments)


def test_pick_small_window():
    for per in around_pow2(1, 16385):
        assert fc.pick_small_window(per) == (7 if per <= 1024 else 8)
        for forced in range(-2, 20):
            c = fc.pick_small_window(per, {"SPG_SMSM_C": str(forced)})
            assert c in SMALL_INST
            assert c == (forced if 4 <= forced <= 9 else fc.pick_small_window(per))


BCOMB_ENVS = [dict(zip(("SPG_BCOMB_G", "SPG_BCOMB_BS", "SPG_BCOMB_R", "SPG_BCOMB_NOTREE"), map(str, v)))
              for v in itertools.product((0, 4, 8, 11, 5), (0, 64, 128, 256, 100), (0, 1, 2, 3, 16, 64, 128),
                                         (0, 16, 4096))]


def test_bullet_comb_launch():
    pmax = fc.hc().spgh_bullet_parts_max()
    assert pmax == 512
    fell_back = ran = 0
    for env in BCOMB_ENVS:
        for c in (12, 13):
            # a round of a DotProductProofLog of n = 2 P (P a power of two), and comb_msm_parts over n scalars
            sizes = [(1 << k, 1 << k) for k in range(0, 17)] + [(max(2, n), n) for n in around_pow2(1, 1 << 16)]
            for shape_P, P in sizes:
                ok, G, BS, R, wgs = fc.bullet_comb_launch(shape_P, P, c, env)
                assert (c, G, BS) in BULLET_COMB_INST, (env, c, P, G, BS)
                assert R >= 1 and R & (R - 1) == 0 and R <= BS // 4, (env, P, R, BS)
                assert wgs == -(-P * G // (BS // 4)) and wgs >= 1
                assert ok == (wgs * R <= pmax), (env, P, wgs, R)
                fell_back += not ok
                ran += ok
                eg = int(env["SPG_BCOMB_G"])
                # the launch is the size's shape with G = 10 for 11 or 8 over 13-bit windows; only where an 8 became
                # 10 (more workgroups than R was clamped for) is R halved again
                G0, BS0, R0 = fc.bullet_comb_shape(shape_P, env)
                assert BS == BS0 and G == (10 if c == 13 and G0 != 4 else G0)
                assert R == R0 or (c == 13 and eg == 8 and R < R0 and wgs * R0 > pmax), (env, c, P, R, R0)
                if c == 13:
                    assert G == (4 if (eg == 4 or (eg not in (8, 11) and shape_P >= 2048)) else 10)
    assert fell_back and ran
    # the defaults: G = 11 (10 over 13-bit windows) and R = 8 below P = 2048, the parts limit biting first at P = 512
    assert fc.bullet_comb_launch(256, 256, 12) == (True, 11, 256, 8, 44)
    assert fc.bullet_comb_launch(512, 512, 12) == (True, 11, 256, 4, 88)
    assert fc.bullet_comb_launch(512, 512, 13) == (True, 10, 256, 4, 80)
    assert fc.bullet_comb_launch(2048, 2048, 12) == (True, 4, 256, 1, 128)
    assert fc.bullet_comb_launch(1, 1, 13)[:3] == (True, 10, 64)
    assert fc.bullet_comb_launch(128, 128, 13, {"SPG_BCOMB_G": "8"})[1] == 10  # an 8 lands on 10 over 13-bit windows
    assert fc.bullet_comb_launch(512, 512, 13, {"SPG_BCOMB_G": "8"}) == (True, 10, 256, 4, 80)  # .. and still fits


def test_comb_rows_shape():
    envs = [dict(zip(("SPG_COMB_WGS", "SPG_COMB_GMAX", "SPG_COMB_GMIN"), map(str, v)))
            for v in itertools.product((2048, 1, 0, 1 << 20), (4, 1, 2, 8), (1, 2, 4, 3))]
    for env in envs:
        for B in around_pow2(1, 1 << 16):
            for per in around_pow2(1, 16385):
                G, S = fc.comb_rows_shape(B, per, env)
                for c in (9, 10, 11, 12, 13):
                    assert (c, G) in COMB_ACCUM_INST
                assert 1 <= S <= max(1, -(-per // (256 // G))), (env, B, per, G, S)
                gmin = int(env["SPG_COMB_GMIN"])
                assert G >= (gmin if gmin in (2, 4) else 1)
    # the defaults: 4 window groups per scalar for few scalars, 1 from 2^17 scalars on; 2048 workgroups aimed at
    assert fc.comb_rows_shape(64, 256) == (4, 4)
    assert fc.comb_rows_shape(512, 256) == (1, 1)
    assert fc.comb_rows_shape(1024, 1024) == (1, 2)
    assert fc.comb_rows_shape(64, 16384) == (1, 32)


def test_big_digit_blocks():
    for spt in (1, 2, 4, 1000):
        for per in around_pow2(1, 1 << 24):
            G, spb = fc.big_digit_blocks(per, {"SPG_BIG_SPT": str(spt)})
            assert 1 <= G <= 512 and spb >= 1
            assert G * spb >= per > G * (spb - 1)  # the G blocks of spb scalars cover per, no larger than needed
            if per <= 512 * 256 * spt:
                assert spb <= 256 * spt, (per, spt, G, spb)
    # one scalar per thread up to 512 x 256 scalars, more past that
    assert fc.big_digit_blocks(1 << 17) == (512, 256)
    assert fc.big_digit_blocks((1 << 17) + 1) == (512, 257)
    assert fc.big_digit_blocks(20000) == (79, 254)
    assert fc.big_digit_blocks(20000, {"SPG_BIG_SPT": "4"}) == (20, 1000)


ROUTE_ENVS = [{}, {"SPG_SEG_M": "1"}, {"SPG_SEG_M": "4"}, {"SPG_SEG_M": "64"}, {"SPG_SEG_M": "1000000"},
              {"SPG_ROWS_CMAX": "0"}, {"SPG_ROWS_CMAX": "9"}, {"SPG_SEG_QUAD_MAX": "0"}, {"SPG_SMSM_QUAD": "0"},
              {"SPG_FINAL_SL": "32"}, {"SPG_FINAL_SL": "64"}, {"SPG_FINAL_SL": "128"}, {"SPG_FINAL_SL": "7"}]


def test_msm_batch_route():
    for env in ROUTE_ENVS:
        for B in around_pow2(1, 1 << 16):
            for per in around_pow2(1, 1 << 20):
                r = fc.batch_route(B, per, env)
                assert r["c"] == fc.pick_window(per) and r["c"] in DIGITS_INST
                assert r["NB"] == 1 << (r["c"] - 1) and r["W"] == 253 // r["c"] + 1
                assert r["S"] >= 1 and r["m"] * r["S"] == r["NB"] and 1 << r["log2m"] == r["m"]
                assert r["final_sl"] in FINAL_SL_INST
                assert bool(r["rows"]) == (B >= 64 and r["c"] <= fc.knob("SPG_ROWS_CMAX", env))
                assert bool(r["regroup"]) == (bool(r["quad"]) and B <= 16 and r["S"] > 1024)
                assert r["final_S"] == (r["S"] // 8 if r["regroup"] else r["S"]) and r["final_S"] >= 1
                assert bool(r["seg_quad"]) == (bool(r["quad"]) and B * r["S"] <= fc.knob("SPG_SEG_QUAD_MAX", env))
                if "SPG_FINAL_SL" not in env:
                    assert r["final_sl"] == (32 if B >= 256 else 128)


def test_msm_comb_rule():
    for B in around_pow2(1, 1 << 16):
        for n in around_pow2(1, 1 << 17):
            for bl in (False, True):
                tot = B * (n + bl)
                want = B >= 64 and (tot >= 1 << 14 if n <= 1024 else (n <= 16384 and tot >= 1 << 22))
                assert fc.comb_rule(B, n, bl) == want
                assert not fc.comb_rule(B, n, bl, has_idx=True)


def test_layer_grid_and_grid_for():
    envs = [{}, {"SPG_LAYER_ONEWG": "0"}, {"SPG_LAYER_ONEWG": str(1 << 20)}, {"SPG_LAYER_EPT": "1"},
            {"SPG_LAYER_EPT": "8"}]
    for env in envs:
        one_wg, ept = fc.knob("SPG_LAYER_ONEWG", env), fc.knob("SPG_LAYER_EPT", env)
        for W in around_pow2(1, 1 << 26):
            K, BS = fc.layer_grid(W, env)
            assert 1 <= K <= 2048 and BS == (64 if W <= 64 else 256)
            if W <= max(64, one_wg):
                assert K == 1
            else:
                assert K == min(2048, -(-W // (256 * ept)))
    for cap in ("1", "2", "1024", "4096", "100000"):
        env = {"SPG_SC_GRID": cap}
        for total in around_pow2(0, 1 << 30):
            nb = fc.grid_for(total, env)
            assert 1 <= nb <= min(int(cap), 4096)
            assert nb == max(1, min(min(int(cap), 4096), -(-total // 256)))
    assert fc.grid_for(1 << 20) == 1024 and fc.grid_for(1000) == 4


# ---- the sizes tests/test_gpu_msm_forms.py names select the forms they are meant to
def test_bucket_cases_select_their_forms():
    cases = fc.bucket_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    seen_rows, seen_few = set(), set()
    for name, G, B, n, _ in cases:
        assert B >= 5 and n <= G, "past the latency path (B <= 4), within the generator set"
        for bl in (0, 1):
            r = fc.batch_route(B, n + bl)
            # (the blind is one more scalar: the one-scalar rows of window 4 are two-scalar rows of window 5 with it)
            if name.startswith("rows_c"):
                assert r["rows"] and (r["c"] == int(name[6:]) or (bl and n == 1))
                seen_rows.add(r["c"])
            if name.startswith("few_c"):
                assert not r["rows"] and (r["c"] == int(name[5:]) or (bl and n == 1))
                seen_few.add(r["c"])
    assert seen_few == set(fc.WINDOWS) == {c for c, n in SMALLEST_N.items() if n}
    assert seen_rows == {c for c in fc.WINDOWS if c <= fc.knob("SPG_ROWS_CMAX")} and 16 in seen_rows
    by = {c[0]: c for c in cases}
    for old in ("old_128x512", "old_64x1024", "old_512x64"):
        assert fc.comb_rule(by[old][2], by[old][3]) and fc.batch_route(by[old][2], by[old][3])["rows"]
    f32 = by["final32_256x32"]
    assert not fc.comb_rule(f32[2], f32[3], True) and fc.batch_route(f32[2], f32[3])["final_sl"] == 32
    rg = fc.batch_route(by["few_c15"][2], by["few_c15"][3])
    assert rg["regroup"] and rg["S"] == 2048 and rg["final_S"] == 256
    # the widest rows also pass the quad segment limit: the lane k_segments runs at its default setting there
    assert not fc.batch_route(64, by["rows_c16"][3])["seg_quad"]
    # the mid-size shapes of the forms
    assert fc.batch_route(fc.MID[2], fc.MID[3])["rows"] and not fc.batch_route(fc.MID_FEW[2], fc.MID_FEW[3])["rows"]


def test_latency_sizes_cover_the_three_launches():
    """per <= 64, <= 128 and above: 64-, 128- and 256-thread workgroups (launch_small), with the blind and without"""
    pers = {n + bl for n in fc.LATENCY_SIZES for bl in (0, 1)}
    assert {64, 65, 128, 129} <= pers and min(pers) == 1 and max(pers) > 256
    assert all(p <= 16384 for p in pers)


def test_oracle_share_of_the_widest_case(oracle):
    """the oracle's side of the slowest case is four MSMs of the fewest scalars of a 16-bit window (the 64-row batch
    asks for its four distinct rows only): 4 x 42131 points, measured at 4.8 s on one CPU core (1.2 s per row). No
    wall-clock bound is asserted; the work is pinned instead: four rows, and no other case asks for more points."""
    n = fc.smallest_n(16)
    assert len(fc.distinct_rows(oracle, 8, 1)) == 4
    cases = fc.bucket_cases() + [fc.MID, fc.MID_FEW, fc.NARROW] + fc.COMB_SHAPES
    assert max(c[3] for c in cases) == n == 42131
