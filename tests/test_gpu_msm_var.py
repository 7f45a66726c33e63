"""Variable-base MSM over caller-supplied points on the GPU (spg_points, spg_msm_var*; msm_var.hip):
GroupElement::vartime_multiscalar_mul (src/group.rs:98-116) over points that are no generator set. Every result is
compared byte for byte with the oracle's orc_msm (pyoracle.msm), and a batch of single-point MSMs with libsodium's
scalar multiplications (tests/golden/ristretto_sodium.json)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vmsm_cases as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def pts4096(ctx, oracle):
    import spg

    return spg.Points(ctx, vc.points(oracle))


# ---- in-process, default knobs
@pytest.mark.parametrize("n", vc.SIZES)
def test_sizes(ctx, oracle, pts4096, n):
    pts, s = vc.size_case(oracle, n)
    assert pts4096.msm(s) == vc.ref(oracle, "n%d" % n, pts, s)


def test_offset_buf_points_and_empty(ctx, oracle, pts4096):
    import spg

    P = vc.points(oracle)
    rng = np.random.default_rng(5)
    s = vc.rand_fq(oracle, rng, 700)
    assert pts4096.n == 4096 and np.array_equal(pts4096.compressed(), P)
    assert pts4096.msm(s[:300], offset=1000) == oracle.msm(P[1000:1300], s[:300])
    assert pts4096.msm(s[:50], offset=4046) == oracle.msm(P[4046:], s[:50])
    buf = spg.Buf(ctx, s)
    want = oracle.msm(P[10:510], s[200:700])
    assert pts4096.msm_buf(buf, offset=10, s_offset=200, n=500) == want
    assert pts4096.msm_buf(buf, offset=3, s_offset=690, n=10) == oracle.msm(P[3:13], s[690:700])  # host path
    assert spg.msm_points(ctx, P[10:510], s[200:700]) == want
    assert spg.msm_points(ctx, P[:9], s[:9]) == oracle.msm(P[:9], s[:9])
    assert pts4096.msm(np.zeros((0, 4), np.uint64)) == bytes(32)
    assert pts4096.msm_buf(buf, offset=5, s_offset=7, n=0) == bytes(32)
    assert spg.msm_points(ctx, np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.uint64)) == bytes(32)


def test_edge_scalars(ctx, oracle, pts4096):
    for name, (pts, s) in vc.edge_scalar_cases(oracle).items():
        assert pts4096.msm(s) == vc.ref(oracle, name, pts, s), name
    assert pts4096.msm(np.zeros((256, 4), np.uint64)) == bytes(32)  # identity


def test_edge_points(ctx, oracle):
    import spg

    cases = vc.edge_point_cases(oracle)
    for name, (pts, s) in cases.items():
        want = vc.ref(oracle, name, pts, s)
        assert spg.msm_points(ctx, pts, s) == want, name
    assert vc.ref(oracle, "p_and_minus_p", *cases["p_and_minus_p"]) == bytes(32)


def test_libsodium_scalarmult_batch(ctx):
    """16 single-point MSMs in one batch equal libsodium's k * P (independent of the oracle)"""
    import fieldref
    import spg

    sm = json.load(open(os.path.join(G, "ristretto_sodium.json")))["scalarmult"]
    pts = np.array([list(bytes.fromhex(p)) for p, _, _ in sm], dtype=np.uint8)
    ks = [int.from_bytes(bytes.fromhex(k), "little") for _, k, _ in sm]
    assert all(k < fieldref.Q for k in ks)
    s = fieldref.arr_u64([fieldref.to_mont(k) for k in ks])
    P = spg.Points(ctx, pts)
    got = P.msm_batch(np.arange(16), np.ones(16, np.uint64), s)
    assert [g.tobytes().hex() for g in got] == [r for _, _, r in sm]


def test_batch(ctx, oracle, pts4096):
    P = vc.points(oracle)
    rng = np.random.default_rng(9)
    lens = [0, 1, 64, 257, 1000]
    offs = [17, 4095, 100, 130, 3000]
    s = vc.rand_fq(oracle, rng, sum(lens))
    got = pts4096.msm_batch(offs, lens, s)
    at = 0
    for b, (o, n) in enumerate(zip(offs, lens)):
        sb = s[at:at + n]
        want = oracle.msm(P[o:o + n], sb) if n else bytes(32)
        assert got[b].tobytes() == want, b
        assert pts4096.msm(sb, offset=o) == want, b
        at += n
    # two coinciding ranges with different scalars (two L vectors against one commitment), and an overlapping one
    s2 = vc.rand_fq(oracle, rng, 300 + 300 + 200)
    got = pts4096.msm_batch([500, 500, 700], [300, 300, 200], s2)
    assert got[0].tobytes() == oracle.msm(P[500:800], s2[:300])
    assert got[1].tobytes() == oracle.msm(P[500:800], s2[300:600])
    assert got[2].tobytes() == oracle.msm(P[700:900], s2[600:])
    assert got[0].tobytes() != got[1].tobytes()
    # every MSM empty
    assert not pts4096.msm_batch([0, 9], [0, 0], np.zeros((0, 4), np.uint64)).any()


@pytest.mark.parametrize("n", [5, 300])
def test_invalid_encodings(ctx, oracle, n):
    import spg

    P = vc.points(oracle)[:n]
    s = vc.rand_fq(oracle, np.random.default_rng(n), n)
    for idx in ([0], [n - 1], [n - 2, 2]):
        bad = P.copy()
        for i in idx:
            bad[i, 0] ^= 1  # odd s: CompressedRistretto::decompress rejects it
        with pytest.raises(spg.SpgError) as e:
            spg.Points(ctx, bad)
        assert "SPG_E_POINT" in str(e.value) and str(e.value).endswith("index %d" % min(idx))
        with pytest.raises(spg.SpgError) as e:
            spg.msm_points(ctx, bad, s)
        assert "SPG_E_POINT" in str(e.value)
        good = spg.Points(ctx, P)  # the context works on
        assert good.msm(s) == oracle.msm(P, s)
    good = spg.Points(ctx, P)
    for off, k in ((1, n), (n, 1), (n + 1, 0)):
        with pytest.raises(spg.SpgError) as e:
            good.msm(s[:k], offset=off)
        assert "SPG_E_ARG" in str(e.value)
    with pytest.raises(spg.SpgError) as e:
        good.msm_batch([0, n - 1], [1, 2], s[:3])
    assert "SPG_E_ARG" in str(e.value)


# ---- fresh processes that read the knobs
def child(code, env):
    pre = "import sys; sys.path[:0] = [%r, %r, %r]\n" % (os.path.join(ROOT, "spartan-parallel_amd"),
                                                       os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", pre + code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert lines[-2] == "ok", out.stdout[-500:]
    return lines[:-2]


@pytest.mark.parametrize("c", ["4", "6", "7", "8", "11", "13", "14"])
def test_forced_windows_through_the_kernels(oracle, c):
    """SPG_VMSM_HOST_MAX=0 sends every size through the kernels, SPG_VMSM_C forces the window: both sides of the
    64-bucket group boundary (c = 7 | 8), the smallest window, and a bucket split into chunks"""
    lines = child("import vmsm_cases; vmsm_cases.child_main()\n", {"SPG_VMSM_HOST_MAX": "0", "SPG_VMSM_C": c})
    got = dict(line.split() for line in lines)
    cases = vc.child_cases(oracle)
    assert sorted(got) == sorted(cases)
    for name, (pts, s) in cases.items():
        assert got[name] == vc.ref(oracle, name, pts, s).hex(), name


def test_small_chunks_through_the_kernels(oracle):
    """chunks of 64 entries: the n = 1000 buckets of the default window split too, and every group sums many chunks"""
    lines = child("import vmsm_cases; vmsm_cases.child_main()\n", {"SPG_VMSM_HOST_MAX": "0", "SPG_VMSM_CH": "64"})
    got = dict(line.split() for line in lines)
    for name, (pts, s) in vc.child_cases(oracle).items():
        assert got[name] == vc.ref(oracle, name, pts, s).hex(), name


VERIFY_CHILD = """
import spg
from test_gpu_verify import Program
from proof_layout import snark_proof_fields
ctx = spg.Context(0)
prog = Program(ctx, spg.R1CSGens(ctx, b"gens_r1cs_sat", 1 << 24), "b2_x32_q2")
ctx.prof_enable(True)
ctx.prof_read(reset=True)
print("good", *prog.verify())
prof = ctx.prof_read(reset=True)
print("vmsm_load", prof.get("vmsm_load", (0,))[0])
# two rows of one Hyrax commitment swapped: every point still decodes, the weighted sum L * C is another point
groups = {}
for name, s, e in snark_proof_fields(prog.proof):
    if name.startswith("block_comm_vars_list[") and e - s == 32:
        groups.setdefault(name.rsplit("[", 1)[0], []).append((s, e))
rows = [g for g in groups.values() if len(g) >= 2 and prog.proof[g[0][0]:g[0][1]] != prog.proof[g[1][0]:g[1][1]]][0]
(s0, e0), (s1, e1) = rows[0], rows[1]
swapped = bytearray(prog.proof)
swapped[s0:e0], swapped[s1:e1] = prog.proof[s1:e1], prog.proof[s0:e0]
print("swapped", *prog.verify(bytes(swapped)))
flipped = bytearray(prog.proof)
flipped[s0 + 16] ^= 0x04  # one byte of a row commitment changed
print("flipped", *prog.verify(bytes(flipped)))
print("ok")
"""


def test_verifier_opt_in():
    """SPG_VERIFY_VMSM=1 routes the verifier's row-commitment MSMs through spg_points_upload + spg_msm_var_batch (the
    profile counts vmsm_load launches with the knob and none without): the smallest SNARK shape verifies, the same
    proof with two rows of a commitment swapped (all points valid) or one byte of a row changed is rejected, and the
    verdicts equal those of the run without the knob"""
    on = [line.split() for line in child(VERIFY_CHILD, {"SPG_VERIFY_VMSM": "1"})]
    off = [line.split() for line in child(VERIFY_CHILD, {"SPG_VERIFY_VMSM": "0"})]
    assert [x[:2] for x in on] != [] and on[0][:2] == ["good", "True"], on
    assert on[1][0] == "vmsm_load" and int(on[1][1]) > 0, on
    assert off[1] == ["vmsm_load", "0"], off
    assert on[2][:2] == ["swapped", "False"] and on[3][:2] == ["flipped", "False"], on
    assert [x[:2] for x in on if x[0] != "vmsm_load"] == [x[:2] for x in off if x[0] != "vmsm_load"]
