"""DotProductProofLog's device Bullet rounds at every launch shape, through spg_poly_eval_prove with
SPG_BULLET_HOST_MAX=0 (every proof size on the device), against the dense-polynomial checker (tests/polyeval_ref.py
over the oracle's headers): the prove needs L.Z and the opening, not the commitment, so the CPU side stays cheap.

Every round of an n-point proof runs its two MSMs over n / 2 generators (the generators are not folded: proto.hip
passes the full n to each round), so one proof runs one launch shape log2(n) times. Four polynomials therefore: 14, 16
and 18 variables (rows of 128, 256 and 512: P = 64, 128 and 256 points per MSM, the 64-, 128- and 256-thread kernels)
and 19 variables (rows of 1024: P = 512 is where the limit on parts per MSM first clamps the points a workgroup
leaves for the host). One fresh child process per environment, one at a time.

Every child reads the kernel profile, and the test predicts it from the knobs and csrc/msm_plan.hpp alone:
msm_bullet_round launches (one per round on the device, none otherwise) and their modelled bytes (the comb round's
scope carries 96 bytes per table entry, the bucket round's none: a comb form that quietly fell back to the bucket
kernel has the same count and the same proof, and is told apart here), msm_comb_parts launches (Cx and delta: 2, 1 or
0), msm_delta_scalars (the device delta scalars) and whether any latency-path bucket launch ran. The proof must also
verify with spg_poly_eval_verify_plain."""
import hashlib
import os
import subprocess
import sys

import pytest

import msm_form_cases as fc
import polyeval_cases as pc
import polyeval_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL, TLABEL = b"gens_bullet_forms", b"bullet_forms"
NVS = [14, 16, 18, 19]
DEV = {"SPG_BULLET_HOST_MAX": "0"}

FORMS = {
    "default": DEV,
    # SPG_COMB_C in {12, 13} x SPG_BCOMB_G in {unset, 4, 8}, with SPG_BCOMB_R = 1, 2, 16, SPG_BCOMB_BS = 64, 256 and
    # SPG_BCOMB_NOTREE = 16, 4096 spread over them (all four feed one shape function)
    "c12_r1_bs64": dict(DEV, SPG_COMB_C="12", SPG_BCOMB_R="1", SPG_BCOMB_BS="64"),
    "c12_g4_r2_bs256": dict(DEV, SPG_COMB_C="12", SPG_BCOMB_G="4", SPG_BCOMB_R="2", SPG_BCOMB_BS="256"),
    "c12_g8_r16": dict(DEV, SPG_COMB_C="12", SPG_BCOMB_G="8", SPG_BCOMB_R="16"),
    "c13_notree16": dict(DEV, SPG_COMB_C="13", SPG_BCOMB_NOTREE="16"),
    "c13_g4_notree4096": dict(DEV, SPG_COMB_C="13", SPG_BCOMB_G="4", SPG_BCOMB_NOTREE="4096"),
    "c13_g8": dict(DEV, SPG_COMB_C="13", SPG_BCOMB_G="8"),  # the 8 lands on 10
    # k_bullet_round_q<7, 64 | 128 | 256>, Cx and delta on the latency-path buckets
    "bucket_rounds": dict(DEV, SPG_BULLET_COMB="0"),
    "state_on_host": dict(DEV, SPG_BULLET_DEV="0"),
    "round0_not_ahead": dict(DEV, SPG_BULLET_AHEAD="0"),
    "no_mapped_buckets": dict(DEV, SPG_MAPPED_BUCKETS="0"),
    "delta_scalars_from_host": dict(DEV, SPG_DELTA_DEV="0"),
    "delta_bucket_msm": dict(DEV, SPG_DELTA_COMB="0"),
    # the host fold of n >= 256 is the only site that reads SPG_BULLET_OVERLAP
    "host_proof_no_overlap": {"SPG_BULLET_HOST_MAX": "4096", "SPG_BULLET_OVERLAP": "0"},
}
SCOPES = ("msm_bullet_round", "msm_comb_parts", "msm_small_bucket", "msm_delta_scalars")


def inputs(nv):
    Z, r = pc.scalars(700 + nv, 1 << nv), pc.scalars(800 + nv, nv)
    return Z, r, pc.evaluate(Z, r, nv)


def child_main():
    import spg
    import workload

    ctx = spg.Context(0)
    for nv in NVS:
        g = spg.PolyGens(ctx, LABEL, nv)
        Z, r, Zr = inputs(nv)
        buf = spg.Buf(ctx, Z)
        ctx.prof_enable(True)
        ctx.prof_read(reset=True)
        proof, _ = spg.poly_eval_prove(ctx, g, buf, r, Zr, spg.Transcript(TLABEL),
                                       spg.RandomTape(ref.TAPE, workload.tape_seed()))
        prof = ctx.prof_read(reset=True)
        ctx.prof_enable(False)
        comm = spg.poly_commit(ctx, g, buf, nv)
        ok, why = spg.poly_eval_verify_plain(ctx, g, r, Zr, comm, spg.Transcript(TLABEL), proof)
        print(nv, hashlib.sha256(proof).hexdigest(), int(bool(ok)), *(prof.get(k, (0,))[0] for k in SCOPES),
              repr(float(prof.get("msm_bullet_round", (0, 0, 0.0))[2])))
        buf.free()
        g.free()
    print("ok")


@pytest.fixture(scope="module")
def wanted(oracle):
    import workload

    out = {}
    for nv in NVS:
        Z, r, Zr = inputs(nv)
        w = ref.prove(LABEL, nv, TLABEL, workload.tape_seed(), Z, r, Zr)
        assert w.verified
        out[nv] = hashlib.sha256(w.proof).hexdigest()
    return out


def on(env, name):
    return fc.knob(name, env) != 0


def windows(env):
    """the comb table's window widths an environment can give these generator sets"""
    return [int(env["SPG_COMB_C"])] if "SPG_COMB_C" in env else [12, 13]


def comb_takes(env, shape_P, P):
    """whether the comb launch of P points per MSM runs under env: the shape function's answer, which does not depend
    on the table's window width at these sizes (asserted)"""
    oks = {fc.bullet_comb_launch(shape_P, P, c, env)[0] for c in windows(env)}
    assert len(oks) == 1
    return oks.pop() and on(env, "SPG_BULLET_COMB")


def cx_from_comb(env, n):
    """comb_msm_parts over the n scalars of Cx (and of delta)"""
    return comb_takes(env, max(2, n), n)


def comb_round_bytes(n, c):
    """the modelled bytes of the log2(n) comb rounds of an n-point proof (bullet_round_comb's KScope): per round every
    nonzero digit's 96-byte entry, 96 nk for the aa fold (nk = n, n / 2, .., 2) and 68 n for cw and the indices"""
    rounds = n.bit_length() - 1
    entries = float(n) * (253 // c + 1) * (1.0 - 1.0 / float(1 << c))
    return rounds * (96.0 * entries + 68.0 * n) + 96.0 * (2 * n - 2)


def predicted(env, n):
    """(rounds, comb round bytes per window width or [0.0], comb parts launches, any bucket launch, delta scalars)"""
    on_host = n <= fc.knob("SPG_BULLET_HOST_MAX", env)
    dev = not on_host and on(env, "SPG_BULLET_DEV") and on(env, "SPG_MAPPED_BUCKETS")
    if on_host:
        return 0, [0.0], 0, False, 0
    if not dev:  # every MSM of the proof through the latency-path buckets
        return 0, [0.0], 0, True, 0
    rounds = n.bit_length() - 1
    nbytes = [comb_round_bytes(n, c) for c in windows(env)] if comb_takes(env, n // 2, n // 2) else [0.0]
    cx = on(env, "SPG_BULLET_AHEAD") and cx_from_comb(env, n)
    delta = on(env, "SPG_DELTA_COMB") and cx_from_comb(env, n)
    dscal = int(on(env, "SPG_DELTA_COMB") and on(env, "SPG_DELTA_DEV"))
    return rounds, nbytes, int(cx) + int(delta), not (cx and delta), dscal


def test_shapes_the_sizes_select():
    """from csrc/msm_plan.hpp alone: the four proof sizes run the three workgroup sizes and the clamp of R, 13-bit
    windows turn 8 or 11 groups into 10, every form moves the shape it names, and the forms' predictions differ from
    the default's where the issue's knobs are meant to act"""
    pmax = fc.hc().spgh_bullet_parts_max()
    # 64-thread workgroups over the 1024 scalars of Cx are 704 workgroups, more than the parts limit even at one point
    # each: there comb_msm_parts declines and the latency-path buckets run (the rounds, of half as many points, fit)
    small_wgs = FORMS["c12_r1_bs64"]
    assert cx_from_comb(small_wgs, 512) and not cx_from_comb(small_wgs, 1024)
    assert all(cx_from_comb(env, n) == on(env, "SPG_BULLET_COMB") for name, env in FORMS.items()
               if name != "c12_r1_bs64" for n in (128, 256, 512, 1024))
    for c in (12, 13):
        assert [fc.bullet_comb_launch(P, P, c)[2] for P in (64, 128, 256, 512)] == [64, 128, 256, 256]
        ok, G, BS, R, wgs = fc.bullet_comb_launch(512, 512, c)
        assert ok and R == 4 and wgs * 8 > pmax >= wgs * R
        assert fc.bullet_comb_launch(256, 256, c)[3] == 8
    for name, env in FORMS.items():
        c = int(env.get("SPG_COMB_C", 13))
        for P in (512, 256, 128, 64):
            ok, G, BS, R, wgs = fc.bullet_comb_launch(P, P, c, env)
            assert ok, (name, P)
            eg = env.get("SPG_BCOMB_G")
            assert G == ({None: 10, "4": 4, "8": 10}[eg] if c == 13 else {None: 11, "4": 4, "8": 8}[eg]), (name, P, G)
            if "SPG_BCOMB_BS" in env:
                assert BS == int(env["SPG_BCOMB_BS"])
            if "SPG_BCOMB_NOTREE" in env and P <= int(env["SPG_BCOMB_NOTREE"]):
                assert R == min(BS // 4, max(r for r in (1, 2, 4, 8, 16, 32, 64) if wgs * r <= pmax and r <= BS // 4))
            elif "SPG_BCOMB_R" in env:
                want = int(env["SPG_BCOMB_R"])
                while want > 1 and wgs * want > pmax:
                    want //= 2
                assert R == want, (name, P, R)
    base = predicted(FORMS["default"], 512)
    assert base == (9, [comb_round_bytes(512, 12), comb_round_bytes(512, 13)], 2, False, 1)
    for name in ("bucket_rounds", "state_on_host", "round0_not_ahead", "no_mapped_buckets", "delta_scalars_from_host",
                 "delta_bucket_msm", "host_proof_no_overlap"):
        assert predicted(FORMS[name], 512) != base, name


@pytest.mark.parametrize("form", sorted(FORMS))
def test_bullet_forms(wanted, form):
    env = FORMS[form]
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\nimport test_gpu_bullet_forms\ntest_gpu_bullet_forms.child_main()\n"
            % (os.path.join(ROOT, "spartan-parallel_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [line.split() for line in out.stdout.strip().split("\n")]
    assert lines[-1] == ["ok"] and [int(w[0]) for w in lines[:-1]] == NVS, out.stdout[-500:]
    for nv, sha, ok, rounds, parts, small, dscal, nbytes in lines[:-1]:
        nv, n = int(nv), 1 << (int(nv) - int(nv) // 2)
        got = (int(rounds), float(nbytes), int(parts), int(small) > 0, int(dscal))
        assert sha == wanted[nv], (form, nv, "proof bytes differ from the checker's", got)
        assert ok == "1", (form, nv, "spg_poly_eval_verify_plain rejected the proof")
        p_rounds, p_bytes, p_parts, p_small, p_dscal = predicted(env, n)
        assert got[0] == p_rounds, (form, nv, got)
        assert any(abs(got[1] - b) <= 1e-9 * max(b, 1.0) for b in p_bytes), (form, nv, got, p_bytes)
        assert got[2] == p_parts, (form, nv, got)
        assert got[3] == p_small, (form, nv, got)
        assert got[4] == p_dscal, (form, nv, got)
