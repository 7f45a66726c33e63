"""R1CSProof::prove on the GPU (libspg.so, spg_r1cs_prove) vs the CPU oracle: identical bincode bytes
and identical challenge vectors under the same transcript label and RandomTape seed."""
import numpy as np
import pytest

from r1cs_cases import CASES, GPU_CASES

pytestmark = pytest.mark.gpu
ALL = dict(CASES, **GPU_CASES)
GENS_LABEL = b"gens_r1cs_sat"
GENS_NV = 1 << 24  # TOTAL_NUM_VARS_BOUND = 10^7 -> 2^24 (examples/interface.rs:557-563)


@pytest.fixture(scope="module")
def r1cs_gens(ctx):
    import spg

    return spg.R1CSGens(ctx, GENS_LABEL, GENS_NV)


def test_r1cs_gens_match_oracle(ctx, oracle, r1cs_gens):
    comp = r1cs_gens.compressed()
    ref = oracle.gens_stream(GENS_LABEL, comp.shape[0])
    assert comp.shape[0] == 4098 and np.array_equal(comp, ref)


def gpu_prove(ctx, gens, wl, seed, label=b"r1cs_test"):
    import spg
    import workload

    v = workload.CViews(wl)
    inst = spg.R1CSInst(ctx, v.inst)
    wit = spg.R1CSWitness(ctx, v.secs, wl.nws)
    t = spg.Transcript(label)
    tape = spg.RandomTape(b"proof", seed)
    return spg.r1cs_prove(ctx, gens, inst, wit, wl.P, wl.max_num_proofs, wl.num_proofs, wl.max_num_inputs,
                          wl.num_inputs, t, tape)


@pytest.mark.parametrize("case", sorted(ALL))
def test_r1cs_proof_bytes_match_oracle(ctx, oracle, r1cs_gens, case):
    import workload

    nc, npf, nws, shared = ALL[case]
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    seed = workload.tape_seed()
    ref, ref_ch = oracle.r1cs_prove(wl, seed, gens_label=GENS_LABEL, gens_num_vars=GENS_NV)
    got, got_ch = gpu_prove(ctx, r1cs_gens, wl, seed)
    for a, b in zip(got_ch, ref_ch):
        assert np.array_equal(a, b)
    assert len(got) == len(ref)
    if got != ref:
        from proof_layout import first_diff

        pytest.fail(f"proof bytes differ first at field {first_diff(got, ref)}")


def test_r1cs_proof_is_repeatable(ctx, r1cs_gens):
    import workload

    wl = workload.R1CSWorkload([64, 64], [8, 8], num_sections=2)
    a, _ = gpu_prove(ctx, r1cs_gens, wl, workload.tape_seed())
    b, _ = gpu_prove(ctx, r1cs_gens, wl, workload.tape_seed())
    c, _ = gpu_prove(ctx, r1cs_gens, wl, workload.tape_seed(b"x"))
    assert a == b and a != c


@pytest.mark.parametrize("case", ["p3_ragged_3secs", "shared_p2", "p2_x1024_q64", "p40_ragged_2secs"])
def test_multi_evaluate_matches_oracle(ctx, oracle, case):
    """R1CSInstance::multi_evaluate on the GPU (k_sparse_eval) vs the oracle at random (rx, ry)."""
    import spg
    import workload

    nc, npf, nws, shared = ALL[case]
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    rng = np.random.default_rng(5)
    nx = (wl.max_num_cons - 1).bit_length()
    ny = (wl.num_vars - 1).bit_length()
    r = oracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * (nx + ny), dtype=np.uint8).tobytes())
    rx, ry = r[:nx], r[nx:]
    v = workload.CViews(wl)
    inst = spg.R1CSInst(ctx, v.inst)
    got = spg.r1cs_multi_evaluate(ctx, inst, len(wl.entries), rx, ry)
    ref = oracle.r1cs_multi_evaluate(wl, rx, ry)
    assert np.array_equal(got, ref)


def _int(m):
    import workload

    v = sum(int(m[i]) << (64 * i) for i in range(4))
    return v * pow(workload.R, -1, workload.Q) % workload.Q


def _eq_table(r):
    import workload

    t = [1]
    for x in r:
        t = [v * (1 - x) % workload.Q for v in t] + [v * x % workload.Q for v in t]
        t = [t[i // 2 + (i % 2) * (len(t) // 2)] for i in range(len(t))]
    return t


@pytest.mark.parametrize("case", sorted(CASES))
def test_r1cs_verify(ctx, r1cs_gens, case):
    """spg_r1cs_verify (R1CSProof::verify) accepts the GPU proof with the witness commitments and the rp-bound
    evaluations (multi_evaluate_bound_rp), returns the prover's challenges, and rejects altered claims"""
    import spg
    import workload

    nc, npf, nws, shared = CASES[case]
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    proof, ch = gpu_prove(ctx, r1cs_gens, wl, workload.tape_seed())
    rp, rx, rwry = ch[0], ch[2], ch[3]
    v = workload.CViews(wl)
    ev = spg.r1cs_multi_evaluate(ctx, spg.R1CSInst(ctx, v.inst), len(wl.entries), rx, rwry)
    eq = _eq_table([_int(x) for x in rp])
    if len(wl.entries) == 1:
        bound = [_int(ev[k]) for k in range(3)]
    else:
        bound = [sum(eq[p] * _int(ev[3 * p + k]) for p in range(wl.P)) % workload.Q for k in range(3)]
    sections = []
    for w in range(wl.nws):
        mats = wl.sections[w]
        sections.append(([m.shape[0] for m in mats], [m.shape[1] for m in mats],
                         [spg.r1cs_gens_commit(ctx, r1cs_gens, m.reshape(-1, 4)) for m in mats]))
    args = (ctx, r1cs_gens, wl.P, wl.max_num_proofs, wl.num_proofs, wl.max_num_inputs, sections, wl.max_num_cons)
    ok, why, vch = spg.r1cs_verify(*args, workload.to_mont_limbs(bound), spg.Transcript(b"r1cs_test"), proof)
    assert ok, why
    for a, b in zip(vch, ch):
        assert np.array_equal(a, b)
    bad = list(bound)
    bad[1] = (bad[1] + 1) % workload.Q
    ok, _, _ = spg.r1cs_verify(*args, workload.to_mont_limbs(bad), spg.Transcript(b"r1cs_test"), proof)
    assert not ok
    other = list(sections)
    other[0] = (other[0][0], other[0][1], [list(reversed(c)) if len(c) > 1 else c for c in other[0][2]])
    if other[0][2] != sections[0][2]:
        ok, _, _ = spg.r1cs_verify(*args[:6], other, wl.max_num_cons, workload.to_mont_limbs(bound),
                                   spg.Transcript(b"r1cs_test"), proof)
        assert not ok


@pytest.mark.parametrize("case,env", [
    ("p2_x1024_q64", {"SPG_SC_QUAD_MAX": "0"}),                       # row-factored x rounds, J = 8, 4, 2
    ("p2_x1024_q64", {"SPG_SC_QUAD_MAX": "0", "SPG_P1_ROWS": "0"}),   # the per-point thread form throughout
    ("p8_x256_q32_shared", {"SPG_SC_QUAD_MAX": "0"}),                 # shared matrix, J = 2 at round 0
    ("p2_x256_2secs", {"SPG_SC_QUAD_MAX": "0", "SPG_SC_FUSE": "0"}),  # row form without the fused folds
    ("p2_x1024_q64", {"SPG_P1_PAIR": "0"}),                           # phase 1 one round per launch throughout
    ("p8_x256_q32_shared", {"SPG_P1_PAIR_MAX": "32"}),                # phase-1 pairs only for each mode's last rounds
    ("p2_x1024_q64", {"SPG_Z_TILED": "0", "SPG_SPMV_TILED": "0"}),  # one-element Z fill and Az/Bz/Cz stores
    ("p40_ragged_2secs", {"SPG_Q_BOUND_ALL": "0"}),                   # phase 2's Z prep one q fold per challenge
    ("p2_x1024_q64", {"SPG_P2_PAIR": "0"}),                           # phase 2 one y round per launch throughout
    ("p2_x256_2secs", {"SPG_P2_PAIR_MAX": "32"}),                     # phase-2 pairs only after single y rounds
    ("p2_x1024_q64", {"SPG_P1_PAIR_MAX": "32768", "SPG_P2_PAIR_MAX": "32768"}),  # pairs at their largest
    ("p3_ragged_3secs", {"SPG_TAPE_AHEAD": "0"}),                     # every sumcheck round commits its own points
    ("p3_ragged_3secs", {"SPG_SIGMA_AHEAD": "0"}),                    # each sigma protocol commits on its own
])
def test_r1cs_thread_form_rounds(oracle, case, env):
    """the thread-per-point phase-1 evaluations (k_phase1_eval, and k_phase1_eval_x's row-factored x rounds: one eq
    factor Ap Aq per row and J points per lane) at sizes the oracle proves in seconds, forced by SPG_SC_QUAD_MAX=0 in
    a fresh process: the oracle's bytes"""
    import os
    import subprocess
    import sys

    import workload

    nc, npf, nws, shared = ALL[case]
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    seed = workload.tape_seed()
    ref, _ = oracle.r1cs_prove(wl, seed, gens_label=GENS_LABEL, gens_num_vars=GENS_NV)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, hashlib; sys.path[:0] = [%r, %r]\n"
        "import spg, workload\n"
        "from r1cs_cases import ALL_R1CS\n"
        "from test_gpu_r1cs import gpu_prove, GENS_LABEL, GENS_NV\n"
        "ctx = spg.Context(0)\n"
        "nc, npf, nws, shared = ALL_R1CS[%r]\n"
        "wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)\n"
        "p, _ = gpu_prove(ctx, spg.R1CSGens(ctx, GENS_LABEL, GENS_NV), wl, workload.tape_seed())\n"
        "print(hashlib.sha256(p).hexdigest())\n"
    ) % (os.path.join(root, "spartan-parallel_amd"), os.path.join(root, "tests"), case)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    import hashlib

    assert out.stdout.split()[-1] == hashlib.sha256(ref).hexdigest()


def test_witness_upload_releases_caller_buffers(ctx, r1cs_gens):
    """spg_r1cs_witness_new streams the witness through the page-locked upload ring (h2d_stream) and returns once the
    caller's buffers have been read, with DMAs still in flight: overwriting the caller's arrays right after the call
    must not change the proof, and freeing a witness whose upload may be in flight must be safe. 3 x 2^10 executions x
    512 inputs = 48 MiB, so the 32 MiB ring wraps."""
    import spg
    import workload

    shape = ([256] * 3, [1024] * 3)
    seed = workload.tape_seed()

    def prove(wl, scribble):
        v = workload.CViews(wl)
        inst = spg.R1CSInst(ctx, v.inst)
        spg.R1CSWitness(ctx, v.secs, wl.nws)  # dropped at once: freed with its upload possibly in flight
        wit = spg.R1CSWitness(ctx, v.secs, wl.nws)
        if scribble:
            for mats in wl.sections:
                for m in mats:
                    m[...] = 0xFFFFFFFFFFFFFFFF  # the caller reuses its buffers
            for arr in v.keep:
                if arr.ndim == 3:
                    arr[...] = 0xFFFFFFFFFFFFFFFF
        pf, _ = spg.r1cs_prove(ctx, r1cs_gens, inst, wit, wl.P, wl.max_num_proofs, wl.num_proofs, wl.max_num_inputs,
                               wl.num_inputs, spg.Transcript(b"upload_test"), spg.RandomTape(b"proof", seed))
        return pf

    a = prove(workload.R1CSWorkload(*shape), scribble=True)
    b = prove(workload.R1CSWorkload(*shape), scribble=False)
    assert a == b
