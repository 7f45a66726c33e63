"""CPU: the test helper behind tests/test_gpu_r1cs_seams.py (tests/r1cs_seams_ref.py over the oracle's own
R1CSProof::prove pieces) checked on its own: new_rev against an index permutation, the eval tables against the
reference loop restated on Python integers, and the helper's ZK sumcheck verifier on the helper's own proofs."""
import numpy as np
import pytest

import r1cs_cases
import r1cs_seams_ref as ref

Q = 2**252 + 27742317777372353535851937790883648493
R = 2**256
RINV = pow(R, -1, Q)


def to_int(v):
    return sum(int(v[i]) << (64 * i) for i in range(4)) * RINV % Q


def rand_fq(oracle, rng, n):
    return oracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * n, dtype=np.uint8).tobytes()).reshape(n, 4)


def workload_of(oracle, case, seed=1):
    """the case's R1CSWorkload with random matrix values, and its z_mat flat in (p, q, w, x) order"""
    import workload

    nc, npf, nws, shared = r1cs_cases.ALL_R1CS[case]
    wl = workload.R1CSWorkload(nc, npf, num_sections=nws, shared_instance=shared)
    rng = np.random.default_rng(seed + len(case))
    for mats in wl.entries:
        for m in mats:
            m[:, 2:] = rand_fq(oracle, rng, m.shape[0])
    z = np.concatenate([np.stack([wl.sections[w][p][q] for w in range(wl.nws)]).reshape(-1, 4)
                        for p in range(wl.P) for q in range(wl.num_proofs[p])])
    return wl, z


def rev(v, bits):
    return int(format(v, "0%db" % bits)[::-1], 2) if bits else 0


def new_rev_index(num_proofs, nws, num_inputs):
    """perm with out[perm[i]] = z[i] for DensePolynomialPqx::new_rev (src/custom_dense_mlpoly.rs:67-111)"""
    perm, off = [], 0
    for npf, ni in zip(num_proofs, num_inputs):
        lq, lx = npf.bit_length() - 1, ni.bit_length() - 1
        for q in range(npf):
            for w in range(nws):
                for x in range(ni):
                    perm.append(off + (rev(q, lq) * nws + w) * ni + rev(x, lx))
        off += npf * nws * ni
    return np.asarray(perm)


@pytest.mark.parametrize("case", ["p3_ragged_3secs", "p2_q_single_5secs", "p5_q1"])
def test_new_rev_is_the_index_permutation(oracle, case):
    wl, z = workload_of(oracle, case)
    got, (dims, npf, nin) = ref.new_rev(z, wl.num_proofs, wl.max_num_proofs, wl.nws, wl.num_inputs, wl.max_num_inputs)
    want = np.zeros_like(z)
    want[new_rev_index(wl.num_proofs, wl.nws, wl.num_inputs)] = z
    assert z.any() and np.array_equal(got, want)
    assert dims == (1 << (wl.P - 1).bit_length(), wl.max_num_proofs, 1 << (wl.nws - 1).bit_length(), wl.max_num_inputs)
    assert npf == list(wl.num_proofs) and nin == list(wl.num_inputs)


def test_eval_tables_match_python_integers(oracle):
    """sparse_mlpoly.rs:534-540: out[col / max_num_cols][col % max_num_cols] += rx[row] * val, per matrix"""
    import workload

    wl, _ = workload_of(oracle, "p3_ragged_3secs")
    v = workload.CViews(wl)
    rx = rand_fq(oracle, np.random.default_rng(4), wl.max_num_cons)
    got = ref.eval_tables(v.inst, wl.nws, wl.max_num_inputs, wl.num_inputs, rx)
    rxi = [to_int(x) for x in rx]
    for m in range(3):
        want = []
        for p in range(wl.P):
            tab = [[0] * wl.num_inputs[p] for _ in range(wl.nws)]
            for e in wl.entries[p][m]:
                row, col = int(e[0]), int(e[1])
                tab[col // wl.max_num_inputs][col % wl.max_num_inputs] += rxi[row] * to_int(e[2:])
            want += [x % Q for sec in tab for x in sec]
        assert any(want) and [to_int(x) for x in got[m]] == want
    # the combination and its new_rev: r_A A + r_B B + r_C C at the bit-reversed x
    rs = rand_fq(oracle, np.random.default_rng(5), 3)
    abc, (dims, npf, nin) = ref.abc_poly(v.inst, wl.P, wl.nws, wl.max_num_inputs, wl.num_inputs, rx, *rs)
    comb = [sum(to_int(r) * to_int(t[i]) for r, t in zip(rs, got)) % Q for i in range(got[0].shape[0])]
    perm = new_rev_index([1] * wl.P, wl.nws, wl.num_inputs)
    want = [0] * len(comb)
    for i, j in enumerate(perm):
        want[j] = comb[i]
    assert [to_int(x) for x in abc] == want
    assert dims == (4, 1, 4, wl.max_num_inputs) and npf == [1] * wl.P and nin == list(wl.num_inputs)


@pytest.mark.parametrize("case", ["p3_ragged_3secs", "shared_p2"])
def test_helper_verifier_accepts_helper_proofs(oracle, case):
    """phase 1 on multiply_vec_block's tables and phase 2 on abc_poly and new_rev(z): the helper's
    ZKSumcheckProof::verify accepts both, returns the provers' challenges and ends in the provers' transcript state"""
    import workload

    wl, z = workload_of(oracle, case)
    v = workload.CViews(wl)
    seed = workload.tape_seed()
    rng = np.random.default_rng(8)
    lx, lq = (wl.max_num_cons - 1).bit_length(), (wl.max_num_proofs - 1).bit_length()
    lp, lw, ly = (wl.P - 1).bit_length(), (wl.nws - 1).bit_length(), (wl.max_num_inputs - 1).bit_length()
    nc = [wl.num_cons[0 if wl.shared else p] for p in range(wl.P)]
    tabs = oracle.r1cs_multiply_vec_block(wl, z, wl.num_inputs)
    eqs = [rand_fq(oracle, rng, 1 << n) for n in (lp, lq, lx)]
    zero = np.zeros(4, np.uint64)
    p1 = ref.phase1(b"p1", seed, lx, lq, lp, *eqs, wl.num_proofs, nc, *tabs)
    assert len(p1["proof"]) == ref.zk_len(lx + lq + lp) and p1["claims"].any()
    ok, post, r, check = ref.verify(b"p1", ref.commit1(zero, zero), lx + lq + lp, p1["proof"])
    assert ok and np.array_equal(r, p1["r"]) and check == p1["check"]
    assert post == p1["proof"][16 + 32 * (lx + lq + lp) + 32 * (lx + lq + lp - 1):][:32]  # the last comm_eval
    # the claims are the bound tables' first entries and the eq factors' product
    assert np.array_equal(p1["claims"][1], p1["B"][0]) and p1["sizes"][0] == (1, 1, 1, 1)
    assert to_int(p1["claims"][0]) == to_int(p1["eq3"][0]) * to_int(p1["eq3"][1]) * to_int(p1["eq3"][2]) % Q

    rx = rand_fq(oracle, rng, wl.max_num_cons)
    rs = rand_fq(oracle, rng, 3)
    abc, (_, _, abc_ni) = ref.abc_poly(v.inst, wl.P, wl.nws, wl.max_num_inputs, wl.num_inputs, rx, *rs)
    claim, blind = rand_fq(oracle, rng, 2)
    rq = rand_fq(oracle, rng, max(lq, 1))[:lq]
    p2 = ref.phase2(b"p2", seed, claim, blind, ly, lw, lp, wl.shared, wl.nws, rand_fq(oracle, rng, 1 << lp), abc_ni,
                    abc, wl.num_proofs, wl.max_num_proofs, wl.num_inputs, z, rq)
    assert len(p2["proof"]) == ref.zk_len(ly + lw + lp) and p2["claims"].any()
    ok, _, r, check = ref.verify(b"p2", ref.commit1(claim, blind), ly + lw + lp, p2["proof"])
    assert ok and np.array_equal(r, p2["r"]) and check == p2["check"]
    assert np.array_equal(p2["claims"][2], p2["Z"][0]) and np.array_equal(p2["claims"][0], p2["eq0"])
    # a wrong claim commitment, a wrong round count and a cut proof are rejected
    assert not ref.verify(b"p2", ref.commit1(claim, zero), ly + lw + lp, p2["proof"])[0]
    assert not ref.verify(b"p2", ref.commit1(claim, blind), ly + lw + lp - 1, p2["proof"])[0]
    assert not ref.verify(b"p2", ref.commit1(claim, blind), ly + lw + lp, p2["proof"][:-1])[0]
    assert not ref.verify(b"p2", ref.commit1(claim, blind), ly + lw + lp, p2["proof"] + b"\0")[0]
