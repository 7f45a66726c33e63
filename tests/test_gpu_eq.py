"""EqPolynomial::evals (src/dense_mlpoly.rs:76-92) on the GPU (spg_eq_evals -> dev_eq_table) vs the oracle's
field arithmetic running the reference's doubling loop, bit-exact. The sizes cover every launch form of the
device table: one partial block (ell <= 8), whole blocks with a high-bit product (9..16), and the factored
hi (x) lo form (> 16). The restatement itself is pinned against
plain Python integers on the CPU."""
import numpy as np
import pytest

Q = 2**252 + 27742317777372353535851937790883648493
R = 2**256


def eq_ref(oracle, r):
    """src/dense_mlpoly.rs:79-90: evals[2k+1] = evals[k] * r_j, evals[2k] = evals[k] - evals[2k+1]"""
    t = oracle.fq_from_u64(1).reshape(1, 4)
    for x in r:
        hi = oracle.fq_op("mul", t, np.repeat(x.reshape(1, 4), t.shape[0], axis=0))
        lo = oracle.fq_op("sub", t, hi)
        t = np.stack([lo, hi], axis=1).reshape(-1, 4)
    return t


ELLS = [0, 1, 2, 3, 4, 7, 8, 9, 11, 12, 13, 16, 17, 20]


def challenges(oracle, ell):
    rng = np.random.default_rng(100 + ell)
    return oracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * ell, dtype=np.uint8).tobytes()) if ell else \
        np.zeros((0, 4), dtype=np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("ell", ELLS)
def test_eq_evals_match_oracle(ctx, oracle, ell):
    import spg

    r = challenges(oracle, ell)
    got = spg.Buf.eq_evals(ctx, r).download()
    assert got.shape == (1 << ell, 4)
    assert np.array_equal(got, eq_ref(oracle, r))


def eq_child_main():
    """prints `ell sha256(table)` per size, then the eq_table launch count of the profile (a fresh process that reads
    SPG_EQ_LDS)"""
    import hashlib

    import pyoracle
    import spg

    ctx = spg.Context(0)
    ctx.prof_enable(True)
    ctx.prof_read(reset=True)
    for ell in ELLS:
        got = spg.Buf.eq_evals(ctx, challenges(pyoracle, ell)).download()
        print(ell, got.shape[0], hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest())
    print("eq_table", ctx.prof_read().get("eq_table", (0,))[0])
    print("ok")


@pytest.mark.gpu
def test_eq_evals_one_lane_per_entry(oracle):
    """SPG_EQ_LDS=0: every size again through k_eq_table<false>, one lane per entry up to ell = 12 and the factored
    form (two of them, then k_eq_combine) above, where the LDS kernel factors only past 16. spg_eq_evals reads the
    switch unconditionally on its way to the launch, so every table here is built by the switched kernels; the
    profile's eq_table count (one scope per table in either form) only confirms that each table was a device launch."""
    import hashlib
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\nimport test_gpu_eq\ntest_gpu_eq.eq_child_main()\n"
            % (os.path.join(root, "spartan-parallel_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPG_EQ_LDS="0"), capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [line.split() for line in out.stdout.split("\n")[:-1]]
    assert lines[-1] == ["ok"] and lines[-2] == ["eq_table", str(len(ELLS))], lines[-2:]
    assert [int(w[0]) for w in lines[:-2]] == ELLS
    for ell, n, h in lines[:-2]:
        want = eq_ref(oracle, challenges(oracle, int(ell)))
        assert int(n) == 1 << int(ell)
        assert h == hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest(), "ell = %s" % ell


@pytest.mark.gpu
def test_eq_evals_edge_challenges(ctx, oracle):
    """r_j in {0, 1, q - 1}: the table has exact zeros, ones and signed ones"""
    import spg

    zero, one = oracle.fq_from_u64(0), oracle.fq_from_u64(1)
    minus_one = oracle.fq_op("neg", one).reshape(4)
    r = np.stack([zero, one, minus_one, one, zero, minus_one, minus_one, one, zero, one])
    got = spg.Buf.eq_evals(ctx, r).download()
    assert np.array_equal(got, eq_ref(oracle, r))


def test_eq_ref_matches_python_integers(oracle):
    """CPU: the oracle-arithmetic restatement equals the reference loop run on Python integers"""
    rng = np.random.default_rng(7)
    r = oracle.fq_from_bytes_wide(rng.integers(0, 256, 64 * 6, dtype=np.uint8).tobytes())
    to_int = lambda m: sum(int(m[i]) << (64 * i) for i in range(4)) * pow(R, -1, Q) % Q
    ri = [to_int(x) for x in r]
    ev = [1] * (1 << len(ri))
    size = 1
    for j in range(len(ri)):
        size *= 2
        for i in range(size - 1, 0, -2):
            s = ev[i // 2]
            ev[i] = s * ri[j] % Q
            ev[i - 1] = (s - ev[i]) % Q
    assert [to_int(x) for x in eq_ref(oracle, r)] == ev


@pytest.mark.gpu
def test_mle_kat_on_device_eq_table(ctx, oracle):
    """src/dense_mlpoly.rs:1234-1252: Z = [1, 2, 1, 4] evaluated at r = [4, 3] through the device chi table is 28"""
    import spg

    def m(x):
        v = x * R % Q
        return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

    chi = spg.Buf.eq_evals(ctx, np.stack([m(4), m(3)])).download()
    Z = np.stack([m(x) for x in (1, 2, 1, 4)])
    acc = np.zeros(4, np.uint64)
    for z, c in zip(Z, chi):
        acc = oracle.fq_op("add", acc, oracle.fq_op("mul", z, c))[0]
    assert np.array_equal(acc, m(28))
