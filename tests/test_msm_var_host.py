"""The variable-base MSM's sort, group sums and host finish without a GPU: libspg_hostcheck.so's spgh_vmsm_emulate runs
the kernels' recode and key function (vmsm.hpp), fills the buckets on the host from the (key, entry) pairs in the
device's group layout and finishes with the device path's host code; every result equals the oracle's orc_msm
byte for byte, for window widths on both sides of the 64-bucket group boundary."""
import ctypes

import numpy as np
import pytest

import fieldref
import vmsm_cases as vc

CS = [4, 7, 8, 11, 14]


@pytest.fixture(scope="module")
def hc():
    import spg

    lib = spg.hostcheck()
    assert hasattr(lib, "spgh_vmsm_emulate") and hasattr(lib, "spgh_vmsm_digits")
    return lib


def emulate(hc, pts, s, c):
    pts = np.ascontiguousarray(pts, dtype=np.uint8).reshape(-1, 32)
    s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(32, np.uint8)
    bad = ctypes.c_long(-1)
    rc = hc.spgh_vmsm_emulate(pts.ctypes.data_as(ctypes.c_void_p), s.ctypes.data_as(ctypes.c_void_p),
                              ctypes.c_size_t(pts.shape[0]), ctypes.c_int(c), out.ctypes.data_as(ctypes.c_void_p),
                              ctypes.byref(bad))
    return rc, out.tobytes(), bad.value


@pytest.mark.parametrize("c", CS)
def test_emulation_sizes(hc, oracle, c):
    for n in [n for n in vc.SIZES if n <= 1000]:
        pts, s = vc.size_case(oracle, n)
        rc, got, _ = emulate(hc, pts, s, c)
        assert rc == 0 and got == vc.ref(oracle, "n%d" % n, pts, s), n
    rc, got, _ = emulate(hc, np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.uint64), c)
    assert rc == 0 and got == bytes(32)


@pytest.mark.parametrize("c", CS)
def test_emulation_edge_scalars(hc, oracle, c):
    for name, (pts, s) in vc.edge_scalar_cases(oracle).items():
        rc, got, _ = emulate(hc, pts, s, c)
        assert rc == 0 and got == vc.ref(oracle, name, pts, s), name
    pts, s = vc.edge_scalar_cases(oracle)["zeros"]
    assert emulate(hc, pts, s, c)[1] == bytes(32)


@pytest.mark.parametrize("c", CS)
def test_emulation_edge_points(hc, oracle, c):
    cases = vc.edge_point_cases(oracle)
    for name, (pts, s) in cases.items():
        rc, got, _ = emulate(hc, pts, s, c)
        assert rc == 0 and got == vc.ref(oracle, name, pts, s), name
    assert vc.ref(oracle, "p_and_minus_p", *cases["p_and_minus_p"]) == bytes(32)


@pytest.mark.parametrize("c", range(4, 15))
def test_recode_digits_resum(hc, c):
    """vmsm_digit's digits re-sum to the scalar, stay in (-NB, NB], and equal fieldref.recode, on the carry patterns"""
    W, NB = 253 // c + 1, 1 << (c - 1)
    vals = fieldref.recode_patterns(c) + fieldref.api_carry_scalars()
    for v in vals:
        m = fieldref.arr_u64([fieldref.to_mont(v)])
        out = (ctypes.c_int * W)()
        assert hc.spgh_vmsm_digits(m.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(c), out) == W
        d = list(out)
        assert sum(x << (c * w) for w, x in enumerate(d)) == v % fieldref.Q, hex(v)
        assert all(-NB < x <= NB for x in d)
        assert d == fieldref.recode(v % fieldref.Q, c)


def test_emulation_invalid_encoding(hc, oracle):
    pts, s = vc.size_case(oracle, 65)
    for idx in ([0], [64], [40, 13]):
        bad = pts.copy()
        for i in idx:
            bad[i, 0] ^= 1  # odd s: not a valid encoding
        rc, _, where = emulate(hc, bad, s, 8)
        assert rc == -4 and where == min(idx)  # SPG_E_POINT, the lowest index
    assert emulate(hc, pts, s, 3)[0] == -1 and emulate(hc, pts, s, 15)[0] == -1
