"""spg_eqs_check's semantics without a GPU: libspg_hostcheck.so's spgh_eqs_check makes the argument check of the
device entry and evaluates every equation on the host (eqcheck.hpp, hcurve.hpp). Status codes, the lowest rejected
term, the empty equation and every sum equal the oracle's (pyoracle.msm) on the cases of tests/eqs_cases.py, the ones
tests/test_gpu_eqs.py runs through the kernels."""
import ctypes

import numpy as np
import pytest

import eqs_cases as ec


@pytest.fixture(scope="module")
def hc():
    import spg

    lib = spg.hostcheck()
    assert hasattr(lib, "spgh_eqs_check")
    return lib


def host_check(hc, oracle, forms, operands, scalars, first, compressed=None, extended=None, sums=True):
    """(rc, status, sums, lowest rejected term, (term grid, sum grid))"""
    import spg

    comp, ext, f, o, s, fi = spg.eqs_pack(forms, operands, scalars, first, compressed, extended)
    base = np.ascontiguousarray(ec.base_points(oracle))
    E = fi.shape[0] - 1
    status = np.full(max(E, 1), 255, np.uint8)
    out = np.zeros((max(E, 1), 32), np.uint8)
    bad = ctypes.c_long(-2)
    plan = (ctypes.c_uint * 2)()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = hc.spgh_eqs_check(p(base), ctypes.c_size_t(base.shape[0]), p(comp), ctypes.c_size_t(comp.shape[0]), p(ext),
                           ctypes.c_size_t(ext.shape[0]), p(f), p(o), p(s), p(fi), ctypes.c_size_t(E),
                           p(out) if sums else None, p(status), ctypes.byref(bad), plan)
    return rc, status[:E], out[:E] if sums else None, bad.value, (plan[0], plan[1])


@pytest.mark.parametrize("name", ec.NAMES)
def test_host_evaluation_equals_oracle(hc, oracle, name):
    call = ec.get(oracle, name)
    rc, status, sums, bad, plan = host_check(hc, oracle, *call.arrays())
    assert rc == 0
    call.check(oracle, status, sums, bad)
    T = call.first[-1]
    assert plan == ((T + 63) // 64, (call.E + 3) // 4)  # one lane per term, one wavefront per equation


def test_status_codes_and_lowest_rejected_term(hc, oracle):
    """all three codes in one call, the rejected terms in equations 2, 5 and 6 and the lowest of them reported; an
    equation without terms is the identity; without a sums pointer the statuses are the same"""
    call = ec.get(oracle, "invalid_at_4")
    rc, status, _, bad, _ = host_check(hc, oracle, *call.arrays(), sums=False)
    assert rc == 0 and list(status) == [1, 1, 2, 1, 1, 2, 2, 1] and bad == 2 * 9 + 4
    points = ec.get(oracle, "edge_points")
    assert set(points.expected(oracle)[0]) == {0, 1}
    rc, status, sums, bad, _ = host_check(hc, oracle, [], [], np.zeros((0, 4), np.uint64), [0, 0, 0])
    assert rc == 0 and list(status) == [0, 0] and bad == -1 and sums.tobytes() == bytes(64)
    assert ec.get(oracle, "lengths").expected(oracle)[0][0] == 0


def test_argument_check(hc, oracle):
    ok, cases = ec.bad_argument_cases(oracle)
    assert host_check(hc, oracle, **ok)[0] == 0
    for name, kw in cases.items():
        assert host_check(hc, oracle, **kw)[0] == -1, name
