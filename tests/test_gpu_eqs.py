"""spg_eqs_check on the device against the oracle: every sum byte for byte against pyoracle.msm over the same terms,
every status against "the oracle's sum is the 32 zero bytes", on the cases of tests/eqs_cases.py -- equation lengths on
both sides of a wavefront and a workgroup, equation counts on both sides of the sum kernel's workgroup, edge scalars,
edge points, the three operand forms, rejected encodings, and the argument errors that launch nothing."""
import numpy as np
import pytest

import eqs_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base(ctx, oracle):
    import spg

    P = spg.Points(ctx, ec.base_points(oracle))
    yield P
    P.free()


@pytest.mark.parametrize("name", ec.NAMES)
def test_sums_and_statuses_equal_oracle(ctx, oracle, base, name):
    import spg

    call = ec.get(oracle, name)
    forms, operands, s, first, comp, ext = call.arrays()
    status, sums, bad = spg.eqs_check(ctx, forms, operands, s, first, comp, ext, base)
    call.check(oracle, status, sums, bad)


def test_statuses_without_sums(ctx, oracle, base):
    """the sums pointer is optional: the same statuses and lowest rejected term without it"""
    import spg

    for name in ("edge_points", "invalid_at_8"):
        call = ec.get(oracle, name)
        forms, operands, s, first, comp, ext = call.arrays()
        status, sums, bad = spg.eqs_check(ctx, forms, operands, s, first, comp, ext, base, sums=False)
        assert sums is None
        call.check(oracle, status, None, bad)


def test_empty_calls(ctx, base):
    import spg

    none = np.zeros((0, 4), np.uint64)
    status, sums, bad = spg.eqs_check(ctx, [], [], none, [0, 0, 0], base=base)
    assert list(status) == [0, 0] and sums.tobytes() == bytes(64) and bad == -1
    status, sums, bad = spg.eqs_check(ctx, [], [], none, [0])
    assert len(status) == 0 and bad == -1


def test_argument_errors_launch_nothing(ctx, oracle, base):
    import spg

    ok, cases = ec.bad_argument_cases(oracle)
    status, _, bad = spg.eqs_check(ctx, base=base, **ok)
    assert len(status) == 2 and bad == -1
    ctx.prof_enable(True)
    ctx.prof_read()
    try:
        for name, kw in cases.items():
            with pytest.raises(spg.SpgError, match="SPG_E_ARG"):
                spg.eqs_check(ctx, base=base, **kw)
        with pytest.raises(spg.SpgError, match="SPG_E_ARG"):  # an index operand without a handle
            spg.eqs_check(ctx, **ok)
        assert "eqs_check" not in ctx.prof_read(), "an argument error reached a launch"
        spg.eqs_check(ctx, base=base, **ok)
        assert ctx.prof_read()["eqs_check"][0] == 1
    finally:
        ctx.prof_enable(False)
