"""Resources of the short-sum kernels (eqcheck.hip), read from the built libspg.so's gfx950 code objects as
tests/test_kernel_resources.py does. CPU only: it reads the build, it runs nothing on a GPU."""
from test_kernel_resources import private_segments
from test_msm_var_resources import LDS_PER_CU, one

VGPRS_PER_SIMD = 512     # per lane, gfx950
TERM_WAVES_PER_SIMD = 2  # k_eqs_term's __launch_bounds__(64, 2)


def test_kernels_present(tmp_path):
    sizes = private_segments(tmp_path)
    for k in ("k_eqs_term", "k_eqs_sum"):
        one(sizes, k)


def test_term_kernel_has_no_scratch_and_fits_its_launch_bounds(tmp_path):
    """the double-and-add loop keeps its accumulator, the operand's cached form and the product temporaries in
    registers: no private segment, and within the registers of the two wavefronts per SIMD its launch bounds ask for;
    it stages nothing in LDS"""
    assert one(private_segments(tmp_path), "k_eqs_term") == 0
    vgpr = one(private_segments(tmp_path, "vgpr_count"), "k_eqs_term")
    assert 0 < vgpr <= VGPRS_PER_SIMD // TERM_WAVES_PER_SIMD, vgpr
    lds = one(private_segments(tmp_path, "group_segment_fixed_size"), "k_eqs_term")
    assert lds <= LDS_PER_CU // (4 * TERM_WAVES_PER_SIMD), lds


def test_sum_kernel_has_no_scratch(tmp_path):
    """the shuffle tree reduces in registers: no private segment, no LDS tree"""
    assert one(private_segments(tmp_path), "k_eqs_sum") == 0
    assert one(private_segments(tmp_path, "group_segment_fixed_size"), "k_eqs_sum") == 0
