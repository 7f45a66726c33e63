"""Resources of the satisfiability kernel (satcheck.hip), read from the built libspg.so's gfx950 code objects as
tests/test_eqs_resources.py does. CPU only: it reads the build, it runs nothing on a GPU."""
from test_kernel_resources import HOT, private_segments
from test_msm_var_resources import one


def test_kernel_present_and_outside_the_hot_list(tmp_path):
    one(private_segments(tmp_path), "k_sat_check")
    assert not any(h in "k_sat_check" for h in HOT)


def test_sat_kernel_has_no_scratch_and_next_to_no_lds(tmp_path):
    """a lane holds three scalars and a product in registers; the wavefront reduces by ballot and shuffles, so there is
    no private segment and at most a block reduce's worth of LDS (a few hundred bytes; the shuffle form uses none)"""
    assert one(private_segments(tmp_path), "k_sat_check") == 0
    assert one(private_segments(tmp_path, "group_segment_fixed_size"), "k_sat_check") <= 512
