"""Resources of the variable-base MSM's kernels (msm_var.hip), read from the built libspg.so's gfx950 code objects as
tests/test_kernel_resources.py does. CPU only: it reads the build, it runs nothing on a GPU."""
from test_kernel_resources import private_segments

LDS_PER_CU = 160 * 1024  # gfx950
ACCUM_WGS_PER_CU = 4     # k_vmsm_accum's __launch_bounds__(256, 4)


def one(sizes, name):
    hit = {k: v for k, v in sizes.items() if name in k}
    assert len(hit) == 1, (name, sorted(hit))
    return next(iter(hit.values()))


def test_accum_has_no_scratch_and_fits_four_workgroups(tmp_path):
    """the accumulation streams one mixed addition per entry: no private segment, and its LDS (the 256 lane sums)
    leaves room for the 4 workgroups per CU its launch bounds ask for"""
    assert one(private_segments(tmp_path), "k_vmsm_accum") == 0
    lds = one(private_segments(tmp_path, "group_segment_fixed_size"), "k_vmsm_accum")
    assert 0 < lds <= LDS_PER_CU // ACCUM_WGS_PER_CU, lds
    assert one(private_segments(tmp_path, "vgpr_count"), "k_vmsm_accum") <= 512 // ACCUM_WGS_PER_CU


def test_points_load_scratch_no_more_than_decompress(tmp_path):
    """k_points_load is k_decompress without ext_to_niels' inversion: no private segment beyond k_decompress's, read
    from the same code objects"""
    sizes = private_segments(tmp_path)
    assert one(sizes, "k_points_load") <= one(sizes, "k_decompress")


def test_sort_kernels_present(tmp_path):
    sizes = private_segments(tmp_path)
    for k in ("k_vmsm_digits", "k_vmsm_scatter", "k_vmsm_nchunks", "k_vmsm_chunks"):
        one(sizes, k)
