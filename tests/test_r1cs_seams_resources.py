"""The kernels behind the R1CS seams keep no private (scratch) segment: the eval-table kernel in both of its forms
(k_abc<false>: the prover's weighted sum in new_rev order; k_abc<true>: the three tables of spg_r1cs_eval_tables), the
phase-1 evaluation kernels the p-round seam reaches on a caller's table (k_phase1_eval / k_phase1_eval_q, unfused),
the fold that binds the p variable (k_pqx_fold), the one-pass q binds and the new_rev reordering. Reads the built libspg.so's code-object
metadata as tests/test_kernel_resources.py does; CPU only."""
import re

from test_kernel_resources import private_segments


def test_seam_kernels_have_no_scratch(tmp_path):
    sizes = private_segments(tmp_path)
    want = {
        "k_abc<false>": r"k_abcILb0E", "k_abc<true>": r"k_abcILb1E",
        "k_phase1_eval<false>": r"k_phase1_evalILb0E", "k_phase1_eval_q<false>": r"k_phase1_eval_qILb0E",
        "k_pqx_fold": r"k_pqx_fold[^0-9a-z_]", "k_pqx_new_rev": r"k_pqx_new_rev", "k_pqx_bound_q": r"k_pqx_bound_qILi",
        "k_pqx_bound_q_prefix": r"k_pqx_bound_q_prefix",
    }
    for name, pat in want.items():
        hit = {k: v for k, v in sizes.items() if re.search(pat, k)}
        assert hit, (name, sorted(sizes)[:10])
        assert not any(hit.values()), (name, hit)
