"""Ledger of the C ABI's entry points that no Python code of this repository reaches.

A symbol of include/gko_cdna4.h is *reached* if its name, or its stem before the type suffixes, occurs in
tests/*.py or ginkgo_amd/*.py (the package and the tests build most names as "stem_" + type).  The ones
that are not reached are called only by the C++ binding (ginkgo_amd/gko_binding/) and run only under
Ginkgo's own suites, which need the Ginkgo source tree.  They are listed, by group, in
tests/abi_not_reached.txt; this test fails in both directions, so a new entry point cannot arrive untested
without an explicit line there, and a line whose symbol has since got a test has to be deleted."""
import glob
import os
import re

from test_abi import ROOT, declared_symbols

LEDGER = os.path.join(ROOT, "tests", "abi_not_reached.txt")
_SUFFIX = re.compile(r"(_(f64|f32|c128|c64|i32|i64|u64))+$")
# families this repository tests directly (tests/test_idr_gpu.py, test_cb_gmres_gpu.py, test_dense_gpu.py,
# test_csr_struct_gpu.py, test_csr_diag_gpu.py, test_dist_partition_gpu.py, test_dist_index_gpu.py,
# test_cdense_gpu.py, test_format_helpers_gpu.py, test_array_components_gpu.py, test_gmres_kernels_gpu.py,
# test_mixed_triples_gpu.py, test_krylov_steps_gpu.py, test_jacobi_kernels_gpu.py, test_format_spmv_gpu.py,
# test_format_setup_gpu.py)
MUST_BE_REACHED = ("idr", "cb_gmres", "dense_simple_apply", "dense_apply", "dense_convert", "compute_norm1",
                   "compute_mean", "reduce_add_array", "prefix_sum", "csr_spgemm_reuse", "csr_spgeam_numeric",
                   "in_index_set", "from_index_set", "csr_build_lookup", "csr_row_wise_absolute_sum",
                   "ccsr_row_scan", "gkoc_diagonal_", "gkoc_sparsity_csr_", "gkoc_partition_", "gkoc_index_map_",
                   "gkoc_dist_separate_", "gkoc_dist_vector_build_local", "gkoc_assembly_count_non_owning",
                   "gkoc_assembly_fill_send_buffers", "gkoc_cdense_", "gkoc_ccsr_scale_by_diagonal", "gkoc_ccoo_spmv2",
                   "gkoc_cjacobi_", "gkoc_ell_copy", "gkoc_ell_extract_diagonal", "gkoc_sellp_extract_diagonal",
                   "gkoc_dense_absolute", "gkoc_dense_fill_in_matrix_data", "gkoc_dense_add_scaled_identity_real",
                   "gkoc_jacobi_initialize_precisions", "gkoc_fill_array", "gkoc_convert_precision", "gkoc_conj_array",
                   "gkoc_narrow_i64_to_i32", "gkoc_x_residual_norm_then_cg_step_1", "gkoc_gmres_", "gkoc_common_gmres_",
                   "gkoc_x_gmres_", "gkoc_csr_spmv_mixed", "gkoc_ell_spmv_mixed", "gkoc_dense_row_gather_mixed",
                   "gkoc_bicgstab_", "gkoc_cgs_", "gkoc_fcg_", "gkoc_pipe_cg_", "gkoc_bicg_", "gkoc_gcr_", "gkoc_minres_",
                   "gkoc_chebyshev_", "gkoc_x_pipe_cg_step_", "gkoc_jacobi_find_blocks", "gkoc_jacobi_generate",
                   "gkoc_jacobi_simple_apply", "gkoc_jacobi_apply", "gkoc_jacobi_transpose", "gkoc_jacobi_convert_storage",
                   "gkoc_x_jacobi_", "gkoc_x_cg_step_2_jacobi_apply", "gkoc_x_pipe_cg_steps_jacobi",
                   "gkoc_ell_spmv", "gkoc_ell_advanced_spmv", "gkoc_sellp_spmv", "gkoc_sellp_advanced_spmv",
                   "gkoc_compute_max_row_nnz", "gkoc_sellp_compute_slice_sets", "gkoc_convert_ptrs_to_sizes",
                   "gkoc_convert_idxs_to_ptrs", "gkoc_fill_seq_array", "gkoc_aos_to_soa", "gkoc_csr_convert_to_ell",
                   "gkoc_csr_convert_to_sellp")


def stem(name):
    return _SUFFIX.sub("", name)


def python_sources():
    text = []
    for pattern in ("tests/*.py", "ginkgo_amd/*.py"):
        for path in sorted(glob.glob(os.path.join(ROOT, pattern))):
            if os.path.samefile(path, __file__):
                continue            # the names this file spells out below reach nothing
            text.append(open(path, errors="replace").read())
    return "\n".join(text)


def not_reached():
    text = python_sources()
    return sorted(s for s in declared_symbols() if s not in text and stem(s) not in text)


def ledger():
    names = []
    group_has_comment = False
    for line in open(LEDGER):
        line = line.strip()
        if not line:
            group_has_comment = False
        elif line.startswith("#"):
            group_has_comment = True
        else:
            assert group_has_comment, f"{line}: every group of abi_not_reached.txt starts with a comment line"
            names.append(line)
    return names


def test_suffix_stems():
    assert stem("gkoc_csr_spmv_f64_i32") == "gkoc_csr_spmv" and stem("gkoc_idr_step_1_c128") == "gkoc_idr_step_1"
    assert stem("gkoc_dense_convert_f64_f32") == "gkoc_dense_convert" and stem("gkoc_malloc") == "gkoc_malloc"


def test_ledger_matches_what_python_does_not_reach():
    listed = ledger()
    assert len(listed) == len(set(listed)), "duplicate lines in abi_not_reached.txt"
    missing = sorted(set(not_reached()) - set(listed))
    stale = sorted(set(listed) - set(not_reached()))
    assert not missing, f"entry points no Python test or class reaches, and not in the ledger: {missing}"
    assert not stale, f"ledger lines whose symbol is reached (or gone) - delete them: {stale}"


def test_directly_tested_families_are_not_in_the_ledger():
    for name in ledger():
        assert not any(f in name for f in MUST_BE_REACHED), name
