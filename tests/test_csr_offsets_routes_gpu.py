"""Every route that must drop the column-offset plan of a CSR matrix drops it (include/gko_cdna4.h, "The
column-offset plan": the CONTRACT), and nothing else does.

While a plan is in use the product never reads col_idxs again, so an entry of the library that writes an index
array and forgets to say so (gkoc::csr_structure_written) makes the next product return GKOC_OK and the product
of the OLD matrix.  The scheme, per route: the 130 x 138 tridiagonal A of two_structures with arena index arrays
and a plan in use (state 1 after two products under GKOC_TUNE_CSR_OFFSETS = 1); the entry is called with one of
A's index arrays as ONE of its output arrays - inputs so small that the output fits the allocation; the state is
-1 DIRECTLY AFTER THE CALL (this is what a missing hook turns red, whatever the route wrote); both arrays are
read back, a valid second structure is restored with gkoc_memcpy_h2d if what they hold is no CSR structure of A's
shape; the next product has the bits of the oracle on what the arrays now hold, through a new plan.
An entry with several output index arrays runs once per array, so that each hook call is seen alone.
tests/test_csr_plan_contract_cpu.py keeps the list of routes honest: ROUTES here is compared with the header.
"""
import ctypes as C
import gc
import re

import numpy as np
import pytest
import torch

import csr_offsets_cases as oc
import csr_struct_refs as cr
from binding_gpu import Dev, by_value, raises_invalid
from csr_offsets_cases import arena_csr, arena_tensor, bits, key, plain, plan_info

pytestmark = pytest.mark.gpu

DT = np.dtype(np.float64)
I32 = np.int32


def _call(name, *args):
    from ginkgo_amd._lib import call
    call(name, *args)


def _size_t_fn(name):
    from ginkgo_amd import _lib
    f = getattr(_lib.lib(), name)
    f.restype = C.c_size_t
    return f


class Base:
    """A with a plan in use, b, and the oracle's product"""

    def __init__(self, ex, oracle):
        self.ex, self.oracle = ex, oracle
        self.m1, self.m2 = oc.two_structures(DT)
        self.shape = self.m1[0]
        self.b = np.random.default_rng(9).uniform(-1, 1, self.shape[1]).astype(DT)
        self.a = arena_csr(ex, *self.m1)
        self.vals = self.m1[3]
        got = plain(ex, self.a, self.b)
        assert np.array_equal(bits(got), bits(oracle.csr_spmv(self.m1[1], self.m1[2], self.vals, self.b)))
        info = plan_info(self.a)
        assert (info["state"], info["products"], info["eligible"]) == (1, 2, 3), info
        ex.synchronize()

    def state(self):
        return plan_info(self.a)["state"]

    def arrays(self):
        self.ex.synchronize()
        return self.a.row_ptrs.cpu().numpy(), self.a.col_idxs.cpu().numpy()

    def upload(self, tensor, host):
        host = np.ascontiguousarray(host)
        _call("gkoc_memcpy_h2d", C.c_void_p(tensor.data_ptr()), host.ctypes.data_as(C.c_void_p),
              C.c_size_t(host.nbytes), self.ex.stream)
        self.ex.synchronize()

    def dropped_then_right(self, what):
        """the plan is gone; then: what the arrays hold (restored to the second structure if it is no CSR
        structure) is multiplied right, through a new plan"""
        assert self.state() == -1, "%s did not drop the plan" % what
        rp, ci = self.arrays()
        if not oc.is_csr(rp, ci, self.shape):
            self.upload(self.a.row_ptrs, self.m2[1])
            self.upload(self.a.col_idxs, self.m2[2])
            assert self.state() == -1
            rp, ci = self.arrays()
            assert np.array_equal(rp, self.m2[1]) and np.array_equal(ci, self.m2[2])
        self.multiplied_right(rp, ci, 2, what)

    def multiplied_right(self, rp, ci, products, what):
        got = plain(self.ex, self.a, self.b)
        assert np.array_equal(bits(got), bits(self.oracle.csr_spmv(rp, ci, self.vals, self.b))), what
        model = oc.plan_model(rp, ci)
        info = plan_info(self.a)
        assert info["state"] == model.state and info["eligible"] == model.eligible, (what, info)
        assert info["products"] == (products if model.state == 1 else 0), (what, info)


@pytest.fixture
def base(gexec, oracle):
    with key(1):
        yield Base(gexec, oracle)
    gc.collect()


# ================================================================ the output-array entries
# The source of every conversion: S, 4 x 4, 7 entries, a full diagonal, sorted rows.
S_RP = np.array([0, 2, 3, 6, 7], I32)
S_CI = np.array([0, 1, 1, 0, 2, 3, 3], I32)
S_V = np.arange(1.0, 8.0)
S_DENSE = np.zeros((4, 4))
for _r in range(4):
    S_DENSE[_r, S_CI[S_RP[_r]:S_RP[_r + 1]]] = S_V[S_RP[_r]:S_RP[_r + 1]]


class Outputs:
    """hands out the output arrays of one call: the parameter `aliased` is one of A's index arrays (the bytes an
    entry may write are checked against the array's size), every other one a scratch buffer of its own"""

    def __init__(self, base, aliased, target):
        self.base, self.aliased, self.keep, self.used = base, aliased, [], False
        self.target = base.a.row_ptrs if target == "rp" else base.a.col_idxs

    def __call__(self, name, n, dtype=I32, init=None):
        nbytes = int(n) * np.dtype(dtype).itemsize
        if name == self.aliased:
            assert nbytes <= self.target.numel() * 4, "the output would not fit A's array"
            if init is not None:      # an in/out parameter: the route's input goes there by a torch copy (no hook)
                raw = torch.from_numpy(np.asarray(init, dtype).view(I32).copy()).to(self.target.device)
                self.target[:raw.numel()].copy_(raw)
                self.base.ex.synchronize()
                assert self.base.state() == 1
            self.used = True
            return C.c_void_p(self.target.data_ptr())
        d = Dev(self.base.ex, np.zeros(max(int(n), 1) + 8, dtype) if init is None else
                np.concatenate((np.asarray(init, dtype), np.zeros(8, dtype))))
        self.keep.append(d)
        return d


def dev(ex, a):
    return Dev(ex, np.ascontiguousarray(a))


def r_sort_row_major(ex, st, o):
    rows, cols = o("row_idxs", 7, init=[2, 0, 1, 2, 0, 3, 2]), o("col_idxs", 7, init=[3, 1, 1, 0, 0, 3, 2])
    need = int(_size_t_fn("gkoc_sort_row_major_workspace_bytes")(C.c_int64(7), C.c_size_t(8), C.c_size_t(4)))
    work = dev(ex, np.zeros(max(need, 1), np.uint8))
    _call("gkoc_sort_row_major_f64_i32", st, 7, rows, cols, dev(ex, S_V), work, C.c_size_t(need))


def _compact(ex, st, count_name, count_args, fill_name, rows, cols, vals, o):
    need = int(_size_t_fn("gkoc_compact_workspace_bytes")(C.c_int64(rows.shape[0])))
    work = dev(ex, np.zeros(max(need, 1), np.uint8))
    kept = C.c_int64(-1)
    _call(count_name, st, rows.shape[0], *count_args, work, C.c_size_t(need), C.byref(kept))
    assert 0 < kept.value < rows.shape[0]
    _call(fill_name, st, rows.shape[0], rows, cols, vals, work, o("out_rows", kept.value), o("out_cols", kept.value),
          dev(ex, np.zeros(kept.value + 8)))


def r_remove_zeros_fill(ex, st, o):
    rows, cols = dev(ex, np.repeat(np.arange(4), np.diff(S_RP)).astype(I32)), dev(ex, S_CI)
    vals = dev(ex, np.array([1.0, 0.0, 3.0, 0.0, 5.0, 6.0, 7.0]))
    _compact(ex, st, "gkoc_remove_zeros_count_f64", (vals,), "gkoc_remove_zeros_fill_f64_i32", rows, cols, vals, o)


def r_sum_duplicates_fill(ex, st, o):
    rows, cols = dev(ex, np.array([0, 0, 1, 1, 2, 2, 2], I32)), dev(ex, np.array([0, 0, 1, 2, 2, 2, 3], I32))
    _compact(ex, st, "gkoc_sum_duplicates_count_i32", (rows, cols), "gkoc_sum_duplicates_fill_f64_i32", rows, cols,
             dev(ex, S_V), o)


def r_dense_to_csr(ex, st, o):
    _call("gkoc_dense_to_csr_f64_i32", st, 4, 4, dev(ex, S_DENSE), 4, dev(ex, S_RP), o("out_cols", 7),
          dev(ex, np.zeros(15)))


def r_cdense_to_csr(ex, st, o):
    _call("gkoc_cdense_to_csr_c128_i32", st, 4, 4, dev(ex, S_DENSE.astype(np.complex128)), 4, dev(ex, S_RP),
          o("out_cols", 7), dev(ex, np.zeros(15, np.complex128)))


def _ell(k):
    """S's first k entries per row, column-major with stride 4, padding (-1, 0)"""
    cols, vals = np.full((k, 4), -1, I32), np.zeros((k, 4))
    for r in range(4):
        for j, p in enumerate(range(S_RP[r], min(S_RP[r + 1], S_RP[r] + k))):
            cols[j, r], vals[j, r] = S_CI[p], S_V[p]
    return cols.reshape(-1), vals.reshape(-1)


def r_ell_to_csr(ex, st, o):
    cols, vals = _ell(3)
    _call("gkoc_ell_to_csr_f64_i32", st, 4, 3, 4, dev(ex, cols), dev(ex, vals), dev(ex, S_RP), o("out_cols", 7),
          dev(ex, np.zeros(15)))


def r_sellp_to_csr(ex, st, o):
    cols, vals = _ell(3)          # one slice of 4 rows and 3 columns has the layout of Ell with stride 4
    _call("gkoc_sellp_to_csr_f64_i32", st, 4, 4, dev(ex, np.array([0, 3], np.uint64)), dev(ex, cols), dev(ex, vals),
          dev(ex, S_RP), o("out_cols", 7), dev(ex, np.zeros(15)))


def r_hybrid_to_csr(ex, st, o):
    cols, vals = _ell(2)
    lens = np.diff(S_RP)
    ell_rp = np.concatenate(([0], np.cumsum(np.minimum(lens, 2)))).astype(I32)
    coo_rp = np.concatenate(([0], np.cumsum(np.maximum(lens - 2, 0)))).astype(I32)
    _call("gkoc_hybrid_to_csr_f64_i32", st, 4, 2, 4, dev(ex, cols), dev(ex, vals), dev(ex, np.array([3, 0], I32)),
          dev(ex, np.array([6.0, 0.0])), dev(ex, ell_rp), dev(ex, coo_rp), o("out_row_ptrs", 5), o("out_cols", 7),
          dev(ex, np.zeros(15)))


def r_csr_permute(ex, st, o):
    _call("gkoc_csr_permute_f64_i32", st, 4, dev(ex, S_RP), dev(ex, S_CI), dev(ex, S_V),
          dev(ex, np.array([2, 0, 3, 1], I32)), 0, None, None, None, 0, o("out_rp", 5), o("out_ci", 7),
          dev(ex, np.zeros(15)))


def r_csr_submatrix(ex, st, o):
    # rows 1 .. 2, columns 0 .. 2: [1] and [0, 2]
    _call("gkoc_csr_submatrix_f64_i32", st, 2, 1, 0, 3, dev(ex, S_RP), dev(ex, S_CI), dev(ex, S_V),
          dev(ex, np.array([0, 1, 3], I32)), o("out_ci", 3), dev(ex, np.zeros(11)))


def r_csr_submatrix_from_index_set(ex, st, o):
    rs, cs = cr.IndexSet([(1, 3)], 4), cr.IndexSet([(0, 3)], 4)
    sets = [dev(ex, x.astype(I32)) for x in (rs.begin, rs.superset, cs.begin, cs.end, cs.superset)]
    _call("gkoc_csr_submatrix_from_index_set_f64_i32", st, rs.num_elems, rs.num_subsets, sets[0], sets[1],
          cs.num_subsets, sets[2], sets[3], sets[4], cs.size, dev(ex, S_RP), dev(ex, S_CI), dev(ex, S_V),
          dev(ex, np.array([0, 1, 3], I32)), o("out_ci", 3), dev(ex, np.zeros(11)))


def r_csr_add_diagonal_fill(ex, st, o):
    # S without its last diagonal entry: one is added
    rp, ci = dev(ex, np.array([0, 2, 3, 6, 6], I32)), dev(ex, S_CI[:6])
    shift, miss = dev(ex, np.zeros(5 + 8, I32)), C.c_int64(-1)
    _call("gkoc_csr_missing_diagonal_shift_i32", st, 4, 4, rp, ci, shift, C.byref(miss))
    assert miss.value == 1
    _call("gkoc_csr_add_diagonal_fill_f64_i32", st, 4, rp, ci, dev(ex, S_V[:6]), shift, o("new_rp", 5),
          o("new_ci", 7), dev(ex, np.zeros(15)))


def r_convert_ptrs_to_idxs(ex, st, o):
    _call("gkoc_convert_ptrs_to_idxs_i32", st, dev(ex, S_RP), 4, o("idxs", 7))


def r_csr_sort_by_column_index(ex, st, o):
    _call("gkoc_csr_sort_by_column_index_f64_i32", st, 4, dev(ex, S_RP), o("col_idxs", 7, init=[1, 0, 1, 3, 0, 2, 3]),
          dev(ex, S_V))


def _split_count(ex, st, o):
    """S as the four rows of a rank that owns the columns 0 .. 1 of 4"""
    col_map = dev(ex, np.zeros(5 + 8, I32))
    l_ptrs, nl_full = o("local_row_ptrs", 5), o("nl_row_ptrs_full", 5)
    cnt = [C.c_int64(-5) for _ in range(4)]
    _call("gkoc_dist_split_count_i32", st, 4, dev(ex, S_RP), dev(ex, S_CI), 0, 2, 4, col_map, l_ptrs, nl_full,
          *[C.byref(c) for c in cnt])
    return col_map, l_ptrs, nl_full, [c.value for c in cnt]


def r_dist_split_count(ex, st, o):
    _split_count(ex, st, o)


def _scratch(base):
    return Outputs(base, None, "rp")


def r_dist_split_fill(ex, st, o):
    col_map, l_ptrs, nl_full, (n_halo, nnz_l, nnz_nl, n_nl_rows) = _split_count(ex, st, _scratch(o.base))
    assert (n_halo, nnz_l, nnz_nl, n_nl_rows) == (2, 4, 3, 2)
    _call("gkoc_dist_split_fill_f64_i32", st, 4, dev(ex, S_RP), dev(ex, S_CI), dev(ex, S_V), 0, 2, 4, col_map, l_ptrs,
          nl_full, o("local_cols", nnz_l), dev(ex, np.zeros(nnz_l + 8)), dev(ex, np.zeros(n_nl_rows + 8, I32)),
          o("nl_ptrs", n_nl_rows + 1), o("nl_cols", nnz_nl), dev(ex, np.zeros(nnz_nl + 8)),
          dev(ex, np.zeros(n_halo + 8, I32)))


def r_dist_boundary_count(ex, st, o):
    nnz = C.c_int64(-1)
    _call("gkoc_dist_boundary_count_i32", st, 2, dev(ex, np.array([0, 3], I32)), dev(ex, S_RP), o("out_ptrs", 3),
          C.byref(nnz))
    assert nnz.value == 3


def r_dist_boundary_fill(ex, st, o):
    col_map = _split_count(ex, st, _scratch(o.base))[0]
    _call("gkoc_dist_boundary_fill_f64_i32", st, 2, dev(ex, np.array([0, 3], I32)), dev(ex, S_RP), dev(ex, S_CI),
          dev(ex, S_V), 0, 2, 32, col_map, dev(ex, np.array([0, 2, 3], I32)), o("out_cols", 3), dev(ex, np.zeros(11)))


def r_fbcsr_convert_to_csr(ex, st, o):
    # two block rows of 2 x 2 blocks, one block each
    _call("gkoc_fbcsr_convert_to_csr_f64_i32", st, 2, 2, dev(ex, np.array([0, 1, 2], I32)),
          dev(ex, np.array([0, 1], I32)), dev(ex, np.arange(1.0, 9.0)), o("csr_row_ptrs", 5), o("csr_col_idxs", 8),
          dev(ex, np.zeros(16)))


def r_aos_to_soa(ex, st, o):
    from ginkgo_amd.matrix import entry_dtype
    e = np.zeros(7, entry_dtype(np.float64, I32))
    e["row"], e["column"], e["value"] = np.repeat(np.arange(4), np.diff(S_RP)), S_CI, S_V
    _call("gkoc_aos_to_soa_f64_i32", st, 7, dev(ex, e.view(np.uint8)), o("row_idxs", 7), o("col_idxs", 7),
          dev(ex, np.zeros(15)))


S_ROWS = np.repeat(np.arange(4), np.diff(S_RP))


def r_convert_idxs_to_ptrs(ex, st, o):
    _call("gkoc_convert_idxs_to_ptrs_i32", st, 7, dev(ex, S_ROWS.astype(I32)), 4, o("ptrs", 5))


def r_convert_idxs_to_ptrs_i64_i32(ex, st, o):
    _call("gkoc_convert_idxs_to_ptrs_i64_i32", st, 7, dev(ex, S_ROWS.astype(np.int64)), 4, o("ptrs", 5))


def r_convert_idxs_to_ptrs_i32_i64(ex, st, o):
    _call("gkoc_convert_idxs_to_ptrs_i32_i64", st, 7, dev(ex, S_ROWS.astype(I32)), 4, o("ptrs", 5, np.int64))


def r_diagonal_convert_to_csr(ex, st, o):
    _call("gkoc_diagonal_convert_to_csr_f64_i32", st, 4, dev(ex, np.arange(1.0, 5.0)), o("row_ptrs", 5), o("cols", 4),
          dev(ex, np.zeros(12)))


def r_sparsity_csr_remove_diagonal(ex, st, o):
    rp, ci, counts = dev(ex, S_RP), dev(ex, S_CI), dev(ex, np.zeros(5 + 8, I32))
    _call("gkoc_sparsity_csr_count_diagonal_i32", st, 4, rp, ci, counts)
    _call("gkoc_prefix_sum_nonnegative_i32", st, counts, 5)
    _call("gkoc_sparsity_csr_remove_diagonal_i32", st, 4, rp, ci, counts, o("adj_ptrs", 5), o("adj_idxs", 3))


def _stencil_ptrs(ex, st, o):
    """the 2-D stencil on a 3 x 3 grid: 9 rows"""
    rp, nnz = o("row_ptrs", 10), C.c_int64(-1)
    _call("gkoc_stencil_row_ptrs_i32", st, C.c_int(2), 3, C.c_int(0), 0, 3, rp, C.byref(nnz))
    assert 9 <= nnz.value <= 81
    return rp, nnz.value


def r_stencil_row_ptrs(ex, st, o):
    _stencil_ptrs(ex, st, o)


def r_stencil_fill(ex, st, o):
    rp, nnz = _stencil_ptrs(ex, st, _scratch(o.base))
    _call("gkoc_stencil_fill_f64_i32", st, C.c_int(2), 3, C.c_int(0), 0, 3, rp, o("cols", nnz),
          dev(ex, np.zeros(nnz + 8)))


def r_csr_transpose(ex, st, o):
    need = int(_size_t_fn("gkoc_csr_transpose_workspace_bytes")(C.c_int64(7), C.c_int64(4), C.c_size_t(4)))
    work = dev(ex, np.zeros(max(need, 1), np.uint8))
    _call("gkoc_csr_transpose_f64_i32", st, 4, 4, dev(ex, S_RP), dev(ex, S_CI), dev(ex, S_V), 7, o("t_row_ptrs", 5),
          o("t_col_idxs", 7), dev(ex, np.zeros(15)), work, C.c_size_t(need))


def _l_u_ptrs(ex, st, o):
    l_rp, u_rp = o("l_row_ptrs", 5), o("u_row_ptrs", 5)
    _call("gkoc_factorization_initialize_row_ptrs_l_u_i32", st, 4, dev(ex, S_RP), dev(ex, S_CI), l_rp, u_rp)
    return l_rp, u_rp


def r_factorization_initialize_row_ptrs_l_u(ex, st, o):
    _l_u_ptrs(ex, st, o)


# S: L holds (0,0) (1,1) (2,0) (2,2) (3,3) = 5 entries, U holds (0,0) (0,1) (1,1) (2,2) (2,3) (3,3) = 6
def r_sor_initialize_weighted_l(ex, st, o):
    l_rp, _ = _l_u_ptrs(ex, st, _scratch(o.base))
    _call("gkoc_sor_initialize_weighted_l_f64_i32", st, 4, dev(ex, S_RP), dev(ex, S_CI), dev(ex, S_V), C.c_double(1.2),
          l_rp, o("l_ci", 5), dev(ex, np.zeros(13)))


def r_sor_initialize_weighted_l_u(ex, st, o):
    l_rp, u_rp = _l_u_ptrs(ex, st, _scratch(o.base))
    _call("gkoc_sor_initialize_weighted_l_u_f64_i32", st, 4, dev(ex, S_RP), dev(ex, S_CI), dev(ex, S_V),
          C.c_double(1.2), l_rp, o("l_ci", 5), dev(ex, np.zeros(13)), u_rp, o("u_ci", 6), dev(ex, np.zeros(14)))


# entry (name stem of the header's contract) -> (function, ((output parameter, which of A's arrays it aliases), ...))
ROUTES = {
    "gkoc_sort_row_major": (r_sort_row_major, (("row_idxs", "rp"), ("col_idxs", "ci"))),
    "gkoc_remove_zeros_fill": (r_remove_zeros_fill, (("out_rows", "rp"), ("out_cols", "ci"))),
    "gkoc_sum_duplicates_fill": (r_sum_duplicates_fill, (("out_rows", "rp"), ("out_cols", "ci"))),
    "gkoc_dense_to_csr": (r_dense_to_csr, (("out_cols", "ci"),)),
    "gkoc_cdense_to_csr": (r_cdense_to_csr, (("out_cols", "ci"),)),
    "gkoc_ell_to_csr": (r_ell_to_csr, (("out_cols", "ci"),)),
    "gkoc_sellp_to_csr": (r_sellp_to_csr, (("out_cols", "ci"),)),
    "gkoc_hybrid_to_csr": (r_hybrid_to_csr, (("out_row_ptrs", "rp"), ("out_cols", "ci"))),
    "gkoc_csr_permute": (r_csr_permute, (("out_rp", "rp"), ("out_ci", "ci"))),
    "gkoc_csr_submatrix": (r_csr_submatrix, (("out_ci", "ci"),)),
    "gkoc_csr_submatrix_from_index_set": (r_csr_submatrix_from_index_set, (("out_ci", "ci"),)),
    "gkoc_csr_add_diagonal_fill": (r_csr_add_diagonal_fill, (("new_rp", "rp"), ("new_ci", "ci"))),
    "gkoc_convert_ptrs_to_idxs": (r_convert_ptrs_to_idxs, (("idxs", "ci"),)),
    "gkoc_csr_sort_by_column_index": (r_csr_sort_by_column_index, (("col_idxs", "ci"),)),
    "gkoc_dist_split_count": (r_dist_split_count, (("local_row_ptrs", "rp"), ("nl_row_ptrs_full", "rp"))),
    "gkoc_dist_split_fill": (r_dist_split_fill, (("local_cols", "ci"), ("nl_ptrs", "rp"), ("nl_cols", "ci"))),
    "gkoc_dist_boundary_count": (r_dist_boundary_count, (("out_ptrs", "rp"),)),
    "gkoc_dist_boundary_fill": (r_dist_boundary_fill, (("out_cols", "ci"),)),
    "gkoc_fbcsr_convert_to_csr": (r_fbcsr_convert_to_csr, (("csr_row_ptrs", "rp"), ("csr_col_idxs", "ci"))),
    "gkoc_aos_to_soa": (r_aos_to_soa, (("row_idxs", "rp"), ("col_idxs", "ci"))),
    "gkoc_convert_idxs_to_ptrs": (r_convert_idxs_to_ptrs, (("ptrs", "rp"),)),
    "gkoc_convert_idxs_to_ptrs_i64_i32": (r_convert_idxs_to_ptrs_i64_i32, (("ptrs", "rp"),)),
    "gkoc_convert_idxs_to_ptrs_i32_i64": (r_convert_idxs_to_ptrs_i32_i64, (("ptrs", "rp"),)),
    "gkoc_diagonal_convert_to_csr": (r_diagonal_convert_to_csr, (("row_ptrs", "rp"), ("cols", "ci"))),
    "gkoc_sparsity_csr_remove_diagonal": (r_sparsity_csr_remove_diagonal, (("adj_ptrs", "rp"), ("adj_idxs", "ci"))),
    "gkoc_stencil_row_ptrs": (r_stencil_row_ptrs, (("row_ptrs", "rp"),)),
    "gkoc_stencil_fill": (r_stencil_fill, (("cols", "ci"),)),
    "gkoc_csr_transpose": (r_csr_transpose, (("t_row_ptrs", "rp"), ("t_col_idxs", "ci"))),
    "gkoc_factorization_initialize_row_ptrs_l_u": (r_factorization_initialize_row_ptrs_l_u,
                                                   (("l_row_ptrs", "rp"), ("u_row_ptrs", "rp"))),
    "gkoc_sor_initialize_weighted_l": (r_sor_initialize_weighted_l, (("l_ci", "ci"),)),
    "gkoc_sor_initialize_weighted_l_u": (r_sor_initialize_weighted_l_u, (("l_ci", "ci"), ("u_ci", "ci"))),
}
# the routes of the other sections of this file
RANGE_ENTRIES = ("gkoc_memcpy_h2d", "gkoc_memcpy_d2d", "gkoc_memset", "gkoc_fill_array", "gkoc_fill_seq_array",
                 "gkoc_prefix_sum_nonnegative", "gkoc_prefix_sum_nonnegative_checked")
OTHER = ("gkoc_free", "gkoc_csr_structure_changed")      # tests/test_csr_offsets_gpu.py::test_invalidation

OUTPUT_CASES = [(name, param) for name, (_, outs) in ROUTES.items() for param, _ in outs]


def test_routes_are_the_headers():
    """every entry the header's contract names has a case in this file (or in test_invalidation), and the
    reverse; the parameters are the non-const index pointers the entry announces"""
    import test_csr_plan_contract_cpu as contract
    here = {re.sub(r"_i(32|64)_i(32|64)$", "", name) for name in ROUTES} | set(RANGE_ENTRIES) | set(OTHER)
    named = set().union(*contract.header_names())
    hooked = {s for s, e in contract.scan().items() if e["some_hooked"]}
    assert here == hooked, (sorted(here - hooked), sorted(hooked - here))
    assert here - {"gkoc_csr_structure_changed"} <= named      # (the notification itself: its own sentence)
    told = {}
    for path in sorted(contract.CSRC.glob("*.hip")):
        for name, stem, params, body in contract.definitions(path):
            if contract.HOOK in body:
                told.setdefault(stem, set()).update(
                    set(re.findall(contract.HOOK + r"\(\s*(\w+)", body)) & set(contract.index_outputs(params)))
    for name, (_, outs) in ROUTES.items():
        stem = re.sub(r"_i(32|64)_i(32|64)$", "", name)
        assert {p for p, _ in outs} == told[stem], (name, told[stem])


@pytest.mark.parametrize("name,param", OUTPUT_CASES, ids=["%s-%s" % (n[5:], p) for n, p in OUTPUT_CASES])
def test_output_array_drops_the_plan(base, name, param):
    fn, outs = ROUTES[name]
    o = Outputs(base, param, dict(outs)[param])
    fn(base.ex, base.ex.stream, o)
    assert o.used, "the route never asked for " + param
    base.dropped_then_right("%s(%s)" % (name, param))


# ================================================================ the range routes
def _range_call(base, entry, ptr, nbytes):
    """one call of a range entry that writes exactly [ptr, ptr + nbytes) (nbytes a multiple of 4)"""
    ex, st, n = base.ex, base.ex.stream, nbytes // 4
    if entry == "memcpy_h2d":
        src = np.arange(n, dtype=I32)
        _call("gkoc_memcpy_h2d", C.c_void_p(ptr), src.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), st)
        ex.synchronize()
    elif entry == "memcpy_d2d":
        src = dev(ex, np.arange(n, dtype=I32))
        _call("gkoc_memcpy_d2d", C.c_void_p(ptr), src, C.c_size_t(nbytes), st)
        ex.synchronize()
    elif entry == "memset":
        _call("gkoc_memset", C.c_void_p(ptr), C.c_int(0), C.c_size_t(nbytes), st)
    elif entry == "fill_array_i32":
        _call("gkoc_fill_array_i32", st, C.c_void_p(ptr), n, by_value(np.int32(1)))
    elif entry == "fill_array_small":
        _call("gkoc_fill_array_small", st, C.c_void_p(ptr), nbytes // 2, 2, C.c_uint32(1))
    elif entry == "fill_seq_array_i32":
        _call("gkoc_fill_seq_array_i32", st, C.c_void_p(ptr), n)
    elif entry == "prefix_sum_nonnegative_i32":
        _call("gkoc_prefix_sum_nonnegative_i32", st, C.c_void_p(ptr), n)
    else:
        assert entry == "prefix_sum_nonnegative_checked_i32"
        _call("gkoc_prefix_sum_nonnegative_checked_i32", st, C.c_void_p(ptr), n)
    ex.synchronize()


RANGE_CALLS = ("memcpy_h2d", "memcpy_d2d", "memset", "fill_array_i32", "fill_array_small", "fill_seq_array_i32",
               "prefix_sum_nonnegative_i32", "prefix_sum_nonnegative_checked_i32")
# where in A: (array, first byte (negative: from the end), bytes (None: all))
PLACES = {"all of row_ptrs": ("rp", 0, None), "all of col_idxs": ("ci", 0, None), "first 4 bytes": ("rp", 0, 4),
          "last 4 bytes": ("ci", -4, 4), "4 bytes inside row_ptrs": ("rp", 200, 4),
          "4 bytes inside col_idxs": ("ci", 600, 4)}


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("entry", RANGE_CALLS)
def test_range_write_drops_the_plan(base, entry, place):
    """every range entry, over a whole index array and over one word at its start, its end and inside it"""
    which, first, nbytes = PLACES[place]
    t = base.a.row_ptrs if which == "rp" else base.a.col_idxs
    total = t.numel() * 4
    first = total + first if first < 0 else first
    nbytes = total if nbytes is None else nbytes
    assert 0 <= first and first + nbytes <= total
    _range_call(base, entry, t.data_ptr() + first, nbytes)
    base.dropped_then_right("%s, %s" % (entry, place))


@pytest.mark.parametrize("nbytes", [16, 512])
def test_memcpy_d2d_both_paths(base, nbytes):
    """16 bytes go through the library's own small_copy_kernel, 512 through the runtime's copy; the copy arrives"""
    src = dev(base.ex, np.arange(100, 100 + nbytes // 4, dtype=I32))
    _call("gkoc_memcpy_d2d", C.c_void_p(base.a.col_idxs.data_ptr() + 64), src, C.c_size_t(nbytes), base.ex.stream)
    assert base.state() == -1
    _, ci = base.arrays()
    assert np.array_equal(ci[16:16 + nbytes // 4], np.arange(100, 100 + nbytes // 4))
    base.dropped_then_right("memcpy_d2d of %d bytes" % nbytes)


# ================================================================ negative controls
@pytest.mark.parametrize("entry", RANGE_CALLS)
def test_a_write_elsewhere_keeps_the_plan(base, oracle, entry):
    """the same range entries over ALL of, and exactly, A's value array, b's device copy and both index arrays of a
    second arena matrix B allocated right after A: the plan stays, and the next product goes through it.  (What
    the call wrote is put back by a torch copy, which no hook sees.)"""
    import ginkgo_amd as g
    ex = base.ex
    bm = oc.two_structures(DT)[1]
    bmat = arena_csr(ex, *bm)
    db = g.Dense.from_numpy(ex, base.b.reshape(-1, 1))
    done = 2
    targets = (("A's values", base.a.values, base.vals), ("b", db.values, base.b.reshape(db.values.shape)),
               ("B's row_ptrs", bmat.row_ptrs, bm[1]), ("B's col_idxs", bmat.col_idxs, bm[2]))
    for what, t, host in targets:
        nbytes = t.numel() * t.element_size()
        if entry.startswith("prefix_sum"):
            t.zero_()         # (a prefix sum wants non-negative integers it can add up, not the bits of doubles)
        _range_call(base, entry, t.data_ptr(), nbytes)
        assert base.state() == 1, (entry, what)
        t.copy_(torch.from_numpy(np.ascontiguousarray(host)))
        ex.synchronize()
        base.multiplied_right(base.m1[1], base.m1[2], done + 2, (entry, what))
        done += 2


def test_another_matrix_keeps_the_plan(base, oracle):
    """B multiplied (a plan of its own), B freed, and calls of zero bytes / zero entries aimed at A's arrays
    (they return before the hook and write nothing)"""
    ex, st = base.ex, base.ex.stream
    bm = oc.two_structures(DT)[1]
    bmat = arena_csr(ex, *bm)
    got = plain(ex, bmat, base.b)
    assert np.array_equal(bits(got), bits(oracle.csr_spmv(bm[1], bm[2], bm[3], base.b)))
    assert plan_info(bmat)["state"] == 1 and base.state() == 1
    base.multiplied_right(base.m1[1], base.m1[2], 4, "B multiplied")
    old = (bmat.row_ptrs.data_ptr(), bmat.col_idxs.data_ptr())
    del bmat
    gc.collect()
    assert oc.plan_info_at(*old)["state"] == -1 and base.state() == 1
    base.multiplied_right(base.m1[1], base.m1[2], 6, "B freed")
    src = np.zeros(4, I32)
    for t in (base.a.row_ptrs, base.a.col_idxs):
        p = C.c_void_p(t.data_ptr())
        _call("gkoc_memcpy_h2d", p, src.ctypes.data_as(C.c_void_p), C.c_size_t(0), st)
        _call("gkoc_memcpy_d2d", p, C.c_void_p(base.a.values.data_ptr()), C.c_size_t(0), st)
        _call("gkoc_memset", p, C.c_int(0), C.c_size_t(0), st)
        _call("gkoc_fill_array_i32", st, p, 0, by_value(np.int32(7)))
        _call("gkoc_fill_array_small", st, p, 0, 4, C.c_uint32(7))
        _call("gkoc_fill_seq_array_i32", st, p, 0)
        _call("gkoc_prefix_sum_nonnegative_i32", st, p, 0)
        _call("gkoc_prefix_sum_nonnegative_checked_i32", st, p, 0)
    ex.synchronize()
    assert base.state() == 1
    rp, ci = base.arrays()
    assert np.array_equal(rp, base.m1[1]) and np.array_equal(ci, base.m1[2])
    base.multiplied_right(rp, ci, 8, "empty calls")


# ================================================================ refused calls
def test_refused_calls(base):
    """a call that the entry refuses before any launch.  What each does to the plan is pinned here (the hook of
    most entries stands in front of the argument checks, so the refusal drops the plan; gkoc_fill_array_small checks
    first); the arrays are untouched and the product afterwards is right either way."""
    ex, st = base.ex, base.ex.stream
    rp_ptr = C.c_void_p(base.a.row_ptrs.data_ptr())
    # a negative dimension
    assert raises_invalid("gkoc_convert_idxs_to_ptrs_i32", st, -1, dev(ex, S_ROWS.astype(I32)), 4, rp_ptr)
    assert base.state() == -1
    rp, ci = base.arrays()
    assert np.array_equal(rp, base.m1[1]) and np.array_equal(ci, base.m1[2])
    base.multiplied_right(rp, ci, 2, "negative dimension")
    # a null pointer
    cols, vals = _ell(2)
    assert raises_invalid("gkoc_hybrid_to_csr_f64_i32", st, 4, 2, 4, dev(ex, cols), dev(ex, vals), dev(ex, S_CI),
                          dev(ex, S_V), None, None, rp_ptr, dev(ex, np.zeros(16, I32)), dev(ex, np.zeros(16)))
    assert base.state() == -1
    base.multiplied_right(rp, ci, 2, "null pointer")
    # an element size that does not exist: refused in front of the hook
    assert raises_invalid("gkoc_fill_array_small", st, rp_ptr, 4, 3, C.c_uint32(1))
    assert base.state() == 1
    rp2, ci2 = base.arrays()
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    base.multiplied_right(rp, ci, 4, "bad element size")
