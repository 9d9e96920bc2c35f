"""Triangular incomplete sparse approximate inverses - mirror of include/ginkgo/core/preconditioner/isai.hpp
(preconditioner::LowerIsai / UpperIsai; core/preconditioner/isai.cpp).

`LowerIsai.build().with_skip_sorting(False).with_sparsity_power(1).on(exec).generate(tri)` computes a sparse W
on the pattern of |tri|^power with (W tri)(i, S_i) = e_i(S_i) for every row i, S_i = the columns stored in
row i of the pattern (gkoc_isai_generate_tri_inverse_*: all rows in one launch, no level schedule).
`apply(b, x)` is then x = W b, ONE CSR SpMV, where LowerTrs needs a launch per level.

`tri` must be triangular on the stated side and store every diagonal entry: sorted, the diagonal is the last
entry of a lower row and the first of an upper one, the layouts factorization.Ilu / Ic and Sor produce.
Unsorted input is sorted on a copy (unless with_skip_sorting(True)); the caller's matrix is never changed.

Pattern: with power 1, W shares tri's row_ptrs / col_idxs - no copy, no index array is written.  With power
p > 1 it is the pattern of |tri|^p, made p - 1 times through the triplet pipeline on a matrix of ones
(gkoc_csr_spgemm_count / _expand, gkoc_sort_row_major, gkoc_sum_duplicates_count / _fill,
gkoc_convert_idxs_to_ptrs).  Every diagonal is stored, so the powers are nested and every row keeps its
diagonal at the required end.

The values are bit-identical to the substitution stated in include/gko_cdna4.h.  A row with a non-finite
entry (a zero pivot) becomes the identity's row, as in Ginkgo.

`with_excess_limit`, `with_excess_solver_factory` and `with_excess_solver_reduction` are accepted for API
compatibility and have no effect: Ginkgo moves rows longer than 32 entries into an excess system that an
iterative solver handles; the kernel here has no cap on the row length, so no row is ever moved.
"""
import ctypes as C

import torch

from ._lib import IT, VT, DimensionMismatch, GkoError, NotSupported, call
from .base import LinOp
from .executor import MEM_INDICES, MEM_VALUES
from .matrix import Csr, DeviceMatrixData, Fbcsr


def row_limits():
    """the pattern-row lengths at which the generate kernel changes path (gkoc_isai_row_limits)"""
    limits, count = (C.c_int * 4)(), C.c_int(0)
    call("gkoc_isai_row_limits", limits, C.byref(count))
    return [int(limits[p]) for p in range(count.value)]


class _IsaiFactory:
    def __init__(self, cls):
        self.cls = cls
        self.skip_sorting = False
        self.sparsity_power = 1
        self.excess_limit = 0
        self.excess_solver_factory = None
        self.excess_solver_reduction = 1e-6
        self.exec = None

    def with_skip_sorting(self, v):
        self.skip_sorting = bool(v)
        return self

    def with_sparsity_power(self, v):
        self.sparsity_power = int(v)
        return self

    def with_excess_limit(self, v):
        """accepted for API compatibility: no row is ever moved into an excess system"""
        self.excess_limit = int(v)
        return self

    def with_excess_solver_factory(self, v):
        """accepted for API compatibility: there is no excess system to solve"""
        self.excess_solver_factory = v
        return self

    def with_excess_solver_reduction(self, v):
        """accepted for API compatibility: there is no excess system to solve"""
        self.excess_solver_reduction = float(v)
        return self

    def on(self, exec_):
        self.exec = exec_
        return self

    def generate(self, system_matrix):
        if isinstance(system_matrix, Fbcsr):
            # any other matrix type goes through convert_to(Csr), as for Sor
            csr = system_matrix.convert_to_csr()
            prec = self.cls(self, csr)
            csr.exec.synchronize()      # the converted copy is released on return
            return prec
        return self.cls(self, system_matrix)


def _pattern_power(ex, a, power):
    """(row_ptrs, col_idxs) of the pattern of |a|^power, rows sorted: power - 1 products with a matrix of ones
    through the triplet pipeline.  Nothing cancels (all values are positive) and the pipeline drops no zero."""
    n = a.size[0]
    it, suf = IT[a.col_idxs.dtype], f"{VT[a.dtype]}_{IT[a.col_idxs.dtype]}"
    ones = ex.alloc((a.values.numel(),), a.dtype, MEM_VALUES).fill_(1)
    rp, ci, v = a.row_ptrs, a.col_idxs, ones
    for _ in range(power - 1):
        offsets, total = ex.alloc((n + 1,), torch.int64), C.c_int64(0)
        call("gkoc_csr_spgemm_count_" + it, ex.stream, n, rp, ci, a.row_ptrs, None, offsets, C.byref(total))
        t = max(total.value, 1)
        rows, cols = ex.alloc((t,), ci.dtype), ex.alloc((t,), ci.dtype)
        vals = ex.alloc((t,), a.dtype)
        call("gkoc_csr_spgemm_expand_" + suf, ex.stream, n, None, rp, ci, v, a.row_ptrs, a.col_idxs, ones, None,
             None, None, None, offsets, rows, cols, vals)
        data = DeviceMatrixData(ex, a.size, rows[:total.value], cols[:total.value], vals[:total.value])
        data.sum_duplicates()
        # the values are path counts; only the pattern is kept, so they are set back to 1 (no overflow)
        rp, ci, v = Csr.read(data).row_ptrs, data.col_idxs, data.values.fill_(1)
    # the product's triplets live with the vectors; W's indices go where a matrix' read-only arrays belong
    out_rp, out_ci = ex.alloc((n + 1,), rp.dtype, MEM_INDICES), ex.alloc((ci.numel(),), ci.dtype, MEM_INDICES)
    out_rp.copy_(rp)
    out_ci.copy_(ci)
    ex.synchronize()                    # the intermediate patterns are released on return
    return out_rp, out_ci


class _Isai(LinOp):
    _LOWER = True
    _OTHER = None       # the class of the transpose, set below

    def __init__(self, factory, a):
        name = type(self).__name__
        if not isinstance(a, Csr):
            raise NotSupported(f"{name}.generate needs a Csr system matrix")
        if a.size[0] != a.size[1]:
            raise DimensionMismatch(f"{name} needs a square matrix")
        if a.dtype not in VT:
            raise NotSupported(f"{name}: real value types only")
        if factory.sparsity_power < 1:
            raise GkoError(f"{name}: the sparsity power must be at least 1, got {factory.sparsity_power}")
        super().__init__(factory.exec or a.exec, a.size)
        ex, n = self.exec, a.size[0]
        self.dtype = a.dtype
        self.sparsity_power = factory.sparsity_power
        if not factory.skip_sorting and not a.is_sorted_by_column_index():
            a = Csr(ex, a.size, a.values.clone(), a.col_idxs.clone(), a.row_ptrs,
                    a.strategy).sort_by_column_index()
        if self.sparsity_power == 1:
            rp, ci = a.row_ptrs, a.col_idxs
        else:
            rp, ci = _pattern_power(ex, a, self.sparsity_power)
        w = ex.alloc((ci.numel(),), a.dtype, MEM_VALUES)
        call(f"gkoc_isai_generate_tri_inverse_{VT[a.dtype]}_{IT[ci.dtype]}", ex.stream, n,
             C.c_int(int(self._LOWER)), a.row_ptrs, a.col_idxs, a.values, rp, ci, w)
        self.inverse = Csr(ex, a.size, w, ci, rp)
        ex.synchronize()                # a sorted copy is released on return

    @classmethod
    def _holding(cls, inverse, power):
        """an object of this class around a finished inverse"""
        obj = cls.__new__(cls)
        LinOp.__init__(obj, inverse.exec, inverse.size)
        obj.dtype, obj.sparsity_power, obj.inverse = inverse.dtype, power, inverse
        return obj

    def get_approximate_inverse(self):
        return self.inverse

    def transpose(self):
        """the other class around Csr.transpose() of the inverse (Isai::transpose)"""
        return self._OTHER._holding(self.inverse.transpose(), self.sparsity_power)

    conj_transpose = transpose

    def apply_impl(self, b, x):
        self.inverse.apply_impl(b, x)

    def apply_advanced_impl(self, alpha, b, beta, x):
        self.inverse.apply_advanced_impl(alpha, b, beta, x)


class LowerIsai(_Isai):
    """W ~ L^-1 on the pattern of |L|^power for a lower triangular L; apply is one CSR SpMV."""
    _LOWER = True

    @staticmethod
    def build():
        return _IsaiFactory(LowerIsai)


class UpperIsai(_Isai):
    """W ~ U^-1 on the pattern of |U|^power for an upper triangular U; apply is one CSR SpMV."""
    _LOWER = False

    @staticmethod
    def build():
        return _IsaiFactory(UpperIsai)


LowerIsai._OTHER, UpperIsai._OTHER = UpperIsai, LowerIsai
