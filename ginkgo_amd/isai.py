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

`GeneralIsai` and `SpdIsai` (preconditioner::GeneralIsai / SpdIsai) take the system matrix itself: nothing is
factorised, every row of W solves one small dense system with partial pivoting
(gkoc_isai_generate_general_inverse_*), so generate is one launch per path.  GeneralIsai applies W (one SpMV),
SpdIsai applies W^T W (two SpMVs over a lower triangular W); see the classes.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import IT, VT, DimensionMismatch, GkoError, NotSupported, call
from .base import LinOp
from .executor import MEM_INDICES, MEM_VALUES
from .matrix import Csr, Dense, DeviceMatrixData, Fbcsr


def row_limits():
    """the pattern-row lengths at which the generate kernel changes path (gkoc_isai_row_limits)"""
    return _lib.row_limits("gkoc_isai_row_limits")


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
    _ENTRY, _FLAG = "gkoc_isai_generate_tri_inverse_", 1    # the generate entry and its is_lower / spd argument
    _LOWER_PATTERN = False      # W lives on the lower triangle of the pattern (SpdIsai)
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
        if self._LOWER_PATTERN:
            rp, ci = _lower_pattern(ex, a.size, rp, ci, a.dtype)
        w = ex.alloc((ci.numel(),), a.dtype, MEM_VALUES)
        call(f"{self._ENTRY}{VT[a.dtype]}_{IT[ci.dtype]}", ex.stream, n, C.c_int(self._FLAG), a.row_ptrs,
             a.col_idxs, a.values, rp, ci, w)
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
    _FLAG = 1

    @staticmethod
    def build():
        return _IsaiFactory(LowerIsai)


class UpperIsai(_Isai):
    """W ~ U^-1 on the pattern of |U|^power for an upper triangular U; apply is one CSR SpMV."""
    _FLAG = 0

    @staticmethod
    def build():
        return _IsaiFactory(UpperIsai)


LowerIsai._OTHER, UpperIsai._OTHER = UpperIsai, LowerIsai


def general_row_limits():
    """the pattern-row lengths at which the general / spd generate kernel changes path; the last one is the
    cap, the longest pattern row it takes (gkoc_isai_general_row_limits)"""
    return _lib.row_limits("gkoc_isai_general_row_limits")


def _lower_pattern(ex, size, rp, ci, dtype):
    """(row_ptrs, col_idxs) of the lower triangle, diagonal included, of the sorted pattern (rp, ci): the index
    arrays of the Sor / Ic set-up (every row must store its diagonal, which then is its last entry)"""
    n, it = size[0], IT[ci.dtype]
    shift, missing = ex.alloc((n + 1,), rp.dtype), C.c_int64(0)
    call("gkoc_csr_missing_diagonal_shift_" + it, ex.stream, n, n, rp, ci, shift, C.byref(missing))
    if missing.value:
        raise GkoError(f"SpdIsai: {missing.value} rows of the system matrix store no diagonal entry")
    l_rp = ex.alloc((n + 1,), rp.dtype, MEM_INDICES)
    call("gkoc_factorization_initialize_row_ptrs_l_u_" + it, ex.stream, n, rp, ci, l_rp, None)
    nnz = int(l_rp[-1].item())
    l_ci = ex.alloc((nnz,), ci.dtype, MEM_INDICES)
    ones, unused = ex.alloc((ci.numel(),), dtype).fill_(1), ex.alloc((nnz,), dtype)
    call(f"gkoc_sor_initialize_weighted_l_{VT[dtype]}_{it}", ex.stream, n, rp, ci, ones, C.c_double(1.0), l_rp,
         l_ci, unused)
    ex.synchronize()                    # `shift`, `ones` and `unused` are released on return
    return l_rp, l_ci


class GeneralIsai(_Isai):
    """W ~ A^-1 on the pattern of |A|^power for any square A: (W A)(i, S_i) = e_i(S_i), one small dense system
    per row, solved by Gauss-Jordan with partial pivoting (gkoc_isai_generate_general_inverse_*, spd = 0; the
    arithmetic is stated in include/gko_cdna4.h).  Nothing is factorised and no row depends on another, so
    generate is one launch (two if the pattern has rows on both sides of 64 entries).  apply is one CSR SpMV.

    With power 1 W shares A's row_ptrs / col_idxs; with power p > 1 the pattern is made as for LowerIsai.
    Unsorted input is sorted on a copy unless with_skip_sorting(True); the caller's matrix is never changed.

    There is no excess system: Ginkgo moves rows longer than 32 entries to an iterative solver; here pattern
    rows up to general_row_limits()[-1] entries are solved exactly and a longer one is refused (NotSupported).
    with_excess_limit, with_excess_solver_factory and with_excess_solver_reduction are accepted without effect."""

    _ENTRY, _FLAG = "gkoc_isai_generate_general_inverse_", 0

    @staticmethod
    def build():
        return _IsaiFactory(GeneralIsai)


GeneralIsai._OTHER = GeneralIsai        # transpose(): a GeneralIsai around Csr.transpose() of the inverse


class SpdIsai(_Isai):
    """W^T W ~ A^-1 for a symmetric positive definite A, W lower triangular on the lower triangle (diagonal
    included) of the pattern of |A|^power: row i of W solves its dense system (both triangles of A are read)
    and is divided by the square root of its diagonal entry (gkoc_isai_generate_general_inverse_*, spd = 1).
    Every row of A must store its diagonal.  The lower pattern comes from the index arrays of the Sor / Ic
    set-up; W^T is made once at generate with Csr.transpose().

    apply is x = W^T (W b), two CSR SpMVs through an intermediate vector that is kept per column count and
    value type (allocated at the first apply with that shape); apply(alpha, b, beta, x) is
    x = alpha W^T (W b) + beta x.  No apply copies to the host or synchronises.

    get_approximate_inverse() returns W; transpose() returns self (the operator is symmetric).  As for
    GeneralIsai there is no excess system: rows up to general_row_limits()[-1] entries are solved exactly,
    longer ones refused, and the three excess setters are accepted without effect."""
    _ENTRY, _FLAG, _LOWER_PATTERN = "gkoc_isai_generate_general_inverse_", 1, True

    @staticmethod
    def build():
        return _IsaiFactory(SpdIsai)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        self.inverse_t = self.inverse.transpose()
        self._between = {}

    def _intermediate(self, b):
        key = (b.size[1], b.dtype)
        t = self._between.get(key)
        if t is None:
            t = self._between[key] = Dense.create(self.exec, (self.size[0], b.size[1]), b.dtype)
        return t

    def transpose(self):
        return self

    conj_transpose = transpose

    def apply_impl(self, b, x):
        t = self._intermediate(b)
        self.inverse.apply_impl(b, t)
        self.inverse_t.apply_impl(t, x)

    def apply_advanced_impl(self, alpha, b, beta, x):
        t = self._intermediate(b)
        self.inverse.apply_impl(b, t)
        self.inverse_t.apply_advanced_impl(alpha, t, beta, x)
