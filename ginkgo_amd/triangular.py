"""Sparse triangular solvers - mirror of include/ginkgo/core/solver/triangular.hpp
(solver::LowerTrs / UpperTrs; core/solver/{lower,upper}_trs.cpp).

`LowerTrs.build().with_unit_diagonal(False).with_num_rhs(1).on(exec).generate(csr)` analyses the
sparsity pattern once (lower_trs::generate: the level of every row, rows grouped by level) and
`apply(b, x)` runs the level schedule on the device (lower_trs::solve): one launch per level with
more than `wide_threshold` rows, one single-workgroup launch per run of smaller levels.  The result
is the reference's row-by-row loop bit for bit.  The full matrix may be passed: entries on the other
side of the diagonal are ignored.
"""
import ctypes as C

import numpy as np

from ._lib import IT, VT, DimensionMismatch, NotSupported, call, lib
from .base import LinOp
from .matrix import Csr


class _TrsFactory:
    def __init__(self, cls):
        self.cls = cls
        self.unit_diagonal = False
        self.num_rhs = 1
        self.exec = None

    def with_unit_diagonal(self, v):
        self.unit_diagonal = bool(v)
        return self

    def with_num_rhs(self, v):
        """accepted for API compatibility: the schedule does not depend on it"""
        self.num_rhs = int(v)
        return self

    def on(self, exec_):
        self.exec = exec_
        return self

    def generate(self, system_matrix):
        return self.cls(self, system_matrix)


class _Trs(LinOp):
    _GENERATE = _SOLVE = None

    def __init__(self, factory, a):
        self._struct = None
        if not isinstance(a, Csr):
            raise NotSupported(f"{type(self).__name__}.generate needs a Csr system matrix")
        if a.size[0] != a.size[1]:
            raise DimensionMismatch(f"{type(self).__name__} needs a square matrix")
        if a.dtype not in VT:
            raise NotSupported(f"{type(self).__name__}: real value types only")
        super().__init__(factory.exec or a.exec, a.size)
        self.system_matrix = a
        self.unit_diagonal = factory.unit_diagonal
        self.dtype = a.dtype
        self._suf = f"{VT[a.dtype]}_{IT[a.col_idxs.dtype]}"
        handle = C.c_void_p()
        call(self._GENERATE + IT[a.col_idxs.dtype], self.exec.stream, a.size[0], a.row_ptrs, a.col_idxs,
             C.byref(handle))
        self._struct = handle
        n, up, lv, nl, w = C.c_int64(), C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
        call("gkoc_trs_struct_info", handle, C.byref(n), C.byref(up), C.byref(lv), C.byref(nl), C.byref(w))
        self.num_levels, self.num_launches, self.wide_threshold = lv.value, nl.value, w.value

    def __del__(self):
        handle, self._struct = getattr(self, "_struct", None), None
        if handle:
            try:
                lib().gkoc_trs_struct_destroy(handle)
            except Exception:   # interpreter shutdown
                pass

    def get_system_matrix(self):
        return self.system_matrix

    def levels(self):
        """(level_ptrs, level_rows) of the schedule, copied from the device"""
        ptrs = np.zeros(self.num_levels + 1, np.int64)
        rows = np.zeros(self.size[0], np.int64)
        call("gkoc_trs_struct_levels", self._struct, ptrs.ctypes.data_as(C.c_void_p),
             rows.ctypes.data_as(C.c_void_p))
        return ptrs, rows

    def apply_impl(self, b, x):
        a = self.system_matrix
        if b.dtype != self.dtype or x.dtype != self.dtype:
            raise NotSupported(f"{type(self).__name__}: vectors must have the matrix' value type")
        call(self._SOLVE + self._suf, self.exec.stream, self._struct, C.c_int(int(self.unit_diagonal)),
             self.size[0], b.size[1], a.row_ptrs, a.col_idxs, a.values, b.values, b.ld, x.values, x.ld)

    def apply_advanced_impl(self, alpha, b, beta, x):
        # x = beta * x + alpha * solve(b), through a clone like the iterative solvers
        xc = x.clone()
        self.apply_impl(b, xc)
        x.scale(beta)
        x.add_scaled(alpha, xc)


class LowerTrs(_Trs):
    _GENERATE, _SOLVE = "gkoc_lower_trs_generate_", "gkoc_lower_trs_solve_"

    @staticmethod
    def build():
        return _TrsFactory(LowerTrs)


class UpperTrs(_Trs):
    _GENERATE, _SOLVE = "gkoc_upper_trs_generate_", "gkoc_upper_trs_solve_"

    @staticmethod
    def build():
        return _TrsFactory(UpperTrs)
