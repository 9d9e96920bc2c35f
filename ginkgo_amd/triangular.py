"""Sparse triangular solvers - mirror of include/ginkgo/core/solver/triangular.hpp
(solver::LowerTrs / UpperTrs; core/solver/{lower,upper}_trs.cpp).

`LowerTrs.build().with_unit_diagonal(False).with_num_rhs(1).on(exec).generate(csr)` analyses the
sparsity pattern once (lower_trs::generate: the level of every row, rows grouped by level) and
`apply(b, x)` runs the level schedule on the device (lower_trs::solve): one launch per level with
more than `wide_threshold` rows, one single-workgroup launch per run of smaller levels.  The result
is the reference's row-by-row loop bit for bit.  The full matrix may be passed: entries on the other
side of the diagonal are ignored.

`Direct` - mirror of include/ginkgo/core/solver/direct.hpp (experimental::solver::Direct) - solves A x = b
exactly, up to rounding: `Direct.build().with_factorization(f).with_num_rhs(k).on(exec).generate(a)` factorizes
with factorization.Lu (the default) or factorization.Cholesky and applies the two level-scheduled solves, L (unit
diagonal for Lu) then U or L^T.  The vectors it needs are allocated at generate time for `num_rhs` columns, so an
application enqueues kernels only and can be captured.  No pivoting; the matrix is factorized in the order it has -
reorder.ScaledReordered with reorder.NestedDissection puts a fill-reducing ordering around it.
"""
import ctypes as C

import numpy as np

from . import factorization as _factorization
from ._lib import IT, VT, DimensionMismatch, NotSupported, call, lib
from .base import LinOp
from .matrix import Csr, Dense


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


class _DirectFactory:
    def __init__(self):
        self.factorization = None
        self.num_rhs = 1
        self.exec = None

    def with_factorization(self, factory):
        """the factory of factorization.Lu (default) or factorization.Cholesky"""
        self.factorization = factory
        return self

    def with_num_rhs(self, v):
        """the number of right-hand sides the work vectors are allocated for at generate time; an application
        with another number allocates its own on first use"""
        self.num_rhs = int(v)
        return self

    def on(self, exec_):
        self.exec = exec_
        return self

    def generate(self, system_matrix):
        return Direct(self, system_matrix)


class Direct(LinOp):
    """x = U^-1 L^-1 b on the factors of factorization.Lu, x = L^-T L^-1 b on those of factorization.Cholesky.
    `generate` takes a system matrix or a generated Lu / Cholesky object."""

    @staticmethod
    def build():
        return _DirectFactory()

    def __init__(self, factory, a):
        kinds = (_factorization.Lu, _factorization.Cholesky)
        ex = factory.exec or a.exec
        if not isinstance(a, kinds):
            a = (factory.factorization or _factorization.Lu.build()).on(ex).generate(a)
            if not isinstance(a, kinds):
                raise NotSupported(f"Direct: with_factorization gave a {type(a).__name__}; a direct solve needs "
                                   "factorization.Lu or factorization.Cholesky")
        super().__init__(ex, a.size)
        self.factorization, self.dtype = a, a.dtype
        if isinstance(a, _factorization.Lu):
            lower, upper, unit = a.get_l_factor(), a.get_u_factor(), True
        else:
            lt = a.get_lt_factor()
            lower, upper, unit = a.get_l_factor(), a.get_l_factor().transpose() if lt is None else lt, False
        self._lower = LowerTrs.build().with_unit_diagonal(unit).on(ex).generate(lower)
        self._upper = UpperTrs.build().on(ex).generate(upper)
        self._vectors = {}
        self._work(max(1, factory.num_rhs))

    def _work(self, cols):
        """(the vector between the solves, the result of the advanced form) for `cols` right-hand sides"""
        vs = self._vectors.get(cols)
        if vs is None:
            vs = self._vectors[cols] = tuple(Dense.create(self.exec, (self.size[0], cols), self.dtype)
                                             for _ in range(2))
        return vs

    def get_lower_solver(self):
        return self._lower

    def get_upper_solver(self):
        return self._upper

    def get_factorization(self):
        return self.factorization

    def apply_impl(self, b, x):
        if b.dtype != self.dtype or x.dtype != self.dtype:
            raise NotSupported("Direct: vectors must have the matrix' value type")
        tmp = self._work(b.size[1])[0]
        self._lower.apply(b, tmp)
        self._upper.apply(tmp, x)

    def apply_advanced_impl(self, alpha, b, beta, x):
        # x = beta * x + alpha * solve(b)
        solved = self._work(b.size[1])[1]
        self.apply_impl(b, solved)
        x.scale(beta)
        x.add_scaled(alpha, solved)
