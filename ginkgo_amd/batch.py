"""Batched solvers: the mirror of Ginkgo's gko::batch namespace (include/ginkgo/core/base/batch_multi_vector.hpp,
matrix/batch_csr.hpp, matrix/batch_ell.hpp, solver/batch_cg.hpp, solver/batch_bicgstab.hpp,
preconditioner/batch_jacobi.hpp, log/batch_logger.hpp).

Many small independent systems that share ONE sparsity pattern; every item has its own values, right-hand side
and solution.  A solve is ONE library call - one kernel, one workgroup per item, the working set in LDS as far as
it fits (csrc/batch.hip; the arithmetic is fixed bit for bit in include/gko_cdna4.h, "Batched solvers").  Values
are float64 or float32, indices int32, one right-hand side per item in the solvers.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import matrix as _matrix
from ._lib import DimensionMismatch, GkoError, NotSupported, VT, call
from .executor import MEM_INDICES, MEM_VALUES, MEM_VECTOR

__all__ = ["MultiVector", "Csr", "Ell", "Cg", "Bicgstab", "Jacobi", "plan", "Plan"]

_SOLVER = {"cg": 0, "bicgstab": 1}          # GKOC_BATCH_CG / _BICGSTAB
_FORMAT = {"csr": 0, "ell": 1}              # GKOC_BATCH_CSR / _ELL
_TOLERANCE = {"absolute": 0, "relative": 1}  # GKOC_BATCH_ABSOLUTE / _RELATIVE
_SOLVE = {("cg", "csr"): "gkoc_batch_cg_csr_", ("cg", "ell"): "gkoc_batch_cg_ell_",
          ("bicgstab", "csr"): "gkoc_batch_bicgstab_csr_", ("bicgstab", "ell"): "gkoc_batch_bicgstab_ell_"}


class _PlanInfo(C.Structure):
    """gkoc_batch_plan_info"""
    _fields_ = [("w", C.c_int32), ("resident_vectors", C.c_int32), ("total_vectors", C.c_int32),
                ("values_cached", C.c_int32), ("lds_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


Plan = namedtuple("Plan", "w resident_vectors total_vectors values_cached lds_bytes workspace_bytes")


def _value_bytes(dtype):
    name = dtype.__name__ if isinstance(dtype, type) else str(dtype)
    if name in ("torch.float64", "float64", "f64", "8"):
        return 8
    if name in ("torch.float32", "float32", "f32", "4"):
        return 4
    raise NotSupported("batch: float64 or float32 values")


def plan(solver, format, preconditioner, dtype, n_rows, stored_per_item):
    """gkoc_batch_plan (host only, no device needed): what a solve of `solver` ("cg" / "bicgstab") on `format`
    ("csr" / "ell") with `preconditioner` (None / "jacobi") launches for systems of n_rows rows and
    stored_per_item values (Csr: nnz, Ell: slots x stride): the width W of the workgroup and of the reduction,
    how many of the solver's vectors are LDS-resident out of how many, whether the values are cached in LDS, the
    LDS bytes and the workspace bytes per item."""
    info = _PlanInfo()
    pre = 0 if preconditioner in (None, "none", "identity") else 1
    if pre and preconditioner != "jacobi" and not isinstance(preconditioner, (Jacobi, _JacobiFactory)):
        raise NotSupported("batch: the preconditioner is None or scalar Jacobi")
    call("gkoc_batch_plan", C.c_int(_SOLVER[solver]), C.c_int(_FORMAT[format]), C.c_int(pre),
         C.c_int(_value_bytes(dtype)), int(n_rows), int(stored_per_item), C.byref(info))
    return Plan(info.w, info.resident_vectors, info.total_vectors, bool(info.values_cached), info.lds_bytes,
                info.workspace_bytes)


class MultiVector:
    """batch::MultiVector: items x rows x cols, row-major with a row stride, item after item.  `values` is a
    3-D torch view whose row stride is the stride."""

    def __init__(self, exec_, values):
        if values.dim() != 3:
            raise GkoError("batch.MultiVector: values are items x rows x cols")
        if values.dtype not in VT:
            raise NotSupported("batch.MultiVector: float64 or float32 values")
        items, rows, cols = values.shape
        if values.numel() and (values.stride(2) != 1 or values.stride(0) != rows * values.stride(1)):
            raise GkoError("batch.MultiVector: column stride 1 and item stride rows x row stride")
        self.exec, self.values = exec_, values
        self.num_items, self.size = int(items), (int(rows), int(cols))

    @staticmethod
    def create(exec_, num_items, size, dtype=torch.float64, stride=None):
        rows, cols = size
        stride = cols if stride is None else stride
        if stride < cols:
            raise GkoError("batch.MultiVector: stride smaller than number of columns")
        store = exec_.alloc((num_items, rows, max(stride, 1)), dtype, MEM_VECTOR)
        return MultiVector(exec_, store[:, :, :cols])

    @staticmethod
    def from_numpy(exec_, array, stride=None):
        a = np.asarray(array)
        if a.ndim == 2:
            a = a[:, :, None]
        v = MultiVector.create(exec_, a.shape[0], a.shape[1:], torch.from_numpy(a[:0]).dtype, stride)
        v.values.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return v

    def to_numpy(self):
        return self.values.detach().cpu().numpy().copy()

    @property
    def dtype(self):
        return self.values.dtype

    @property
    def ld(self):
        return int(self.values.stride(1)) if self.values.numel() else max(self.size[1], 1)

    def get_num_batch_items(self):
        return self.num_items

    def get_common_size(self):
        return self.size

    def create_view_for_item(self, i):
        """a Dense over the item's part of this multi-vector's memory"""
        return _matrix.Dense(self.exec, self.values[i])

    def clone(self):
        out = MultiVector.create(self.exec, self.num_items, self.size, self.dtype, self.ld)
        out.values.copy_(self.values)
        return out

    # -- scalars: items x 1 x 1 (one per item) or items x 1 x cols (one per column), dense
    def _scalars(self, alpha, name):
        if (not isinstance(alpha, MultiVector) or alpha.num_items != self.num_items or alpha.size[0] != 1
                or alpha.size[1] not in (1, self.size[1])):
            raise DimensionMismatch(f"{name}: the scalars are items x 1 x 1 or items x 1 x cols")
        if alpha.dtype != self.dtype:
            raise NotSupported(f"{name}: one value type")
        if alpha.ld != alpha.size[1]:
            raise GkoError(f"{name}: the scalars are stored without padding")
        return alpha.values, alpha.size[1]

    def _same(self, b, name):
        if not isinstance(b, MultiVector) or b.num_items != self.num_items or b.size != self.size:
            raise DimensionMismatch(f"{name}: {b.num_items} x {b.size} against {self.num_items} x {self.size}")
        if b.dtype != self.dtype:
            raise NotSupported(f"{name}: one value type")

    def scale(self, alpha):
        av, acols = self._scalars(alpha, "scale")
        call("gkoc_batch_scale_" + VT[self.dtype], self.exec.stream, self.num_items, self.size[0], self.size[1],
             av, acols, self.values, self.ld)
        return self

    def add_scaled(self, alpha, b):
        av, acols = self._scalars(alpha, "add_scaled")
        self._same(b, "add_scaled")
        call("gkoc_batch_add_scaled_" + VT[self.dtype], self.exec.stream, self.num_items, self.size[0],
             self.size[1], av, acols, b.values, b.ld, self.values, self.ld)
        return self

    def _result(self, result, name):
        if (not isinstance(result, MultiVector) or result.num_items != self.num_items
                or result.size != (1, self.size[1]) or result.ld != self.size[1] or result.dtype != self.dtype):
            raise DimensionMismatch(f"{name}: the result is items x 1 x cols, stored without padding")

    def compute_dot(self, b, result):
        self._same(b, "compute_dot")
        self._result(result, "compute_dot")
        call("gkoc_batch_compute_dot_" + VT[self.dtype], self.exec.stream, self.num_items, self.size[0],
             self.size[1], self.values, self.ld, b.values, b.ld, result.values)
        return result

    def compute_norm2(self, result):
        self._result(result, "compute_norm2")
        call("gkoc_batch_compute_norm2_" + VT[self.dtype], self.exec.stream, self.num_items, self.size[0],
             self.size[1], self.values, self.ld, result.values)
        return result


def _int32(exec_, a):
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.int32:
            raise NotSupported("batch: int32 indices")
        return exec_.to_device(a, MEM_INDICES)
    return exec_.to_device(np.ascontiguousarray(np.asarray(a).astype(np.int32, casting="same_kind")), MEM_INDICES)


def _item_values(exec_, values, per_item):
    if not isinstance(values, torch.Tensor):
        values = np.ascontiguousarray(np.asarray(values))
        if values.ndim != 2:
            raise GkoError("batch: the values are items x stored entries")
    values = exec_.to_device(values, MEM_VALUES)
    if values.dim() != 2 or values.shape[1] != per_item:
        raise GkoError(f"batch: the values are items x {per_item}, got {tuple(values.shape)}")
    if values.dtype not in VT:
        raise NotSupported("batch: float64 or float32 values")
    return values


class _BatchMatrix:
    """what batch::matrix::Csr and Ell share: the operand checks and the two applies"""

    def get_num_batch_items(self):
        return self.num_items

    def get_common_size(self):
        return self.size

    @property
    def dtype(self):
        return self.values.dtype

    def _operands(self, b, x):
        for v in (b, x):
            if not isinstance(v, MultiVector) or v.num_items != self.num_items:
                raise DimensionMismatch("batch apply: multi-vectors with the matrix' number of items")
            if v.dtype != self.dtype:
                raise NotSupported("batch apply: one value type")
        if b.size[0] != self.size[1] or x.size[0] != self.size[0] or b.size[1] != x.size[1]:
            raise DimensionMismatch(f"batch apply: operator {self.size}, b {b.size}, x {x.size}")

    def _scalar(self, a):
        if (not isinstance(a, MultiVector) or a.num_items != self.num_items or a.size != (1, 1) or a.ld != 1
                or a.dtype != self.dtype):
            raise DimensionMismatch("batch apply: alpha and beta are items x 1 x 1 of the matrix' value type")
        return a.values

    def apply(self, *args):
        """apply(b, x): x = A b; apply(alpha, b, beta, x): x = alpha A b + beta x with per-item alpha, beta"""
        if len(args) == 2:
            b, x = args
            self._operands(b, x)
            self._apply(None, b, None, x)
        elif len(args) == 4:
            alpha, b, beta, x = args
            self._operands(b, x)
            self._apply(self._scalar(alpha), b, self._scalar(beta), x)
        else:
            raise TypeError("apply(b, x) or apply(alpha, b, beta, x)")
        return x


def _same_pattern(mats, attrs, what):
    first = mats[0]
    for m in mats[1:]:
        for name in attrs:
            a, b = getattr(first, name), getattr(m, name)
            same = torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
            if not same:
                raise GkoError(f"batch.{what}: the matrices do not share one sparsity pattern ({name})")
        if m.dtype != first.dtype:
            raise GkoError(f"batch.{what}: the matrices do not share one value type")


class Csr(_BatchMatrix):
    """batch::matrix::Csr: one (row_ptrs, col_idxs) for all items, values items x nnz.  The pattern is checked
    once, here (gkoc_batch_csr_check_i32); a bad one raises GkoError."""

    def __init__(self, exec_, size, values, col_idxs, row_ptrs):
        self.exec, self.size = exec_, (int(size[0]), int(size[1]))
        if row_ptrs.dtype != torch.int32 or col_idxs.dtype != torch.int32:
            raise NotSupported("batch.Csr: int32 indices")
        if row_ptrs.numel() != self.size[0] + 1:
            raise GkoError("batch.Csr: row_ptrs must have num_rows + 1 entries")
        if values.dim() != 2 or values.shape[1] != col_idxs.numel():
            raise GkoError("batch.Csr: the values are items x nnz")
        if values.dtype not in VT:
            raise NotSupported("batch.Csr: float64 or float32 values")
        self.values, self.col_idxs, self.row_ptrs = values, col_idxs, row_ptrs
        self.num_items = int(values.shape[0])
        call("gkoc_batch_csr_check_i32", exec_.stream, self.size[0], self.size[1], int(col_idxs.numel()),
             row_ptrs, col_idxs)

    @staticmethod
    def from_numpy(exec_, size, row_ptrs, col_idxs, values):
        ci = _int32(exec_, col_idxs)
        return Csr(exec_, size, _item_values(exec_, values, ci.numel()), ci, _int32(exec_, row_ptrs))

    @staticmethod
    def from_matrices(matrices):
        """a list of ginkgo_amd.Csr with identical patterns (otherwise GkoError); the values are copied"""
        mats = list(matrices)
        if not mats or not all(isinstance(m, _matrix.Csr) for m in mats):
            raise GkoError("batch.Csr: a non-empty list of Csr matrices")
        if any(m.size != mats[0].size or m.values.numel() != mats[0].values.numel() for m in mats):
            raise GkoError("batch.Csr: the matrices do not share one sparsity pattern (size)")
        _same_pattern(mats, ("row_ptrs", "col_idxs"), "Csr")
        ex = mats[0].exec
        values = ex.alloc((len(mats), mats[0].values.numel()), mats[0].dtype, MEM_VALUES)
        for i, m in enumerate(mats):
            values[i].copy_(m.values)
        return Csr(ex, mats[0].size, values, mats[0].col_idxs, mats[0].row_ptrs)

    @staticmethod
    def duplicate(csr, num_items):
        return Csr.from_matrices([csr] * int(num_items))

    def get_num_stored_elements_per_item(self):
        return int(self.col_idxs.numel())

    def create_view_for_item(self, i):
        """a Csr over the shared pattern and the item's part of the values"""
        return _matrix.Csr(self.exec, self.size, self.values[i], self.col_idxs, self.row_ptrs)

    def convert_to_ell(self):
        """the pattern once, as a single matrix; the values of all items in one call"""
        ex, nnz = self.exec, self.get_num_stored_elements_per_item()
        one = self.values[0] if self.num_items else ex.zeros((nnz,), self.dtype, MEM_VALUES)
        ell = _matrix.Csr(ex, self.size, one, self.col_idxs, self.row_ptrs).convert_to_ell()
        k, stride = ell.num_stored_per_row, ell.stride
        values = ex.alloc((self.num_items, k * stride), self.dtype, MEM_VALUES)
        call("gkoc_batch_csr_to_ell_values_" + VT[self.dtype] + "_i32", ex.stream, self.num_items, self.size[0],
             nnz, self.row_ptrs, k, stride, self.values, values)
        return Ell(ex, self.size, values, ell.col_idxs, k, stride)

    def _apply(self, alpha, b, beta, x):
        suf = VT[self.dtype] + "_i32"
        nnz = self.get_num_stored_elements_per_item()
        if alpha is None:
            call("gkoc_batch_csr_apply_" + suf, self.exec.stream, self.num_items, self.size[0], self.size[1], nnz,
                 self.row_ptrs, self.col_idxs, self.values, b.values, b.ld, x.values, x.ld, b.size[1])
        else:
            call("gkoc_batch_csr_advanced_apply_" + suf, self.exec.stream, self.num_items, self.size[0],
                 self.size[1], nnz, alpha, self.row_ptrs, self.col_idxs, self.values, b.values, b.ld, beta,
                 x.values, x.ld, b.size[1])


class Ell(_BatchMatrix):
    """batch::matrix::Ell: one column-major slot array (padding -1) for all items, values items x
    (num_stored_per_row * stride).  The pattern is checked once, here (gkoc_batch_ell_check_i32)."""

    def __init__(self, exec_, size, values, col_idxs, num_stored_per_row, stride):
        self.exec, self.size = exec_, (int(size[0]), int(size[1]))
        self.num_stored_per_row, self.stride = int(num_stored_per_row), int(stride)
        if col_idxs.dtype != torch.int32:
            raise NotSupported("batch.Ell: int32 indices")
        if self.stride < self.size[0]:
            raise GkoError("batch.Ell: stride smaller than number of rows")
        per_item = self.num_stored_per_row * self.stride
        if col_idxs.numel() != per_item or values.dim() != 2 or values.shape[1] != per_item:
            raise GkoError("batch.Ell: col_idxs has slots x stride entries and the values are items x as many")
        if values.dtype not in VT:
            raise NotSupported("batch.Ell: float64 or float32 values")
        self.values, self.col_idxs = values, col_idxs
        self.num_items = int(values.shape[0])
        call("gkoc_batch_ell_check_i32", exec_.stream, self.size[0], self.size[1], self.num_stored_per_row,
             self.stride, col_idxs)

    @staticmethod
    def from_numpy(exec_, size, col_idxs, values, num_stored_per_row, stride=None):
        stride = int(size[0]) if stride is None else int(stride)
        ci = _int32(exec_, np.asarray(col_idxs).reshape(-1))
        return Ell(exec_, size, _item_values(exec_, values, int(num_stored_per_row) * stride), ci,
                   num_stored_per_row, stride)

    @staticmethod
    def from_matrices(matrices):
        mats = list(matrices)
        if not mats or not all(isinstance(m, _matrix.Ell) for m in mats):
            raise GkoError("batch.Ell: a non-empty list of Ell matrices")
        _same_pattern(mats, ("size", "num_stored_per_row", "stride", "col_idxs"), "Ell")
        ex = mats[0].exec
        values = ex.alloc((len(mats), mats[0].values.numel()), mats[0].dtype, MEM_VALUES)
        for i, m in enumerate(mats):
            values[i].copy_(m.values)
        return Ell(ex, mats[0].size, values, mats[0].col_idxs, mats[0].num_stored_per_row, mats[0].stride)

    @staticmethod
    def duplicate(ell, num_items):
        return Ell.from_matrices([ell] * int(num_items))

    def get_num_stored_elements_per_item(self):
        return self.num_stored_per_row * self.stride

    def create_view_for_item(self, i):
        return _matrix.Ell(self.exec, self.size, self.values[i], self.col_idxs, self.num_stored_per_row,
                           self.stride)

    def convert_to_csr(self):
        ex, n, k, stride = self.exec, self.size[0], self.num_stored_per_row, self.stride
        ptrs = ex.zeros((n + 1,), torch.int32, MEM_INDICES)
        call("gkoc_ell_count_nonzeros_per_row_i32", ex.stream, n, k, stride, self.col_idxs, ptrs)
        call("gkoc_prefix_sum_nonnegative_i32", ex.stream, ptrs, n + 1)
        nnz = int(ptrs[-1].item())
        cols = ex.alloc((nnz,), torch.int32, MEM_INDICES)
        values = ex.alloc((self.num_items, nnz), self.dtype, MEM_VALUES)
        one = self.values[0] if self.num_items else ex.zeros((k * stride,), self.dtype, MEM_VALUES)
        call("gkoc_ell_to_csr_" + VT[self.dtype] + "_i32", ex.stream, n, k, stride, self.col_idxs, one, ptrs,
             cols, ex.alloc((nnz,), self.dtype, MEM_VALUES))
        call("gkoc_batch_ell_to_csr_values_" + VT[self.dtype] + "_i32", ex.stream, self.num_items, n, k, stride,
             self.col_idxs, nnz, ptrs, self.values, values)
        return Csr(ex, self.size, values, cols, ptrs)

    def _apply(self, alpha, b, beta, x):
        suf = VT[self.dtype] + "_i32"
        if alpha is None:
            call("gkoc_batch_ell_apply_" + suf, self.exec.stream, self.num_items, self.size[0], self.size[1],
                 self.num_stored_per_row, self.stride, self.col_idxs, self.values, b.values, b.ld, x.values,
                 x.ld, b.size[1])
        else:
            call("gkoc_batch_ell_advanced_apply_" + suf, self.exec.stream, self.num_items, self.size[0],
                 self.size[1], self.num_stored_per_row, self.stride, alpha, self.col_idxs, self.values, b.values,
                 b.ld, beta, x.values, x.ld, b.size[1])


class _JacobiFactory:
    def __init__(self):
        self.max_block_size = 1

    def with_max_block_size(self, max_block_size):
        if int(max_block_size) != 1:
            raise NotSupported("batch.Jacobi: scalar Jacobi only (max_block_size 1)")
        return self

    def on(self, exec_):
        return self

    def generate(self, batch_matrix):
        return Jacobi(batch_matrix)


class Jacobi:
    """batch::preconditioner::Jacobi, scalar: z_i = r_i / a_ii.  Nothing is generated: the solver kernel takes
    the diagonal from the item's own values in its prologue."""

    def __init__(self, batch_matrix):
        self.matrix = batch_matrix

    @staticmethod
    def build():
        return _JacobiFactory()


class _SolverFactory:
    def __init__(self, cls):
        self.cls = cls
        self.max_iterations, self.tolerance, self.tolerance_type = 100, 1e-11, "absolute"
        self.preconditioner, self.exec = None, None

    def with_max_iterations(self, max_iterations):
        if int(max_iterations) < 0:
            raise GkoError("batch solver: negative max_iterations")
        self.max_iterations = int(max_iterations)
        return self

    def with_tolerance(self, tolerance):
        self.tolerance = float(tolerance)
        return self

    def with_tolerance_type(self, tolerance_type):
        if tolerance_type not in _TOLERANCE:
            raise GkoError('batch solver: the tolerance type is "absolute" or "relative"')
        self.tolerance_type = tolerance_type
        return self

    def with_preconditioner(self, preconditioner):
        if preconditioner is not None and not isinstance(preconditioner, (_JacobiFactory, Jacobi)):
            raise NotSupported("batch solver: the preconditioner is None or batch.Jacobi")
        self.preconditioner = preconditioner
        return self

    def on(self, exec_):
        self.exec = exec_
        return self

    def generate(self, batch_matrix):
        if self.exec is None:
            raise GkoError("batch solver: on(exec) before generate")
        return self.cls(self, batch_matrix)


class _BatchSolver:
    """One apply = one library call; nothing is read back.  After it iteration_counts, residual_norms and
    converged (one entry per item) are device tensors: the log::BatchConvergence of the solve."""
    _name = None

    def __init__(self, factory, batch_matrix):
        if not isinstance(batch_matrix, (Csr, Ell)):
            raise NotSupported("batch solver: a batch.Csr or batch.Ell system matrix")
        if batch_matrix.size[0] != batch_matrix.size[1]:
            raise DimensionMismatch(f"batch solver: the systems are square, got {batch_matrix.size}")
        self.exec, self.matrix = factory.exec, batch_matrix
        self.max_iterations, self.tolerance = factory.max_iterations, factory.tolerance
        self.tolerance_type = factory.tolerance_type
        self.preconditioner = factory.preconditioner
        self._pre = 0 if factory.preconditioner is None else 1
        self._format = "csr" if isinstance(batch_matrix, Csr) else "ell"
        items, ex = batch_matrix.num_items, self.exec
        self.plan = plan(self._name, self._format, "jacobi" if self._pre else None, batch_matrix.dtype,
                         batch_matrix.size[0], batch_matrix.get_num_stored_elements_per_item())
        self.workspace = ex.alloc((max(self.plan.workspace_bytes * items, 1),), torch.uint8, MEM_VECTOR)
        self.iteration_counts = ex.zeros((items,), torch.int32)
        self.residual_norms = ex.zeros((items,), batch_matrix.dtype)
        self.converged = ex.zeros((items,), torch.int32)

    @classmethod
    def build(cls):
        return _SolverFactory(cls)

    def get_system_matrix(self):
        return self.matrix

    def apply(self, b, x):
        """solves every item, starting from x"""
        m = self.matrix
        for v in (b, x):
            if not isinstance(v, MultiVector) or v.num_items != m.num_items or v.size != (m.size[0], 1):
                raise DimensionMismatch("batch solver: b and x are items x rows x 1 multi-vectors")
            if v.dtype != m.dtype:
                raise NotSupported("batch solver: one value type")
        entry = _SOLVE[self._name, self._format] + VT[m.dtype] + "_i32"
        tail = (m.values, C.c_int(self._pre), b.values, b.ld, x.values, x.ld, C.c_double(self.tolerance),
                C.c_int(_TOLERANCE[self.tolerance_type]), self.max_iterations, self.workspace,
                C.c_size_t(self.workspace.numel()), self.iteration_counts, self.residual_norms, self.converged)
        if self._format == "csr":
            call(entry, self.exec.stream, m.num_items, m.size[0], m.get_num_stored_elements_per_item(),
                 m.row_ptrs, m.col_idxs, *tail)
        else:
            call(entry, self.exec.stream, m.num_items, m.size[0], m.num_stored_per_row, m.stride, m.col_idxs,
                 *tail)
        return x


class Cg(_BatchSolver):
    """batch::solver::Cg"""
    _name = "cg"


class Bicgstab(_BatchSolver):
    """batch::solver::Bicgstab"""
    _name = "bicgstab"
