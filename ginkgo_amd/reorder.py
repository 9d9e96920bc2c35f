"""Reorderings - mirror of include/ginkgo/core/reorder/{nested_dissection,scaled_reordered}.hpp
(experimental::reorder::NestedDissection / ScaledReordered).

`NestedDissection.build().with_leaf_size(k).on(exec).generate(csr)` returns a `matrix.Permutation` p, p[k] = the
original index of the vertex at the new position k, that makes the elimination forest of the permuted matrix
bushy: factorization.Cholesky / Lu and the level-scheduled solves then have many rows per level.  Ginkgo's class
calls METIS on the host; this one computes the deterministic dissection that include/gko_cdna4.h states
("Nested dissection": two breadth-first sweeps per region, the median level as separator, no refinement) on the
device, all regions of a recursion depth at once.  Integer-exact against tests/reorder_refs.py.  The pattern is
symmetrised first (pattern(A) + pattern(A^T) through the triplet pipeline, like factorization.Cholesky); values
are not read.  One dissection round is components, regroup, levels, far_roots, levels, split, regroup
(gkoc_reorder_*); a level step is a launch the host waits for, so the cost grows with the diameters
(docs/KERNELS.md 45).  `launches` counts the sweeps and steps, `rounds` the dissection rounds.

`ScaledReordered.build().with_inner_operator(f).with_reordering(r).on(exec).generate(A)` computes P with the
reordering factory r, permutes A symmetrically (Csr.permute) and generates the inner operator on P A P^T.
apply: b' = P b, x' = P x (an inner iterative solver continues from it), inner apply, x = P^T x'.  Launches only:
Multigrid stays capturable with ScaledReordered(Direct) as coarsest solver.  The scalings of Ginkgo's class are
not built: with_row_scaling / with_col_scaling refuse anything but None.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import IT, DimensionMismatch, GkoError, NotSupported, call
from .base import LinOp
from .executor import MEM_INDICES
from .matrix import Csr, Dense, DeviceMatrixData, Fbcsr, Permutation

# the leaf size with the shortest numeric phase of Cholesky on the 2687-row coarse operator (docs/KERNELS.md 45)
DEFAULT_LEAF_SIZE = 8


def row_limits():
    """the row lengths at which the graph kernels change path (gkoc_reorder_row_limits)"""
    return _lib.row_limits("gkoc_reorder_row_limits")


def symmetrized_pattern(a):
    """(row_ptrs, col_idxs) of pattern(a) + pattern(a^T), rows sorted: the triplets of a and, rows and columns
    exchanged, of a^T through the triplet pipeline, all values 1"""
    ex, n, idx, it = a.exec, a.size[0], a.col_idxs.dtype, IT[a.col_idxs.dtype]
    nnz = a.col_idxs.numel()
    rows, cols = ex.alloc((2 * nnz,), idx), ex.alloc((2 * nnz,), idx)
    call("gkoc_convert_ptrs_to_idxs_" + it, ex.stream, a.row_ptrs, n, rows[:nnz])
    cols[:nnz].copy_(a.col_idxs)
    rows[nnz:].copy_(a.col_idxs)
    cols[nnz:].copy_(rows[:nnz])
    data = DeviceMatrixData(ex, a.size, rows, cols, ex.alloc((2 * nnz,), torch.float32).fill_(1))
    data.sum_duplicates()
    rp = Csr.read(data).row_ptrs
    ex.synchronize()                    # the triplets are released on return
    return rp, data.col_idxs


class _NestedDissectionFactory:
    def __init__(self):
        self.leaf_size = DEFAULT_LEAF_SIZE
        self.exec = None

    def with_leaf_size(self, v):
        if int(v) < 1:
            raise GkoError("with_leaf_size needs a size >= 1")
        self.leaf_size = int(v)
        return self

    def on(self, exec_):
        self.exec = exec_
        return self

    def generate(self, system_matrix):
        return NestedDissection(self, system_matrix).permutation


class NestedDissection:
    """the run of one dissection: `permutation` is the result, `rounds` and `launches` what it took"""

    @staticmethod
    def build():
        return _NestedDissectionFactory()

    def __init__(self, factory, a):
        if isinstance(a, Fbcsr):
            a = a.convert_to_csr()
        if not isinstance(a, Csr):
            raise NotSupported("reorder.NestedDissection.generate needs a Csr system matrix")
        if a.size[0] != a.size[1]:
            raise DimensionMismatch("reorder.NestedDissection needs a square matrix")
        ex = self.exec = factory.exec or a.exec
        n, idx, it = a.size[0], a.col_idxs.dtype, IT[a.col_idxs.dtype]
        leaf = self.leaf_size = factory.leaf_size
        self.rounds = self.launches = 0
        order = torch.arange(n, dtype=idx, device=ex.device)
        if n > leaf:
            rp, ci = symmetrized_pattern(a)
            pattern = (ex.stream, n, ci.numel(), rp, ci)
            region = ex.zeros((n,), idx)
            label, level, far, cls = (ex.alloc((n,), idx) for _ in range(4))
            live, waited = C.c_longlong(n), C.c_longlong(0)

            def regroup(final_from, key):
                call("gkoc_reorder_regroup_" + it, ex.stream, n, leaf, final_from, key, order, region,
                     C.byref(live))

            def levels(root):
                call("gkoc_reorder_levels_" + it, *pattern, region, root, level, C.byref(waited))
                self.launches += waited.value

            while live.value:
                if self.rounds >= n:
                    raise GkoError("reorder.NestedDissection: a round that divides nothing")
                self.rounds += 1
                call("gkoc_reorder_components_" + it, *pattern, region, label, C.byref(waited))
                self.launches += waited.value
                regroup(n, label)
                if not live.value:
                    break
                levels(order)           # a segment is ascending: its first vertex is r0 = min R
                call("gkoc_reorder_far_roots_" + it, ex.stream, n, region, level, far)
                levels(far)
                call("gkoc_reorder_split_" + it, *pattern, order, region, level, cls)
                regroup(2, cls)
            ex.synchronize()            # the state arrays are released on return
        perm = ex.alloc((n,), idx, MEM_INDICES)
        perm.copy_(order)
        self.permutation = Permutation(ex, perm)


class _ScaledReorderedFactory:
    def __init__(self):
        self.inner_operator = self.reordering = self.exec = None

    def with_inner_operator(self, factory):
        self.inner_operator = factory
        return self

    def with_reordering(self, factory):
        self.reordering = factory
        return self

    def _no_scaling(self, which, v):
        if v is not None:
            raise NotSupported(f"reorder.ScaledReordered: with_{which}_scaling is not built (pass None)")
        return self

    def with_row_scaling(self, v):
        return self._no_scaling("row", v)

    def with_col_scaling(self, v):
        return self._no_scaling("col", v)

    def on(self, exec_):
        self.exec = exec_
        return self

    def generate(self, system_matrix):
        return ScaledReordered(self, system_matrix)


class ScaledReordered(LinOp):
    """x = P^T M(P A P^T) P b for the inner operator M and the permutation P of the reordering."""

    @staticmethod
    def build():
        return _ScaledReorderedFactory()

    def __init__(self, factory, a):
        if isinstance(a, Fbcsr):
            a = a.convert_to_csr()
        if not isinstance(a, Csr):
            raise NotSupported("reorder.ScaledReordered.generate needs a Csr system matrix")
        if a.size[0] != a.size[1]:
            raise DimensionMismatch("reorder.ScaledReordered needs a square matrix")
        ex = factory.exec or a.exec
        super().__init__(ex, a.size)
        self.dtype = a.dtype
        for f in (factory.inner_operator, factory.reordering):
            if f is not None and getattr(f, "exec", None) is None and hasattr(f, "on"):
                f.on(ex)
        n, idx = a.size[0], a.col_idxs.dtype
        if factory.reordering is None:
            self.permutation = Permutation(ex, torch.arange(n, dtype=idx, device=ex.device))
            self.system_matrix = a
        else:
            self.permutation = factory.reordering.generate(a)
            self.system_matrix = a.permute(self.permutation, "symmetric")
        self.inverse_permutation = self.permutation.compute_inverse()
        self.inner = None if factory.inner_operator is None else factory.inner_operator.generate(self.system_matrix)
        self._vectors = {}
        self._work(1)

    def _work(self, cols):
        """(P b, P x, the result of the advanced form) for `cols` right-hand sides"""
        vs = self._vectors.get(cols)
        if vs is None:
            vs = self._vectors[cols] = tuple(Dense.create(self.exec, (self.size[0], cols), self.dtype)
                                             for _ in range(3))
        return vs

    def get_permutation(self):
        return self.permutation

    def get_system_matrix(self):
        """the permuted matrix P A P^T the inner operator was generated on"""
        return self.system_matrix

    def get_inner_operator(self):
        return self.inner

    def apply_impl(self, b, x):
        if b.dtype != self.dtype or x.dtype != self.dtype:
            raise NotSupported("reorder.ScaledReordered: vectors must have the matrix' value type")
        pb, px, _ = self._work(b.size[1])
        self.permutation.apply(b, pb)
        self.permutation.apply(x, px)
        if self.inner is None:
            px.copy_from(pb)
        else:
            self.inner.apply(pb, px)
        self.inverse_permutation.apply(px, x)

    def apply_advanced_impl(self, alpha, b, beta, x):
        # x = beta * x + alpha * solve(b), composed as in Direct
        solved = self._work(b.size[1])[2]
        solved.copy_from(x)
        self.apply_impl(b, solved)
        x.scale(beta)
        x.add_scaled(alpha, solved)
