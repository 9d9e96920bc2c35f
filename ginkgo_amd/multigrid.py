"""Aggregation multigrid - mirror of include/ginkgo/core/multigrid/pgm.hpp (multigrid::Pgm) and
include/ginkgo/core/solver/multigrid.hpp (solver::Multigrid).

`Pgm.build().with_max_iterations(15).with_max_unassign_ratio(0.05).on(exec).generate(a)` groups the rows of a
square Csr (or Fbcsr, through convert_to_csr()) into aggregates by parallel graph matching and builds the
coarse operator P^T A P, P(i, agg_i) = 1.  The aggregation is specified bit for bit in include/gko_cdna4.h
("Pgm aggregation"): every round reads the aggregation as it was when the round began and ties are decided by
a symmetric hash of the pair, so the result depends on nothing but the matrix - `with_deterministic` is
accepted and has no effect.  Unsorted input is sorted on a copy (unless with_skip_sorting(True)); the caller's
matrix is never changed.  P and P^T are not stored: `get_restrict_op()` / `get_prolong_op()` apply them from agg
and the member lists (gkoc_pgm_restrict_*, gkoc_pgm_prolong_add_*).

`Multigrid.build().with_mg_level(Pgm.build()).with_cycle("v")...on(exec).generate(a)` stacks such levels and is
both a solver and, with `with_criteria(Iteration(1))` or none, a preconditioner factory for every solver class.
One cycle on a level: pre-smooth, r = b - A x, b_c = restrict(r), recurse from x_c = 0 (under "w" a second time,
continuing from the first x_c), prolong-add, post-smooth.  The built-in smoother is `smoother_iters` sweeps of
x <- x + relax D^-1 (b - A x) (the first sweep on a zero guess is x = relax D^-1 b, without a product), the
built-in coarsest solver 4 such sweeps.  A user's `with_pre_smoother(f)` / `with_post_smoother(f)` /
`with_coarsest_solver(f)` takes any LinOp factory: an iterative solver is applied with x as its initial guess,
any other operator M as x <- x + relax M (b - A x).

Every level vector and D^-1 is allocated at generate or on the first apply for a column count.  With only
Iteration criteria (or none) an application issues no device-to-host copy and no stream synchronisation; with a
ResidualNorm criterion the residual is checked once per cycle on the finest level.

Real value types, one device.  Complex values and a distributed Pgm are out of scope.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import IT, VT, DimensionMismatch, GkoError, NotSupported, call
from .base import LinOp
from .executor import MEM_INDICES, MEM_VALUES
from .krylov import _Stationary
from .matrix import Csr, Dense, DeviceMatrixData, Fbcsr, _np_dtype, entry_dtype, scalar
from .solver import _IterativeSolver, _SolverFactory
from . import stop as _stop


def row_limits():
    """the row lengths of the weight matrix at which the selection kernel changes path (gkoc_pgm_row_limits)"""
    return _lib.row_limits("gkoc_pgm_row_limits")


class _PgmFactory:
    def __init__(self):
        self.max_iterations = 15
        self.max_unassign_ratio = 0.05
        self.skip_sorting = False
        self.deterministic = True
        self.exec = None

    def with_max_iterations(self, v):
        self.max_iterations = int(v)
        return self

    def with_max_unassign_ratio(self, v):
        self.max_unassign_ratio = float(v)
        return self

    def with_skip_sorting(self, v):
        self.skip_sorting = bool(v)
        return self

    def with_deterministic(self, v):
        """accepted for API compatibility: the result never depends on thread order"""
        self.deterministic = bool(v)
        return self

    def on(self, exec_):
        self.exec = exec_
        return self

    def generate(self, system_matrix):
        if isinstance(system_matrix, Fbcsr):
            csr = system_matrix.convert_to_csr()
            level = Pgm(self, csr)
            level.fine = system_matrix
            return level
        return Pgm(self, system_matrix)


def _placed(ex, csr):
    """the matrix with its arrays where a matrix' read-only arrays belong (the triplet pipeline's output lives
    with the vectors)"""
    rp = ex.alloc((csr.row_ptrs.numel(),), csr.row_ptrs.dtype, MEM_INDICES)
    ci = ex.alloc((csr.col_idxs.numel(),), csr.col_idxs.dtype, MEM_INDICES)
    v = ex.alloc((csr.values.numel(),), csr.dtype, MEM_VALUES)
    rp.copy_(csr.row_ptrs)
    ci.copy_(csr.col_idxs)
    v.copy_(csr.values)
    return Csr(ex, csr.size, v, ci, rp)


class _Restrict(LinOp):
    """b_c = P^T r: every aggregate's members summed in ascending order (gkoc_pgm_restrict_*)"""

    def __init__(self, level):
        super().__init__(level.exec, (level.num_aggregates, level.size[0]))
        self.level = level

    def apply_impl(self, b, x):
        lv = self.level
        call("gkoc_pgm_restrict_" + lv._suf, self.exec.stream, lv.num_aggregates, b.size[1], lv.member_ptrs,
             lv.members, b.values, b.ld, x.values, x.ld)

    def apply_advanced_impl(self, alpha, b, beta, x):
        t = Dense.create(self.exec, x.size, x.dtype)
        self.apply_impl(b, t)
        x.scale(beta)
        x.add_scaled(alpha, t)


class _Prolong(LinOp):
    """x = P e; apply(one, e, one, x) is x += P e, one add per entry (gkoc_pgm_prolong_add_*)"""

    def __init__(self, level):
        super().__init__(level.exec, (level.size[0], level.num_aggregates))
        self.level = level

    def add(self, e, x):
        lv = self.level
        call("gkoc_pgm_prolong_add_" + lv._suf, self.exec.stream, lv.size[0], e.size[1], lv.agg, e.values, e.ld,
             x.values, x.ld)

    def apply_impl(self, b, x):
        x.fill(0.0)
        self.add(b, x)

    def apply_advanced_impl(self, alpha, b, beta, x):
        # off the hot path (Multigrid calls add()): the two scalars are read
        if float(alpha.to_numpy()[0, 0]) == 1.0 and float(beta.to_numpy()[0, 0]) == 1.0:
            return self.add(b, x)
        t = Dense.create(self.exec, x.size, x.dtype)
        self.apply_impl(b, t)
        x.scale(beta)
        x.add_scaled(alpha, t)


class Pgm:
    """one multigrid level: the aggregation of the rows of `a`, the coarse operator and the two transfers"""

    @staticmethod
    def build():
        return _PgmFactory()

    def __init__(self, factory, a):
        if not isinstance(a, Csr):
            raise NotSupported("Pgm.generate needs a Csr (or Fbcsr) system matrix")
        if a.size[0] != a.size[1]:
            raise DimensionMismatch("Pgm needs a square matrix")
        if a.dtype not in VT:
            raise NotSupported("Pgm: real value types only")
        if factory.max_iterations < 1:
            raise GkoError(f"Pgm: max_iterations must be at least 1, got {factory.max_iterations}")
        ex = self.exec = factory.exec or a.exec
        self.size, self.dtype, self.fine = a.size, a.dtype, a
        n, idt = a.size[0], a.col_idxs.dtype
        it = IT[idt]
        self._suf = f"{VT[a.dtype]}_{it}"
        if not factory.skip_sorting and not a.is_sorted_by_column_index():
            a = Csr(ex, a.size, a.values.clone(), a.col_idxs.clone(), a.row_ptrs,
                    a.strategy).sort_by_column_index()
        nnz = a.get_num_stored_elements()
        rows = ex.alloc((nnz,), idt)
        call("gkoc_convert_ptrs_to_idxs_" + it, ex.stream, a.row_ptrs, n, rows)
        w, d = self._weights(ex, a, rows)
        # ---- the rounds: every one reads agg as it was when it began
        agg = ex.alloc((n,), idt, MEM_INDICES).fill_(-1)
        proposals = ex.alloc((n,), idt)
        count, previous, self.rounds = C.c_longlong(n), None, 0
        for _ in range(factory.max_iterations if n else 0):
            call("gkoc_pgm_select_" + self._suf, ex.stream, n, w.row_ptrs, w.col_idxs, w.values, d, agg, proposals)
            call("gkoc_pgm_match_" + it, ex.stream, n, proposals, agg, C.byref(count))
            self.rounds += 1
            if count.value == 0 or count.value == previous or count.value < factory.max_unassign_ratio * n:
                break
            previous = count.value
        self.num_leftover = count.value if n else 0
        if self.num_leftover:
            before = agg.clone()
            call("gkoc_pgm_leftover_" + self._suf, ex.stream, n, w.row_ptrs, w.col_idxs, w.values, d, before, agg)
        coarse = C.c_longlong(0)
        call("gkoc_pgm_renumber_" + it, ex.stream, n, agg, C.byref(coarse))
        self.agg, self.num_aggregates = agg, coarse.value
        nc = self.num_aggregates
        # ---- the member lists: the rows sorted by (aggregate, row), stable
        keys, members = agg.clone(), ex.alloc((n,), idt, MEM_INDICES)
        call("gkoc_fill_seq_array_" + it, ex.stream, members, n)
        DeviceMatrixData(ex, (nc, n), keys, members, ex.alloc((n,), a.dtype)).sort_row_major()
        self.member_ptrs = ex.alloc((nc + 1,), idt, MEM_INDICES)
        call("gkoc_convert_idxs_to_ptrs_" + it, ex.stream, n, keys, nc, self.member_ptrs)
        self.members = members
        # the transfer kernels check nothing on the device: this does, once
        call("gkoc_pgm_check_transfers_" + it, ex.stream, n, nc, agg, self.member_ptrs, members)
        # ---- A_c = P^T A P: the fine triplets mapped through agg, in storage order, as matrix_data entries; then
        # the triplet pipeline
        width = entry_dtype(_np_dtype(a.dtype), _np_dtype(idt)).itemsize
        entries = ex.alloc((max(nnz * width, 1),), torch.uint8)
        call("gkoc_pgm_map_entries_" + self._suf, ex.stream, nnz, n, nc, agg, rows, a.col_idxs, a.values, entries)
        crows, ccols, cvals = ex.alloc((nnz,), idt), ex.alloc((nnz,), idt), ex.alloc((nnz,), a.dtype)
        call("gkoc_aos_to_soa_" + self._suf, ex.stream, nnz, entries, crows, ccols, cvals)
        data = DeviceMatrixData(ex, (nc, nc), crows, ccols, cvals)
        if nnz:
            data.sum_duplicates()
        self.coarse = _placed(ex, Csr.read(data))
        self.restrict_op, self.prolong_op = _Restrict(self), _Prolong(self)
        ex.synchronize()        # the weights, the triplets and a sorted copy are released on return

    @staticmethod
    def _weights(ex, a, rows):
        """W = 0.5 |A| + 0.5 |A^T| on the pattern of A u A^T and its diagonal: the triplets of A and, with rows
        and columns exchanged, of A^T, halved (exact), through the triplet pipeline - a run has one or two
        entries, 0 + v0 (+ v1), so the sum does not depend on their order"""
        n, nnz, idt = a.size[0], a.get_num_stored_elements(), a.col_idxs.dtype
        wr, wc = ex.alloc((2 * nnz,), idt), ex.alloc((2 * nnz,), idt)
        wv = ex.alloc((2 * nnz,), a.dtype)
        wr[:nnz].copy_(rows)
        wr[nnz:].copy_(a.col_idxs)
        wc[:nnz].copy_(a.col_idxs)
        wc[nnz:].copy_(rows)
        wv[:nnz].copy_(a.values)
        wv[nnz:].copy_(a.values)
        vt = VT[a.dtype]
        call("gkoc_dense_absolute_" + vt, ex.stream, 2 * nnz, 1, wv, 1, wv, 1)
        call("gkoc_dense_scale_" + vt, ex.stream, 2 * nnz, 1, scalar(ex, 0.5, a.dtype).values, 1, wv, 1)
        data = DeviceMatrixData(ex, a.size, wr, wc, wv)
        if nnz:
            data.sum_duplicates()
        w = Csr.read(data)
        return w, w.extract_diagonal()

    # -- accessors (multigrid::MultigridLevel / Pgm)
    def get_agg(self):
        return self.agg

    def get_num_aggregates(self):
        return self.num_aggregates

    def get_fine_op(self):
        return self.fine

    def get_coarse_op(self):
        return self.coarse

    def get_restrict_op(self):
        return self.restrict_op

    def get_prolong_op(self):
        return self.prolong_op


class _Sweeps(LinOp):
    """`count` sweeps of x <- x + relax D^-1 (b - A x): the built-in smoother and coarsest solver.  As a LinOp
    it starts from a zero guess.  winv = relax D^-1 is made once; a sweep is a copy, an advanced SpMV and
    gkoc_jacobi_scalar_apply, the first sweep on a zero guess gkoc_jacobi_simple_scalar_apply alone."""

    def __init__(self, a, count, relax):
        super().__init__(a.exec, a.size)
        ex, n = a.exec, a.size[0]
        self.a, self.count, self.dtype = a, int(count), a.dtype
        self.winv = ex.alloc((n,), a.dtype)
        call("gkoc_jacobi_invert_diagonal_" + VT[a.dtype], ex.stream, n, a.extract_diagonal(), self.winv)
        call("gkoc_dense_scale_" + VT[a.dtype], ex.stream, n, 1, scalar(ex, relax, a.dtype).values, 1, self.winv, 1)
        self.one, self.neg_one = scalar(ex, 1.0, a.dtype), scalar(ex, -1.0, a.dtype)
        self._r = {}

    def run(self, b, x, zero, r):
        ex, vt = self.exec, VT[self.dtype]
        n, cols = b.size
        if zero and self.count == 0:
            x.fill(0.0)
        for k in range(self.count):
            if zero and k == 0:
                call("gkoc_jacobi_simple_scalar_apply_" + vt, ex.stream, n, cols, self.winv, b.values, b.ld,
                     x.values, x.ld)
            else:
                r.copy_from(b)
                self.a.apply(self.neg_one, x, self.one, r)
                call("gkoc_jacobi_scalar_apply_" + vt, ex.stream, n, cols, self.winv, self.one.values, r.values,
                     r.ld, self.one.values, x.values, x.ld)

    def apply_impl(self, b, x):
        r = self._r.get(b.size[1])
        if r is None:
            r = self._r[b.size[1]] = Dense.create(self.exec, b.size, b.dtype)
        self.run(b, x, True, r)

    def apply_advanced_impl(self, alpha, b, beta, x):
        t = Dense.create(self.exec, x.size, x.dtype)
        self.apply_impl(b, t)
        x.scale(beta)
        x.add_scaled(alpha, t)


class Multigrid(_Stationary):
    """solver::Multigrid over Pgm levels; see the module docstring"""

    @staticmethod
    def build():
        return _SolverFactory(Multigrid)

    def __init__(self, factory, a):
        if isinstance(a, Fbcsr):
            a = a.convert_to_csr()
        if not isinstance(a, Csr):
            raise NotSupported("Multigrid.generate needs a Csr (or Fbcsr) system matrix")
        super().__init__(factory, a)
        p, ex = self.params, self.exec
        self.cycle = str(p.get("cycle", "v")).lower()
        if self.cycle not in ("v", "w"):
            raise GkoError(f"Multigrid: cycle must be 'v' or 'w', got {self.cycle!r}")
        self.initial_guess = str(p.get("default_initial_guess", "zero"))
        if self.initial_guess not in ("zero", "provided"):
            raise GkoError(f"Multigrid: default_initial_guess must be 'zero' or 'provided', "
                           f"got {self.initial_guess!r}")
        self.relax = float(p.get("smoother_relax", 0.9))
        iters = int(p.get("smoother_iters", 1))
        max_levels, min_rows = int(p.get("max_levels", 10)), int(p.get("min_coarse_rows", 64))
        level_factory = p.get("mg_level") or Pgm.build()
        if level_factory.exec is None:
            level_factory.on(ex)
        # ---- the levels: stop at max_levels, at <= min_coarse_rows rows, or when a level does not get smaller
        self.mg_levels, ops = [], [a]
        while len(ops) < max_levels and ops[-1].size[0] > min_rows:
            level = level_factory.generate(ops[-1])
            if level.get_num_aggregates() >= ops[-1].size[0]:
                break
            self.mg_levels.append(level)
            ops.append(level.get_coarse_op())
        self.ops = ops

        def made(f, op):
            if f is None:
                return None
            if getattr(f, "exec", None) is None and hasattr(f, "on"):
                f.on(ex)
            return f.generate(op)

        pre_f, post_f = p.get("pre_smoother"), p.get("post_smoother")
        self.pre = [made(pre_f, op) or _Sweeps(op, iters, self.relax) for op in ops[:-1]]
        # post uses pre's setting (and its generated operators) unless it has a factory of its own
        self.post = self.pre if post_f is None or post_f is pre_f else [made(post_f, op) for op in ops[:-1]]
        self.smoother_iters = iters
        self.coarsest = made(p.get("coarsest_solver"), ops[-1]) or _Sweeps(ops[-1], 4, self.relax)
        self.omega = scalar(ex, self.relax, a.dtype)
        self.one, self.neg_one = scalar(ex, 1.0, a.dtype), scalar(ex, -1.0, a.dtype)
        self._vectors = {}

    @property
    def capturable(self):
        """whether an application can be captured into a graph (Cg's hipGraph mode asks): not with a criterion
        that reads a residual back, nor with an iterative solver as smoother or coarsest solver"""
        return all(c is None or c.cls is _stop.Iteration for c in self.criteria) and \
            not any(isinstance(s, _IterativeSolver) for s in self.pre + self.post + [self.coarsest])

    def get_mg_level_list(self):
        return list(self.mg_levels)

    def get_coarsest_solver(self):
        return self.coarsest

    # -- workspace: per column count, per level r and t (finest included), b and x (coarse levels)
    def _level_vectors(self, cols, dtype):
        vs = self._vectors.get((cols, dtype))
        if vs is None:
            vs = self._vectors[(cols, dtype)] = [
                {k: Dense.create(self.exec, (op.size[0], cols), dtype) for k in (("r", "t") if l == 0 else
                                                                                 ("r", "t", "b", "x"))}
                for l, op in enumerate(self.ops)]
        return vs

    def _smooth(self, s, a, b, x, zero, v):
        if isinstance(s, _Sweeps):
            return s.run(b, x, zero, v["r"])
        if isinstance(s, _IterativeSolver):
            if zero:
                x.fill(0.0)
            return s.apply(b, x)        # the solver continues from x
        # any other operator M: x <- x + relax M (b - A x)
        for k in range(self.smoother_iters):
            if zero and k == 0:
                s.apply(b, x)
                x.scale(self.omega)
            else:
                v["r"].copy_from(b)
                a.apply(self.neg_one, x, self.one, v["r"])
                s.apply(v["r"], v["t"])
                x.add_scaled(self.omega, v["t"])
        if zero and self.smoother_iters == 0:
            x.fill(0.0)

    def _cycle(self, l, b, x, zero, vs):
        a, v = self.ops[l], vs[l]
        if l == len(self.ops) - 1:
            s = self.coarsest
            if isinstance(s, (_Sweeps, _IterativeSolver)):
                return self._smooth(s, a, b, x, zero, v)
            if zero:
                return s.apply(b, x)
            v["r"].copy_from(b)
            a.apply(self.neg_one, x, self.one, v["r"])
            s.apply(v["r"], v["t"])
            return x.add_scaled(self.one, v["t"])
        level, nxt = self.mg_levels[l], vs[l + 1]
        self._smooth(self.pre[l], a, b, x, zero, v)
        v["r"].copy_from(b)
        a.apply(self.neg_one, x, self.one, v["r"])
        level.restrict_op.apply_impl(v["r"], nxt["b"])
        self._cycle(l + 1, nxt["b"], nxt["x"], True, vs)
        if self.cycle == "w":
            self._cycle(l + 1, nxt["b"], nxt["x"], False, vs)
        level.prolong_op.add(nxt["x"], x)
        self._smooth(self.post[l], a, b, x, False, v)

    def apply_impl(self, b, x):
        if b.dtype != self.system_matrix.dtype or x.dtype != b.dtype:
            raise NotSupported("Multigrid: the vectors must have the matrix' value type")
        vs = self._level_vectors(b.size[1], b.dtype)
        zero = self.initial_guess == "zero"
        if all(c is None or c.cls is _stop.Iteration for c in self.criteria):
            # no criterion that looks at a residual: the cycles are enqueued, nothing is read back
            count = min((int(c.params["max_iters"]) for c in self.criteria if c is not None), default=1)
            for k in range(count):
                self._cycle(0, b, x, zero and k == 0, vs)
            if count == 0 and zero:
                x.fill(0.0)
            self.num_iterations = count
            return
        a = self.system_matrix
        if zero:
            x.fill(0.0)
        ex, one, neg_one, stop = self._common(b)
        r = self._vec("r", b)
        call("gkoc_ir_initialize", ex.stream, b.size[1], stop)
        r.copy_from(b)
        a.apply(neg_one, x, one, r)
        crit = _stop.combine(self.criteria, a, b, x, r)
        it = -1
        while True:
            it += 1
            if self._update_residual(crit, it, a, b, x, r, one, neg_one, stop):
                break
            self._cycle(0, b, x, False, vs)
        self._finish_stationary(it, stop, a, b, x, r, one, neg_one)
