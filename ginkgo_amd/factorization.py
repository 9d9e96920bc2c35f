"""Incomplete factorizations - mirror of include/ginkgo/core/factorization/{ilu,ic}.hpp
(factorization::Ilu / Ic; core/factorization/{ilu,ic}.cpp).

`Ilu.build().with_skip_sorting(False).on(exec).generate(csr)` works on a copy of the matrix: it sorts
the rows (unless told not to), inserts an explicit zero wherever a diagonal entry is missing
(factorization::add_diagonal_elements), computes the exact ILU(0) in place on the level schedule of the
lower triangular solve (gkoc_lower_trs_generate_* + gkoc_ilu_factorize_*) and splits the result
(factorization::initialize_row_ptrs_l_u + initialize_l_u; the column indices of the factors come from
the Sor set-up entry, which writes the same structure): `get_l_factor()` has a unit diagonal, stored
last in each row, `get_u_factor()` its diagonal first.

`Ic.build().with_both_factors(True).on(exec).generate(csr)` takes the lower triangle with its diagonal
(factorization::initialize_l) and computes the exact IC(0) in place (gkoc_ic_factorize_*):
`get_l_factor()`, and `get_lt_factor()` = its transpose (None with `with_both_factors(False)`).

Both results are bit-identical to the sequential loops stated in include/gko_cdna4.h.  Pivots are not
checked: a zero or negative pivot gives inf / NaN entries, as in the reference.

`ParIlu` / `ParIc` - mirror of include/ginkgo/core/factorization/{par_ilu,par_ic}.hpp - compute the same
factors by `with_iterations(k)` fixed-point sweeps (gkoc_par_ilu_sweeps_* / gkoc_par_ic_sweeps_*) in place of
the level schedule: one launch per sweep over all rows, no host analysis.  The preparation and the split are
those of Ilu / Ic.  The sweeps are row-synchronous and specified bit for bit (include/gko_cdna4.h): after as
many sweeps as the lower solve has levels the factors ARE the exact ones, before that they approximate them -
on the 27-point stencil to 4e-3 after 3 sweeps and 2e-4 after 5.  `with_iterations(0)`, Ginkgo's default
value, stands for DEFAULT_SWEEPS.  A departure from Ginkgo: an entry that becomes inf / NaN is written like
any other (Ginkgo keeps the old value), so that a value never depends on the history of the iteration.

`ParIlut` / `ParIct` - mirror of include/ginkgo/core/factorization/{par_ilut,par_ict}.hpp - let the factors
choose their own pattern by magnitude: `with_iterations(k)` (5) rounds of "add the pattern of L U (L L^T), give
the candidates their residual-based values, sweep, keep the `with_fill_in_limit(f)` (2.0) times nnz largest
entries of either triangle, sweep" (include/gko_cdna4.h, "ParIlut / ParIct"; gkoc_par_ilut_* / gkoc_par_ict_*,
gkoc_par_ilu_sweeps_from_* / gkoc_par_ic_sweeps_from_*; every new pattern comes from the triplet pipeline).  Bit-identical to the
restatement in tests/par_ilut_refs.py.  The selection is always exact: `with_approximate_select` and
`with_deterministic_sample` are accepted without effect.  A limit below 1.0 is refused.  Pivots are not checked;
ParIct in particular can break down where IC(0) does not (docs/KERNELS.md 43).

`Cholesky` / `Lu` - mirror of include/ginkgo/core/factorization/{cholesky,lu}.hpp (experimental::factorization) -
are the DIRECT factorizations: the pattern of L is computed on the device (symbolic Cholesky of S = pattern(A) +
pattern(A^T) + every diagonal: gkoc_symbolic_forest_* / _post_keys_* / _cholesky_count_* / _cholesky_expand_*, the
triplet pipeline makes the sorted Csr), A is placed on it with +0 elsewhere (gkoc_par_ilut_gather_*) and the
contracts of Ic / Ilu run on the filled pattern, where they ARE the Cholesky factorization and the LU factorization
without pivoting (docs/KERNELS.md 44): bit-identical to tests/factorization_refs.py on the pattern of
tests/symbolic_refs.py.  `Cholesky` reads the lower triangle of A only.  `Lu`'s combined pattern is L's row followed
by the row of L^T.  A departure from Ginkgo: `with_symbolic_algorithm` accepts "general", "near_symmetric" and
"symmetric" and all three run on the symmetrised pattern - for an unsymmetric pattern that is a superset of the
true LU fill, whose extra entries come out as exact zeros.  `with_symbolic_factorization(csr)` takes a given
pattern instead (for Cholesky its lower triangle); it is checked for square shape, sorted rows and stored diagonals
only, and an entry of A outside it is dropped - with A's own pattern the result is Ilu's / Ic's.  Pivots are not
checked and nothing is permuted: a zero pivot (negative for Cholesky) gives inf / NaN entries as in Ilu / Ic.  The
factorizations keep the order they are given: in natural order the 27-point stencil's forest is a chain, so the
fill is large and the numeric phase has n levels.  A fill-reducing ordering comes from outside:
reorder.NestedDissection computes one, Csr.permute applies it, and reorder.ScaledReordered wraps Direct (or any
solver) in it (docs/KERNELS.md 45 says what it buys).
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import IT, VT, DimensionMismatch, GkoError, NotSupported, call, lib
from .executor import MEM_INDICES, MEM_VALUES
from .isai import _lower_pattern
from .matrix import Csr, DeviceMatrixData, Fbcsr, _np_dtype, entry_dtype


def row_limits():
    """the row lengths at which the factorization kernels change path (gkoc_factorization_row_limits)"""
    return _lib.row_limits("gkoc_factorization_row_limits")


def symbolic_row_limits():
    """the numbers of strictly-lower entries of a row at which the symbolic kernels change path
    (gkoc_symbolic_row_limits)"""
    return _lib.row_limits("gkoc_symbolic_row_limits")


class _Factory:
    def __init__(self, cls):
        self.cls = cls
        self.skip_sorting = False
        self.both_factors = True
        self.exec = None

    def with_skip_sorting(self, v):
        self.skip_sorting = bool(v)
        return self

    def on(self, exec_):
        self.exec = exec_
        return self

    def generate(self, system_matrix):
        if isinstance(system_matrix, Fbcsr):
            # any other matrix type goes through convert_to(Csr), as for Sor
            csr = system_matrix.convert_to_csr()
            fact = self.cls(self, csr)
            csr.exec.synchronize()      # the converted copy is released on return
            return fact
        return self.cls(self, system_matrix)


class _IcFactory(_Factory):
    def with_both_factors(self, v):
        self.both_factors = bool(v)
        return self


# The sweeps of ParIlu / ParIc when the factory says 0 (Ginkgo's "pick for me").  A design choice: on the
# 27-point stencil the largest relative error of an entry is 1e-1, 2e-2, 4e-3, 2e-4 after 1, 2, 3, 5 sweeps,
# and PCG with the IC factor of 3 sweeps already needs the iterations of the exact one.
DEFAULT_SWEEPS = 5


class _SweepsMixin:
    """with_iterations of the two Par* factories"""
    iterations = 0

    def with_iterations(self, v):
        if int(v) < 0:
            raise GkoError("with_iterations needs a number of sweeps >= 0 (0: the default, DEFAULT_SWEEPS)")
        self.iterations = int(v)
        return self


class _ParFactory(_SweepsMixin, _Factory):
    pass


class _ParIcFactory(_SweepsMixin, _IcFactory):
    pass


class _ThresholdMixin:
    """the parameters of the two threshold factories (par_ilut.hpp / par_ict.hpp), Ginkgo's defaults"""
    iterations = 5
    fill_in_limit = 2.0
    approximate_select = True
    deterministic_sample = False

    def with_iterations(self, v):
        if int(v) < 1:
            raise GkoError("with_iterations needs at least one iteration")
        self.iterations = int(v)
        return self

    def with_fill_in_limit(self, v):
        if not float(v) >= 1.0:
            raise GkoError(f"with_fill_in_limit needs a limit >= 1.0, got {v}: the factors hold at least the "
                           "entries of the system matrix")
        self.fill_in_limit = float(v)
        return self

    def with_approximate_select(self, v):
        """accepted for API compatibility: the selection is always exact"""
        self.approximate_select = bool(v)
        return self

    def with_deterministic_sample(self, v):
        """accepted for API compatibility: nothing is sampled"""
        self.deterministic_sample = bool(v)
        return self


class _ParIlutFactory(_ThresholdMixin, _Factory):
    pass


class _ParIctFactory(_ThresholdMixin, _IcFactory):
    pass


class _DirectMixin:
    """with_symbolic_factorization of the two direct factories"""
    symbolic = None

    def with_symbolic_factorization(self, pattern):
        """a Csr whose pattern is used instead of the computed fill pattern (None: compute it)"""
        if pattern is not None and not isinstance(pattern, Csr):
            raise NotSupported("with_symbolic_factorization takes a Csr (its values are not read) or None")
        self.symbolic = pattern
        return self


class _CholeskyFactory(_DirectMixin, _IcFactory):
    pass


SYMBOLIC_ALGORITHMS = ("general", "near_symmetric", "symmetric")


class _LuFactory(_DirectMixin, _Factory):
    symbolic_algorithm = "general"

    def with_symbolic_algorithm(self, name):
        """accepted for API compatibility: every algorithm runs on the symmetrised pattern"""
        if name not in SYMBOLIC_ALGORITHMS:
            raise GkoError(f"with_symbolic_algorithm: {name!r} is none of {SYMBOLIC_ALGORITHMS}")
        self.symbolic_algorithm = name
        return self


def keep_counts(fill_in_limit, n_lower, n_upper):
    """(keep_L, keep_U): the entries a triangle of the threshold factors may hold beside ties"""
    return tuple(max(1, int(math.floor(fill_in_limit * count))) for count in (n_lower, n_upper))


class _Factorization:
    """the work shared by Ilu and Ic: checks, the sorted copy with every diagonal stored, the schedule"""

    def __init__(self, factory, a):
        name = type(self).__name__
        if not isinstance(a, Csr):
            raise NotSupported(f"factorization.{name}.generate needs a Csr system matrix")
        if a.size[0] != a.size[1]:
            raise DimensionMismatch(f"factorization.{name} needs a square matrix")
        if a.dtype not in VT:
            raise NotSupported(f"factorization.{name}: real value types only")
        self.exec = factory.exec or a.exec
        self.size = a.size
        self.dtype = a.dtype
        self._idx = a.col_idxs.dtype
        self._it = IT[a.col_idxs.dtype]
        self._suf = f"{VT[a.dtype]}_{self._it}"

    def _prepared(self, factory, a):
        """a sorted copy of `a` in which every row stores its diagonal"""
        ex, n = self.exec, self.size[0]
        work = Csr(ex, a.size, a.values.clone(), a.col_idxs.clone(), a.row_ptrs, a.strategy)
        if not factory.skip_sorting and not work.is_sorted_by_column_index():
            work.sort_by_column_index()
        idx = a.row_ptrs.dtype
        shift, missing = ex.alloc((n + 1,), idx, MEM_INDICES), C.c_int64(0)
        call("gkoc_csr_missing_diagonal_shift_" + self._it, ex.stream, n, n, work.row_ptrs, work.col_idxs,
             shift, C.byref(missing))
        if missing.value:
            nnz = work.values.numel() + missing.value
            rp, ci = ex.alloc((n + 1,), idx, MEM_INDICES), ex.alloc((nnz,), idx, MEM_INDICES)
            v = ex.alloc((nnz,), a.dtype, MEM_VALUES)
            call("gkoc_csr_add_diagonal_fill_" + self._suf, ex.stream, n, work.row_ptrs, work.col_idxs,
                 work.values, shift, rp, ci, v)
            ex.synchronize()            # `shift` and the unfilled copy are released here
            work = Csr(ex, a.size, v, ci, rp, a.strategy)
        return work

    def _factorize(self, entry, m):
        """the lower solve's level schedule of `m`, then the in-place factorization on it"""
        ex, n = self.exec, self.size[0]
        handle = C.c_void_p()
        call("gkoc_lower_trs_generate_" + self._it, ex.stream, n, m.row_ptrs, m.col_idxs, C.byref(handle))
        try:
            call(entry + self._suf, ex.stream, handle, n, m.row_ptrs, m.col_idxs, m.values)
        finally:
            lib().gkoc_trs_struct_destroy(handle)

    def _split(self, m, with_u, diag_sqrt=False):
        """the factors of the split of `m` as Csr: L (strictly-lower entries, then 1 or the diagonal) and,
        with_u, U (the diagonal, then the strictly-upper entries).  The index arrays are the ones of the
        Sor set-up (weight 1); the new entries write the values"""
        ex, n = self.exec, self.size[0]
        idx = m.row_ptrs.dtype
        l_rp = ex.alloc((n + 1,), idx, MEM_INDICES)
        u_rp = ex.alloc((n + 1,), idx, MEM_INDICES) if with_u else None
        call("gkoc_factorization_initialize_row_ptrs_l_u_" + self._it, ex.stream, n, m.row_ptrs, m.col_idxs,
             l_rp, u_rp)
        out = []
        for rp in (l_rp, u_rp) if with_u else (l_rp,):
            nnz = int(rp[-1].item())
            out += [rp, ex.alloc((nnz,), idx, MEM_INDICES), ex.alloc((nnz,), m.dtype, MEM_VALUES)]
        src = (ex.stream, n, m.row_ptrs, m.col_idxs, m.values)
        if with_u:
            l_rp, l_ci, l_v, u_rp, u_ci, u_v = out
            call("gkoc_sor_initialize_weighted_l_u_" + self._suf, *src, C.c_double(1.0), l_rp, l_ci, l_v,
                 u_rp, u_ci, u_v)
            call("gkoc_factorization_initialize_l_u_" + self._suf, *src, l_rp, l_v, u_rp, u_v)
            return Csr(ex, self.size, l_v, l_ci, l_rp), Csr(ex, self.size, u_v, u_ci, u_rp)
        l_rp, l_ci, l_v = out
        call("gkoc_sor_initialize_weighted_l_" + self._suf, *src, C.c_double(1.0), l_rp, l_ci, l_v)
        call("gkoc_factorization_initialize_l_" + self._suf, *src, l_rp, l_v, C.c_int(int(diag_sqrt)))
        return Csr(ex, self.size, l_v, l_ci, l_rp)

    def _sweeps(self, entry, factory, m):
        """`iterations` fixed-point sweeps on the values of `m`: a Csr on m's index arrays with the result.
        No schedule: one launch per sweep."""
        ex, n = self.exec, self.size[0]
        self.iterations = factory.iterations or DEFAULT_SWEEPS
        nnz = m.values.numel()
        out = ex.alloc((nnz,), m.dtype, MEM_VALUES)
        work = ex.alloc((nnz,), m.dtype, MEM_VALUES) if self.iterations > 1 else None
        # the entry's counter is a uint64; a count of entries reads the same through an int64 tensor
        self._changed_dev, self._changed = ex.alloc((1,), torch.int64), None
        call(entry + self._suf, ex.stream, n, nnz, m.row_ptrs, m.col_idxs, m.values, self.iterations, work, out,
             self._changed_dev)
        return Csr(ex, m.size, out, m.col_idxs, m.row_ptrs, m.strategy)

    # ---- ParIlut / ParIct: one iteration of the threshold loop (include/gko_cdna4.h, steps 1-6)
    def _product_pattern(self, left, right, a):
        """(row_ptrs, col_idxs) of pattern(left * right) + pattern(a), rows sorted: the product's triplets with
        D = a through the triplet pipeline, all values 1 (nothing cancels, the pipeline drops no zero)"""
        ex, n, dt = self.exec, self.size[0], a.dtype
        ones = [ex.alloc((m.values.numel(),), dt).fill_(1) for m in (left, right, a)]
        offsets, total = ex.alloc((n + 1,), torch.int64), C.c_int64(0)
        call("gkoc_csr_spgemm_count_" + self._it, ex.stream, n, left.row_ptrs, left.col_idxs, right.row_ptrs,
             a.row_ptrs, offsets, C.byref(total))
        t = max(total.value, 1)
        rows, cols = ex.alloc((t,), a.col_idxs.dtype), ex.alloc((t,), a.col_idxs.dtype)
        vals = ex.alloc((t,), dt)
        call("gkoc_csr_spgemm_expand_" + self._suf, ex.stream, n, None, left.row_ptrs, left.col_idxs, ones[0],
             right.row_ptrs, right.col_idxs, ones[1], None, a.row_ptrs, a.col_idxs, ones[2], offsets, rows, cols,
             vals)
        data = DeviceMatrixData(ex, a.size, rows[:total.value], cols[:total.value], vals[:total.value])
        data.sum_duplicates()
        rp = Csr.read(data).row_ptrs
        ex.synchronize()                # the triplets and the ones are released on return
        return rp, data.col_idxs

    def _gather(self, rp, ci, src):
        """the values of the sorted Csr `src` at the positions of the pattern, +0 where it stores none"""
        ex = self.exec
        out = ex.alloc((ci.numel(),), src.dtype)
        call("gkoc_par_ilut_gather_" + self._suf, ex.stream, self.size[0], ci.numel(), rp, ci,
             src.values.numel(), src.row_ptrs, src.col_idxs, src.values, out)
        return out

    def _sweep_from(self, entry, rp, ci, a_vals, v0):
        out = self.exec.alloc((ci.numel(),), v0.dtype)
        call(entry + self._suf, self.exec.stream, self.size[0], ci.numel(), rp, ci, a_vals, v0, 1, None, out, None)
        return out

    def _threshold_iteration(self, lower_only, a, src, m, keep):
        """M_t from M_{t-1} = m.  a: the prepared matrix; src: what the sweeps take as their input values (a,
        or its lower triangle for ict); keep: (keep_L, keep_U)"""
        ex, n, suf = self.exec, self.size[0], self._suf
        if lower_only:
            rp, ci = self._product_pattern(m, m.transpose(), a)
            rp, ci = _lower_pattern(ex, self.size, rp, ci, a.dtype)
            candidates, sweeps = "gkoc_par_ict_candidate_values_", "gkoc_par_ic_sweeps_from_"
        else:
            l, u = self._split(m, True)
            rp, ci = self._product_pattern(l, u, a)
            candidates, sweeps = "gkoc_par_ilut_candidate_values_", "gkoc_par_ilu_sweeps_from_"
        nnz = ci.numel()
        v0 = ex.alloc((nnz,), a.dtype)
        call(candidates + suf, ex.stream, n, nnz, rp, ci, a.values.numel(), a.row_ptrs, a.col_idxs, a.values,
             m.values.numel(), m.row_ptrs, m.col_idxs, m.values, v0)
        v = self._sweep_from(sweeps, rp, ci, self._gather(rp, ci, src), v0)
        # the thresholds stay on the device: the select reads nothing back
        f = lib().gkoc_par_ilut_select_workspace_bytes
        f.restype = C.c_size_t
        work = ex.alloc((int(f()),), torch.uint8)
        thr = ex.alloc((2,), a.dtype)
        for part in (0,) if lower_only else (0, 1):
            call("gkoc_par_ilut_threshold_select_" + suf, ex.stream, n, rp, ci, v, C.c_int(part), keep[part],
                 work, C.c_size_t(work.numel()), thr[part:part + 1])
        mask = ex.alloc((nnz,), a.dtype)
        call("gkoc_par_ilut_keep_mask_" + suf, ex.stream, n, nnz, rp, ci, v, thr[0:1],
             None if lower_only else thr[1:2], mask)
        rows = ex.alloc((nnz,), ci.dtype)
        call("gkoc_convert_ptrs_to_idxs_" + self._it, ex.stream, rp, n, rows)
        data = DeviceMatrixData(ex, self.size, rows, ci, mask).remove_zeros()
        kept_rp, kept_ci = Csr.read(data).row_ptrs, data.col_idxs
        out = self._sweep_from(sweeps, kept_rp, kept_ci, self._gather(kept_rp, kept_ci, src),
                               self._gather(kept_rp, kept_ci, Csr(ex, self.size, v, ci, rp)))
        ex.synchronize()                # the iteration's buffers are released on return
        return Csr(ex, self.size, out, kept_ci, kept_rp)

    def _threshold_loop(self, factory, lower_only, a, src, m):
        self.iterations, self.fill_in_limit = factory.iterations, factory.fill_in_limit
        # the sizes of A's triangles from the row pointers of its split: each ends at the triangle + a diagonal
        ex, n = self.exec, self.size[0]
        l_rp, u_rp = ex.alloc((n + 1,), a.row_ptrs.dtype), ex.alloc((n + 1,), a.row_ptrs.dtype)
        call("gkoc_factorization_initialize_row_ptrs_l_u_" + self._it, ex.stream, n, a.row_ptrs, a.col_idxs,
             l_rp, u_rp)
        self.keep = keep_counts(self.fill_in_limit, int(l_rp[-1].item()) - n, int(u_rp[-1].item()) - n)
        for _ in range(self.iterations):
            m = self._threshold_iteration(lower_only, a, src, m, self.keep)
        return m

    # ---- Cholesky / Lu: the symbolic phase (include/gko_cdna4.h, "Symbolic Cholesky / sparse direct")
    def _union_pattern(self, patterns):
        """(row_ptrs, col_idxs) of the union of the sorted patterns [(rp, ci), ...]: their triplets side by side
        through the triplet pipeline, all values 1"""
        ex, n, idx = self.exec, self.size[0], patterns[0][1].dtype
        total = sum(ci.numel() for _, ci in patterns)
        rows, cols = ex.alloc((total,), idx), ex.alloc((total,), idx)
        at = 0
        for rp, ci in patterns:
            call("gkoc_convert_ptrs_to_idxs_" + self._it, ex.stream, rp, n, rows[at:at + ci.numel()])
            cols[at:at + ci.numel()].copy_(ci)
            at += ci.numel()
        data = DeviceMatrixData(ex, self.size, rows, cols, ex.alloc((total,), self.dtype).fill_(1))
        data.sum_duplicates()
        rp = Csr.read(data).row_ptrs
        ex.synchronize()                # the triplets are released on return
        return rp, data.col_idxs

    def _symmetrized_lower(self, m):
        """the lower triangle, diagonal last, of S = pattern(m) + pattern(m^T) for the prepared matrix m"""
        ex = self.exec
        mt = m.transpose()
        return self._union_pattern([_lower_pattern(ex, self.size, x.row_ptrs, x.col_idxs, self.dtype)
                                    for x in (m, mt)])

    def _symbolic_cholesky(self, s_rp, s_ci):
        """(row_ptrs, col_idxs) of L, rows sorted, from the lower triangle of S: the forest on the host, the rows
        by the skeleton walk on the device, the sorted pattern from the triplet pipeline"""
        ex, n, it, idx = self.exec, self.size[0], self._it, s_ci.dtype
        nnz = s_ci.numel()
        parent, post, first, inv_post = (ex.alloc((n,), idx) for _ in range(4))
        call("gkoc_symbolic_forest_" + it, ex.stream, n, nnz, s_rp, s_ci, parent, post, first)
        keys = ex.alloc((nnz,), idx)
        call("gkoc_symbolic_post_keys_" + it, ex.stream, n, nnz, s_rp, s_ci, post, keys, inv_post)
        # the row sort orders every row's neighbours by post rank; its values are not read afterwards
        Csr(ex, self.size, ex.zeros((nnz,), self.dtype), keys, s_rp).sort_by_column_index()
        offsets, total = ex.alloc((n + 1,), torch.int64), C.c_longlong(0)
        forest = (ex.stream, n, nnz, s_rp, keys, parent, post, first, inv_post)
        call("gkoc_symbolic_cholesky_count_" + it, *forest, offsets, C.byref(total))
        # the pattern leaves as matrix_data entries (row, col, 1); the triplet pipeline takes them from there
        t = total.value
        width = entry_dtype(_np_dtype(self.dtype), _np_dtype(idx)).itemsize
        entries = ex.alloc((t * width,), torch.uint8)
        call("gkoc_symbolic_cholesky_expand_" + self._suf, *forest, offsets, t, entries)
        rows, cols, vals = ex.alloc((t,), idx), ex.alloc((t,), idx), ex.alloc((t,), self.dtype)
        call("gkoc_aos_to_soa_" + self._suf, ex.stream, t, entries, rows, cols, vals)
        data = DeviceMatrixData(ex, self.size, rows, cols, vals)
        data.sort_row_major()
        rp = Csr.read(data).row_ptrs
        ex.synchronize()                # the forest, the keys and the offsets are released on return
        return rp, data.col_idxs

    def _given_pattern(self, pattern, skip_sorting):
        """the index arrays of a caller's pattern after the three checks it gets"""
        name = type(self).__name__
        if tuple(pattern.size) != tuple(self.size):
            raise DimensionMismatch(f"factorization.{name}: the symbolic factorization is {tuple(pattern.size)}, "
                                    f"the system matrix {tuple(self.size)}")
        if pattern.col_idxs.dtype != self._idx:
            raise NotSupported(f"factorization.{name}: the symbolic factorization has another index type")
        if not skip_sorting and not pattern.is_sorted_by_column_index():
            raise GkoError(f"factorization.{name}: the rows of the symbolic factorization are not sorted")
        ex, n = self.exec, self.size[0]
        shift, missing = ex.alloc((n + 1,), self._idx), C.c_int64(0)
        call("gkoc_csr_missing_diagonal_shift_" + self._it, ex.stream, n, n, pattern.row_ptrs, pattern.col_idxs,
             shift, C.byref(missing))
        if missing.value:
            raise GkoError(f"factorization.{name}: {missing.value} rows of the symbolic factorization store no "
                           "diagonal entry")
        return pattern.row_ptrs, pattern.col_idxs

    def _in_matrix_memory(self, rp, ci, values):
        """a Csr on copies of the three arrays where a matrix' read-only arrays belong (the originals live with
        the vectors)"""
        ex, idx = self.exec, ci.dtype
        m_rp, m_ci = ex.alloc((rp.numel(),), idx, MEM_INDICES), ex.alloc((ci.numel(),), idx, MEM_INDICES)
        m_v = ex.alloc((ci.numel(),), values.dtype, MEM_VALUES)
        m_rp.copy_(rp)
        m_ci.copy_(ci)
        m_v.copy_(values)
        return Csr(ex, self.size, m_v, m_ci, m_rp)

    def _on_pattern(self, rp, ci, src):
        """a Csr on a copy of the pattern in the matrix' memory classes, with the values of `src` gathered"""
        return self._in_matrix_memory(rp, ci, self._gather(rp, ci, src))

    def last_sweep_changes(self):
        """the number of entries whose bits the last sweep changed; 0: the factors are a fixed point of the
        sweep, which is the exact factorization.  Read back from the device on first use."""
        if self._changed is None:
            self.exec.synchronize()
            self._changed = int(self._changed_dev.item())
        return self._changed

    def get_executor(self):
        return self.exec

    def get_size(self):
        return self.size


class _LuFactors(_Factorization):
    """the accessors of a factorization A ~ L U"""

    def get_l_factor(self):
        return self.l

    def get_u_factor(self):
        return self.u


class _LltFactors(_Factorization):
    """the accessors of a factorization A ~ L L^T, and the transpose it keeps unless the factory says no"""

    def _keep_l(self, factory, l):
        self.l = l
        self.both_factors = factory.both_factors
        self.lt = self.l.transpose() if self.both_factors else None

    def get_l_factor(self):
        return self.l

    def get_lt_factor(self):
        return self.lt


class Ilu(_LuFactors):
    """A ~ L U on the pattern of A: L unit lower triangular, U upper triangular (exact ILU(0))."""

    @staticmethod
    def build():
        return _Factory(Ilu)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        ex = self.exec
        m = self._prepared(factory, a)
        self._factorize("gkoc_ilu_factorize_", m)
        self.l, self.u = self._split(m, True)
        ex.synchronize()                # the factored copy is released on return


class Ic(_LltFactors):
    """A ~ L L^T on the pattern of A's lower triangle (exact IC(0))."""

    @staticmethod
    def build():
        return _IcFactory(Ic)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        ex = self.exec
        m = self._prepared(factory, a)
        l = self._split(m, False)
        self._factorize("gkoc_ic_factorize_", l)
        self._keep_l(factory, l)
        ex.synchronize()                # the prepared copy is released on return


class ParIlu(_LuFactors):
    """A ~ L U on the pattern of A by `iterations` fixed-point sweeps; the exact ILU(0) once the sweeps reach
    the number of levels of the lower solve, an approximation of it before."""

    @staticmethod
    def build():
        return _ParFactory(ParIlu)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        ex = self.exec
        m = self._prepared(factory, a)
        self.l, self.u = self._split(self._sweeps("gkoc_par_ilu_sweeps_", factory, m), True)
        ex.synchronize()                # the prepared copy and the sweeps' buffers are released on return


class ParIc(_LltFactors):
    """A ~ L L^T on the pattern of A's lower triangle by `iterations` fixed-point sweeps; the exact IC(0) once
    the sweeps reach the number of levels of the lower solve, an approximation of it before."""

    @staticmethod
    def build():
        return _ParIcFactory(ParIc)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        ex = self.exec
        m = self._prepared(factory, a)
        self._keep_l(factory, self._sweeps("gkoc_par_ic_sweeps_", factory, self._split(m, False)))
        ex.synchronize()                # the prepared copy and the sweeps' buffers are released on return


class ParIlut(_LuFactors):
    """A ~ L U on a pattern the factorization chooses by magnitude: `iterations` rounds of "add the pattern of
    L U, sweep, keep the fill_in_limit * nnz largest entries of either triangle, sweep" (steps 1-6 of
    include/gko_cdna4.h).  `keep` holds the two limits."""

    @staticmethod
    def build():
        return _ParIlutFactory(ParIlut)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        ex = self.exec
        m = self._prepared(factory, a)
        self.l, self.u = self._split(self._threshold_loop(factory, False, m, m, m), True)
        ex.synchronize()                # the prepared copy and the last iterate are released on return


class ParIct(_LltFactors):
    """A ~ L L^T on a pattern the factorization chooses by magnitude: the loop of ParIlut on the lower
    triangle, with one limit."""

    @staticmethod
    def build():
        return _ParIctFactory(ParIct)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        ex = self.exec
        m = self._prepared(factory, a)
        last = self._threshold_loop(factory, True, m, self._split(m, False), self._split(m, False, diag_sqrt=True))
        # the iterate's arrays live with the vectors; the factor's go where a matrix' read-only arrays belong
        self._keep_l(factory, self._in_matrix_memory(last.row_ptrs, last.col_idxs, last.values))
        ex.synchronize()                # the prepared copy and the last iterate are released on return


class Cholesky(_LltFactors):
    """A = L L^T exactly, up to rounding: the contract of Ic on the pattern of L that the symbolic phase computes
    (or that `with_symbolic_factorization` gives).  Reads the lower triangle of A."""

    @staticmethod
    def build():
        return _CholeskyFactory(Cholesky)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        ex = self.exec
        m = self._prepared(factory, a)
        if factory.symbolic is None:
            rp, ci = self._symbolic_cholesky(*self._symmetrized_lower(m))
        else:
            rp, ci = _lower_pattern(ex, self.size, *self._given_pattern(factory.symbolic, factory.skip_sorting),
                                    self.dtype)
        l = self._on_pattern(rp, ci, self._split(m, False))
        self._factorize("gkoc_ic_factorize_", l)
        self._keep_l(factory, l)
        self._symbolic = None
        ex.synchronize()                # the prepared copy and the pattern's first copy are released on return

    def get_symbolic(self):
        """the pattern of L as a Csr of ones on the factor's own index arrays"""
        if self._symbolic is None:
            ones = self.exec.alloc((self.l.values.numel(),), self.dtype, MEM_VALUES).fill_(1)
            self._symbolic = Csr(self.exec, self.size, ones, self.l.col_idxs, self.l.row_ptrs)
        return self._symbolic


class Lu(_LuFactors):
    """A = L U exactly, up to rounding, without pivoting: the contract of Ilu on the combined pattern - row i of
    the symbolic Cholesky factor of the symmetrised pattern, then row i of its transpose - or on the pattern that
    `with_symbolic_factorization` gives.  L has a unit diagonal, stored last; U its diagonal first."""

    @staticmethod
    def build():
        return _LuFactory(Lu)

    def __init__(self, factory, a):
        super().__init__(factory, a)
        ex = self.exec
        self.symbolic_algorithm = factory.symbolic_algorithm
        m = self._prepared(factory, a)
        if factory.symbolic is None:
            rp, ci = self._symbolic_cholesky(*self._symmetrized_lower(m))
            low = Csr(ex, self.size, ex.alloc((ci.numel(),), self.dtype).fill_(1), ci, rp)
            up = low.transpose()
            # both hold the diagonal: the pipeline keeps one
            rp, ci = self._union_pattern([(low.row_ptrs, low.col_idxs), (up.row_ptrs, up.col_idxs)])
        else:
            rp, ci = self._given_pattern(factory.symbolic, factory.skip_sorting)
        self.combined = self._on_pattern(rp, ci, m)
        self._factorize("gkoc_ilu_factorize_", self.combined)
        self.l, self.u = self._split(self.combined, True)
        ex.synchronize()                # the prepared copy and the pattern's first copy are released on return

    def get_combined(self):
        """the factored matrix on the combined pattern: L strictly below the diagonal, U on and above it"""
        return self.combined
