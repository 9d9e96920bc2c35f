"""The batched classes on the device against the numpy restatement of tests/batch_refs.py.  The kernels promise the
restatement's rounding, so x, iteration counts, residual norms and converged flags are compared with
np.array_equal (NaN equal to NaN: an item that breaks down is NaN in both).  Shapes are the smallest that can
still go wrong: the widths of the reduction and one row to either side, more items than compute units, and the
system sizes at which gkoc_batch_plan changes what lives in LDS."""
import numpy as np
import pytest
import torch

import batch_refs as R
import ginkgo_amd as g
from ginkgo_amd import _lib, batch

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
DTYPE_IDS = ["f64", "f32"]
SOLVER_CLS = {"cg": batch.Cg, "bicgstab": batch.Bicgstab}
# one row to either side of the sizes at which W changes (64 | 128 | 256 | 512) and of the widths themselves
WIDTH_EDGES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769]
_REFS = {}      # reference solves, computed once per key; the tests do not change them


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def device_matrix(ex, fmt, pat, vals, stride=None):
    """-> the batch matrix on the device and the (pattern, values) the reference multiplies with"""
    if fmt == "csr":
        return batch.Csr.from_numpy(ex, pat.size, pat.rp.astype(np.int32), pat.ci.astype(np.int32), vals), pat, vals
    ell, evals = R.csr_to_ell(pat, vals, stride)
    return batch.Ell.from_numpy(ex, pat.size, ell.cols.astype(np.int32), evals, ell.k, ell.stride), ell, evals


def test_widths_follow_the_plan():
    for n in WIDTH_EDGES:
        assert batch.plan("cg", "csr", None, "f64", n, 3 * n).w == R.width(n)
    assert sorted({R.width(n) for n in WIDTH_EDGES}) == [64, 128, 256, 512]
    assert all(w - 1 in WIDTH_EDGES and w in WIDTH_EDGES and w + 1 in WIDTH_EDGES for w in (64, 128, 256, 512, 768))


# ------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("fmt", ["csr", "ell"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_apply(gexec, fmt, dtype):
    """random unsorted patterns with empty rows, Ell padding inside rows and (stride > rows) behind them; cols 1 and
    3 with row strides larger than cols; 1, 3 and 300 items; simple and advanced with per-item alpha and beta"""
    rng = np.random.default_rng(11)
    shapes = [(n, 3, 3) for n in WIDTH_EDGES] + [(65, 1, 1), (65, 1, 3), (65, 300, 1), (65, 300, 3), (129, 3, 1)]
    for n, items, cols in shapes:
        n_cols = n + 2
        pat = R.random_pattern(n, n_cols, min(1.0, 6.0 / n_cols), n, empty_rows=(n // 2,) if n > 2 else ())
        vals = rng.uniform(-1, 1, (items, pat.stored)).astype(dtype)
        a, rpat, rvals = device_matrix(gexec, fmt, pat, vals, stride=n + 3)
        assert a.num_items == items and a.size == (n, n_cols)
        b = rng.uniform(-1, 1, (items, n_cols, cols)).astype(dtype)
        x0 = rng.uniform(-1, 1, (items, n, cols)).astype(dtype)
        alpha, beta = rng.uniform(-1, 1, items).astype(dtype), rng.uniform(-1, 1, items).astype(dtype)
        db = batch.MultiVector.from_numpy(gexec, b, stride=cols + 2)
        dx = batch.MultiVector.from_numpy(gexec, x0, stride=cols + 1)
        assert a.apply(db, dx) is dx
        assert same(dx.to_numpy(), R.product(rpat, rvals, b)), (n, items, cols)
        dx = batch.MultiVector.from_numpy(gexec, x0, stride=cols + 1)
        a.apply(batch.MultiVector.from_numpy(gexec, alpha.reshape(-1, 1, 1)), db,
                batch.MultiVector.from_numpy(gexec, beta.reshape(-1, 1, 1)), dx)
        assert same(dx.to_numpy(), R.advanced_product(rpat, rvals, alpha, b, beta, x0)), (n, items, cols)
        assert same(db.to_numpy(), b)
    with pytest.raises(g.DimensionMismatch):
        a.apply(dx, dx)
    with pytest.raises(g.DimensionMismatch):
        a.apply(db, batch.MultiVector.create(gexec, items + 1, (n, cols), torch.from_numpy(x0).dtype))


# ------------------------------------------------------------------------------------------ multi-vector
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_multi_vector_blas(gexec, dtype):
    rng = np.random.default_rng(12)
    for n in WIDTH_EDGES + [2000]:
        for items, cols in ((3, 3), (300, 1)) if n in (65, 2000) else ((3, 3),):
            u = rng.uniform(-1, 1, (items, n, cols)).astype(dtype)
            v = rng.uniform(-1, 1, (items, n, cols)).astype(dtype)
            du = batch.MultiVector.from_numpy(gexec, u, stride=cols + 2)
            dv = batch.MultiVector.from_numpy(gexec, v, stride=cols + 1)
            out = batch.MultiVector.create(gexec, items, (1, cols), du.dtype)
            w = R.width(n)
            ut, vt = np.swapaxes(u, 1, 2), np.swapaxes(v, 1, 2)          # items x cols x n
            assert same(du.compute_dot(dv, out).to_numpy()[:, 0, :], R.dot(ut, vt, w)), n
            assert same(du.compute_norm2(out).to_numpy()[:, 0, :], R.nrm(ut, w)), n
            for acols in sorted({1, cols}):                              # one scalar per item, one per column
                al = rng.uniform(-1, 1, (items, 1, acols)).astype(dtype)
                dal = batch.MultiVector.from_numpy(gexec, al)
                dx = batch.MultiVector.from_numpy(gexec, u, stride=cols + 2)
                assert same(dx.scale(dal).to_numpy(), al * u)
                assert same(dx.add_scaled(dal, dv).to_numpy(), al * u + al * v)
            assert same(dv.to_numpy(), v)
    with pytest.raises(g.DimensionMismatch):
        du.scale(batch.MultiVector.create(gexec, items, (1, cols + 1), du.dtype))
    with pytest.raises(g.DimensionMismatch):
        du.compute_dot(dv, batch.MultiVector.create(gexec, items, (1, cols + 1), du.dtype))


def test_multi_vector_views_alias(gexec):
    v = batch.MultiVector.from_numpy(gexec, np.arange(24.0).reshape(3, 4, 2), stride=3)
    assert v.get_num_batch_items() == 3 and v.get_common_size() == (4, 2) and v.ld == 3
    one = v.create_view_for_item(1)
    assert isinstance(one, g.Dense) and one.size == (4, 2) and one.values.data_ptr() == v.values[1].data_ptr()
    one.values.zero_()
    assert not v.to_numpy()[1].any() and v.to_numpy()[0].any() and v.to_numpy()[2].all()


# ------------------------------------------------------------------------------------------ conversions
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_conversions_round_trip(gexec, dtype):
    """Csr -> Ell -> Csr returns the original values bit for bit; the item views alias the batch storage"""
    rng = np.random.default_rng(13)
    for n, items in ((1, 2), (37, 5), (257, 3)):
        pat = R.random_pattern(n, n + 2, min(1.0, 6.0 / (n + 2)), n + 7, empty_rows=(n // 2,) if n > 2 else ())
        vals = rng.uniform(-1, 1, (items, pat.stored)).astype(dtype)
        a = batch.Csr.from_numpy(gexec, pat.size, pat.rp.astype(np.int32), pat.ci.astype(np.int32), vals)
        ell = a.convert_to_ell()
        rell, rvals = R.csr_to_ell(pat, vals)
        assert isinstance(ell, batch.Ell) and (ell.num_stored_per_row, ell.stride) == (rell.k, rell.stride)
        assert np.array_equal(ell.col_idxs.cpu().numpy().reshape(rell.k, rell.stride), rell.cols)
        assert same(ell.values.cpu().numpy(), rvals)
        back = ell.convert_to_csr()
        assert np.array_equal(back.row_ptrs.cpu().numpy(), pat.rp) and np.array_equal(back.col_idxs.cpu().numpy(), pat.ci)
        assert same(back.values.cpu().numpy(), vals)
        for m, cls in ((a, g.Csr), (ell, g.Ell)):
            view = m.create_view_for_item(items - 1)
            assert isinstance(view, cls) and view.size == m.size
            assert view.values.data_ptr() == m.values[items - 1].data_ptr()
            assert view.col_idxs.data_ptr() == m.col_idxs.data_ptr()
    # padding in the middle of a row: slot 0 of row 1 is empty
    cols = np.array([[0, -1, 2], [1, 0, -1]], np.int32)
    evals = rng.uniform(-1, 1, (2, 6)).astype(dtype)
    ell = batch.Ell.from_numpy(gexec, (3, 3), cols, evals, 2, 3)
    rcsr, rvals = R.ell_to_csr(R.EllPattern(3, 3, cols, 2, 3), evals)
    csr = ell.convert_to_csr()
    assert np.array_equal(csr.row_ptrs.cpu().numpy(), rcsr.rp) and np.array_equal(csr.col_idxs.cpu().numpy(), rcsr.ci)
    assert same(csr.values.cpu().numpy(), rvals)


def test_from_matrices_and_duplicate(gexec):
    pat, vals = R.tridiagonal(9, 3, np.float64, seed=1)
    singles = [g.Csr.from_arrays(gexec, (9, 9), pat.rp.astype(np.int32), pat.ci.astype(np.int32), vals[i]) for i in range(3)]
    a = batch.Csr.from_matrices(singles)
    assert a.num_items == 3 and same(a.values.cpu().numpy(), vals)
    d = batch.Csr.duplicate(singles[1], 4)
    assert d.num_items == 4 and same(d.values.cpu().numpy(), np.repeat(vals[1:2], 4, axis=0))
    other = g.Csr.from_arrays(gexec, (9, 9), pat.rp.astype(np.int32), np.roll(pat.ci, 1).astype(np.int32), vals[0])
    with pytest.raises(g.GkoError, match="sparsity pattern"):
        batch.Csr.from_matrices([singles[0], other])
    e = batch.Ell.duplicate(singles[0].convert_to_ell(), 2)
    assert e.num_items == 2 and e.convert_to_csr().values.shape == (2, pat.stored)


# ------------------------------------------------------------------------------------------ structure checks
def test_bad_patterns_are_refused(gexec):
    vals = np.ones((2, 4))
    good = (np.array([0, 2, 3, 4], np.int32), np.array([0, 1, 1, 2], np.int32))
    batch.Csr.from_numpy(gexec, (3, 3), *good, vals)
    for rp, ci in (([1, 2, 3, 4], good[1]), ([0, 3, 2, 4], good[1]), ([0, 2, 3, 5], good[1]),
                   (good[0], [0, 1, 3, 2]), (good[0], [0, -1, 1, 2])):
        drp, dci = gexec.to_device(np.array(rp, np.int32)), gexec.to_device(np.array(ci, np.int32))
        dv = gexec.to_device(vals.copy())
        with pytest.raises(g.GkoError):
            batch.Csr(gexec, (3, 3), dv, dci, drp)
        assert drp.cpu().tolist() == list(rp) and dci.cpu().tolist() == list(ci) and same(dv.cpu().numpy(), vals)
    batch.Ell.from_numpy(gexec, (3, 3), np.array([[0, 1, 2], [1, -1, -1]], np.int32), np.ones((2, 6)), 2, 3)
    for bad in ([[0, 1, 2], [3, -1, -1]], [[0, 1, 2], [1, -2, -1]]):
        with pytest.raises(g.GkoError):
            batch.Ell.from_numpy(gexec, (3, 3), np.array(bad, np.int32), np.ones((2, 6)), 2, 3)
    with pytest.raises(g.GkoError):
        batch.Ell.from_numpy(gexec, (3, 3), np.zeros((2, 2), np.int32), np.ones((2, 4)), 2, 2)      # stride < rows


# ------------------------------------------------------------------------------------------ solvers
def solve_on_device(ex, solver, fmt, precond, pat, vals, b, x0, tol, kind, max_it):
    a, _, _ = device_matrix(ex, fmt, pat, vals)
    s = (SOLVER_CLS[solver].build().with_max_iterations(max_it).with_tolerance(tol).with_tolerance_type(kind)
         .with_preconditioner(batch.Jacobi.build() if precond else None).on(ex).generate(a))
    db, dx = batch.MultiVector.from_numpy(ex, b), batch.MultiVector.from_numpy(ex, x0)
    assert s.apply(db, dx) is dx
    assert s.iteration_counts.dtype == torch.int32 and s.converged.dtype == torch.int32
    assert s.iteration_counts.is_cuda and s.residual_norms.is_cuda and s.converged.is_cuda
    return (dx.to_numpy()[:, :, 0], s.iteration_counts.cpu().numpy(), s.residual_norms.cpu().numpy(),
            s.converged.cpu().numpy()), s


def reference(key, solver, precond, pat, vals, b, x0, tol, kind, max_it):
    """Csr and Ell hold the same entries in the same order, so one reference serves both formats"""
    if key not in _REFS:
        _REFS[key] = R.SOLVERS[solver](pat, vals, b, x0, R.width(pat.size[0]), tol, kind, max_it, precond)
        for out in _REFS[key]:
            out.setflags(write=False)
    return _REFS[key]


def check(got, ref, what):
    for name, a, b in zip(("x", "iteration_counts", "residual_norms", "converged"), got, ref):
        assert same(a, b), (what, name, a, b)


def mixed_batch(solver, dtype):
    """9 items of n = 70: good ones that stop at different iterations, the identity, b = 0, an ill-conditioned
    one that runs into max_iterations, and an all-zero one between two good ones"""
    n, items = 70, 9
    pat, vals = R.tridiagonal(n, items, dtype, seed=21, symmetric=solver == "cg")
    vals[:, pat.ci == np.repeat(np.arange(n), pat.lens)] *= np.linspace(1.0, 3.0, items, dtype=dtype)[:, None]
    diag = pat.ci == np.repeat(np.arange(n), pat.lens)
    vals[1] = np.where(diag, 1, 0)                       # the identity
    vals[4] = np.where(diag, 2, -1)                      # the 1-D Laplacian: far from done at max_iterations
    vals[6] = 0                                          # breaks down: ends by the NaN rule
    b = np.random.default_rng(22).uniform(-1, 1, (items, n)).astype(dtype)
    b[2] = 0
    return pat, vals, b


SOLVER_CASES = [(s, f, p, d) for s in ("cg", "bicgstab") for f in ("csr", "ell") for p in (None, "jacobi")
                for d in DTYPES]
SOLVER_IDS = ["-".join([s, f, p or "none", "f64" if d is np.float64 else "f32"]) for s, f, p, d in SOLVER_CASES]


@pytest.mark.parametrize("kind", ["absolute", "relative"])
@pytest.mark.parametrize("solver,fmt,precond,dtype", SOLVER_CASES, ids=SOLVER_IDS)
def test_items_stop_on_their_own(gexec, solver, fmt, precond, dtype, kind):
    pat, vals, b = mixed_batch(solver, dtype)
    tol, max_it = (1e-10, 40) if dtype is np.float64 else (1e-5, 20)
    x0 = np.zeros_like(b)
    ref = reference(("mixed", solver, precond, dtype, kind), solver, precond, pat, vals, b, x0, tol, kind, max_it)
    x, it, res, conv = ref
    # the case is what it claims to be
    assert it[2] == 0 and conv[2] == 1 and it[1] == 1 and conv[1] == 1
    assert it[4] == max_it and conv[4] == 0 and not np.isnan(res[4])
    assert conv[6] == 0 and np.isnan(res[6]) and it[6] < max_it
    good = [0, 3, 5, 7, 8]
    assert conv[good].all() and (it[good] < max_it).all() and len(set(it[good].tolist())) > 1
    got, _ = solve_on_device(gexec, solver, fmt, precond, pat, vals, b, x0, tol, kind, max_it)
    check(got, ref, "mixed")


@pytest.mark.parametrize("solver,fmt,precond,dtype", SOLVER_CASES, ids=SOLVER_IDS)
def test_initial_guess_and_no_iterations(gexec, solver, fmt, precond, dtype):
    n, items = 33, 3
    pat, vals = R.tridiagonal(n, items, dtype, seed=31, symmetric=solver == "cg")
    rng = np.random.default_rng(32)
    b, x0 = rng.uniform(-1, 1, (items, n)).astype(dtype), rng.uniform(-1, 1, (items, n)).astype(dtype)
    tol = 1e-9 if dtype is np.float64 else 1e-5
    for kind, max_it in (("relative", 40), ("absolute", 0)):
        ref = reference(("guess", solver, precond, dtype, kind), solver, precond, pat, vals, b, x0, tol, kind, max_it)
        got, _ = solve_on_device(gexec, solver, fmt, precond, pat, vals, b, x0, tol, kind, max_it)
        check(got, ref, kind)
        if max_it == 0:
            assert same(got[0], x0) and not got[1].any() and not got[3].any()
        else:
            assert got[3].all()


def plan_edges(solver, fmt, precond, dtype):
    """the system sizes at which the plan changes: the largest n with every vector resident and the next one, the
    largest n with all but one and the next one, and so on down to no resident vector (the values are never
    cached, so there is no edge of that kind)"""
    name = "f64" if dtype is np.float64 else "f32"

    def level(n):
        p = batch.plan(solver, fmt, precond, name, n, 3 * n - 2 if fmt == "csr" else 3 * n)
        assert not p.values_cached
        return p.resident_vectors

    hi = 1
    while level(hi) > 0:
        hi *= 2
    edges = []
    for target in range(level(1), 0, -1):
        lo, up = 1, hi                      # level(lo) >= target > level(up)
        while up - lo > 1:
            mid = (lo + up) // 2
            lo, up = (mid, up) if level(mid) >= target else (lo, mid)
        edges += [lo, up]
    return sorted(set(edges))


@pytest.mark.parametrize("solver,fmt,precond,dtype", SOLVER_CASES, ids=SOLVER_IDS)
def test_every_residency(gexec, solver, fmt, precond, dtype):
    """tridiagonal systems, 3 items, at both sides of every size at which a vector leaves LDS: the result does not
    depend on where the vectors live"""
    edges = plan_edges(solver, fmt, precond, dtype)
    total = batch.plan(solver, fmt, precond, "f64", 1, 1).total_vectors
    assert len(edges) == 2 * total
    name = "f64" if dtype is np.float64 else "f32"
    seen = set()
    for j, n in enumerate(edges):
        pat, vals = R.tridiagonal(n, 3, dtype, seed=41, symmetric=solver == "cg")
        rng = np.random.default_rng(42)
        b, x0 = rng.uniform(-1, 1, (3, n)).astype(dtype), rng.uniform(-1, 1, (3, n)).astype(dtype)
        kind, tol, max_it = ("relative", "absolute")[j % 2], 1e-3, 6
        ref = reference(("edge", solver, precond, dtype, n), solver, precond, pat, vals, b, x0, tol, kind, max_it)
        assert ref[1].max() >= 3
        got, s = solve_on_device(gexec, solver, fmt, precond, pat, vals, b, x0, tol, kind, max_it)
        assert s.plan == batch.plan(solver, fmt, precond, name, n, s.matrix.get_num_stored_elements_per_item())
        assert s.workspace.numel() >= 3 * s.plan.workspace_bytes
        seen.add(s.plan.resident_vectors)
        check(got, ref, (n, s.plan))
    assert seen == set(range(total + 1))


def test_one_apply_is_one_library_call(gexec):
    pat, vals = R.tridiagonal(20, 4, np.float64, seed=51)
    b = np.ones((4, 20))
    for fmt in ("csr", "ell"):
        a, _, _ = device_matrix(gexec, fmt, pat, vals)
        for cls in (batch.Cg, batch.Bicgstab):
            s = cls.build().with_preconditioner(batch.Jacobi.build()).on(gexec).generate(a)
            db, dx = batch.MultiVector.from_numpy(gexec, b), batch.MultiVector.from_numpy(gexec, np.zeros_like(b))
            with _lib.record() as tape:
                s.apply(db, dx)
            assert len(tape.calls) == 1 and tape.calls[0][2].startswith("gkoc_batch_"), tape.calls
        with _lib.record() as tape:
            a.apply(db, dx)
        assert len(tape.calls) == 1


def test_solver_refuses_wrong_operands(gexec):
    pat, vals = R.tridiagonal(8, 2, np.float64, seed=61)
    a, _, _ = device_matrix(gexec, "csr", pat, vals)
    s = batch.Cg.build().on(gexec).generate(a)
    ok = batch.MultiVector.create(gexec, 2, (8, 1))
    for bad in (batch.MultiVector.create(gexec, 3, (8, 1)), batch.MultiVector.create(gexec, 2, (8, 2)),
                batch.MultiVector.create(gexec, 2, (7, 1))):
        with pytest.raises(g.DimensionMismatch):
            s.apply(bad, ok)
    with pytest.raises(g.NotSupported):
        s.apply(ok, batch.MultiVector.create(gexec, 2, (8, 1), torch.float32))
    rect = batch.Csr.from_numpy(gexec, (2, 3), np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones((2, 2)))
    with pytest.raises(g.DimensionMismatch):
        batch.Cg.build().on(gexec).generate(rect)
