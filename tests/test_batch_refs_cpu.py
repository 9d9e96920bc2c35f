"""The numpy restatement of the batched solvers' contract (tests/batch_refs.py) is itself correct: R_W sums, the
product multiplies, and both solvers solve - checked against math.fsum, scipy's products and
scipy.sparse.linalg.spsolve.  No device."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

import batch_refs as R

# max over the items of ||b - A x|| / ||b|| (np.longdouble) of the reference's x, measured on the CPU, for
# relative tolerance 1e-10 on the diagonally dominant tridiagonal items below (n = 50, 6 items, float64)
MEASURED = {("cg", None): 9.471e-11, ("cg", "jacobi"): 7.672e-11,
            ("bicgstab", None): 8.425e-11, ("bicgstab", "jacobi"): 9.470e-11}


@pytest.mark.parametrize("w", [64, 256, 512])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reduction_sums_to_rounding(w, dtype):
    """any summation order of n terms is within (n - 1) u sum|t| of the exact sum (to first order; n u is used)"""
    rng = np.random.default_rng(w)
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000):
        t = rng.uniform(-1, 1, (3, n)).astype(dtype)
        got = R.reduce_w(t, w)
        assert got.dtype == dtype and got.shape == (3,)
        for i in range(3):
            exact = math.fsum(float(v) for v in t[i])
            bound = n * float(np.finfo(dtype).eps) * math.fsum(abs(float(v)) for v in t[i])
            assert abs(float(got[i]) - exact) <= bound, (n, i)
    assert R.reduce_w(np.zeros((2, 0), dtype), w).tolist() == [0.0, 0.0]
    assert [R.width(n) for n in (1, 64, 65, 128, 129, 768, 769, 10 ** 6)] == [64, 64, 128, 128, 256, 256, 512, 512]


def _scipy_of(pat, vals, item):
    if pat.format == "csr":
        return sp.csr_matrix((vals[item], pat.ci, pat.rp), shape=pat.size)
    dense = np.zeros(pat.size)
    for rows, at, cols in pat.slots():
        np.add.at(dense, (rows, cols), vals[item, at])
    return sp.csr_matrix(dense)


def test_product_and_conversions():
    pat = R.random_pattern(37, 29, 0.2, 5, empty_rows=(0, 11))
    rng = np.random.default_rng(6)
    vals = rng.uniform(-1, 1, (4, pat.stored))
    u = rng.uniform(-1, 1, (4, 29, 3))
    y = R.product(pat, vals, u)
    ell, evals = R.csr_to_ell(pat, vals, stride=40)
    assert (ell.cols[:, 37:] == -1).all() and ell.k == int(pat.lens.max())
    assert np.array_equal(R.product(ell, evals, u), y)         # the same entries in the same order
    for item in range(4):
        assert np.allclose(y[item], _scipy_of(pat, vals, item) @ u[item], rtol=0, atol=1e-13)
    back, bvals = R.ell_to_csr(ell, evals)
    assert np.array_equal(back.rp, pat.rp) and np.array_equal(back.ci, pat.ci) and np.array_equal(bvals, vals)
    alpha, beta = rng.uniform(-1, 1, 4), rng.uniform(-1, 1, 4)
    x = rng.uniform(-1, 1, y.shape)
    assert np.array_equal(R.advanced_product(pat, vals, alpha, u, beta, x),
                          alpha[:, None, None] * y + beta[:, None, None] * x)


def test_jacobi_takes_the_first_diagonal_entry():
    # row 0: (0,0) stored twice, row 1: no diagonal, row 2: a zero diagonal
    pat = R.CsrPattern(3, 3, [0, 3, 4, 6], [0, 1, 0, 0, 2, 1])
    vals = np.array([[4.0, 1.0, 8.0, 1.0, 0.0, 1.0]])
    assert R.jacobi(pat, vals).tolist() == [[0.25, 1.0, 1.0]]


@pytest.mark.parametrize("precond", [None, "jacobi"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_solvers_solve(solver, precond):
    """Measured here (see MEASURED): the largest true relative residual of the items, for relative tolerance
    1e-10: cg 9.471e-11, cg + jacobi 7.672e-11, bicgstab 8.425e-11, bicgstab + jacobi 9.470e-11.  The run is
    deterministic; the factor 4 only covers another numpy build.  No item may run into max_iterations."""
    n, items, max_it = 50, 6, 200
    pat, vals = R.tridiagonal(n, items, np.float64, seed=3, symmetric=solver == "cg")
    b = np.random.default_rng(4).uniform(-1, 1, (items, n))
    x, it, res, conv = R.SOLVERS[solver](pat, vals, b, np.zeros_like(b), R.width(n), 1e-10, "relative", max_it, precond)
    assert conv.all() and (it < max_it).all() and (it > 0).all()
    worst = 0.0
    for i in range(items):
        a = _scipy_of(pat, vals, i)
        al = a.toarray().astype(np.longdouble)
        true = float(np.linalg.norm(b[i].astype(np.longdouble) - al @ x[i].astype(np.longdouble))
                     / np.linalg.norm(b[i].astype(np.longdouble)))
        worst = max(worst, true)
        exact = spsolve(a.tocsc(), b[i])
        # ||x - x*|| / ||x*|| <= cond(A) ||b - A x|| / ||b||
        assert np.linalg.norm(x[i] - exact) / np.linalg.norm(exact) <= np.linalg.cond(a.toarray()) * 4 * MEASURED[solver, precond]
        # the reported norm is the recurrence's, which the true one follows to rounding
        assert res[i] <= 1e-10 * np.linalg.norm(b[i]) * (1 + 1e-12)
    print(f"{solver} {precond}: iterations {it.tolist()}, worst true relative residual {worst:.3e}")
    assert worst <= 4 * MEASURED[solver, precond]


def test_stopping_rules():
    """b = 0 stops at once under both tolerance types, max_iterations = 0 does nothing, an all-zero item ends by
    the NaN rule without touching its neighbours, and items stop on their own"""
    n = 20
    pat, vals = R.tridiagonal(n, 4, np.float64, seed=8)
    vals[1, pat.rp[:-1] + (np.arange(n) > 0)] = 1.0          # item 1: unit diagonal ...
    vals[1, pat.ci != np.repeat(np.arange(n), pat.lens)] = 0.0   # ... and nothing else: the identity
    vals[2] = 0.0
    b = np.random.default_rng(9).uniform(-1, 1, (4, n))
    b[3] = 0.0
    for solver in ("cg", "bicgstab"):
        for kind in ("absolute", "relative"):
            x, it, res, conv = R.SOLVERS[solver](pat, vals, b, np.zeros_like(b), 64, 1e-9, kind, 50, None)
            assert it[3] == 0 and conv[3] == 1 and res[3] == 0 and not x[3].any()
            assert it[1] == 1 and conv[1] == 1 and np.array_equal(x[1], b[1])
            assert conv[2] == 0 and np.isnan(res[2]) and it[2] == 1
            assert conv[0] == 1 and 1 < it[0] < 50
            alone = R.SOLVERS[solver](pat, vals[:1], b[:1], np.zeros_like(b[:1]), 64, 1e-9, kind, 50, None)
            assert np.array_equal(alone[0][0], x[0]) and alone[1][0] == it[0]
        x, it, res, conv = R.SOLVERS[solver](pat, vals, b, np.ones_like(b), 64, 1e-9, "absolute", 0, "jacobi")
        assert not it.any() and np.array_equal(x, np.ones_like(b)) and conv.tolist() == [0, 0, 0, 0]
