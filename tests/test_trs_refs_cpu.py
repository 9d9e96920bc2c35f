"""The numpy references of tests/trs_refs.py against planted solutions, scipy and hand-computed
figures - no GPU.  On dyadic inputs every intermediate is exact, so equality is the check."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular

import trs_refs as tr


def _scipy(rp, ci, v, n):
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("kind", ["chain", "tiers"])
def test_planted_solution_exact(kind, upper, dtype):
    rng = np.random.default_rng(11)
    rows = tr.chain_rows(300, rng) if kind == "chain" else tr.tiers_rows(16, rng)
    if upper:
        rows = tr.mirror(rows)
    x, b = tr.planted(rows, rng, nrhs=2)
    rp, ci, v = tr.from_rows(rows, dtype=dtype)
    got = tr.trs_solve(rp, ci, v, b.astype(dtype), upper=upper)
    assert got.dtype == dtype and np.array_equal(got, x)
    a = _scipy(rp, ci, v.astype(np.float64), len(rows))
    a.sort_indices()
    assert np.array_equal(spsolve_triangular(a, b, lower=not upper), x)


def test_unit_diagonal_and_missing_diagonal():
    rows = [[(0, 7.0)], [(0, 2.0)], [(1, -1.0), (0, 1.0), (2, 0.5)]]     # row 1 has no diagonal, row 2 unsorted
    rp, ci, v = tr.from_rows(rows)
    b = np.array([[7.0], [5.0], [3.0]])
    assert np.array_equal(tr.trs_solve(rp, ci, v, b), [[1.0], [3.0], [10.0]])
    assert np.array_equal(tr.trs_solve(rp, ci, v, b, unit_diag=True), [[7.0], [-9.0], [-13.0]])


def test_other_triangle_is_ignored():
    rng = np.random.default_rng(5)
    a = sp.random(60, 60, 0.2, random_state=rng, format="csr") + 4 * sp.eye(60)
    rp, ci, v = tr.csr_of(a)
    b = rng.uniform(-1, 1, (60, 1))
    for upper in (False, True):
        tri = sp.triu(a, format="csr") if upper else sp.tril(a, format="csr")
        assert np.array_equal(tr.trs_solve(rp, ci, v, b, upper=upper),
                              tr.trs_solve(*tr.csr_of(tri), b, upper=upper))
        assert all(np.array_equal(p, q) for p, q in zip(tr.levels(rp, ci, upper),
                                                        tr.levels(*tr.csr_of(tri)[:2], upper)))


@pytest.mark.parametrize("grid,n_levels,widest", [(6, 36, 9), (12, 78, 36)])
def test_levels_of_the_stencil(oracle, grid, n_levels, widest):
    rp, ci, _ = oracle.stencil_csr(3, grid)
    for upper in (False, True):
        ptrs, rows, level = tr.levels(rp, ci, upper)
        assert len(ptrs) - 1 == n_levels == 7 * (grid - 1) + 1
        assert np.diff(ptrs).max() == widest
        assert np.array_equal(np.sort(rows), np.arange(grid ** 3))
        assert all((np.diff(rows[ptrs[l]:ptrs[l + 1]]) > 0).all() for l in range(n_levels))
        assert np.array_equal(level[rows], np.repeat(np.arange(n_levels), np.diff(ptrs)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_weighted_factors(oracle, dtype):
    rp, ci, v = oracle.stencil_csr(3, 4)
    v = v.astype(dtype)
    n = 64
    l_rp, l_ci, l_v, u_rp, u_ci, u_v = tr.weighted_l_u(rp, ci, v, 1.2)
    assert all(np.array_equal(p, q) for p, q in zip(tr.weighted_l(rp, ci, v, 1.2), (l_rp, l_ci, l_v)))
    w = dtype(1.2)
    assert np.array_equal(u_v[u_rp[:-1]], np.full(n, dtype(1) / (dtype(2) - w)))
    assert np.array_equal(u_ci[u_rp[:-1]], np.arange(n)) and np.array_equal(l_ci[l_rp[1:] - 1], np.arange(n))
    a = _scipy(rp, ci, v.astype(np.float64), n)
    d = a.diagonal()
    assert np.array_equal(l_v[l_rp[1:] - 1], (d.astype(dtype) / w))
    # L U is the SSOR matrix (D/w + L_A) w/(2-w) D^-1 (D/w + U_A)
    lo, up = _scipy(l_rp, l_ci, l_v.astype(np.float64), n), _scipy(u_rp, u_ci, u_v.astype(np.float64), n)
    wd = float(w)
    ssor = (sp.diags(d / wd) + sp.tril(a, -1)) @ sp.diags(wd / (2 - wd) / d) @ (sp.diags(d / wd) + sp.triu(a, 1))
    assert abs(lo @ up - ssor).max() < 50 * np.finfo(dtype).eps * abs(ssor).max()
