"""The numpy references of tests/factorization_refs.py against facts that do not depend on them: dense LU
without pivoting, the defining property of an incomplete factorization on its pattern, planted factors with
exactly representable entries, the relation between IC(0) and ILU(0) of an SPD matrix.  No device."""
import numpy as np
import pytest
import scipy.sparse as sp

import factorization_refs as fr

DTYPES = [np.float64, np.float32]


def dense_lu(a):
    """Doolittle without pivoting, (L - I + U) in one array, in a's dtype"""
    a = a.copy()
    n = a.shape[0]
    for k in range(n):
        a[k + 1:, k] = a[k + 1:, k] / a[k, k]
        a[k + 1:, k + 1:] = a[k + 1:, k + 1:] - np.outer(a[k + 1:, k], a[k, k + 1:])
    return a


def wider(dtype):
    return np.longdouble if dtype == np.float64 else np.float64


def dominant(rng, n, mask):
    a = rng.uniform(-1, 1, (n, n)) * mask
    np.fill_diagonal(a, 0)
    return a + np.diag(1.0 + np.abs(a).sum(1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("band", [None, 2])
def test_ilu0_on_a_pattern_without_fill_is_dense_lu(dtype, band):
    """full and banded patterns take no fill, so ILU(0) is LU.  Each entry of either result is a_ij minus
    at most n products, divided once: the two orders of the same sums differ by at most (n + 1) roundings of
    terms bounded by (|L||U|)_ij - the bound used below, with |L||U| from the dense result"""
    n = 24
    rng = np.random.default_rng(5)
    idx = np.arange(n)
    mask = np.ones((n, n), bool) if band is None else np.abs(idx[:, None] - idx[None, :]) <= band
    a = dominant(rng, n, mask).astype(dtype)
    rp, ci, v = fr.on_pattern(a, mask, dtype=dtype)
    got = fr.dense_of(rp, ci, fr.ilu0(rp, ci, v))
    want = dense_lu(a)
    assert got.dtype == dtype
    lo, up = np.tril(want, -1) + np.eye(n, dtype=dtype), np.triu(want)
    bound = (n + 1) * np.finfo(dtype).eps * (np.abs(lo).astype(wider(dtype)) @ np.abs(up).astype(wider(dtype)))
    # a lower entry is that sum divided by the pivot
    bound = np.where(idx[:, None] > idx[None, :], bound / np.abs(np.diag(want))[None, :], bound)
    assert (np.abs(got.astype(wider(dtype)) - want) <= bound).all()
    # dyadic data: exact
    rng = np.random.default_rng(6)
    lo = np.eye(n) + np.tril(rng.integers(-2, 3, (n, n)), -1) * mask
    up = (np.triu(rng.integers(-2, 3, (n, n)), 1) + np.diag(rng.choice([1.0, 2.0, 4.0], n))) * mask
    a = (lo @ up).astype(dtype)
    rp, ci, v = fr.on_pattern(a, mask, dtype=dtype)
    got = fr.dense_of(rp, ci, fr.ilu0(rp, ci, v))
    assert np.array_equal(got, (lo - np.eye(n) + up).astype(dtype))


def spd_matrices():
    rng = np.random.default_rng(11)
    yield "stencil", fr.stencil27(5)
    yield "random", fr.from_lower_pattern(fr.random_pattern(300, rng), rng, spd=True)
    yield "hub", fr.from_lower_pattern(fr.hub_pattern(120, 60, 30, 30), rng, spd=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_product_of_the_factors_matches_the_matrix_on_its_pattern(dtype):
    """(LU)_ij = a_ij and (L L^T)_ij = a_ij wherever (i, j) is stored.  The computed entry is a_ij minus m
    products (m < the length of row i), then one division or root: backward error analysis bounds the
    residual by (m + 2) eps (|L||U|)_ij; the product is formed in the next wider type"""
    eps = np.finfo(dtype).eps
    w = wider(dtype)
    for name, a in spd_matrices():
        rp, ci, v = fr.arrays(a, dtype=dtype)
        n = len(rp) - 1
        longest = int(np.diff(rp).max())
        stored = fr.dense_of(rp, ci, np.ones_like(v)) != 0
        a_w = fr.dense_of(rp, ci, v).astype(w)
        l_rp, l_ci, l_v, u_rp, u_ci, u_v = fr.ilu_factors(rp, ci, v)
        lo, up = fr.dense_of(l_rp, l_ci, l_v).astype(w), fr.dense_of(u_rp, u_ci, u_v).astype(w)
        assert np.array_equal(np.diag(lo), np.ones(n)) and not np.triu(lo, 1).any() and not np.tril(up, -1).any()
        err = np.abs(lo @ up - a_w)
        assert (err[stored] <= ((longest + 2) * eps * (np.abs(lo) @ np.abs(up)))[stored]).all(), name
        assert err[~stored].max() > 100 * eps, name + ": no fill was dropped, the case shows nothing"
        c_rp, c_ci, c_v = fr.ic_factor(rp, ci, v)
        ch = fr.dense_of(c_rp, c_ci, c_v).astype(w)
        err = np.abs(ch @ ch.T - a_w)
        low = np.tril(stored)
        assert (err[low] <= ((longest + 2) * eps * (np.abs(ch) @ np.abs(ch).T))[low]).all(), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_factors_come_back_exactly(dtype):
    rng = np.random.default_rng(3)
    for a, lo, up in (fr.planted_chain(200, rng), fr.planted_blocks(8, rng)):
        mask = (lo != 0) | (up != 0)
        rp, ci, v = fr.on_pattern(a, mask, dtype=dtype)
        l_rp, l_ci, l_v, u_rp, u_ci, u_v = fr.ilu_factors(rp, ci, v)
        assert np.array_equal(fr.dense_of(l_rp, l_ci, l_v), lo.astype(dtype))
        assert np.array_equal(fr.dense_of(u_rp, u_ci, u_v), up.astype(dtype))
        spd, low = fr.planted_cholesky(lo)
        rp, ci, v = fr.on_pattern(spd, (low != 0) | (low != 0).T, dtype=dtype)
        c_rp, c_ci, c_v = fr.ic_factor(rp, ci, v)
        assert np.array_equal(fr.dense_of(c_rp, c_ci, c_v), low.astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ic_is_ilu_scaled_by_the_root_of_the_pivots_on_spd_matrices(dtype):
    """for symmetric A the ILU(0) rows satisfy U = D L^T, so L_ic = L_ilu sqrt(D) in exact arithmetic.  The
    matrices are strictly diagonally dominant (pivots >= 1, |l_ij| < 1), every entry takes fewer than
    `longest` updates: the two computations differ by a modest multiple of longest * eps"""
    for name, a in spd_matrices():
        rp, ci, v = fr.arrays(a, dtype=dtype)
        longest = int(np.diff(rp).max())
        l_rp, l_ci, l_v, u_rp, u_ci, u_v = fr.ilu_factors(rp, ci, v)
        c_rp, c_ci, c_v = fr.ic_factor(rp, ci, v)
        assert np.array_equal(c_rp, l_rp) and np.array_equal(c_ci, l_ci)
        pivots = u_v[u_rp[:-1]].astype(np.float64)
        assert (pivots >= 1).all()
        want = fr.dense_of(l_rp, l_ci, l_v).astype(np.float64) * np.sqrt(pivots)[None, :]
        got = fr.dense_of(c_rp, c_ci, c_v).astype(np.float64)
        assert np.abs(got - want).max() <= 8 * longest * np.finfo(dtype).eps * np.abs(want).max(), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_split_puts_every_entry_in_one_factor(dtype):
    rng = np.random.default_rng(17)
    a = sp.random(60, 60, 0.1, random_state=rng, format="csr") + sp.identity(60) * 3.0
    rp, ci, v = fr.arrays(a, np.int64, dtype)
    l_rp, l_ci, l_v, u_rp, u_ci, u_v = fr.split_l_u(rp, ci, v)
    assert l_rp.dtype == np.int64 and l_v.dtype == dtype
    lo, up = fr.dense_of(l_rp, l_ci, l_v), fr.dense_of(u_rp, u_ci, u_v)
    # (L - I) + U in this order: every sum has a zero term, nothing is rounded
    assert np.array_equal((lo - np.eye(60, dtype=dtype)) + up, fr.dense_of(rp, ci, v))
    assert (l_ci[l_rp[1:] - 1] == np.arange(60)).all() and (l_v[l_rp[1:] - 1] == 1).all()
    assert (u_ci[u_rp[:-1]] == np.arange(60)).all()
    for root in (False, True):
        s_rp, s_ci, s_v = fr.split_l(rp, ci, v, root)
        want = np.tril(fr.dense_of(rp, ci, v))
        if root:
            np.fill_diagonal(want, np.sqrt(np.diag(want)))
        assert np.array_equal(fr.dense_of(s_rp, s_ci, s_v), want) and np.array_equal(s_rp, l_rp)
        assert (s_ci[s_rp[1:] - 1] == np.arange(60)).all()
