"""numpy restatement of the general / spd ISAI contract (include/gko_cdna4.h, ginkgo_amd/csrc/isai.hip): one
dense system per pattern row, Gauss-Jordan with implicit partial pivoting, every operation in the array's own
dtype, one multiply and one subtract per update, the pivot rule (largest magnitude, a NaN as the largest, the
smallest row on a tie), the spd scaling and the non-finite rule.  Rows are sorted by column; every pattern row
contains its diagonal."""
import numpy as np
import scipy.sparse as sp

from isai_refs import pattern_power, residual_on_pattern  # noqa: F401  (shared with the triangular tests)


def lower_pattern_power(rp, ci, p):
    """(row_ptrs, col_idxs) of the lower triangle, diagonal included, of the pattern of |A|^p (int32 arrays)"""
    n = len(rp) - 1
    f_rp, f_ci = pattern_power(rp, ci, p)
    low = sp.tril(sp.csr_matrix((np.ones(len(f_ci)), f_ci, f_rp), shape=(n, n)), 0).tocsr()
    low.sort_indices()
    return low.indptr.astype(np.int32), low.indices.astype(np.int32)


def dense_block(where, a_v, cols):
    """M[j][k] = a[c_k, c_j] where A stores the entry, 0 elsewhere; `where` holds position + 1 of A's entries"""
    at = where[cols][:, cols].toarray().T
    return np.where(at != 0, a_v[at - 1], a_v.dtype.type(0))


def solve_row(m_, p, spd, stats=None):
    """w of one row: the m x m system `m_` (changed in place), right-hand side e_p"""
    m = m_.shape[0]
    dt = m_.dtype.type
    rhs = np.zeros(m, m_.dtype)
    rhs[p] = dt(1)
    used = np.zeros(m, bool)
    q_of = np.zeros(m, np.int64)
    rows = np.arange(m)
    for col in range(m):
        key = np.where(np.isnan(m_[:, col]), dt(np.inf), np.abs(m_[:, col]))
        key[used] = dt(-1)
        q = int(np.argmax(key))         # the first of the largest: the smallest row on a tie
        used[q] = True
        q_of[col] = q
        others = rows != q
        f = (m_[:, col] / m_[q, col]).astype(m_.dtype)
        prod = (f[:, None] * m_[q, col + 1:][None, :]).astype(m_.dtype)
        m_[others, col + 1:] = (m_[:, col + 1:] - prod).astype(m_.dtype)[others]
        rhs[others] = (rhs - (f * rhs[q]).astype(m_.dtype)).astype(m_.dtype)[others]
    w = (rhs[q_of] / m_[q_of, rows]).astype(m_.dtype)
    if spd:
        w = (w / np.sqrt(w[m - 1])).astype(m_.dtype)
    if not np.isfinite(w).all():
        w[:] = 0
        w[p] = dt(1)
    if stats is not None:
        stats.setdefault("pivots", []).append(q_of)
        stats["rows_pivoted_off_the_diagonal"] = stats.get("rows_pivoted_off_the_diagonal", 0) \
            + int(not np.array_equal(q_of, rows))
    return w


def general_inverse(a_rp, a_ci, a_v, w_rp, w_ci, spd, stats=None):
    """the values of W on the pattern (w_rp, w_ci).  For row i with the pattern columns c_0 < ... < c_{m-1},
    i at position p: M[j][k] = a[c_k, c_j], r = e_p; for col = 0 .. m-1 the pivot q is the unused row with the
    largest |M[r][col]|, every other row r takes f = M[r][col] / M[q][col], M[r][k] -= f * M[q][k] (k > col),
    r[r] -= f * r[q]; w[c_col] = r[q(col)] / M[q(col)][col].  spd: every column of the row is <= i, and the row
    is divided by sqrt(w[c_{m-1}]).  A row with a non-finite w becomes zeros with 1 at p.
    `stats`, if given, gets every row's pivot sequence q(0 .. m-1) under "pivots" and the number of rows whose
    pivots left the order 0, 1, ..., m-1 under "rows_pivoted_off_the_diagonal"."""
    n = len(a_rp) - 1
    where = sp.csr_matrix((np.arange(1, len(a_ci) + 1), a_ci, a_rp), shape=(n, n))
    w_v = np.zeros(len(w_ci), a_v.dtype)
    with np.errstate(all="ignore"):
        for i in range(n):
            cols = w_ci[w_rp[i]:w_rp[i + 1]]
            p = int(np.searchsorted(cols, i))
            assert p < len(cols) and cols[p] == i, "row %d of the pattern does not contain its diagonal" % i
            assert not spd or p == len(cols) - 1, "spd: row %d of the pattern has an entry above the diagonal" % i
            w_v[w_rp[i]:w_rp[i + 1]] = solve_row(dense_block(where, a_v, cols), p, spd, stats)
    return w_v


def lapack_inverse(a_rp, a_ci, a_v, w_rp, w_ci, spd):
    """the same W by numpy.linalg.solve on the dense blocks, in float64 (no identity rows: the caller's
    matrices are regular)"""
    n = len(a_rp) - 1
    where = sp.csr_matrix((np.arange(1, len(a_ci) + 1), a_ci, a_rp), shape=(n, n))
    a64 = a_v.astype(np.float64)
    w_v = np.zeros(len(w_ci))
    for i in range(n):
        cols = w_ci[w_rp[i]:w_rp[i + 1]]
        e = (cols == i).astype(np.float64)
        w = np.linalg.solve(dense_block(where, a64, cols), e)
        w_v[w_rp[i]:w_rp[i + 1]] = w / np.sqrt(w[-1]) if spd else w
    return w_v


def identity_rows(w_rp, w_ci, w_v):
    """mask of the rows of W that are the identity's"""
    n = len(w_rp) - 1
    rows = np.repeat(np.arange(n), np.diff(w_rp))
    differs = np.bincount(rows, weights=(w_v != (w_ci == rows)).astype(np.float64), minlength=n)
    return differs == 0


def weak_diagonal(n=400, density=0.02, seed=11, dtype=np.float64):
    """(rp, ci, v) of a random matrix on which pivoting matters: off-diagonals in [-1, 1], diagonal in
    [0.01, 0.1]"""
    rng = np.random.default_rng(seed)
    a = sp.random(n, n, density, random_state=rng, format="lil", data_rvs=lambda k: rng.uniform(-1, 1, k))
    a.setdiag(rng.uniform(0.01, 0.1, n))
    a = a.tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(dtype)


def convection(g=8, dtype=np.float64):
    """(rp, ci, v) of a nonsymmetric 7-point convection-diffusion operator on g^3 points: -laplace plus an
    upwind first derivative of a different strength in every direction"""
    t = sp.diags([np.ones(g - 1), np.ones(g - 1)], [-1, 1])
    d = sp.diags([np.ones(g - 1)], [-1])
    eye = sp.identity(g)
    lap = sp.kron(sp.kron(t, eye), eye) + sp.kron(sp.kron(eye, t), eye) + sp.kron(sp.kron(eye, eye), t)
    wind = 0.75 * sp.kron(sp.kron(d, eye), eye) + 0.5 * sp.kron(sp.kron(eye, d), eye) \
        + 0.25 * sp.kron(sp.kron(eye, eye), d)
    a = (sp.identity(g ** 3) * 7.5 - lap - wind).tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(dtype)


def hub(length, spd, seed=5, dtype=np.float64):
    """(rp, ci, v) of a symmetric, diagonally dominant matrix in which ONE row, the hub, and its symmetric
    column store `length` consecutive columns and every other row at most 3 entries.  The matrix is
    tridiagonal outside the hub's span; inside it a row stores its diagonal and the hub's column only.
    General (spd false): the hub's row has `length` entries, hub - length + 2 .. hub + 1.  spd: its LOWER part
    has, hub - length + 1 .. hub, so that the lower pattern's longest row is `length`."""
    assert length >= 4
    rng = np.random.default_rng(seed + length)
    n, hub_row = length + 60, length + 19
    first = hub_row - length + (1 if spd else 2)
    a = sp.lil_matrix((n, n))
    for i in range(n - 1):
        inside = first <= i < hub_row or first <= i + 1 < hub_row
        if not inside:
            a[i, i + 1] = a[i + 1, i] = rng.uniform(0.1, 1.0) * rng.choice([-1.0, 1.0])
    for j in range(first, hub_row):
        a[hub_row, j] = a[j, hub_row] = rng.uniform(0.1, 1.0) * rng.choice([-1.0, 1.0])
    a.setdiag(1.0 + np.asarray(abs(a.tocsr()).sum(axis=1)).ravel())
    a = a.tocsr()
    a.sort_indices()
    counts = np.diff(sp.tril(a).tocsr().indptr if spd else a.indptr)
    assert counts.max() == counts[hub_row] == length and np.sort(counts)[-2] <= 3
    assert np.diff(a.indptr).max() == length + (1 if spd else 0) and np.sort(np.diff(a.indptr))[-2] <= 3
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(dtype)
