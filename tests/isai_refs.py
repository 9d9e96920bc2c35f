"""numpy restatement of the triangular ISAI contract (include/gko_cdna4.h, ginkgo_amd/csrc/isai.hip): every
operation in the array's own dtype, one multiply and one subtract per update, the updates of an entry in the
stated order, and the non-finite rule.  Rows are sorted by column; A stores its diagonal last (lower) or first
(upper) in every row."""
import numpy as np
import scipy.sparse as sp


def pattern_power(rp, ci, p):
    """(row_ptrs, col_idxs) of the pattern of |A|^p, rows sorted (int32 arrays)"""
    n = len(rp) - 1
    one = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    out = one
    for _ in range(p - 1):
        out = (out @ one).tocsr()
    out.sort_indices()
    return out.indptr.astype(np.int32), out.indices.astype(np.int32)


def tri_inverse(a_rp, a_ci, a_v, w_rp, w_ci, lower):
    """the values of W on the pattern (w_rp, w_ci).
    lower: c_0 < ... < c_{m-1} = i; for t = m-1 .. 0: s = (c_t == i); for u = m-1 .. t+1 with (c_u, c_t)
    stored in A: s = s - w[c_u] * a[c_u, c_t]; w[c_t] = s / a[c_t, c_t].  upper: the mirror image.
    A row with a non-finite w becomes the identity's row.

    Carried out column-wise, which is the same sequence of operations for every entry: as soon as w[c_u] is
    final it is subtracted from every entry still open, and u runs in the stated direction."""
    n = len(a_rp) - 1
    dt = a_v.dtype.type
    # position + 1 of every stored entry of A: one gather per row gives the block and says what is stored
    where = sp.csr_matrix((np.arange(1, len(a_ci) + 1), a_ci, a_rp), shape=(n, n))
    w_v = np.zeros(len(w_ci), a_v.dtype)
    with np.errstate(all="ignore"):
        for i in range(n):
            cols = w_ci[w_rp[i]:w_rp[i + 1]]
            m = len(cols)
            assert m and cols[-1 if lower else 0] == i, "row %d of the pattern: the diagonal is not at its end" % i
            at = where[cols][:, cols].toarray()
            mask = at != 0
            block = np.where(mask, a_v[at - 1], dt(0))
            s = np.zeros(m, a_v.dtype)
            s[m - 1 if lower else 0] = dt(1)
            for u in (range(m - 1, -1, -1) if lower else range(m)):
                assert mask[u, u], "A does not store the diagonal of row %d" % cols[u]
                s[u] = dt(s[u] / block[u, u])
                still = slice(0, u) if lower else slice(u + 1, m)
                prod = (s[u] * block[u, still]).astype(a_v.dtype)
                s[still] = np.where(mask[u, still], (s[still] - prod).astype(a_v.dtype), s[still])
            if not np.isfinite(s).all():
                s[:] = 0
                s[m - 1 if lower else 0] = dt(1)
            w_v[w_rp[i]:w_rp[i + 1]] = s
    return w_v


def residual_on_pattern(a_rp, a_ci, a_v, w_rp, w_ci, w_v):
    """(max over the pattern of |(W A - I)(i, j)|, the largest row sum of |W| |A|), in float64"""
    n = len(a_rp) - 1
    a = sp.csr_matrix((a_v.astype(np.float64), a_ci, a_rp), shape=(n, n))
    w = sp.csr_matrix((w_v.astype(np.float64), w_ci, w_rp), shape=(n, n))
    on = sp.csr_matrix((np.ones(len(w_ci)), w_ci, w_rp), shape=(n, n))
    err = abs((w @ a - sp.identity(n)).multiply(on)).max()
    scale = (abs(w) @ abs(a)).sum(axis=1).max()
    return float(err), float(scale)


def transposed(rp, ci, v):
    n = len(rp) - 1
    t = sp.csr_matrix((v, ci, rp), shape=(n, n)).T.tocsr()
    t.sort_indices()
    return t.indptr.astype(rp.dtype), t.indices.astype(ci.dtype), t.data


def flipped(rp, ci, v):
    """rows and columns in reverse order: a lower triangular matrix becomes an upper triangular one with the
    same row lengths (row i becomes row n-1-i), rows sorted"""
    n = len(rp) - 1
    rev = np.arange(n - 1, -1, -1)
    t = sp.csr_matrix((v, ci, rp), shape=(n, n))[rev][:, rev].tocsr()
    t.sort_indices()
    return t.indptr.astype(rp.dtype), t.indices.astype(ci.dtype), t.data


def lower_from_pattern(lower, rng, dtype=np.float64):
    """(rp, ci, v) of a lower triangular matrix from the strictly-lower columns of every row (the lists of
    factorization_refs.random_pattern / chain_pattern): off-diagonals in +-[0.1, 1], a_ii = 1 + the absolute
    row sum"""
    n = len(lower)
    rows, cols, vals = [], [], []
    for i, ks in enumerate(lower):
        ks = sorted(ks)
        off = (rng.uniform(0.1, 1.0, len(ks)) * rng.choice([-1.0, 1.0], len(ks))).tolist()
        rows += [i] * (len(ks) + 1)
        cols += ks + [i]
        vals += off + [1.0 + sum(abs(x) for x in off)]
    a = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(dtype)


def hub_lower(length, rng, dtype=np.float64):
    """(rp, ci, v) of a lower triangular matrix with the sub-diagonals 1 and 3, in which ONE row, the hub,
    stores the `length` columns hub - length + 1 .. hub: its pattern row has exactly `length` entries, every
    other row at most 3"""
    assert length >= 4
    n, hub = length + 60, length + 19
    rows, cols = [], []
    for i in range(n):
        ks = list(range(hub - length + 1, hub)) if i == hub else [k for k in (i - 3, i - 1) if k >= 0]
        rows += [i] * (len(ks) + 1)
        cols += ks + [i]
    vals = rng.uniform(0.1, 1.0, len(cols)) * rng.choice([-1.0, 1.0], len(cols))
    a = sp.csr_matrix((vals, (rows, cols)), shape=(n, n)).tolil()
    a.setdiag(1.0 + np.asarray(abs(a.tocsr()).sum(axis=1)).ravel())
    a = a.tocsr()
    a.sort_indices()
    counts = np.diff(a.indptr)
    assert counts.max() == counts[hub] == length and np.sort(counts)[-2] <= 3
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(dtype)
