"""numpy restatements of the ILU(0) / IC(0) loops and of the factor split (the contract stated in
include/gko_cdna4.h, ginkgo_amd/csrc/factorization.hip): every operation in the array's own dtype, one
multiply and one subtract per update, updates of an entry in ascending k.  Rows are sorted by column."""
import numpy as np
import scipy.sparse as sp


def _positions(rp, ci):
    """per row {column: position}"""
    return [{int(ci[p]): p for p in range(rp[i], rp[i + 1])} for i in range(len(rp) - 1)]


def ilu0(rp, ci, vals):
    """the factored values: for i, for stored k < i ascending, a_ik /= a_kk, then a_ij -= a_ik * a_kj for
    every stored j > k of row k with (i, j) stored.  Every row stores its diagonal."""
    n = len(rp) - 1
    dt = vals.dtype.type
    v = vals.copy()
    at = _positions(rp, ci)
    diag = [at[i][i] for i in range(n)]
    with np.errstate(all="ignore"):
        for i in range(n):
            row = at[i]
            for p in range(rp[i], diag[i]):
                k = int(ci[p])
                a_ik = dt(v[p] / v[diag[k]])
                v[p] = a_ik
                for q in range(diag[k] + 1, rp[k + 1]):
                    pos = row.get(int(ci[q]))
                    if pos is not None:
                        v[pos] = dt(v[pos] - dt(a_ik * v[q]))
    return v


def ic0(rp, ci, vals):
    """the factored values of a lower-triangular matrix with the diagonal last in every row: for stored
    (i, j), columns ascending, s = a_ij; for ascending k < j with (i, k) and (j, k) stored, s -= l_ik * l_jk;
    l_ij = s / l_jj (j < i), l_ii = sqrt(s)"""
    n = len(rp) - 1
    dt = vals.dtype.type
    v = vals.copy()
    at = _positions(rp, ci)
    with np.errstate(all="ignore"):
        for i in range(n):
            assert ci[rp[i + 1] - 1] == i, "the diagonal is not the last entry of row %d" % i
            for p in range(rp[i], rp[i + 1]):
                j = int(ci[p])
                s = v[p]
                other = at[j]
                for q in range(rp[i], p):
                    pos = q if j == i else other.get(int(ci[q]))
                    if pos is not None:
                        s = dt(s - dt(v[q] * v[pos]))
                v[p] = dt(s / v[rp[j + 1] - 1]) if j < i else dt(np.sqrt(s))
    return v


def _split(rp, ci, vals, with_u, diag_sqrt=False):
    n = len(rp) - 1
    dt = vals.dtype.type
    l_rp, u_rp = np.zeros(n + 1, rp.dtype), np.zeros(n + 1, rp.dtype)
    l_ci, l_v, u_ci, u_v = [], [], [], []
    for row in range(n):
        diag = dt(1)
        ks = range(rp[row], rp[row + 1])
        for k in ks:
            if ci[k] < row:
                l_ci.append(ci[k])
                l_v.append(vals[k])
            elif ci[k] == row:
                diag = vals[k]
        l_ci.append(row)
        with np.errstate(all="ignore"):
            l_v.append(dt(1) if with_u else (dt(np.sqrt(diag)) if diag_sqrt else diag))
        l_rp[row + 1] = len(l_ci)
        u_ci.append(row)
        u_v.append(diag)
        for k in ks:
            if ci[k] > row:
                u_ci.append(ci[k])
                u_v.append(vals[k])
        u_rp[row + 1] = len(u_ci)
    lower = (l_rp, np.array(l_ci, rp.dtype), np.array(l_v, vals.dtype))
    if not with_u:
        return lower
    return lower + (u_rp, np.array(u_ci, rp.dtype), np.array(u_v, vals.dtype))


def split_l_u(rp, ci, vals):
    """(l_rp, l_ci, l_v, u_rp, u_ci, u_v): L = strictly-lower entries in storage order, then 1;
    U = the diagonal, then the strictly-upper entries in storage order"""
    return _split(rp, ci, vals, True)


def split_l(rp, ci, vals, diag_sqrt=False):
    """(l_rp, l_ci, l_v): strictly-lower entries in storage order, then the diagonal (its root with diag_sqrt)"""
    return _split(rp, ci, vals, False, diag_sqrt)


def ilu_factors(rp, ci, vals):
    """what factorization.Ilu returns for a sorted matrix that stores every diagonal"""
    return split_l_u(rp, ci, ilu0(rp, ci, vals))


def ic_factor(rp, ci, vals):
    """what factorization.Ic returns as L for a sorted matrix that stores every diagonal"""
    l_rp, l_ci, l_v = split_l(rp, ci, vals)
    return l_rp, l_ci, ic0(l_rp, l_ci, l_v)


def arrays(a, index_dtype=np.int32, dtype=np.float64):
    """(rp, ci, v) of a scipy matrix, rows sorted, explicit zeros kept"""
    a = sp.csr_matrix(a)
    a.sort_indices()
    return a.indptr.astype(index_dtype), a.indices.astype(index_dtype), a.data.astype(dtype)


def on_pattern(dense, mask, index_dtype=np.int32, dtype=np.float64):
    """(rp, ci, v) of the entries of `dense` where `mask` is set - zeros among them stay stored"""
    n = dense.shape[0]
    rows, cols = np.nonzero(mask)
    rp = np.zeros(n + 1, index_dtype)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return rp, cols.astype(index_dtype), dense[rows, cols].astype(dtype)


def dense_of(rp, ci, v, dtype=None):
    n = len(rp) - 1
    return np.asarray(sp.csr_matrix((v, ci, rp), shape=(n, n)).toarray(), dtype or v.dtype)


# ------------------------------------------------------------------ matrices of the tests
def from_lower_pattern(lower, rng, spd):
    """a matrix with a symmetric pattern from the strictly-lower columns of every row: off-diagonals in
    +-[0.1, 1] (symmetric values with spd, independent ones without), a_ii = 1 + the absolute sum of row i
    and of column i - strictly diagonally dominant by rows and by columns, SPD when symmetric"""
    n = len(lower)
    rows, cols, vals = [], [], []
    weight = np.zeros(n)
    for i, ks in enumerate(lower):
        for k in ks:
            a, b = (rng.uniform(0.1, 1.0, 2) * rng.choice([-1.0, 1.0], 2)).tolist()
            if spd:
                b = a
            rows += [i, k]
            cols += [k, i]
            vals += [a, b]
            weight[i] += abs(a) + abs(b)
            weight[k] += abs(a) + abs(b)
    rows += list(range(n))
    cols += list(range(n))
    vals += (1.0 + weight).tolist()
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def chain_pattern(n):
    return [[i - 1] if i else [] for i in range(n)]


def tiers_pattern(w, rng, deps=4, chain=40):
    """2w+37 rows without dependencies, w+1 rows with `deps` dependencies into them, a chain: with the
    wide threshold w the lower schedule is a wide level, a wide level and a narrow run"""
    n0, n1 = 2 * w + 37, w + 1
    lower = [[] for _ in range(n0)]
    lower += [sorted(int(c) for c in rng.choice(n0, deps, replace=False)) for _ in range(n1)]
    lower += [[i - 1] for i in range(n0 + n1, n0 + n1 + chain)]
    return lower


def random_pattern(n, rng, deps=2):
    return [sorted(int(c) for c in rng.choice(i, min(i, deps), replace=False)) if i else [] for i in range(n)]


def hub_pattern(n, hub, n_lower, n_upper):
    """tridiagonal, and row `hub` stores the columns hub - n_lower .. hub + n_upper (the pattern is
    symmetric, so column `hub` stores those rows): the hub row has n_lower + n_upper + 1 entries, its lower
    triangle n_lower + 1, every other row at most 4"""
    assert 1 <= n_lower <= hub and 1 <= n_upper < n - hub
    lower = chain_pattern(n)
    lower[hub] = list(range(hub - n_lower, hub))
    for j in range(hub + 2, hub + n_upper + 1):
        lower[j] = [hub, j - 1]
    return lower


def stencil27(g):
    """the 27-point stencil on g^3 points: diagonal 26, off-diagonals -1"""
    t = sp.diags([np.ones(g - 1), np.ones(g), np.ones(g - 1)], [-1, 0, 1])
    pattern = sp.kron(sp.kron(t, t), t).tocsr()
    return (sp.identity(g ** 3) * 27.0 - pattern).tocsr()


def planted_chain(n, rng):
    """(A, L, U) dense, A = L U exactly: L unit lower bidiagonal, U upper bidiagonal, dyadic entries"""
    lo = np.eye(n) + np.diag(rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], n - 1), -1)
    up = np.diag(rng.choice([0.5, 1.0, 2.0, 4.0], n)) + np.diag(rng.choice([-2.0, -1.0, 1.0, 2.0], n - 1), 1)
    return lo @ up, lo, up


def planted_blocks(count, rng, size=5):
    """(A, L, U) dense, block diagonal with dense blocks, A = L U exactly, dyadic entries"""
    n = count * size
    lo, up = np.eye(n), np.zeros((n, n))
    for b in range(count):
        s = slice(b * size, (b + 1) * size)
        lo[s, s] += np.tril(rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (size, size)), -1)
        up[s, s] = np.triu(rng.choice([-2.0, -1.0, 1.0, 2.0], (size, size)), 1) \
            + np.diag(rng.choice([0.5, 1.0, 2.0, 4.0], size))
    return lo @ up, lo, up


def planted_cholesky(lo):
    """(A, L): the L of a planted L U with its unit diagonal replaced by powers of two; A = L L^T exactly"""
    low = np.tril(lo, -1) + np.diag(np.resize([1.0, 2.0, 0.5, 4.0], lo.shape[0]))
    return low @ low.T, low
