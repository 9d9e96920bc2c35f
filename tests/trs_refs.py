"""numpy restatements of the triangular-solve and Sor set-up loops (the contract of
ginkgo_amd/csrc/trs.hip, i.e. Ginkgo's reference kernels): every operation in the array's own dtype,
one multiply and one subtract per entry, entries in storage order."""
import numpy as np
import scipy.sparse as sp


def trs_solve(rp, ci, vals, b, upper=False, unit_diag=False):
    """x with T x = b for the lower (upper) triangle of the CSR matrix; b is (n, nrhs)"""
    n = len(rp) - 1
    b = np.asarray(b)
    dt = vals.dtype.type
    x = np.zeros((n, b.shape[1]), vals.dtype)
    rows = range(n - 1, -1, -1) if upper else range(n)
    for j in range(b.shape[1]):
        for row in rows:
            t = dt(b[row, j])
            diag = dt(1)
            for k in range(rp[row], rp[row + 1]):
                col = ci[k]
                if (col > row) if upper else (col < row):
                    t = dt(t - dt(vals[k] * x[col, j]))
                elif col == row:
                    diag = vals[k]
            x[row, j] = t if unit_diag else dt(t / diag)
    return x


def levels(rp, ci, upper=False):
    """(level_ptrs, level_rows, level): level[row] = 1 + max level of its dependencies (0 without any);
    rows grouped by level, ascending inside a level"""
    n = len(rp) - 1
    level = np.zeros(n, np.int64)
    for row in (range(n - 1, -1, -1) if upper else range(n)):
        lv = 0
        for k in range(rp[row], rp[row + 1]):
            col = ci[k]
            if (col > row) if upper else (col < row):
                lv = max(lv, level[col] + 1)
        level[row] = lv
    n_levels = int(level.max()) + 1 if n else 0
    level_rows = np.argsort(level, kind="stable").astype(np.int64)
    level_ptrs = np.zeros(n_levels + 1, np.int64)
    np.cumsum(np.bincount(level, minlength=n_levels), out=level_ptrs[1:])
    return level_ptrs, level_rows, level


def _weighted(rp, ci, vals, w, with_u):
    n = len(rp) - 1
    dt = vals.dtype.type
    w = dt(w)
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
        l_v.append(dt(diag / w))
        l_rp[row + 1] = len(l_ci)
        two_minus_w = dt(dt(2) - w)
        u_ci.append(row)
        u_v.append(dt(dt(1) / two_minus_w))
        for k in ks:
            if ci[k] > row:
                u_ci.append(ci[k])
                u_v.append(dt(dt(w * vals[k]) / dt(two_minus_w * diag)))
        u_rp[row + 1] = len(u_ci)
    lower = (l_rp, np.array(l_ci, rp.dtype), np.array(l_v, vals.dtype))
    if not with_u:
        return lower
    return lower + (u_rp, np.array(u_ci, rp.dtype), np.array(u_v, vals.dtype))


def weighted_l(rp, ci, vals, w):
    """(l_rp, l_ci, l_v): strictly-lower entries in storage order, then a_ii / w"""
    return _weighted(rp, ci, vals, w, False)


def weighted_l_u(rp, ci, vals, w):
    """weighted_l plus (u_rp, u_ci, u_v): 1 / (2 - w), then (w a_ij) / ((2 - w) a_ii)"""
    return _weighted(rp, ci, vals, w, True)


# ------------------------------------------------------------------ matrices of the tests
def csr_of(a, index_dtype=np.int32, dtype=np.float64):
    a = sp.csr_matrix(a)
    return a.indptr.astype(index_dtype), a.indices.astype(index_dtype), a.data.astype(dtype)


def from_rows(rows, index_dtype=np.int32, dtype=np.float64):
    """CSR from a list of per-row [(col, val), ...] lists, kept in that order (unsorted allowed)"""
    rp = np.zeros(len(rows) + 1, index_dtype)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c, _ in r], index_dtype)
    v = np.array([x for r in rows for _, x in r], dtype)
    return rp, ci, v


def mirror(rows):
    """the upper-triangular twin of a lower-triangular row list: index i -> n-1-i"""
    n = len(rows)
    return [[(n - 1 - c, v) for c, v in rows[n - 1 - i]] for i in range(n)]


def dyadic(rng, n, count=3):
    """small exactly representable values: off-diagonals in {-2..2}, diagonals in {0.5, 1, 2, 4}"""
    return rng.integers(-2, 3, (n, count)).astype(np.float64), rng.choice([0.5, 1.0, 2.0, 4.0], n)


def chain_rows(n, rng):
    """bidiagonal: row i depends on row i-1 - n levels of one row"""
    off, diag = dyadic(rng, n, 1)
    return [([(i - 1, off[i, 0])] if i else []) + [(i, diag[i])] for i in range(n)]


def tiers_rows(w, rng, deps=4, chain=40):
    """2w+37 rows without dependencies, w+1 rows with `deps` random dependencies into them, a chain of
    `chain` rows: with wide threshold w that is a wide level, a wide level and a narrow run"""
    n0, n1 = 2 * w + 37, w + 1
    n = n0 + n1 + chain
    off, diag = dyadic(rng, n, deps)
    rows = [[(i, diag[i])] for i in range(n0)]
    for i in range(n0, n0 + n1):
        cols = rng.choice(n0, deps, replace=False)
        rows.append([(int(c), off[i, k]) for k, c in enumerate(cols)] + [(i, diag[i])])
    for i in range(n0 + n1, n):
        rows.append([(i - 1, off[i, 0]), (i, diag[i])])
    return rows


def planted(rows, rng, nrhs=1):
    """(x, b) with b = T x exactly: x integer in [-3, 3], dyadic entries - every intermediate of the
    solve is an exactly representable number, whatever the order"""
    n = len(rows)
    x = rng.integers(-3, 4, (n, nrhs)).astype(np.float64)
    b = np.zeros((n, nrhs))
    for i, r in enumerate(rows):
        for c, v in r:
            b[i] += v * x[c]
    return x, b
