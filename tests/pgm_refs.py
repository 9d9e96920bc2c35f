"""numpy restatement of the Pgm aggregation contract (include/gko_cdna4.h, "Pgm aggregation"), of the coarse
operator and the two transfers, and of the Multigrid cycle - written from the contract, not from the kernels.

Everything takes and returns host arrays.  Matrices are (row_ptrs, col_idxs, values) triples with sorted rows
and no duplicates; `dtype` is the value type T in which the contract's arithmetic is done (np.float32,
np.float64, or np.longdouble for the cycle's yardstick)."""
import numpy as np
import scipy.sparse as sp


# --------------------------------------------------------------------------- matrices of the tests
def stencil27(g):
    """27-point stencil on a g^3 grid, diagonal 26, off-diagonals -1, x-fastest numbering, sorted rows"""
    one = sp.diags([np.ones(g - 1), np.ones(g), np.ones(g - 1)], [-1, 0, 1])
    a = -sp.kron(sp.kron(one, one), one).tocsr()
    a.setdiag(26.0)
    a = a.tocsr()
    a.sort_indices()
    return a


def chain(n):
    return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()


def star(leaves):
    """hub 0 with `leaves` leaves: hub diagonal `leaves`, leaf diagonal 2, off-diagonals -1"""
    n = leaves + 1
    rows = np.concatenate([np.arange(n), np.zeros(leaves, int), np.arange(1, n)])
    cols = np.concatenate([np.arange(n), np.arange(1, n), np.zeros(leaves, int)])
    vals = np.concatenate([[float(leaves)], 2.0 * np.ones(leaves), -np.ones(2 * leaves)])
    a = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    a.sort_indices()
    return a


def triple(a, dtype=np.float64, index_dtype=np.int64):
    a = a.tocsr()
    return a.indptr.astype(index_dtype), a.indices.astype(index_dtype), np.asarray(a.data).astype(dtype)


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


# --------------------------------------------------------------------------- sums in storage order
def _run_sums(starts, lengths, vals, dtype):
    """for every run (start, length) of vals: 0 + v0 + v1 + ... added one after the other in `dtype`"""
    sums = np.zeros(len(starts), dtype)
    for k in range(int(lengths.max()) if len(lengths) else 0):
        sel = np.nonzero(lengths > k)[0]
        sums[sel] = sums[sel] + vals[starts[sel] + k]
    return sums


def _sum_sorted_triplets(rows, cols, vals, dtype):
    """stable sort by (row, column), then one entry per (row, column) with the run's sum in storage order"""
    order = np.lexsort((cols, rows))            # stable
    rows, cols, vals = rows[order], cols[order], vals[order]
    first = np.ones(len(rows), bool)
    first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    starts = np.nonzero(first)[0]
    lengths = np.diff(np.append(starts, len(rows)))
    return rows[starts], cols[starts], _run_sums(starts, lengths, vals, dtype)


def _ptrs(rows, n):
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)


def spmv(rp, ci, v, x):
    """y = A x, every row summed in storage order in the dtype of v; x is (n, cols)"""
    lengths = np.diff(rp)
    y = np.zeros((len(rp) - 1, x.shape[1]), v.dtype)
    for k in range(int(lengths.max()) if len(lengths) else 0):
        sel = np.nonzero(lengths > k)[0]
        pos = rp[sel] + k
        y[sel] = y[sel] + v[pos, None] * x[ci[pos]]
    return y


# --------------------------------------------------------------------------- weights
def weights(rp, ci, v, dtype):
    """W = 0.5 |A| + 0.5 |A^T| on the pattern of A u A^T, rows sorted, and d = diag(W) (0 where not stored)"""
    n = len(rp) - 1
    ri = rows_of(rp)
    half = np.asarray(0.5, dtype) * np.abs(v.astype(dtype))
    wr, wc, wv = _sum_sorted_triplets(np.concatenate([ri, ci]), np.concatenate([ci.astype(np.int64), ri]),
                                      np.concatenate([half, half]), dtype)
    d = np.zeros(n, dtype)
    on_diag = wr == wc
    d[wr[on_diag]] = wv[on_diag]
    return _ptrs(wr, n), wc, wv, d


def pair_hash(i, j):
    lo = np.minimum(i, j).astype(np.uint64) & 0xFFFFFFFF
    hi = np.maximum(i, j).astype(np.uint64) & 0xFFFFFFFF
    m = np.uint64(0xFFFFFFFF)
    h = ((lo * np.uint64(0x9E3779B1)) & m) ^ ((hi * np.uint64(0x85EBCA77)) & m)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    return h


def _best(mask, ri, cj, s, h, n):
    """per row the column of the entry with the largest key (s, h, j) among the entries in `mask`, -1: none"""
    idx = np.nonzero(mask)[0]
    out = np.full(n, -1, np.int64)
    if len(idx):
        order = idx[np.lexsort((cj[idx], h[idx], s[idx], ri[idx]))]
        last = np.ones(len(order), bool)
        last[:-1] = ri[order][1:] != ri[order][:-1]
        out[ri[order][last]] = cj[order][last]
    return out


def aggregate(rp, ci, v, dtype, max_iterations=15, max_unassign_ratio=0.05):
    """-> dict(agg (coarse indices), roots (agg before renumbering), n_coarse, rounds, leftover)"""
    n = len(rp) - 1
    w_rp, w_ci, w_v, d = weights(rp, ci, v, dtype)
    ri, cj = rows_of(w_rp), w_ci
    with np.errstate(divide="ignore", invalid="ignore"):
        s = w_v / np.maximum(d[ri], d[cj])              # one division in T
    valid = (cj != ri) & (s >= 0)
    h = pair_hash(ri, cj)
    agg = np.full(n, -1, np.int64)
    everyone = np.arange(n)
    rounds, previous, count = 0, None, n
    for _ in range(max_iterations):
        free = agg == -1                                 # the snapshot the whole round reads
        u = _best(valid & free[ri] & free[cj], ri, cj, s, h, n)
        g = _best(valid & free[ri] & ~free[cj], ri, cj, s, h, n)
        proposal = np.where(u >= 0, u, everyone)
        joins = free & (u < 0) & (g >= 0)
        proposes = free & ~joins
        new = agg.copy()
        new[joins] = agg[g[joins]]
        i = everyone[proposes]
        k = proposal[i]
        mutual = proposes[k] & (proposal[k] == i)
        new[i[mutual]] = np.minimum(i, k)[mutual]
        agg = new
        rounds += 1
        count = int((agg == -1).sum())
        if count == 0 or count == previous or count < max_unassign_ratio * n:
            break
        previous = count
    leftover = count
    if leftover:
        free = agg == -1
        g = _best(valid & free[ri] & ~free[cj], ri, cj, s, h, n)
        new = agg.copy()
        new[free] = np.where(g[free] >= 0, agg[np.maximum(g[free], 0)], everyone[free])
        agg = new
    is_root = agg == everyone
    rank = np.cumsum(is_root) - 1
    return {"roots": agg, "agg": rank[agg], "n_coarse": int(is_root.sum()), "rounds": rounds,
            "leftover": leftover}


# --------------------------------------------------------------------------- coarse operator, transfers
def coarse_operator(rp, ci, v, agg, n_coarse, dtype):
    """P^T A P through the triplets (agg_i, agg_j, a_ij) in storage order: stable sort, sequential sums"""
    rows, cols, vals = _sum_sorted_triplets(agg[rows_of(rp)], agg[ci], v.astype(dtype), dtype)
    return _ptrs(rows, n_coarse), cols, vals


def restrict(agg, n_coarse, r):
    """b_c[J] = the sum over the members of J, ascending, one after the other; r is (n, cols)"""
    order = np.argsort(agg, kind="stable")
    ptrs = _ptrs(agg, n_coarse)
    out = np.zeros((n_coarse, r.shape[1]), r.dtype)
    lengths = np.diff(ptrs)
    for k in range(int(lengths.max())):
        sel = np.nonzero(lengths > k)[0]
        out[sel] = out[sel] + r[order[ptrs[sel] + k]]
    return out


def prolong_add(agg, e, x):
    return x + e[agg]


# --------------------------------------------------------------------------- hierarchy and cycle
def hierarchy(rp, ci, v, dtype, max_levels=10, min_coarse_rows=64, aggs=None, agg_dtype=None, **pgm):
    """list of levels {rp, ci, v, agg, n_coarse}; the last has agg None.  `aggs`: take these aggregations
    (of another value type's hierarchy) instead of computing them - the longdouble yardstick does"""
    levels = []
    v = v.astype(dtype)
    while True:
        n = len(rp) - 1
        level = {"rp": rp, "ci": ci, "v": v, "agg": None, "n_coarse": None}
        levels.append(level)
        if len(levels) >= max_levels or n <= min_coarse_rows:
            break
        if aggs is not None:
            if len(levels) > len(aggs):
                break
            agg, n_c = aggs[len(levels) - 1]
        else:
            res = aggregate(rp, ci, v, agg_dtype or dtype, **pgm)
            agg, n_c = res["agg"], res["n_coarse"]
        if n_c >= n:
            break
        level["agg"], level["n_coarse"] = agg, n_c
        rp, ci, v = coarse_operator(rp, ci, v, agg, n_c, dtype)
    return levels


def _diag(level):
    rp, ci, v = level["rp"], level["ci"], level["v"]
    d = np.zeros(len(rp) - 1, v.dtype)
    on = rows_of(rp) == ci
    d[rows_of(rp)[on]] = v[on]
    return d


def _sweeps(level, b, x, count, relax):
    """count sweeps x <- x + relax D^-1 (b - A x); x None: the zero guess, whose first sweep needs no product"""
    dtype = b.dtype
    winv = (np.asarray(relax, dtype) * (np.asarray(1, dtype) / _diag(level)))[:, None]
    for _ in range(count):
        if x is None:
            x = b * winv
        else:
            x = x + (b - spmv(level["rp"], level["ci"], level["v"], x)) * winv
    return x


def cycle(levels, b, x=None, kind="v", relax=0.9, iters=1, coarse_iters=4, l=0):
    """one multigrid cycle on level l in the dtype of b ((n, cols)); x None: zero initial guess"""
    level = levels[l]
    if l == len(levels) - 1:
        return _sweeps(level, b, x, coarse_iters, relax)
    x = _sweeps(level, b, x, iters, relax)
    r = b - spmv(level["rp"], level["ci"], level["v"], x)
    bc = restrict(level["agg"], level["n_coarse"], r)
    xc = cycle(levels, bc, None, kind, relax, iters, coarse_iters, l + 1)
    if kind == "w":
        xc = cycle(levels, bc, xc, kind, relax, iters, coarse_iters, l + 1)
    x = prolong_add(level["agg"], xc, x)
    return _sweeps(level, b, x, iters, relax)


def pcg_iterations(a, b, precond, reduction=1e-10, max_iters=1000):
    """iterations of preconditioned CG from a zero guess until ||r|| <= reduction ||b||, counted as Cg does"""
    x, r = np.zeros_like(b), b.copy()
    p, rho_old = np.zeros_like(b), 1.0
    target = reduction * np.linalg.norm(b)
    for it in range(max_iters + 1):
        z = precond(r)
        rho = r @ z
        if np.linalg.norm(r) <= target:
            return it
        p = z + (rho / rho_old) * p
        q = a @ p
        alpha = rho / (p @ q)
        x, r, rho_old = x + alpha * p, r - alpha * q, rho
    return max_iters


def stationary_iterations(a, b, levels, reduction, kind="v", max_iters=100):
    """cycles of x <- cycle(b, x) from a zero guess until ||b - A x|| <= reduction ||b||"""
    x = np.zeros((len(b), 1), b.dtype)
    target = reduction * np.linalg.norm(b)
    for it in range(max_iters + 1):
        if np.linalg.norm(b - a @ x[:, 0]) <= target:
            return it
        x = cycle(levels, b[:, None], x, kind)
    return max_iters
