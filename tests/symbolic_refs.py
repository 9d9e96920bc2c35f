"""numpy restatement of the symbolic Cholesky contract (include/gko_cdna4.h, "Symbolic Cholesky / sparse
direct"): the elimination forest with its postorder, and the pattern of L by ROW MARKS (cs_ereach style) - not
the skeleton walk of ginkgo_amd/csrc/symbolic.hip.  `dense_fill` is boolean elimination, the definition both are
pinned against.  Everything is integer-exact."""
import numpy as np
import scipy.sparse as sp


def symmetrized(a):
    """the pattern S = A + A^T + I of a square scipy matrix (explicit zeros count as stored) as a sorted
    boolean csr matrix"""
    a = sp.csr_matrix(a)
    n = a.shape[0]
    p = sp.csr_matrix((np.ones(len(a.indices)), a.indices, a.indptr), shape=a.shape)
    s = sp.csr_matrix(p + p.T + sp.identity(n))
    s.sort_indices()
    return s


def lower_rows(s):
    """per row the strictly-lower columns of the sorted csr pattern s, ascending"""
    return [[int(c) for c in s.indices[s.indptr[i]:s.indptr[i + 1]] if c < i] for i in range(s.shape[0])]


def forest(lower):
    """(parent, post, first) of the elimination forest of the pattern whose row i has the strictly-lower
    columns lower[i]: Liu's algorithm with path compression; postorder with children and roots in ascending
    index; first[v] = the smallest post rank in the subtree of v"""
    n = len(lower)
    parent, ancestor = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for i in range(n):
        for j in lower[i]:
            r = j
            while r != -1 and r < i:
                nxt = ancestor[r]
                ancestor[r] = i
                if nxt == -1:
                    parent[r] = i
                r = nxt
    children = [[] for _ in range(n)]
    for v in range(n):
        if parent[v] >= 0:
            children[parent[v]].append(v)
    post, first = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rank = 0
    for root in range(n):
        if parent[root] != -1:
            continue
        stack = [(root, 0)]
        while stack:
            v, k = stack.pop()
            if k < len(children[v]):
                stack.append((v, k + 1))
                stack.append((children[v][k], 0))
            else:
                post[v] = rank
                rank += 1
    size = np.ones(n, np.int64)
    for v in range(n):
        if parent[v] >= 0:
            size[parent[v]] += size[v]
    first[:] = post - size + 1
    return parent, post, first


def cholesky_rows(lower, parent=None):
    """per row the sorted columns of L (diagonal last) by row marks: from every strictly-lower neighbour
    climb the forest until a vertex already marked for this row (or the row itself)"""
    n = len(lower)
    if parent is None:
        parent = forest(lower)[0]
    mark = np.full(n, -1, np.int64)
    rows = []
    for i in range(n):
        mark[i] = i
        found = []
        for j in lower[i]:
            a = j
            while mark[a] != i:
                mark[a] = i
                found.append(int(a))
                a = parent[a]
        rows.append(sorted(found) + [i])
    return rows


def skeleton_rows(lower, parent, post, first):
    """the same rows by the device's skeleton rule (symbolic.hip), so that the rule itself is checked without a
    device: the neighbours by post rank, every path cut at the first ancestor of the next neighbour (of the row
    for the last one).  Returns (rows, look-ups): the look-ups are nnz(L) - n exactly."""
    n = len(lower)
    inv = np.zeros(n, np.int64)
    inv[post] = np.arange(n)
    rows, lookups = [], 0
    for i in range(n):
        keys = sorted(int(post[j]) for j in lower[i]) + [int(post[i])]
        found = []
        for t in range(len(keys) - 1):
            a, bound = inv[keys[t]], keys[t + 1]
            while 0 <= a < i and not (first[a] <= bound <= post[a]):
                found.append(int(a))
                a = parent[a]
                lookups += 1
        assert len(set(found)) == len(found), "the pieces of the skeleton overlap"
        rows.append(sorted(found) + [i])
    return rows, lookups


def csr_of_rows(rows, index_dtype=np.int32):
    rp = np.zeros(len(rows) + 1, index_dtype)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    ci = np.array([c for r in rows for c in r], index_dtype)
    return rp, ci


def cholesky_pattern(a, index_dtype=np.int32):
    """(row_ptrs, col_idxs) of L for the square scipy matrix a: what factorization.Cholesky.get_symbolic() and
    get_l_factor() carry"""
    return csr_of_rows(cholesky_rows(lower_rows(symmetrized(a))), index_dtype)


def lu_pattern(a, index_dtype=np.int32):
    """(row_ptrs, col_idxs) of the combined pattern of factorization.Lu: row i of L, then row i of L^T right of
    the diagonal"""
    rp, ci = cholesky_pattern(a, np.int64)
    n = len(rp) - 1
    low = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    m = sp.csr_matrix(low + sp.tril(low, -1).T)
    m.sort_indices()
    return m.indptr.astype(index_dtype), m.indices.astype(index_dtype)


def on_filled_pattern(a, rp, ci, dtype):
    """the values of the scipy matrix a at the positions of the sorted pattern, +0 where a stores none"""
    a = sp.csr_matrix(a)
    a.sort_indices()
    out = np.zeros(len(ci), dtype)
    for i in range(len(rp) - 1):
        cols = a.indices[a.indptr[i]:a.indptr[i + 1]]
        vals = a.data[a.indptr[i]:a.indptr[i + 1]]
        where = dict(zip(cols.tolist(), vals.tolist()))
        for k in range(rp[i], rp[i + 1]):
            out[k] = where.get(int(ci[k]), 0.0)
    return out


def dense_fill(s):
    """the lower triangle (diagonal included) of the filled pattern of the symmetric boolean dense matrix s:
    boolean right-looking elimination, the definition"""
    f = np.array(s, dtype=bool)
    n = f.shape[0]
    f |= f.T
    f |= np.eye(n, dtype=bool)
    for k in range(n):
        below = np.nonzero(f[k + 1:, k])[0] + k + 1
        if len(below):
            f[np.ix_(below, below)] = True
    return np.tril(f)


# ------------------------------------------------------------------ patterns of the tests
def arrow_first(n):
    """dense first row and column: fills completely"""
    return [[0] if i else [] for i in range(n)]


def arrow_last(n):
    """dense last row and column: no fill, one row of n entries"""
    return [[] for _ in range(n - 1)] + [list(range(n - 1))]


def blocks(lower_a, lower_b):
    """two disjoint blocks"""
    shift = len(lower_a)
    return [list(r) for r in lower_a] + [[c + shift for c in r] for r in lower_b]


def matrix_of_lower(lower):
    """the symmetric 0/1 pattern (with every diagonal) as a scipy matrix"""
    n = len(lower)
    rows = [i for i, ks in enumerate(lower) for _ in ks]
    cols = [k for ks in lower for k in ks]
    m = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    return sp.csr_matrix(m + m.T + sp.identity(n))


def unsymmetric(n=200, density=0.01, seed=7):
    """sp.random(n, n, density) + 5 I: an unsymmetric pattern"""
    rng = np.random.default_rng(seed)
    return sp.csr_matrix(sp.random(n, n, density, random_state=rng, format="csr") + 5.0 * sp.identity(n))
