"""numpy restatement of the nested-dissection contract (include/gko_cdna4.h, "Nested dissection"): `order` is the
recursion as the contract words it, on neighbour lists; the functions below it are the stages the device entries
expose, on the same state arrays (order, region), written as plain loops - queues and Python's sort, not the
sweeps, atomics and radix sorts of ginkgo_amd/csrc/reorder.hip.  `by_rounds` drives the stages the way reorder.NestedDissection does; the
CPU tests pin it against the recursion.  Everything is integer-exact."""
from collections import deque

import numpy as np
import scipy.sparse as sp

import symbolic_refs as sr


# ------------------------------------------------------------------ the recursion
def neighbours(a):
    """per vertex the sorted neighbours in G: j != i with (i, j) or (j, i) stored in the square scipy matrix a"""
    s = sr.symmetrized(a)
    return [[int(c) for c in s.indices[s.indptr[i]:s.indptr[i + 1]] if c != i] for i in range(s.shape[0])]


def bfs_levels(adj, inside, root):
    """{vertex: level} of the breadth-first search of G[inside] from root"""
    level = {root: 0}
    queue = deque([root])
    while queue:
        v = queue.popleft()
        for u in adj[v]:
            if u in inside and u not in level:
                level[u] = level[v] + 1
                queue.append(u)
    return level


def components_of(adj, r):
    """the connected components of G[r] as sorted lists, ordered by their smallest vertex"""
    inside, seen, out = set(r), set(), []
    for v in sorted(r):
        if v not in seen:
            comp = sorted(bfs_levels(adj, inside, v))
            seen.update(comp)
            out.append(comp)
    return out


def order(adj, r, leaf_size, trace=None, depth=0):
    """order(R) of the contract.  trace, if a list, receives one dict per split:
    R, A, B, S, m, mstar, h, depth, below (the vertices of a level below m)"""
    r = sorted(r)
    if len(r) <= leaf_size:
        return r
    comps = components_of(adj, r)
    if len(comps) > 1:
        return [v for c in comps for v in order(adj, c, leaf_size, trace, depth)]
    inside = set(r)
    l0 = bfs_levels(adj, inside, r[0])
    last = max(l0.values())
    r1 = min(v for v in r if l0[v] == last)
    lev = bfs_levels(adj, inside, r1)
    h = max(lev.values())
    if h < 2:
        return r
    by_level = sorted(r, key=lambda v: (lev[v], v))
    mstar = lev[by_level[(len(r) + 1) // 2 - 1]]
    m = min(max(mstar, 1), h - 1)
    s = [v for v in r if lev[v] == m and any(u in inside and lev[u] == m + 1 for u in adj[v])]
    in_s = set(s)
    a = [v for v in r if lev[v] < m or (lev[v] == m and v not in in_s)]
    b = [v for v in r if lev[v] > m]
    if trace is not None:
        trace.append(dict(R=r, A=a, B=b, S=s, m=m, mstar=mstar, h=h, depth=depth, below=sum(lev[v] < m for v in r)))
    return order(adj, a, leaf_size, trace, depth + 1) + order(adj, b, leaf_size, trace, depth + 1) + s


def nested_dissection(a, leaf_size, trace=None):
    """perm for the square scipy matrix a: perm[k] = the original index of the vertex at the new position k"""
    adj = neighbours(a)
    return np.array(order(adj, range(len(adj)), leaf_size, trace), np.int64)


def permuted(a, perm):
    """A'[i, j] = A[perm[i], perm[j]] as a sorted csr matrix"""
    m = sp.csr_matrix(sp.csr_matrix(a)[perm][:, perm])
    m.sort_indices()
    return m


def factor_shape(a):
    """(nnz(L), levels of the lower solve with L) for the symbolic Cholesky factor of the scipy matrix a; the
    level of row i is 1 + the largest level of the rows its strictly-lower entries name"""
    rows = sr.cholesky_rows(sr.lower_rows(sr.symmetrized(a)))
    level = np.zeros(len(rows), np.int64)
    for i, cols in enumerate(rows):
        level[i] = 1 + max((level[c] for c in cols[:-1]), default=0)
    return sum(len(r) for r in rows), int(level.max()) if len(rows) else 0


# ------------------------------------------------------------------ the stages, on (row_ptrs, col_idxs) as given
def _row(rp, ci, v):
    return [int(u) for u in ci[rp[v]:rp[v + 1]] if u != v]


def initial_state(n, leaf_size):
    return np.arange(n, dtype=np.int64), np.full(n, -1 if n <= leaf_size else 0, np.int64)


def components(rp, ci, region):
    """(label, sweeps): label[v] = the smallest vertex that v reaches inside its region, -1 for a final v;
    sweeps = 1 + the largest number of edges such a smallest vertex is away (what synchronous min-label
    propagation needs, the last sweep changing nothing)"""
    n = len(region)
    label = np.full(n, -1, np.int64)
    away = 0
    for v in range(n):
        if region[v] < 0 or label[v] >= 0:
            continue
        # v is the smallest unlabelled vertex: with a symmetric pattern what it reaches is its component
        seen = {v: 0}
        queue = deque([v])
        while queue:
            w = queue.popleft()
            for u in _row(rp, ci, w):
                if region[u] == region[w] and u not in seen:
                    seen[u] = seen[w] + 1
                    queue.append(u)
        for u, d in seen.items():
            label[u] = v
            away = max(away, d)
    return label, (away + 1 if n else 0)


def levels(rp, ci, region, root):
    """(level, steps): breadth-first levels of every region from root[region[v]]; -1 for final and unreached
    vertices; steps = 1 + the largest level"""
    n = len(region)
    level = np.full(n, -1, np.int64)
    for s in sorted(set(int(x) for x in region if x >= 0)):
        r = int(root[s])
        if region[r] != s:
            continue
        level[r] = 0
        queue = deque([r])
        while queue:
            w = queue.popleft()
            for u in _row(rp, ci, w):
                if region[u] == s and level[u] < 0:
                    level[u] = level[w] + 1
                    queue.append(u)
    return level, (int(level.max(initial=0)) + 1 if n else 0)


def far_roots(region, level):
    n = len(region)
    far = np.full(n, -1, np.int64)
    for s in set(int(x) for x in region if x >= 0):
        members = [v for v in range(n) if region[v] == s]
        top = max(level[v] for v in members)
        far[s] = min(v for v in members if level[v] == top)
    return far


def split(rp, ci, order_, region, level):
    """class per vertex: 0 = A, 1 = B, 2 = S, 3 = undivided (h < 2), -1 = final"""
    n = len(region)
    cls = np.full(n, -1, np.int64)
    for s in set(int(x) for x in region if x >= 0):
        members = [v for v in range(n) if region[v] == s]
        h = max(level[v] for v in members)
        if h < 2:
            cls[members] = 3
            continue
        by_level = sorted(members, key=lambda v: (level[v], v))
        m = min(max(int(level[by_level[(len(members) + 1) // 2 - 1]]), 1), h - 1)
        for v in members:
            if level[v] != m:
                cls[v] = 0 if level[v] < m else 1
            else:
                cls[v] = 2 if any(region[u] == s and level[u] == m + 1 for u in _row(rp, ci, v)) else 0
    return cls


def regroup(leaf_size, final_from, key, order_, region):
    """(order, region, live) after the stable sort by (segment, key, vertex)"""
    n = len(region)
    pos = np.empty(n, np.int64)
    pos[order_] = np.arange(n)
    keys = [((int(region[v]), int(key[v]), v) if region[v] >= 0 else (int(pos[v]), 0, v)) for v in range(n)]
    new_order = np.array(sorted(range(n), key=lambda v: keys[v]), np.int64).reshape(n)
    new_region = np.full(n, -1, np.int64)
    p = 0
    while p < n:
        q = p
        while q < n and keys[new_order[q]][:2] == keys[new_order[p]][:2]:
            q += 1
        v = new_order[p]
        if region[v] >= 0 and key[v] < final_from and q - p > leaf_size:
            new_region[new_order[p:q]] = p
        p = q
    return new_order, new_region, int((new_region >= 0).sum())


def by_rounds(rp, ci, n, leaf_size):
    """(perm, rounds, launches-that-the-host-waits-for) by the stages, as reorder.NestedDissection drives them"""
    order_, region = initial_state(n, leaf_size)
    live, rounds, waits = int((region >= 0).sum()), 0, 0
    while live:
        assert rounds < n, "a round that divides nothing"
        rounds += 1
        label, sweeps = components(rp, ci, region)
        order_, region, live = regroup(leaf_size, n, label, order_, region)
        waits += sweeps
        if not live:
            break
        level, steps0 = levels(rp, ci, region, order_)
        far = far_roots(region, level)
        level, steps1 = levels(rp, ci, region, far)
        cls = split(rp, ci, order_, region, level)
        order_, region, live = regroup(leaf_size, 2, cls, order_, region)
        waits += steps0 + steps1
    return order_, rounds, waits


# ------------------------------------------------------------------ patterns of the tests
def stencil27(g):
    idx = np.arange(g ** 3).reshape(g, g, g)
    rows, cols = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                src = idx[max(0, -dx):g - max(0, dx), max(0, -dy):g - max(0, dy), max(0, -dz):g - max(0, dz)]
                dst = idx[max(0, dx):g - max(0, -dx), max(0, dy):g - max(0, -dy), max(0, dz):g - max(0, -dz)]
                rows.append(src.ravel())
                cols.append(dst.ravel())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.where(rows == cols, 26.0, -1.0)
    return sp.csr_matrix((vals, (rows, cols)), shape=(g ** 3, g ** 3))


def stencil5(g):
    t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(g, g))
    return sp.csr_matrix(sp.kron(sp.identity(g), t) + sp.kron(t, sp.identity(g)))


def chain(n):
    return sp.csr_matrix(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)))


def of_edges(n, edges, diag=4.0):
    """the symmetric matrix with the given edges (-1) and a diagonal that dominates"""
    r = [i for i, j in edges] + [j for i, j in edges]
    c = [j for i, j in edges] + [i for i, j in edges]
    m = sp.csr_matrix((-np.ones(len(r)), (r, c)), shape=(n, n))
    m.sum_duplicates()
    m.data[:] = -1.0
    deg = np.asarray(abs(m).sum(axis=1)).ravel()
    return sp.csr_matrix(m + sp.diags(deg + diag))


def interleaved(n):
    """two chains, one on the even and one on the odd vertices"""
    return of_edges(n, [(i, i + 2) for i in range(n - 2)])


def clique(n):
    return of_edges(n, [(i, j) for i in range(n) for j in range(i)])


def arrow(n, hub_first):
    hub = 0 if hub_first else n - 1
    return of_edges(n, [(hub, v) for v in range(n) if v != hub])


def star_of_chains(arms, length):
    """vertex 0 with `arms` chains of `length` vertices hanging from it: without 0 it falls into `arms` pieces"""
    edges = []
    for a in range(arms):
        first = 1 + a * length
        edges.append((0, first))
        edges += [(first + k, first + k + 1) for k in range(length - 1)]
    return of_edges(1 + arms * length, edges)


def wide_level():
    """the path 3 - 2 - 1 - 0 with ten more leaves at 2: the second sweep starts at 3, m = 2, S = {1}, and A has
    12 of the 14 vertices"""
    return of_edges(14, [(0, 1), (1, 2), (2, 3)] + [(2, v) for v in range(4, 14)])


def edge_cases():
    """name -> (matrix, leaf_size)"""
    return {
        "empty": (sp.csr_matrix((0, 0)), 8),
        "single": (sp.csr_matrix(np.array([[3.0]])), 8),
        "diagonal": (sp.csr_matrix(sp.identity(30) * 2.0), 8),
        "interleaved": (interleaved(60), 8),
        "clique40": (clique(40), 8),
        "leaf1": (stencil5(7), 1),
        "leaf_all": (interleaved(40), 64),
        "arrow_first": (arrow(100, True), 8),
        "arrow_last": (arrow(100, False), 8),
        "star_of_chains": (star_of_chains(5, 12), 8),
        "wide_level": (wide_level(), 2),
        "unsymmetric": (sr.unsymmetric(), 8),
    }


def csr_arrays(a, index_dtype):
    """(row_ptrs, col_idxs) of the symmetrised pattern, what the class hands to the entries"""
    s = sr.symmetrized(a)
    return s.indptr.astype(index_dtype), s.indices.astype(index_dtype)
