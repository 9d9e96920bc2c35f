"""numpy restatement of ParIlut / ParIct (the contract stated in include/gko_cdna4.h, "ParIlut / ParIct";
ginkgo_amd/csrc/par_ilut.hip, ginkgo_amd/factorization.py) on CSR arrays: the pattern of L U (L L^T) + A', the
candidate values, one sweep, the exact thresholds by rank of u(v) = the bits of |v|, the filter, one sweep.
Every operation in the array's own dtype, one multiply and one subtract per update, updates of an entry in
ascending k.  Rows are sorted by column and every row stores its diagonal.  The sweeps are the row steps of
par_factorization_refs with v^0 given apart from a."""
import math

import numpy as np

import factorization_refs as fr
import par_factorization_refs as pr


# ------------------------------------------------------------------ the pieces (one per entry of the library)
def u_of(v):
    """the bit pattern of |v| as an unsigned integer: -0 is 0, NaN ranks above inf"""
    v = np.ascontiguousarray(v)
    if v.dtype == np.float64:
        return v.view(np.uint64) & np.uint64(0x7fffffffffffffff)
    return v.view(np.uint32) & np.uint32(0x7fffffff)


def value_of(u, dtype):
    return np.array([u], np.uint64 if dtype == np.float64 else np.uint32).view(dtype)[0]


def threshold(values, keep):
    """+0 if there are at most `keep` values, else the non-negative value whose u has rank len - keep (0-based,
    ascending) among them"""
    assert keep >= 1
    count = len(values)
    if count <= keep:
        return values.dtype.type(0)
    return value_of(np.sort(u_of(values))[count - keep], values.dtype)


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def part_threshold(rp, ci, v, part, keep):
    """the threshold of the strictly-lower (part 0) or strictly-upper (part 1) entries"""
    rows = rows_of(rp)
    return threshold(v[ci < rows] if part == 0 else v[ci > rows], keep)


def keep_mask(rp, ci, v, thr_lower, thr_upper=None):
    """1 for a kept entry, 0 for a dropped one: the diagonal always, an off-diagonal iff u(v) >= u(threshold of
    its part); thr_upper None: a lower-triangular factor, nothing right of the diagonal is kept"""
    rows, u = rows_of(rp), u_of(v)
    keep = rows == ci
    keep |= (ci < rows) & (u >= u_of(np.array([thr_lower], v.dtype))[0])
    if thr_upper is not None:
        keep |= (ci > rows) & (u >= u_of(np.array([thr_upper], v.dtype))[0])
    return keep.astype(v.dtype)


def gather(p_rp, p_ci, s_rp, s_ci, s_v):
    """src at the positions of the pattern, +0 where src stores none"""
    at = fr._positions(s_rp, s_ci)
    out = np.zeros(len(p_ci), s_v.dtype)
    for i in range(len(p_rp) - 1):
        for p in range(p_rp[i], p_rp[i + 1]):
            pos = at[i].get(int(p_ci[p]))
            if pos is not None:
                out[p] = s_v[pos]
    return out


def _csr_of_rows(cols, index_dtype):
    rp = np.zeros(len(cols) + 1, index_dtype)
    rp[1:] = np.cumsum([len(c) for c in cols])
    flat = [j for c in cols for j in sorted(c)]
    return rp, np.array(flat, index_dtype)


def ilut_pattern(m_rp, m_ci, a_rp, a_ci):
    """pattern(L U) + pattern(A'), L = the strictly-lower part of M with a unit diagonal, U = the rest"""
    n = len(m_rp) - 1
    upper = [[int(j) for j in m_ci[m_rp[k]:m_rp[k + 1]] if j >= k] for k in range(n)]
    cols = []
    for i in range(n):
        row = set(int(j) for j in a_ci[a_rp[i]:a_rp[i + 1]])
        for k in [int(k) for k in m_ci[m_rp[i]:m_rp[i + 1]] if k < i] + [i]:
            row.update(upper[k])
        cols.append(row)
    return _csr_of_rows(cols, m_rp.dtype)


def ict_pattern(l_rp, l_ci, a_rp, a_ci):
    """the lower triangle of pattern(L L^T) + the lower pattern of A'"""
    n = len(l_rp) - 1
    by_col = [[] for _ in range(n)]                 # rows that store column k
    for i in range(n):
        for k in l_ci[l_rp[i]:l_rp[i + 1]]:
            by_col[int(k)].append(i)
    cols = []
    for i in range(n):
        row = set(int(j) for j in a_ci[a_rp[i]:a_rp[i + 1]] if j <= i)
        for k in l_ci[l_rp[i]:l_rp[i + 1]]:
            row.update(j for j in by_col[int(k)] if j <= i)
        cols.append(row)
    return _csr_of_rows(cols, l_rp.dtype)


def ilut_candidates(p_rp, p_ci, a_rp, a_ci, a_v, m_rp, m_ci, m_v):
    dt = m_v.dtype.type
    m_at, a_at = fr._positions(m_rp, m_ci), fr._positions(a_rp, a_ci)
    out = np.zeros(len(p_ci), m_v.dtype)
    with np.errstate(all="ignore"):
        for i in range(len(p_rp) - 1):
            for p in range(p_rp[i], p_rp[i + 1]):
                j = int(p_ci[p])
                pos = m_at[i].get(j)
                if pos is not None:
                    out[p] = m_v[pos]
                    continue
                pos = a_at[i].get(j)
                s = a_v[pos] if pos is not None else dt(0)
                for q in range(m_rp[i], m_rp[i + 1]):
                    k = int(m_ci[q])
                    if k >= min(i, j):
                        break
                    pos = m_at[k].get(j)
                    if pos is not None:
                        s = dt(s - dt(m_v[q] * m_v[pos]))
                out[p] = dt(s / m_v[m_at[j][j]]) if j < i else s
    return out


def ict_candidates(p_rp, p_ci, a_rp, a_ci, a_v, l_rp, l_ci, l_v):
    dt = l_v.dtype.type
    l_at, a_at = fr._positions(l_rp, l_ci), fr._positions(a_rp, a_ci)
    out = np.zeros(len(p_ci), l_v.dtype)
    with np.errstate(all="ignore"):
        for i in range(len(p_rp) - 1):
            for p in range(p_rp[i], p_rp[i + 1]):
                j = int(p_ci[p])
                pos = l_at[i].get(j)
                if pos is not None:
                    out[p] = l_v[pos]
                    continue
                assert j < i
                pos = a_at[i].get(j)
                s = a_v[pos] if pos is not None else dt(0)
                for q in range(l_rp[i], l_rp[i + 1]):
                    k = int(l_ci[q])
                    if k >= j:
                        break
                    pos = l_at[j].get(k)
                    if pos is not None:
                        s = dt(s - dt(l_v[q] * l_v[pos]))
                out[p] = dt(s / l_v[l_rp[j + 1] - 1])
    return out


def sweep_from(kind, rp, ci, a, v0):
    """one sweep of par_factorization_refs: every row starts from a, other rows are read from v0"""
    at = fr._positions(rp, ci)
    diag = [at[i][i] for i in range(len(rp) - 1)]
    with np.errstate(all="ignore"):
        return (pr._ilu_sweep if kind == "ilu" else pr._ic_sweep)(rp, ci, a, v0, at, diag)


def keep_counts(rp, ci, fill_in_limit):
    """(keep_L, keep_U) of the prepared matrix"""
    rows = rows_of(rp)
    return tuple(max(1, int(math.floor(fill_in_limit * int(np.count_nonzero(part)))))
                 for part in (ci < rows, ci > rows))


def filtered(rp, ci, mask):
    keep = mask != 0
    out = np.zeros_like(rp)
    out[1:] = np.cumsum(np.bincount(rows_of(rp)[keep], minlength=len(rp) - 1))
    return out, ci[keep]


# ------------------------------------------------------------------ the loops
def _iteration(kind, a, low, m, keep):
    """(M_t, the pattern P of the iteration) from M_{t-1}; a = A', low = its lower triangle for ic"""
    if kind == "ilu":
        p_rp, p_ci = ilut_pattern(m[0], m[1], a[0], a[1])
        v = ilut_candidates(p_rp, p_ci, *a, *m)
        src = a
    else:
        p_rp, p_ci = ict_pattern(m[0], m[1], a[0], a[1])
        v = ict_candidates(p_rp, p_ci, *a, *m)
        src = low
    v = sweep_from(kind, p_rp, p_ci, gather(p_rp, p_ci, *src), v)
    thr_lower = part_threshold(p_rp, p_ci, v, 0, keep[0])
    thr_upper = part_threshold(p_rp, p_ci, v, 1, keep[1]) if kind == "ilu" else None
    mask = keep_mask(p_rp, p_ci, v, thr_lower, thr_upper)
    q_rp, q_ci = filtered(p_rp, p_ci, mask)
    v = sweep_from(kind, q_rp, q_ci, gather(q_rp, q_ci, *src), gather(q_rp, q_ci, p_rp, p_ci, v))
    return (q_rp, q_ci, v), (p_rp, p_ci)


def par_ilut_at(rp, ci, vals, counts, fill_in_limit, patterns=None):
    """{iterations: the combined matrix M (rp, ci, v)} of ParIlut on the prepared matrix for the iteration
    counts of `counts`; `patterns` (a list) receives the pattern P of every iteration"""
    a, m = (rp, ci, vals), (rp, ci, vals)
    keep, out = keep_counts(rp, ci, fill_in_limit), {}
    for t in range(1, max(counts) + 1):
        m, p = _iteration("ilu", a, None, m, keep)
        if patterns is not None:
            patterns.append(p)
        if t in counts:
            out[t] = m
    return out


def par_ict_at(rp, ci, vals, counts, fill_in_limit, patterns=None):
    """{iterations: the factor L (rp, ci, v), diagonal last in every row} of ParIct on the prepared matrix"""
    a, low, m = (rp, ci, vals), fr.split_l(rp, ci, vals), fr.split_l(rp, ci, vals, diag_sqrt=True)
    keep, out = keep_counts(rp, ci, fill_in_limit), {}
    for t in range(1, max(counts) + 1):
        m, p = _iteration("ic", a, low, m, keep)
        if patterns is not None:
            patterns.append(p)
        if t in counts:
            out[t] = m
    return out


def par_ilut_factors(rp, ci, vals, iterations, fill_in_limit):
    """(l_rp, l_ci, l_v, u_rp, u_ci, u_v) as factorization.ParIlut returns them"""
    return fr.split_l_u(*par_ilut_at(rp, ci, vals, (iterations,), fill_in_limit)[iterations])


def par_ict_factor(rp, ci, vals, iterations, fill_in_limit):
    """(l_rp, l_ci, l_v) as factorization.ParIct returns it"""
    return par_ict_at(rp, ci, vals, (iterations,), fill_in_limit)[iterations]


# ------------------------------------------------------------------ matrices of the tests
def arrow(n, spd, rng=None):
    """dense first row and column (the hub), a diagonal; strictly diagonally dominant.  One elimination step
    fills the whole matrix, and the lower solve of the full pattern has n levels... of which the fixed-point
    sweeps need few: the Schur complement of the hub is a rank-one change of a diagonal"""
    rng = rng or np.random.default_rng(8)
    a = np.zeros((n, n))
    a[0, 1:] = rng.uniform(0.1, 1.0, n - 1)
    a[1:, 0] = a[0, 1:] if spd else rng.uniform(0.1, 1.0, n - 1)
    a[np.arange(n), np.arange(n)] = 2.0 + np.abs(a).sum(0) + np.abs(a).sum(1)
    return a
