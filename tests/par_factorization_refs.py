"""numpy restatement of the row-synchronous fixed-point sweeps of ParIlu / ParIc (the contract stated in
include/gko_cdna4.h, ginkgo_amd/csrc/par_factorization.hip): sweep t computes every row with the sequential
row step of factorization_refs.ilu0 / ic0, values of OTHER rows from sweep t-1, the row's own values the ones
just computed; v^0 = the input.  Every operation in the array's own dtype, one multiply and one subtract per
update, updates of an entry in ascending k.  Rows are sorted by column.  The matrices of the tests are the
builders of factorization_refs."""
import numpy as np

import factorization_refs as fr


def _bits(v):
    return v.view(np.int64 if v.dtype == np.float64 else np.int32)


def _ilu_sweep(rp, ci, a, prev, at, diag):
    dt = a.dtype.type
    out = a.copy()                          # every row starts from the input
    for i in range(len(rp) - 1):
        row = at[i]
        for p in range(rp[i], diag[i]):
            k = int(ci[p])
            w_ik = dt(out[p] / prev[diag[k]])
            out[p] = w_ik
            for q in range(diag[k] + 1, rp[k + 1]):
                pos = row.get(int(ci[q]))
                if pos is not None:
                    out[pos] = dt(out[pos] - dt(w_ik * prev[q]))
    return out


def _ic_sweep(rp, ci, a, prev, at, diag):
    dt = a.dtype.type
    out = a.copy()
    for i in range(len(rp) - 1):
        assert ci[rp[i + 1] - 1] == i, "the diagonal is not the last entry of row %d" % i
        for p in range(rp[i], rp[i + 1]):
            j = int(ci[p])
            s = a[p]
            other = at[j]
            for q in range(rp[i], p):
                if j == i:
                    s = dt(s - dt(out[q] * out[q]))
                else:
                    pos = other.get(int(ci[q]))
                    if pos is not None:
                        s = dt(s - dt(out[q] * prev[pos]))
            out[p] = dt(s / prev[rp[j + 1] - 1]) if j < i else dt(np.sqrt(s))
    return out


def _sweeps_at(step, rp, ci, vals, counts):
    """{k: (values after k sweeps, entries whose bits sweep k changed)} for the k of `counts`"""
    assert min(counts) >= 1
    at = fr._positions(rp, ci)
    diag = [at[i][i] for i in range(len(rp) - 1)]
    out, v = {}, vals
    with np.errstate(all="ignore"):
        for k in range(1, max(counts) + 1):
            prev, v = v, step(rp, ci, vals, v, at, diag)
            if k in counts:
                out[k] = (v, int(np.count_nonzero(_bits(v) != _bits(prev))))
    return out


def _sweeps(step, rp, ci, vals, iterations):
    return _sweeps_at(step, rp, ci, vals, (iterations,))[iterations]


def ilu_sweeps_at(rp, ci, vals, counts):
    """ilu_sweeps for several numbers of sweeps in one pass: {iterations: (values, changes)}"""
    return _sweeps_at(_ilu_sweep, rp, ci, vals, tuple(counts))


def ic_sweeps_at(rp, ci, vals, counts):
    return _sweeps_at(_ic_sweep, rp, ci, vals, tuple(counts))


def ilu_sweeps(rp, ci, vals, iterations):
    """(values after `iterations` sweeps, the number of entries whose bits the last sweep changed); every row
    stores its diagonal"""
    return _sweeps(_ilu_sweep, rp, ci, vals, iterations)


def ic_sweeps(rp, ci, vals, iterations):
    """the same for a lower-triangular matrix with the diagonal last in every row"""
    return _sweeps(_ic_sweep, rp, ci, vals, iterations)


def num_levels(rp, ci):
    """levels of the lower triangular solve's schedule: level(i) = 1 + the largest level of a stored k < i"""
    n = len(rp) - 1
    level = np.zeros(n, np.int64)
    for i in range(n):
        below = [level[int(k)] for k in ci[rp[i]:rp[i + 1]] if k < i]
        level[i] = 1 + (max(below) if below else 0)
    return int(level.max()) if n else 0


def par_ilu_factors(rp, ci, vals, iterations):
    """(what factorization.ParIlu returns for a sorted matrix that stores every diagonal, the changes)"""
    v, changes = ilu_sweeps(rp, ci, vals, iterations)
    return fr.split_l_u(rp, ci, v), changes


def par_ic_factor(rp, ci, vals, iterations):
    """((l_rp, l_ci, l_v) as factorization.ParIc returns it, the changes)"""
    l_rp, l_ci, l_v = fr.split_l(rp, ci, vals)
    v, changes = ic_sweeps(l_rp, l_ci, l_v, iterations)
    return (l_rp, l_ci, v), changes
