"""The numpy restatement of ParIlut / ParIct (tests/par_ilut_refs.py) pinned on the CPU: what the device tests
compare against is itself right where that can be said without a device."""
import numpy as np
import pytest
import scipy.sparse as sp

import factorization_refs as fr
import par_ilut_refs as tr

N = 8


def pattern_of(m):
    return m[0].tolist(), m[1].tolist()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_closure_anchor_ilu(dtype):
    """the arrow matrix with its hub in row / column 0 and a limit that drops nothing: the pattern is full after
    the first iteration, and after 5 iterations the factors are the exact ILU on the full pattern = the dense LU
    without pivoting, bit for bit"""
    a = tr.arrow(N, False)
    rp, ci, v = fr.on_pattern(a, a != 0, dtype=dtype)
    patterns = []
    out = tr.par_ilut_at(rp, ci, v, (1, 3, 5), 100.0, patterns)
    full = fr.on_pattern(a, np.ones((N, N), bool), dtype=dtype)
    assert all(pattern_of(p) == pattern_of(full) for p in patterns)
    assert all(pattern_of(out[k]) == pattern_of(full) for k in out)
    exact = fr.ilu0(*full)
    assert np.array_equal(out[5][2], exact)
    assert not np.array_equal(out[1][2], exact)
    for got, want in zip(tr.par_ilut_factors(rp, ci, v, 5, 100.0), fr.split_l_u(full[0], full[1], exact)):
        assert np.array_equal(got, want)
    # the dense LU without pivoting, to rounding
    dense = fr.dense_of(full[0], full[1], exact, np.float64)
    lower, upper = np.tril(dense, -1) + np.eye(N), np.triu(dense)
    assert np.abs(lower @ upper - a).max() <= 50 * np.finfo(dtype).eps * np.abs(a).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_closure_anchor_ic(dtype):
    a = tr.arrow(N, True)
    rp, ci, v = fr.on_pattern(a, a != 0, dtype=dtype)
    patterns = []
    out = tr.par_ict_at(rp, ci, v, (1, 5), 100.0, patterns)
    full = fr.on_pattern(a, np.tril(np.ones((N, N), bool)), dtype=dtype)
    assert all(pattern_of(p) == pattern_of(full) for p in patterns)
    exact = fr.ic0(*full)
    assert pattern_of(out[5]) == pattern_of(full) and np.array_equal(out[5][2], exact)
    assert not np.array_equal(out[1][2], exact)
    low = fr.dense_of(full[0], full[1], exact, np.float64)
    assert np.abs(low @ low.T - a).max() <= 50 * np.finfo(dtype).eps * np.abs(a).max()


def random_case(spd, n=60, seed=3):
    """tie-free: off-diagonals are distinct irrationals"""
    rng = np.random.default_rng(seed)
    return fr.from_lower_pattern(fr.random_pattern(n, rng, 3), rng, spd)


def dominant_case(spd, n=60, seed=4):
    """tie-free random values on a random pattern (at most 3 lower entries per row), off-diagonals in
    +-[0.5, 1], diagonal in [40, 41].  Every fill candidate is a sum of at most 3 products l_ik u_kj with
    |l_ik| <= 1 / 39 and |u_kj| <= 1.1, so below 0.09, while an entry on the pattern of A stays above 0.5 - 0.09
    (upper) or that over 41 (lower, where a candidate is at most 0.09 / 39): by magnitude, fill always loses"""
    rng = np.random.default_rng(seed)
    a = fr.from_lower_pattern(fr.random_pattern(n, rng, 3), rng, spd).tolil()
    for i in range(n):
        for j in a.rows[i]:
            if i != j and (not spd or j < i):
                a[i, j] = np.sign(a[i, j]) * (0.5 + 0.5 * abs(a[i, j]))
                if spd:
                    a[j, i] = a[i, j]
    a.setdiag(40.0 + rng.uniform(0, 1, n))
    return a.tocsr()


@pytest.mark.parametrize("kind", ["ilu", "ic"])
def test_fill_in_limit_one_returns_to_the_pattern_of_a(kind):
    a = dominant_case(kind == "ic")
    assert len(np.unique(np.abs(a.data))) == (a.nnz if kind == "ilu" else (a.nnz + a.shape[0]) // 2)
    rp, ci, v = fr.arrays(a)
    patterns = []
    if kind == "ilu":
        out = tr.par_ilut_at(rp, ci, v, (1, 2, 3), 1.0, patterns)
        want = (rp, ci)
    else:
        out = tr.par_ict_at(rp, ci, v, (1, 2, 3), 1.0, patterns)
        want = fr.split_l(rp, ci, v)[:2]
    assert any(len(p[1]) > len(want[1]) for p in patterns), "no candidate anywhere: the case shows nothing"
    for k in out:
        assert pattern_of(out[k]) == pattern_of(want), k


def part_sizes(rp, ci):
    rows = tr.rows_of(rp)
    return int((ci < rows).sum()), int((ci > rows).sum())


@pytest.mark.parametrize("limit", [1.0, 1.5, 2.0, 100.0])
@pytest.mark.parametrize("kind", ["ilu", "ic"])
def test_kept_counts(kind, limit):
    """tie-free values: every part keeps exactly min(count, keep) entries; the constant-coefficient stencil has
    ties: at least that many"""
    for name, a in (("random", random_case(kind == "ic")), ("stencil", fr.stencil27(3))):
        rp, ci, v = fr.arrays(a)
        keep = tr.keep_counts(rp, ci, limit)
        patterns = []
        at = (tr.par_ilut_at if kind == "ilu" else tr.par_ict_at)(rp, ci, v, (1, 2), limit, patterns)
        for t in (1, 2):
            have, offered = part_sizes(*at[t][:2]), part_sizes(*patterns[t - 1])
            for part in (0, 1) if kind == "ilu" else (0,):
                least = min(offered[part], keep[part])
                if name == "random":
                    assert have[part] == least, (name, t, part)
                else:
                    assert have[part] >= least, (name, t, part)
            assert len(at[t][1]) == sum(have) + a.shape[0], "a diagonal was dropped"


def test_keep_counts_floor_and_minimum():
    rp, ci, _ = fr.arrays(sp.csr_matrix(np.array([[1.0, 2, 0], [0, 1, 3], [4, 5, 1]])))
    assert tr.keep_counts(rp, ci, 1.0) == (2, 2) and tr.keep_counts(rp, ci, 1.9) == (3, 3)
    rp, ci, _ = fr.arrays(sp.identity(3, format="csr"))
    assert tr.keep_counts(rp, ci, 2.0) == (1, 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_select_rule(dtype):
    f = dtype
    nan, inf = f(np.nan), f(np.inf)
    # -0 is 0: both zeros rank lowest, the threshold is +0 in bits
    thr = tr.threshold(np.array([-0.0, 0.0, 1.0], dtype), 2)
    assert thr == 0 and not np.signbit(thr)
    thr = tr.threshold(np.array([-0.0, 3.0, -2.0], dtype), 3)          # count <= keep
    assert thr == 0 and not np.signbit(thr)
    # by magnitude, sign ignored; the threshold is non-negative
    assert tr.threshold(np.array([-5.0, 1.0, 3.0, -4.0], dtype), 2) == f(4.0)
    assert tr.threshold(np.array([-5.0, 1.0, 3.0, -4.0], dtype), 1) == f(5.0)
    # NaN ranks above inf, whatever its sign
    assert np.isinf(tr.threshold(np.array([1.0, inf, nan, 2.0], dtype), 2))
    assert np.isnan(tr.threshold(np.array([1.0, -inf, -nan, 2.0], dtype), 1))
    assert tr.threshold(np.array([1.0, -inf, nan, 2.0], dtype), 3) == f(2.0)
    # duplicates straddling the rank: the threshold is the duplicated value, and the mask keeps all of them
    vals = np.array([1.0, 2.0, -2.0, 2.0, 3.0], dtype)
    for keep in (2, 3, 4):
        assert tr.threshold(vals, keep) == f(2.0)
    assert tr.threshold(vals, 1) == f(3.0)
    # ... in a matrix: row 3 holds the values as its strictly-lower... entries of a 6 x 6 lower triangle
    dense = np.eye(6)
    dense[5, :5] = vals
    rp, ci, v = fr.on_pattern(dense, dense != 0, dtype=dtype)
    thr = tr.part_threshold(rp, ci, v, 0, 2)
    mask = tr.keep_mask(rp, ci, v, thr)
    assert thr == f(2.0) and mask[ci < tr.rows_of(rp)].tolist() == [0, 1, 1, 1, 1]
    assert tr.part_threshold(rp, ci, v, 1, 1) == 0           # no upper entry at all
    # the diagonal is kept even when it is 0 and below the threshold
    v[ci == tr.rows_of(rp)] = 0
    assert tr.keep_mask(rp, ci, v, f(2.0), f(2.0))[ci == tr.rows_of(rp)].all()


def test_pieces_on_a_hand_example():
    """3 x 3: M stores (0,0) (0,2) (1,0) (1,1) (2,1) (2,2); A' stores (1,2) and (2,0) in addition, which M dropped"""
    m = fr.on_pattern(np.array([[2.0, 0, 4], [6, 3, 0], [0, 9, 5]]), np.array([[1, 0, 1], [1, 1, 0], [0, 1, 1]]))
    a = fr.on_pattern(np.array([[2.0, 0, 4], [6, 3, 7], [8, 9, 5]]), np.array([[1, 0, 1], [1, 1, 1], [1, 1, 1]]))
    p_rp, p_ci = tr.ilut_pattern(m[0], m[1], a[0], a[1])
    assert p_rp.tolist() == [0, 2, 5, 8] and p_ci.tolist() == [0, 2, 0, 1, 2, 0, 1, 2]
    got = tr.ilut_candidates(p_rp, p_ci, *a, *m)
    # (1,2): a' = 7, k = 0: 7 - 6 * 4 = -17, upper: no division.  (2,0): a' = 8, no k < 0: 8 / m_00 = 4
    assert got.tolist() == [2, 4, 6, 3, -17, 4, 9, 5]
    assert tr.gather(p_rp, p_ci, *a).tolist() == [2, 4, 6, 3, 7, 8, 9, 5]
    assert tr.gather(p_rp, p_ci, *m).tolist() == [2, 4, 6, 3, 0, 0, 9, 5]
