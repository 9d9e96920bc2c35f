"""The references of tests/csr_struct_refs.py against independent formulations (no GPU): SpGEMM / SpGEAM
against a dense long-double product or sum masked to the pattern, the index-set pair against dense fancy
indexing, the lookup tables through their decoder, the small operations against dense restatements."""
import numpy as np
import pytest

import binding_refs as br
import csr_struct_refs as cr

TN = ["f64", "f32", "c128", "c64"]


def _wide(t):
    return np.clongdouble if br.is_complex(t) else np.longdouble


def _matrix(rng, rows, cols, density, t, empty_rows=()):
    p, c = cr.random_pattern(rng, rows, cols, density, empty_rows)
    return p, c, cr.random_values(rng, len(c), t)


def _mask(pattern, shape):
    ptrs, cols = pattern
    m = np.zeros(shape, bool)
    for r in range(shape[0]):
        m[r, cols[ptrs[r]:ptrs[r + 1]]] = True
    return m


def _scatter(pattern, vals, shape, wt):
    return cr.to_dense((pattern[0], pattern[1], vals), shape, wt)


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("m,k,n", [(1, 1, 1), (7, 5, 9), (40, 30, 50)])
def test_spgemm_reuse_against_dense(tn, m, k, n):
    t = br.TYPES[tn]
    wt = _wide(t)
    rng = np.random.default_rng(m + n)
    A, B = _matrix(rng, m, k, 0.3, t, (m // 2,) if m > 1 else ()), _matrix(rng, k, n, 0.3, t)
    D = _matrix(rng, m, n, 0.2, t)
    da, db, dd = cr.to_dense(A, (m, k), wt), cr.to_dense(B, (k, n), wt), cr.to_dense(D, (m, n), wt)
    exact = cr.product_pattern(A[:2], B[:2])
    sup = cr.product_pattern(A[:2], B[:2], D[:2])
    sub = cr.every_other(exact)
    alpha, beta = (0.7 - 0.2j, -1.3 + 0.4j) if br.is_complex(t) else (0.7, -1.3)
    al, be = wt(t(alpha)), wt(t(beta))
    for pat in (exact, sup, sub):
        mask = _mask(pat, (m, n))
        for ar, tol in ((br.hp(t), 64 * np.finfo(np.longdouble).eps), (br.plain(t), 64 * br.eps_of(t))):
            got = _scatter(pat, cr.spgemm_reuse(ar, A, B, pat), (m, n), wt)
            assert np.max(np.abs(got - np.where(mask, da @ db, 0)), initial=0) <= tol * k
            got = _scatter(pat, cr.spgemm_reuse(ar, A, B, pat, t(alpha), t(beta), D), (m, n), wt)
            want = np.where(mask, al * (da @ db) + be * dd, 0)
            assert np.max(np.abs(got - want), initial=0) <= tol * k * 4
    # a superset's extra entries are exactly zero
    extra = _mask(sup, (m, n)) & ~_mask(exact, (m, n))
    got = _scatter(sup, cr.spgemm_reuse(br.plain(t), A, B, sup), (m, n), wt)
    assert np.all(got[extra] == 0)


@pytest.mark.parametrize("tn", TN)
def test_spgeam_numeric_against_dense(tn):
    t = br.TYPES[tn]
    wt = _wide(t)
    rng = np.random.default_rng(5)
    m, n = 30, 40
    A, B = _matrix(rng, m, n, 0.2, t, (3,)), _matrix(rng, m, n, 0.2, t, (3, 7))
    pat = cr.product_pattern((np.arange(m + 1), np.arange(m)), A[:2], B[:2])      # I A + B: the union
    alpha, beta = (0.7 - 0.2j, -1.3 + 0.4j) if br.is_complex(t) else (0.7, -1.3)
    want = wt(t(alpha)) * cr.to_dense(A, (m, n), wt) + wt(t(beta)) * cr.to_dense(B, (m, n), wt)
    for ar, tol in ((br.hp(t), 8 * np.finfo(np.longdouble).eps), (br.plain(t), 8 * br.eps_of(t))):
        vals = cr.spgeam_numeric(ar, t(alpha), A, t(beta), B, pat[0])
        assert np.max(np.abs(_scatter(pat, vals, (m, n), wt) - want)) <= tol * 4
    # a row of C shorter than the merged row is cut, a longer one keeps what it held
    short = np.concatenate([[0], np.cumsum(np.maximum(np.diff(pat[0]) - 1, 0))])
    long_ = np.concatenate([[0], np.cumsum(np.diff(pat[0]) + 1)])
    full = cr.spgeam_numeric(br.plain(t), t(alpha), A, t(beta), B, pat[0])
    cut = cr.spgeam_numeric(br.plain(t), t(alpha), A, t(beta), B, short)
    kept = cr.spgeam_numeric(br.plain(t), t(alpha), A, t(beta), B, long_, c0=np.full(long_[-1], 9, t))
    for r in range(m):
        row = full[pat[0][r]:pat[0][r + 1]]
        assert np.array_equal(cut[short[r]:short[r + 1]], row[:max(len(row) - 1, 0)])
        assert np.array_equal(kept[long_[r]:long_[r + 1]], np.concatenate([row, [t(9)]]))


def _sets():
    return [([(0, 12)], [(0, 15)]),                                   # everything
            ([(2, 3)], [(4, 5)]),                                     # length one
            ([(0, 2), (2, 5), (11, 12)], [(0, 1), (3, 7), (7, 9), (14, 15)]),   # adjacent, first and last
            ([(1, 4), (6, 9)], [(12, 14)])]


def test_index_set_against_dense_indexing():
    rng = np.random.default_rng(3)
    rows, cols = 12, 15
    A = _matrix(rng, rows, cols, 0.4, np.float64, (4,))
    dense = cr.to_dense(A, (rows, cols), np.float64)             # values are non-zero: stored == non-zero
    for rr, cc in _sets():
        for size in (cols, 8):                                   # a bound that cuts the column set
            cc2 = [(b, min(e, size)) for b, e in cc if b < size]
            rs, cs = cr.IndexSet(rr, rows), cr.IndexSet(cc2, size)
            assert rs.superset[-1] == rs.num_elems == len(rs.rows())
            sub = dense[np.ix_(rs.rows(), cs.rows())] if cs.num_subsets else np.zeros((rs.num_elems, 0))
            counts = cr.index_set_count(rs, cs, A[:2])
            assert np.array_equal(counts, np.count_nonzero(sub, axis=1))
            oc, ov = cr.index_set_fill(rs, cs, A)
            ptrs = np.concatenate([[0], np.cumsum(counts)])
            got = cr.to_dense((ptrs, oc, ov), sub.shape, np.float64)
            assert np.array_equal(got, sub)
    # a column at or past the bound is dropped even when a subset would hold it
    cs = cr.IndexSet([(0, 8)], 8)
    cs.size = 5
    assert cs.local(4) == 4 and cs.local(5) is None


def _lookup_rows():
    rows = [[], [5], list(range(10, 30)), list(range(0, 64, 2)), [0, 32], [0, 33], [1, 64], [1, 65, 66],
            [0, 1000], [7, 500, 100000], list(range(0, 320, 9)), [2 ** 31 - 5, 2 ** 31 - 2]]
    rng = np.random.default_rng(11)
    for _ in range(60):
        n = int(rng.integers(0, 40))
        rows.append(sorted(set(rng.integers(0, int(rng.choice([40, 200, 5000])), n).tolist())))
    return rows


@pytest.mark.parametrize("it", [np.int32, np.int64])
@pytest.mark.parametrize("allowed", range(8))
def test_lookup_decoder_finds_every_entry_and_nothing_else(it, allowed):
    rows = _lookup_rows()
    if it == np.int64:
        rows.append([2 ** 32 + 1, 2 ** 32 + 70, 2 ** 33 + 5])
    ptrs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = np.array([c for r in rows for c in r], np.int64)
    bits = np.dtype(it).itemsize * 8
    offs = cr.lookup_offsets(ptrs, cols, allowed, it)
    desc, storage, written = cr.lookup_build(ptrs, cols, allowed, offs, it)
    assert np.array_equal(np.diff(offs.astype(np.int64)), written)      # sizes == what the construction writes
    assert not np.any(storage == -12345)
    kinds = set()
    for r, row in enumerate(rows):
        st = storage[offs[r]:offs[r + 1]]
        kind = int(desc[r]) & 0xffffffff
        kinds.add(kind)
        assert kind == 0 or (kind & allowed)
        for k, c in enumerate(row):
            assert cr.lookup_position(desc[r], st, row, c, bits) == k
        if row and kind:
            lo, hi = row[0] - 1, row[-1] + 1
            probe = range(lo, hi + 1) if hi - lo < 200000 else \
                list(range(lo, lo + 600)) + list(range(hi - 600, hi + 1))
            stored = set(row)
            for c in probe:
                if c not in stored and c >= 0:
                    assert cr.lookup_position(desc[r], st, row, c, bits) == -1
    want = {0: {0}, 1: {0, 1}, 2: {0, 2}, 3: {0, 1, 2}, 4: {4}, 5: {1, 4}, 6: {2, 4}, 7: {1, 2, 4}}[allowed]
    assert kinds == want, kinds


def test_lookup_kind_boundaries():
    """bitmap words against hash slots: 2 ceil(range / 32) <= max(2 len, 1) chooses the bitmap"""
    assert cr._row_kind(2, 64, 7) == (cr.BITMAP, 4)          # equal: bitmap
    assert cr._row_kind(2, 65, 7) == (cr.HASH, 4)            # one column more: a third block
    assert cr._row_kind(2, 63, 7) == (cr.BITMAP, 4)
    assert cr._row_kind(3, 3, 7) == (cr.FULL, 0) and cr._row_kind(3, 3, 6) == (cr.BITMAP, 2)
    assert cr._row_kind(0, 0, 7) == (cr.FULL, 0) and cr._row_kind(0, 0, 4) == (cr.HASH, 1)
    assert cr._row_kind(2, 65, 3) == (0, 0)                  # neither fits and hash is not allowed


@pytest.mark.parametrize("tn", TN)
def test_small_operations_against_dense(tn):
    t = br.TYPES[tn]
    wt = _wide(t)
    rng = np.random.default_rng(9)
    n = 25
    A = list(_matrix(rng, n, n, 0.3, t, (2,)))
    dense = cr.to_dense(A, (n, n), wt)
    diag = cr.random_values(rng, n, t) + t(2)
    b = cr.random_values(rng, n * 4, t).reshape(n, 4)
    eps = br.eps_of(t)
    for ar, tol in ((br.hp(t), 1e-17), (br.plain(t), 8 * eps)):
        assert np.max(np.abs(cr.row_abs_sum(ar, A[0], A[2]) - np.sum(np.abs(dense), axis=1))) <= tol * n
        dl = diag.astype(wt)
        assert np.max(np.abs(cr.diag_apply_dense(ar, diag, b) - dl[:, None] * b.astype(wt))) <= tol * 8
        assert np.max(np.abs(cr.diag_apply_dense(ar, diag, b, True) - b.astype(wt) / dl[:, None])) <= tol * 8
        assert np.max(np.abs(cr.diag_right_apply_dense(ar, diag[:4], b) - b.astype(wt) * dl[None, :4])) <= tol * 8
        got = cr.to_dense((A[0], A[1], cr.diag_apply_csr(ar, diag, A[0], A[2])), (n, n), wt)
        assert np.max(np.abs(got - dl[:, None] * dense)) <= tol * 8
        got = cr.to_dense((A[0], A[1], cr.diag_apply_csr(ar, diag, A[0], A[2], True)), (n, n), wt)
        assert np.max(np.abs(got - dense / dl[:, None])) <= tol * 8
        got = cr.to_dense((A[0], A[1], cr.diag_right_apply_csr(ar, diag, A[1], A[2])), (n, n), wt)
        assert np.max(np.abs(got - dense * dl[None, :])) <= tol * 8
    # Smith's reciprocal on both branches and exactly on powers of two
    z = np.array([2, 2j, 0.5 + 0j, -4j], np.complex128).astype(t) if br.is_complex(t) else np.array([2, 0.5, -4], t)
    assert np.array_equal(cr.reciprocal(br.plain(t), z), (1 / z.astype(wt)).astype(t))
    # diagonal extraction, conversion, fill
    out0 = np.full(n, 7, t)
    has = np.array([r in A[1][A[0][r]:A[0][r + 1]] for r in range(n)])
    got = cr.extract_diagonal(A[0], A[1], A[2], out0)
    assert np.array_equal(got[has], np.diag(dense).astype(t)[has]) and np.all(got[~has] == 7) and not has.all()
    p, c, v = cr.diag_to_csr(diag, np.int32)
    assert np.array_equal(cr.to_dense((p, c, v), (n, n), wt), np.diag(diag.astype(wt)))
    rows = np.repeat(np.arange(n), np.diff(A[0]))
    assert np.array_equal(cr.diag_fill(rows, A[1], A[2], out0), got)


def test_sparsity_csr_against_dense():
    rng = np.random.default_rng(2)
    n = 20
    p, c = cr.random_pattern(rng, n, n, 0.3, (5,))
    # row 3: only the diagonal, row 4: the diagonal twice
    rows = [list(c[p[r]:p[r + 1]]) for r in range(n)]
    rows[3], rows[4] = [3], [1, 4, 4, 9]
    p = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    c = np.array([x for r in rows for x in r], np.int64)
    counts = cr.count_diagonal(p, c)
    assert counts[3] == 1 and counts[4] == 2 and counts[5] == 0 and counts[n] == 0
    prefix = np.concatenate([[0], np.cumsum(counts[:-1])])
    ap, ai = cr.remove_diagonal(p, c, prefix)
    assert ap[-1] == len(ai) == len(c) - counts.sum()
    for r in range(n):
        assert list(ai[ap[r]:ap[r + 1]]) == [x for x in rows[r] if x != r]


def test_stencil7_is_the_7_point_laplacian():
    p, c, v = cr.stencil7(4)
    d = cr.to_dense((p, c, v), (64, 64), np.float64)
    assert np.array_equal(d, d.T) and np.all(np.diag(d) == 6) and p[-1] == 64 * 7 - 6 * 16
    assert all(np.all(np.diff(c[p[r]:p[r + 1]]) > 0) for r in range(64))
