"""tests/format_spmv_refs.py against independent formulations: the scipy.sparse product of the same matrix
in double precision under rule R, the plain-C oracle bit for bit (float / double, both index types),
np.searchsorted and np.diff for the pointer conversions, a trip builder -> dense -> builder, and the coverage
the case lists of the GPU tests promise.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import binding_refs as br
import format_spmv_refs as fr

TYPES = (np.float64, np.float32, np.complex128, np.complex64)


def _scipy_of(rows, n_cols, t):
    wide = np.complex128 if br.is_complex(t) else np.float64
    r = [i for i, slots in enumerate(rows) for c, _ in slots if c >= 0]
    c = [c for slots in rows for c, _ in slots if c >= 0]
    v = [wide(v) for slots in rows for c, v in slots if c >= 0]
    return sp.coo_matrix((np.array(v, wide), (r, c)), shape=(len(rows), n_cols)).tocsr(), wide


def _scipy_product(rows, n_cols, t, b, scal, c):
    a, wide = _scipy_of(rows, n_cols, t)
    p = np.asarray(a @ b.astype(wide))
    if scal is None:
        return p
    alpha, beta = (wide(np.dtype(t).type(s)) for s in scal)
    return alpha * p + (beta * c.astype(wide) if beta != 0 else 0)


def _operands(rng, t, n_rows, n_cols, nrhs, scalars, si):
    b, c = fr.values(rng, (n_cols, nrhs), t), fr.values(rng, (n_rows, nrhs), t)
    scal = scalars[si % len(scalars)]
    kw = {} if scal is None else dict(alpha=scal[0], beta=scal[1], c=None if scal[1] == 0 else c)
    return b, c, scal, kw


@pytest.mark.parametrize("t", TYPES)
def test_ell_product_against_scipy(t):
    rng = np.random.default_rng(1)
    scalars = fr.COMPLEX_SCALARS if br.is_complex(t) else fr.REAL_SCALARS
    for li, n, n_cols, k, stride, family, si in fr.ell_cases()[::5]:
        nrhs = fr.LAYOUTS[li][0][0]
        rows = fr.ell_rows(rng, t, n, n_cols, k, family)
        cols, vals = fr.ell_build(rows, k, stride, t, np.int32)
        b, c, scal, kw = _operands(rng, t, n, n_cols, nrhs, scalars, si)
        ref, plain = fr.ell_product(t, n, k, stride, cols, vals, b, **kw)
        assert plain.dtype == np.dtype(t) and ref.dtype == br.hp(t).wt
        ok, ratio = br.rule_r(_scipy_product(rows, n_cols, t, b, scal, c), ref, plain, t)
        assert ok, (n, n_cols, k, family, scal, ratio)


@pytest.mark.parametrize("t", TYPES)
def test_sellp_product_against_scipy(t):
    rng = np.random.default_rng(2)
    scalars = fr.COMPLEX_SCALARS if br.is_complex(t) else fr.REAL_SCALARS
    for li, n, n_cols, si_, family, si in fr.sellp_cases()[::7]:
        nrhs = fr.LAYOUTS[li][0][0]
        ss, sf = fr.SLICES[si_]
        rows = fr.sellp_rows(rng, t, n, n_cols, ss, family)
        sets, lens, cols, vals = fr.sellp_build(rows, ss, sf, t, np.int64)
        b, c, scal, kw = _operands(rng, t, n, n_cols, nrhs, scalars, si)
        ref, plain = fr.sellp_product(t, n, ss, sets, lens, cols, vals, b, **kw)
        ok, ratio = br.rule_r(_scipy_product(rows, n_cols, t, b, scal, c), ref, plain, t)
        assert ok, (n, n_cols, ss, sf, family, scal, ratio)


@pytest.mark.parametrize("it", [np.int32, np.int64])
@pytest.mark.parametrize("t", [np.float64, np.float32])
def test_real_products_are_the_oracles_bits(oracle, t, it):
    rng = np.random.default_rng(3)
    for li, n, n_cols, k, stride, family, si in fr.ell_cases():
        rows = fr.ell_rows(rng, t, n, n_cols, k, family)
        cols, vals = fr.ell_build(rows, k, stride, t, it)
        b, c, scal, kw = _operands(rng, t, n, n_cols, fr.LAYOUTS[li][0][0], fr.REAL_SCALARS, si)
        _, plain = fr.ell_product(t, n, k, stride, cols, vals, b, **kw)
        want = oracle.ell_spmv(n, k, stride, cols, vals, b) if scal is None else \
            oracle.ell_spmv(n, k, stride, cols, vals, b, scal[0], scal[1], c)
        assert np.array_equal(plain, want), (n, n_cols, k, family, scal)
    for li, n, n_cols, si_, family, si in fr.sellp_cases()[::2]:
        ss, sf = fr.SLICES[si_]
        rows = fr.sellp_rows(rng, t, n, n_cols, ss, family)
        sets, lens, cols, vals = fr.sellp_build(rows, ss, sf, t, it)
        b, c, scal, kw = _operands(rng, t, n, n_cols, fr.LAYOUTS[li][0][0], fr.REAL_SCALARS, si)
        _, plain = fr.sellp_product(t, n, ss, sets, lens, cols, vals, b, **kw)
        want = oracle.sellp_spmv(n, ss, sets, lens, cols, vals, b) if scal is None else \
            oracle.sellp_spmv(n, ss, sets, lens, cols, vals, b, scal[0], scal[1], c)
        assert np.array_equal(plain, want), (n, n_cols, ss, sf, family, scal)


def test_beta_zero_never_reads_c_and_padding_counts_by_column():
    rng = np.random.default_rng(4)
    for t in TYPES:
        rows = [[(fr.PAD, np.dtype(t).type(np.nan)), (1, np.dtype(t).type(2))], [], [(2, np.dtype(t).type(-1))]]
        cols, vals = fr.ell_build(rows, 3, 4, t, np.int32)
        b = fr.values(rng, (3, 2), t)
        b[0] = np.nan
        for prod in (fr.ell_product(t, 3, 3, 4, cols, vals, b),
                     fr.ell_product(t, 3, 3, 4, cols, vals, b, alpha=2.0, beta=0.0, c=np.full((3, 2), np.nan, t))):
            for v in prod:
                assert not np.any(np.isnan(v)) and np.all(v[1] == 0)


@pytest.mark.parametrize("it", [np.int32, np.int64])
@pytest.mark.parametrize("t", [np.float64, np.float32])
def test_conversions_are_the_oracles(oracle, t, it):
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 200):
        lengths = rng.integers(0, 12, n)
        lengths[[0, n // 2, n - 1]] = 0
        ptrs, cols, vals = fr.random_csr(rng, t, it, lengths, 50)
        k = fr.compute_max_row_nnz(ptrs)
        assert k == int(lengths.max())
        for kk, stride in ((k, n), (k + 2, n + 5)):
            fill_c, fill_v = np.full(kk * stride, -1, it), np.zeros(kk * stride, t)
            oc, ov = fr.csr_convert_to_ell(ptrs, cols, vals, kk, stride, fill_c, fill_v)
            _, _, ec, ev = oracle.csr_to_ell(ptrs, cols, vals, kk, stride)
            assert np.array_equal(oc, ec) and np.array_equal(ov, ev)
            # rows n .. stride keep another fill too
            oc2, _ = fr.csr_convert_to_ell(ptrs, cols, vals, kk, stride, np.full(kk * stride, -7, it), fill_v)
            assert np.all(oc2.reshape(kk, stride)[:, n:] == -7) and np.all(oc2.reshape(kk, stride)[:, :n] != -7)
        for ss, sf in fr.SLICES + ((200, 1),):
            sets, lens = fr.sellp_compute_slice_sets(ptrs, ss, sf)
            osets, olens = oracle.sellp_compute_slice_sets(ptrs, ss, sf)
            assert np.array_equal(sets, osets) and np.array_equal(lens, olens)
            total = int(sets[-1]) * ss
            oc, ov = fr.csr_convert_to_sellp(ptrs, cols, vals, ss, sets, np.full(total, -1, it), np.zeros(total, t))
            _, _, sc, sv = oracle.csr_to_sellp(ptrs, cols, vals, ss, sf)
            assert np.array_equal(oc, sc) and np.array_equal(ov, sv)
            # and it is the builder's layout
            rows = [list(zip(cols[ptrs[r]:ptrs[r + 1]].tolist(), vals[ptrs[r]:ptrs[r + 1]])) for r in range(n)]
            bsets, blens, bc, bv = fr.sellp_build(rows, ss, sf, t, it)
            assert np.array_equal(bsets, sets) and np.array_equal(blens, lens)
            assert np.array_equal(bc, oc) and np.array_equal(bv, ov)


def test_slice_sets_without_rows():
    sets, lens = fr.sellp_compute_slice_sets(np.zeros(1, np.int32), 64, 1)
    assert sets.tolist() == [0] and lens.size == 0


@pytest.mark.parametrize("it,pt", [(np.int32, np.int32), (np.int64, np.int64), (np.int32, np.int64),
                                   (np.int64, np.int32)])
def test_pointer_conversions(it, pt):
    rng = np.random.default_rng(6)
    for n in (0, 1, 255, 256, 257, 3001):
        for idxs in (np.sort(rng.integers(0, max(n, 1), 2 * n)) if n else np.zeros(0, int),
                     np.zeros(0, int), np.full(5 if n else 0, max(n - 1, 0))):
            idxs = idxs.astype(it)
            ptrs = fr.convert_idxs_to_ptrs(idxs, n, pt)
            assert ptrs.dtype == np.dtype(pt)
            assert np.array_equal(ptrs, np.searchsorted(idxs, np.arange(n + 1), side="left"))
            assert np.array_equal(fr.convert_ptrs_to_sizes(ptrs), np.diff(ptrs).astype(np.uint64))
            assert fr.compute_max_row_nnz(ptrs) == (int(np.diff(ptrs).max()) if n else 0)


@pytest.mark.parametrize("t", TYPES)
def test_builder_dense_builder(t):
    rng = np.random.default_rng(7)
    for n, n_cols, k in ((17, 37, 9), (65, 300, 25), (129, 37, 8)):
        rows = fr.ell_rows(rng, t, n, n_cols, k, "compact")
        again = fr.rows_of_dense(fr.dense_of(rows, n_cols, np.dtype(t).type))
        a, b = fr.ell_build(rows, k, n + 5, t, np.int32), fr.ell_build(again, k, n + 5, t, np.int32)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        cm, vm = fr.ell_slots(n, k, n + 5, *a)
        assert [[(c, v) for c, v in zip(cr, vr) if c >= 0] for cr, vr in zip(cm.tolist(), vm)] == \
            [[(c, v) for c, v in r] for r in rows]
        for ss, sf in fr.SLICES:
            a, b = fr.sellp_build(rows, ss, sf, t, np.int64), fr.sellp_build(again, ss, sf, t, np.int64)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            cm, vm = fr.sellp_slots(n, ss, *a)
            assert np.array_equal(fr.dense_of([list(zip(cr, vr)) for cr, vr in zip(cm.tolist(), vm)], n_cols,
                                              np.dtype(t).type), fr.dense_of(rows, n_cols, np.dtype(t).type))


def test_case_lists_cover_what_they_promise():
    ell = fr.ell_cases()
    for li in range(len(fr.LAYOUTS)):
        mine = [c for c in ell if c[0] == li]
        assert {c[1] for c in mine} == set(fr.ROWS) and {c[3] for c in mine} == set(fr.ELL_K)
        assert {c[6] for c in mine} == set(range(4)) and {c[5] for c in mine} == {"cycle", "padfront"}
        assert {c[4] - c[1] for c in mine} == {0, 5} and {c[2] for c in mine} == set(fr.COLS)
    sellp = fr.sellp_cases()
    for li in range(len(fr.LAYOUTS)):
        assert {c[1] for c in sellp if c[0] == li} == set(fr.ROWS)
        assert {c[5] for c in sellp if c[0] == li} == set(range(4))
    for si in range(len(fr.SLICES)):
        assert {c[1] for c in sellp if c[3] == si} == set(fr.ROWS)
    # aligned buffers: the branch every layout names (the GPU test asserts it from the pointers it passes)
    for (nrhs, ldb, ldc, bo, co), want in fr.LAYOUTS:
        for size in (4, 8):
            assert fr.branch_of(37, nrhs, ldb, ldc, 4096 + bo * size, 8192 + co * size, size) == want
    assert fr.branch_of(0, 8, 8, 8, 4096, 8192, 8) == "row 8"
    # the shape of the fragment kernel's former out-of-bounds load, per slice size below 64, on a fragment layout
    rng = np.random.default_rng(8)
    seen = set()
    for li, n, n_cols, si, family, _ in sellp:
        ss, sf = fr.SLICES[si]
        if fr.LAYOUTS[li][1].startswith("frag") and family == "empties":
            _, lens, _, _ = fr.sellp_build(fr.sellp_rows(rng, np.float32, n, n_cols, ss, family), ss, sf,
                                           np.float32, np.int32)
            if fr.trailing_empty_slice_in_shared_wave(ss, lens):
                seen.add(ss)
    assert seen >= {1, 2, 32}, seen
    assert fr.trailing_empty_slice_in_shared_wave(2, [3, 3, 3, 3, 0])
    assert not fr.trailing_empty_slice_in_shared_wave(64, [3, 0]) and not fr.trailing_empty_slice_in_shared_wave(2, [0, 0])
