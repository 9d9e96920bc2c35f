"""Format helpers through the C ABI against tests/value_kernel_refs.py: the complex Csr scaling
(gkoc_ccsr_scale_by_diagonal_*) and Coo product (gkoc_ccoo_spmv2_*) of csrc/complex_blas.hip, ell::copy
(gkoc_ell_copy_*, coo.hip), the Ell / Sellp diagonals (gkoc_ell_extract_diagonal_*,
gkoc_sellp_extract_diagonal_*, conversions.hip) and the block storage of Jacobi (gkoc_cjacobi_transpose_*,
gkoc_jacobi_initialize_precisions, jacobi.hip).

Csr scaling: one textbook product per entry, bit-identical to the plain restatement (mode 1: a reciprocal by
Smith's quotient, then the product - rule R; its sweep over the range of the type is in test_cdense_gpu.py).
The Coo product adds with atomics, the one kernel here whose order is not fixed: per output entry
|got - ref| <= (m + 4) eps (|c0| + sum_k |alpha| |v_k| |b_k|), m the number of entries that land on it - the
a-priori bound of any order of m rounded additions of rounded complex products (value_kernel_refs.coo_spmv2) -
and exact on small integers.  Everything else is copies: bit for bit on random bit patterns with NaN payloads.
Inputs are read back and compared bit for bit; outputs are pre-filled and followed by canaries."""
import numpy as np
import pytest

import binding_refs as br
import csr_struct_refs as cr
import value_kernel_refs as vr
from binding_gpu import CANARY, Dev, DevCsr, call as _call, canaries_ok, grid_cap_rows as _grid_cap_rows, \
    out_buf as _out, padded, raises_invalid, same_bits, sync, tail_ok as _tail_ok

pytestmark = pytest.mark.gpu

TN = ["f64", "f32", "c128", "c64"]
CTN = ["c128", "c64"]
IT = {"i32": np.int32, "i64": np.int64}
SIZES = [0, 1, 255, 256, 257, 2049, 100003]
STATS = {}


def _stat(name, tn, ratio):
    STATS[(name, tn)] = max(STATS.get((name, tn), 0.0), ratio)


# ------------------------------------------------------------------------------------ Csr scaling
@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", CTN)
def test_ccsr_scale_by_diagonal(gexec, tn, in_):
    """rows of 0, 1, 63, 64, 65 and 5000 entries and empty rows between them"""
    t, it = br.TYPES[tn], IT[in_]
    rng = np.random.default_rng(61)
    n = 6000
    lengths = [0, 1, 63, 64, 65, 5000, 0, 2] + [int(k) for k in rng.integers(0, 5, n - 8)]
    ptrs = np.concatenate([[0], np.cumsum(lengths)])
    cols = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lengths]).astype(np.int64)
    nnz = len(cols)
    vals = cr.random_values(rng, nnz, t)
    diag = cr.random_values(rng, n, t)
    diag = (diag + np.where(diag.real < 0, -1, 1)).astype(t)
    diag[1::2] = diag[1::2] * t(1j)
    da, dd = DevCsr(gexec, it, ptrs, cols), Dev(gexec, diag)
    for mode in (0, 1, 2):
        dv = Dev(gexec, np.concatenate([vals, np.full(3, CANARY, t)]))
        _call("gkoc_ccsr_scale_by_diagonal_" + tn + "_" + in_, gexec.stream, n, *da.dev, dd, mode, dv)
        sync()
        got = dv.get()
        assert _tail_ok(got, nnz) and da.unchanged() and same_bits(dd.get(), diag)
        want = vr.csr_scale_by_diagonal(br.plain(t), ptrs, cols, diag, mode, vals)
        if mode == 1:
            ok, ratio = br.rule_r(got[:nnz], vr.csr_scale_by_diagonal(br.hp(t), ptrs, cols, diag, 1, vals), want, t)
            assert ok, ratio
            _stat("ccsr_scale_by_diagonal mode 1", tn, ratio)
            STATS[("  ... entries that differ from the plain restatement", tn)] = int(np.count_nonzero(got[:nnz] != want))
        else:
            assert same_bits(got[:nnz], want), (mode, np.flatnonzero(got[:nnz] != want)[:4])
    before = dv.get()
    for mode in (3, -1):
        assert raises_invalid("gkoc_ccsr_scale_by_diagonal_" + tn + "_" + in_, gexec.stream, n, *da.dev, dd, mode, dv)
    _call("gkoc_ccsr_scale_by_diagonal_" + tn + "_" + in_, gexec.stream, 0, *da.dev, dd, 0, dv)       # no rows
    sync()
    assert same_bits(dv.get(), before)


# ------------------------------------------------------------------------------------ Coo product
def _coo_cases(rng, t, integers):
    """(name, n_rows, n_cols, rows, cols, vals): random with duplicate (row, col) pairs; 20 000 entries in one
    row; one entry; none"""
    def values(k):
        if integers:
            return (rng.integers(-3, 4, k) + 1j * rng.integers(-3, 4, k)).astype(t)
        return cr.random_values(rng, k, t)
    r, c = rng.integers(0, 50, 3000), rng.integers(0, 40, 3000)
    r[:300], c[:300] = r[300:600], c[300:600]                 # every one of these positions twice
    r[600:700], c[600:700] = 13, 7                            # and one position a hundred times
    yield "duplicates", 50, 40, r, c, values(3000)
    yield "one row", 50, 40, np.full(20000, 31), rng.integers(0, 40, 20000), values(20000)
    yield "one entry", 50, 40, np.array([49]), np.array([39]), values(1)
    yield "empty", 50, 40, np.zeros(0, np.int64), np.zeros(0, np.int64), values(0)


@pytest.mark.parametrize("with_alpha", [0, 1])
@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", CTN)
def test_ccoo_spmv2(gexec, tn, in_, nrhs, with_alpha):
    """c += [alpha] A b: c starts non-zero; b and c are strided"""
    t, it = br.TYPES[tn], IT[in_]
    eps = br.eps_of(t)
    for integers in (True, False):
        rng = np.random.default_rng(67 + nrhs)
        for name, n_rows, n_cols, rows, cols, vals in _coo_cases(rng, t, integers):
            if integers:
                b = (rng.integers(-2, 3, (n_cols, nrhs)) + 1j * rng.integers(-2, 3, (n_cols, nrhs))).astype(t)
                c0 = (rng.integers(-9, 10, (n_rows, nrhs)) + 0j).astype(t)
                alpha = np.array([2 - 1j], t)
            else:
                b = cr.random_values(rng, n_cols * nrhs, t).reshape(n_cols, nrhs)
                c0 = cr.random_values(rng, n_rows * nrhs, t).reshape(n_rows, nrhs)
                alpha = np.array([0.75 - 1.5j], t)
            fb, fc = padded(b, nrhs + 2), padded(c0, nrhs + 3)
            dr, dc, dv = Dev(gexec, rows.astype(it)), Dev(gexec, cols.astype(it)), Dev(gexec, vals)
            db, dcc, dal = Dev(gexec, fb), Dev(gexec, fc), Dev(gexec, alpha)
            _call("gkoc_ccoo_spmv2_" + tn + "_" + in_, gexec.stream, len(vals), nrhs, dr, dc, dv,
                  dal if with_alpha else None, db, nrhs + 2, dcc, nrhs + 3)
            sync()
            got = dcc.get()
            assert canaries_ok(got, nrhs) and same_bits(db.get(), fb) and same_bits(dv.get(), vals)
            assert same_bits(dr.get(), rows.astype(it)) and same_bits(dc.get(), cols.astype(it))
            assert same_bits(dal.get(), alpha)
            got = got[:, :nrhs]
            ref, m, S = vr.coo_spmv2_fast(rows, cols, vals, b, c0, alpha[0] if with_alpha else None)
            if integers:
                assert np.array_equal(got.astype(np.clongdouble), ref), name          # exact in every order
            err = np.abs(got.astype(np.clongdouble) - ref)
            assert np.all(err <= (m + 4) * eps * S), (name, float(np.max(err / (eps * np.maximum(S, 1e-300)))))
            assert same_bits(got[m == 0], c0[m == 0]), "rows without an entry keep c"
            if not integers and len(vals):
                hit = m > 0
                _stat("ccoo_spmv2: |got - ref| / ((m + 4) eps S)", tn, float(np.max(err[hit] / ((m[hit] + 4) * eps * S[hit]))))
                if name == "one row":
                    assert m[31, 0] == 20000 and np.count_nonzero(m[:, 0]) == 1


# ------------------------------------------------------------------------------------------- Ell
@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_ell_copy(gexec, tn, in_):
    """random bit patterns into another stride; the padding rows n_rows .. dst_stride keep the fill"""
    t, it = br.TYPES[tn], IT[in_]
    rng = np.random.default_rng(71)
    for n, k, ss, ds in [(0, 3, 0, 4), (1, 1, 1, 1), (255, 4, 255, 260), (256, 2, 300, 256), (257, 5, 257, 257),
                         (2049, 3, 2052, 2050), (100003, 2, 100003, 100010), (7, 0, 9, 8)]:
        sc, sv = rng.integers(-1, max(n, 1), ss * k).astype(it), vr.random_bits(rng, ss * k, t)
        dc0, dv0 = np.full(ds * k + 3, -5, it), np.full(ds * k + 3, CANARY, t)
        dsc, dsv, ddc, ddv = Dev(gexec, sc), Dev(gexec, sv), Dev(gexec, dc0), Dev(gexec, dv0)
        _call("gkoc_ell_copy_" + tn + "_" + in_, gexec.stream, n, k, ss, dsc, dsv, ds, ddc, ddv)
        sync()
        wc, wv = vr.ell_copy(n, k, ss, sc, sv, ds, dc0, dv0)
        assert same_bits(ddc.get(), wc) and same_bits(ddv.get(), wv), (n, k)
        assert same_bits(dsc.get(), sc) and same_bits(dsv.get(), sv)
    before = ddc.get()
    assert raises_invalid("gkoc_ell_copy_" + tn + "_" + in_, gexec.stream, 7, 1, 6, dsc, dsv, 8, ddc, ddv)
    assert raises_invalid("gkoc_ell_copy_" + tn + "_" + in_, gexec.stream, 7, 1, 9, dsc, dsv, 6, ddc, ddv)
    sync()
    assert same_bits(ddc.get(), before)


def test_ell_copy_beyond_the_grid_cap(gexec):
    """the grid_for style of coo.hip"""
    n = _grid_cap_rows() + 257
    sc, sv = (np.arange(n) % 1000).astype(np.int32), (np.arange(n) % 13 - 6).astype(np.float32)
    ddc, ddv = _out(gexec, n + 2, np.int32, fill=-5), _out(gexec, n + 2, np.float32)
    _call("gkoc_ell_copy_f32_i32", gexec.stream, n, 1, n, Dev(gexec, sc), Dev(gexec, sv), n + 2, ddc, ddv)
    sync()
    gc, gv = ddc.get(), ddv.get()
    assert _tail_ok(gc, n + 2) and _tail_ok(gv, n + 2) and np.all(gc[n:n + 2] == -5) and np.all(np.isnan(gv[n:n + 2]))
    assert np.array_equal(gc[:n], sc) and np.array_equal(gv[:n], sv), np.flatnonzero(gv[:n] != sv)[:4]


def _diag_rows(rng, n, t):
    """rows of 0 .. 5 entries in storage order, with and without a diagonal entry, the diagonal at the front, in
    the middle or at the end; row 4 (where it exists) stores its column twice, row 5 only padding"""
    rows = []
    for r in range(n):
        k = int(rng.integers(0, 6))
        cols = [int(c) for c in rng.choice(n, min(k, n), replace=False) if c != r]
        if r % 3:
            cols.insert(int(rng.integers(0, len(cols) + 1)), r)
        if r == 4:
            cols = [1, 4, 4]
        if r == 5:
            cols = []
        rows.append(list(zip(cols, vr.random_bits(rng, len(cols), t))))
    return rows


def _diag_table(rng, n, t, width=6):
    """the same kind of rows as an n x width table built with arrays (the 100 003-row cases): 0 .. 5 leading slots
    per row with random columns, rows with r % 3 != 0 get their own column in a random one of them"""
    length = rng.integers(0, width, n)
    C = rng.integers(0, max(n, 1), (n, width))
    r = np.arange(n)
    C[C == r[:, None]] = (r[:, None] + np.zeros((1, width), np.int64))[C == r[:, None]] // 2   # off the diagonal, but for r = 0
    C[0, :] = -1
    length[0] = 0
    want_diag = (r % 3 != 0) & (length > 0)
    slot = rng.integers(0, width, n) % np.maximum(length, 1)
    C[r[want_diag], slot[want_diag]] = r[want_diag]
    C[np.arange(width)[None, :] >= length[:, None]] = -1
    V = vr.random_bits(rng, n * width, t).reshape(n, width)
    return C, V


def test_diag_table_has_rows_with_and_without_a_diagonal():
    C, _ = _diag_table(np.random.default_rng(1), 100003, np.float64)
    has = np.any(C == np.arange(100003)[:, None], axis=1)
    assert 60000 > np.count_nonzero(has) > 40000 and not np.any(has[::3]) and np.count_nonzero(C == -1) > 100003


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_ell_extract_diagonal(gexec, tn, in_):
    t, it = br.TYPES[tn], IT[in_]
    for n in [0, 1, 255, 256, 257, 2049]:
        rng = np.random.default_rng(n + 73)
        rows = _diag_rows(rng, n, t)
        ell_k, stride = 6, n + 3
        cols, vals = vr.ell_from_rows(rows, stride, ell_k, t, it)
        before = np.concatenate([vr.random_bits(rng, n, t), np.full(3, CANARY, t)])
        dc, dv, dd = Dev(gexec, cols), Dev(gexec, vals), Dev(gexec, before)
        _call("gkoc_ell_extract_diagonal_" + tn + "_" + in_, gexec.stream, n, ell_k, stride, dc, dv, dd)
        sync()
        got = dd.get()
        assert _tail_ok(got, n) and same_bits(dc.get(), cols) and same_bits(dv.get(), vals)
        assert same_bits(got[:n], vr.ell_extract_diagonal(n, ell_k, stride, cols, vals, before[:n])), n
        if n > 5:
            assert same_bits(got[[0, 3, 5]], before[[0, 3, 5]]) and same_bits(got[4:5], vals[4 + stride:5 + stride])
    n = 100003
    rng = np.random.default_rng(74)
    C, V = _diag_table(rng, n, t)
    cols, vals = vr.ell_from_table(C, V, n + 3, it)
    before = np.concatenate([vr.random_bits(rng, n, t), np.full(3, CANARY, t)])
    dc, dv, dd = Dev(gexec, cols), Dev(gexec, vals), Dev(gexec, before)
    _call("gkoc_ell_extract_diagonal_" + tn + "_" + in_, gexec.stream, n, 6, n + 3, dc, dv, dd)
    sync()
    got = dd.get()
    assert _tail_ok(got, n) and same_bits(dc.get(), cols) and same_bits(dv.get(), vals)
    assert same_bits(got[:n], vr.ell_extract_diagonal(n, 6, n + 3, cols, vals, before[:n]))
    assert same_bits(got[:n:3], before[:n:3])


@pytest.mark.parametrize("slice_size", [32, 64])
@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_sellp_extract_diagonal(gexec, tn, in_, slice_size):
    """slices of 32 and 64 rows, the last one not full (n = 255, 257, 2049) or full (n = 256)"""
    t, it = br.TYPES[tn], IT[in_]
    for n in [0, 1, 255, 256, 257, 2049]:
        rng = np.random.default_rng(n + 79)
        rows = _diag_rows(rng, n, t)
        sets, cols, vals = vr.sellp_from_rows(rows, slice_size, t, it)
        before = np.concatenate([vr.random_bits(rng, n, t), np.full(3, CANARY, t)])
        ds, dc, dv, dd = Dev(gexec, sets), Dev(gexec, cols), Dev(gexec, vals), Dev(gexec, before)
        _call("gkoc_sellp_extract_diagonal_" + tn + "_" + in_, gexec.stream, n, slice_size, ds, dc, dv, dd)
        sync()
        got = dd.get()
        assert _tail_ok(got, n) and same_bits(dc.get(), cols) and same_bits(dv.get(), vals) and same_bits(ds.get(), sets)
        assert same_bits(got[:n], vr.sellp_extract_diagonal(n, slice_size, sets, cols, vals, before[:n])), n
        if n > 5:
            assert same_bits(got[[0, 3, 5]], before[[0, 3, 5]])
    n = 100003
    rng = np.random.default_rng(80)
    C, V = _diag_table(rng, n, t)
    sets, cols, vals = vr.sellp_from_table(C, V, slice_size, it)
    before = np.concatenate([vr.random_bits(rng, n, t), np.full(3, CANARY, t)])
    ds, dc, dv, dd = Dev(gexec, sets), Dev(gexec, cols), Dev(gexec, vals), Dev(gexec, before)
    _call("gkoc_sellp_extract_diagonal_" + tn + "_" + in_, gexec.stream, n, slice_size, ds, dc, dv, dd)
    sync()
    got = dd.get()
    assert _tail_ok(got, n) and same_bits(dc.get(), cols) and same_bits(dv.get(), vals) and same_bits(ds.get(), sets)
    assert same_bits(got[:n], vr.sellp_extract_diagonal(n, slice_size, sets, cols, vals, before[:n]))
    assert same_bits(got[:n:3], before[:n:3])
    assert raises_invalid("gkoc_sellp_extract_diagonal_" + tn + "_" + in_, gexec.stream, 4, 0, ds, dc, dv, dd)


@pytest.mark.parametrize("fmt", ["ell", "sellp"])
def test_extract_diagonal_does_not_look_at_values(gexec, fmt):
    """a slot counts by its column alone: an explicit zero stored at (r, r) in front of another (r, r) entry is
    the diagonal (-0.0 bit for bit); padding has column -1 and is never one, whatever row it belongs to"""
    t, it = np.float64, np.int32
    rows = [[(0, 0.0), (0, 5.0)], [(0, 1.0)], [(2, -0.0), (1, 3.0), (2, 7.0)], []]
    before = np.array([9.0, 9.0, 9.0, 9.0, CANARY])
    dd = Dev(gexec, before)
    if fmt == "ell":
        cols, vals = vr.ell_from_rows(rows, 5, 3, t, it)
        _call("gkoc_ell_extract_diagonal_f64_i32", gexec.stream, 4, 3, 5, Dev(gexec, cols), Dev(gexec, vals), dd)
    else:
        sets, cols, vals = vr.sellp_from_rows(rows, 32, t, it)
        _call("gkoc_sellp_extract_diagonal_f64_i32", gexec.stream, 4, 32, Dev(gexec, sets), Dev(gexec, cols),
              Dev(gexec, vals), dd)
    sync()
    got = dd.get()
    assert np.count_nonzero(cols == -1) > 0 and np.all(vals[cols == -1] == 0)
    assert same_bits(got, np.array([0.0, 9.0, -0.0, 9.0, CANARY]))


def test_ell_extract_diagonal_beyond_the_grid_cap(gexec):
    """the CV_LAUNCH style of conversions.hip: one slot per row, every third row off the diagonal"""
    n = _grid_cap_rows() + 257
    r = np.arange(n)
    cols = np.where(r % 3 == 0, (r + 1) % n, r).astype(np.int32)
    vals = (r % 17 + 1).astype(np.float32)
    dd = _out(gexec, n, np.float32, fill=-3.0)
    _call("gkoc_ell_extract_diagonal_f32_i32", gexec.stream, n, 1, n, Dev(gexec, cols), Dev(gexec, vals), dd)
    sync()
    got = dd.get()
    want = np.where(r % 3 == 0, np.float32(-3), vals)
    assert _tail_ok(got, n) and np.array_equal(got[:n], want), np.flatnonzero(got[:n] != want)[:4]


# ------------------------------------------------------------------------------------------ Jacobi
def _scheme(max_bs):
    from ginkgo_amd.preconditioner import compute_storage_scheme
    return compute_storage_scheme(max_bs)


@pytest.mark.parametrize("conj", [0, 1])
@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", CTN)
def test_cjacobi_transpose(gexec, tn, in_, conj):
    """blocks of 1 .. 32 rows, mixed, in the block-interleaved storage of compute_storage_scheme; the storage
    between the blocks keeps the fill; applied twice it is the identity"""
    t, it = br.TYPES[tn], IT[in_]
    for max_bs, num in [(32, 67), (32, 1), (13, 300), (4, 1000), (1, 257), (8, 22300)]:      # the last: about 100 000 rows
        rng = np.random.default_rng(max_bs * 1000 + num)
        scheme = _scheme(max_bs)
        sizes = np.concatenate([[max_bs], rng.integers(1, max_bs + 1, num - 1)])
        if max_bs == 32 and num > 40:
            sizes[1:33] = np.arange(1, 33)
        ptrs = np.concatenate([[0], np.cumsum(sizes)]).astype(it)
        total = vr.block_storage_size(scheme, num)
        blocks = vr.random_bits(rng, total, t)
        fill = np.concatenate([np.full(total, 3.5, t), np.full(3, CANARY, t)])
        dp, db, do = Dev(gexec, ptrs), Dev(gexec, blocks), Dev(gexec, fill)
        _call("gkoc_cjacobi_transpose_" + tn + "_" + in_, gexec.stream, num, scheme, dp, db, conj, do)
        sync()
        got = do.get()
        want = vr.jacobi_transpose(scheme, ptrs, blocks, conj, fill[:total])
        assert _tail_ok(got, total) and same_bits(dp.get(), ptrs) and same_bits(db.get(), blocks)
        assert same_bits(got[:total], want), (max_bs, num, np.flatnonzero(got[:total] != want)[:4])
        assert np.count_nonzero(want.view(br.real_of(t))[::2] != 3.5) <= int(np.sum(sizes.astype(np.int64) ** 2))
        back = Dev(gexec, fill)
        _call("gkoc_cjacobi_transpose_" + tn + "_" + in_, gexec.stream, num, scheme, dp, do, conj, back)
        sync()
        again = back.get()
        assert same_bits(again[:total], vr.jacobi_transpose(scheme, ptrs, got[:total], conj, fill[:total]))
        inside = vr.jacobi_transpose(scheme, ptrs, np.ones(total, t), 0, np.zeros(total, t)) == 1
        assert same_bits(again[:total][inside], blocks[inside]), "transposed twice"
    _call("gkoc_cjacobi_transpose_" + tn + "_" + in_, gexec.stream, 0, scheme, dp, db, conj, do)
    sync()
    assert same_bits(do.get(), got)


def test_cjacobi_transpose_beyond_the_grid_cap(gexec):
    """the 4 * max_stream_blocks form of jacobi.hip: blocks of one row (block b is entry b of the storage)"""
    n = _grid_cap_rows() + 257
    scheme = _scheme(1)
    total = vr.block_storage_size(scheme, n)
    blocks = ((np.arange(total) % 7 - 3) + 1j * (np.arange(total) % 5 - 2)).astype(np.complex64)
    do = _out(gexec, total, np.complex64, fill=3.5)
    _call("gkoc_cjacobi_transpose_c64_i32", gexec.stream, n, scheme, Dev(gexec, np.arange(n + 1, dtype=np.int32)),
          Dev(gexec, blocks), 1, do)
    sync()
    got = do.get()
    assert _tail_ok(got, total) and np.all(got[n:total] == 3.5)
    assert np.array_equal(got[:n], np.conj(blocks[:n])), np.flatnonzero(got[:n] != np.conj(blocks[:n]))[:4]


def test_jacobi_initialize_precisions(gexec):
    """precisions[i] = source[i % source_size]: source_size 1, 3 and larger than n"""
    rng = np.random.default_rng(83)
    for n in SIZES:
        for source_size in (1, 3, n + 5):
            source = rng.integers(0, 256, source_size).astype(np.uint8)
            ds = Dev(gexec, source)
            out = Dev(gexec, np.concatenate([np.full(n, 0xAB, np.uint8), np.full(5, 0xCD, np.uint8)]))
            _call("gkoc_jacobi_initialize_precisions", gexec.stream, ds, source_size, out, n)
            sync()
            got = out.get()
            assert np.all(got[n:] == 0xCD) and np.array_equal(got[:n], vr.initialize_precisions(source, n))
            assert np.array_equal(ds.get(), source)
    before = out.get()
    assert raises_invalid("gkoc_jacobi_initialize_precisions", gexec.stream, ds, 0, out, 4)
    assert raises_invalid("gkoc_jacobi_initialize_precisions", gexec.stream, ds, -1, out, 4)
    _call("gkoc_jacobi_initialize_precisions", gexec.stream, ds, 0, out, 0)             # nothing to do: accepted
    sync()
    assert np.array_equal(out.get(), before)


def test_jacobi_initialize_precisions_beyond_the_grid_cap(gexec):
    """the max_stream_blocks form (a quarter of the other cap)"""
    n = _grid_cap_rows() + 257
    source = np.array([1, 2, 0x11], np.uint8)
    out = Dev(gexec, np.concatenate([np.full(n, 0xAB, np.uint8), np.full(5, 0xCD, np.uint8)]))
    _call("gkoc_jacobi_initialize_precisions", gexec.stream, Dev(gexec, source), 3, out, n)
    sync()
    got = out.get()
    assert np.all(got[n:] == 0xCD) and np.array_equal(got[:n], source[np.arange(n) % 3])


@pytest.fixture(scope="module", autouse=True)
def _print_tables():
    """after the last test of this file: the figures its tests gathered (pytest -s)"""
    yield
    if not STATS:
        return
    print("\nlargest observed |kernel - ref| / (eps max|ref|) (rows marked otherwise: that unit)")
    print("| entry point | " + " | ".join(CTN) + " |")
    for name in sorted({k[0] for k in STATS}, key=lambda s: s.strip(" .")):
        print("| " + name + " | " + " | ".join("%.2f" % STATS.get((name, tn), float("nan")) for tn in CTN) + " |")
