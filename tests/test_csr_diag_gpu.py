"""Row scans of Csr, matrix::Diagonal and the SparsityCsr pair through the C ABI against
tests/csr_struct_refs.py: csr::row_wise_absolute_sum and gkoc_ccsr_row_scan (csr_row_scan_kernel,
csrc/complex_blas.hip), the gkoc_diagonal_* group and gkoc_sparsity_csr_* (csrc/misc.hip).

The row sums are left-to-right sums like the plain restatement: rule R, exact on small integers.  The
Diagonal products are one product (and one reciprocal) per entry: bit-identical to the plain restatement.
Everything else is copies and integers.  Inputs are read back and compared bit for bit, outputs are followed
by a canary or sit in padded operands.  The last test prints the largest observed
|kernel - ref| / (eps max|ref|) of the row sums (pytest -s)."""
import numpy as np
import pytest

import binding_refs as br
import csr_struct_refs as cr
from binding_gpu import CANARY, Dev, DevCsr, call as _call, grid_cap_rows as _grid_cap_rows, out_buf as _out, \
    padded, same_bits, sync, tail_ok as _tail_ok

pytestmark = pytest.mark.gpu

TN = ["f64", "f32", "c128", "c64"]
IT = {"i32": np.int32, "i64": np.int64}
STATS = {}
ROW_LENGTHS = [0, 1, 63, 64, 65, 5000, 0, 2]


def _rows_matrix(rng, t, integers=False):
    """rows of ROW_LENGTHS entries, random columns in storage order (row sums do not need sorted rows)"""
    ptrs = np.concatenate([[0], np.cumsum(ROW_LENGTHS)])
    n = int(ptrs[-1])
    cols = np.concatenate([np.sort(rng.choice(6000, k, replace=False)) for k in ROW_LENGTHS]).astype(np.int64)
    if integers:
        re = rng.integers(-4, 5, n).astype(np.float64)
        vals = np.where(rng.integers(0, 2, n).astype(bool), 1j * re, re).astype(t) if br.is_complex(t) \
            else re.astype(t)
    else:
        vals = cr.random_values(rng, n, t)
    return ptrs, cols, vals


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_row_abs_sums(gexec, tn, in_):
    """real types: gkoc_csr_row_wise_absolute_sum; complex types: gkoc_ccsr_row_scan mode 1, |a| the modulus,
    the sum stored as (sum, 0)"""
    t, it = br.TYPES[tn], IT[in_]
    rng = np.random.default_rng(41)
    n = len(ROW_LENGTHS)
    for integers in (True, False):
        A = _rows_matrix(rng, t, integers)
        da = DevCsr(gexec, it, *A)
        out = _out(gexec, n, t)
        if br.is_complex(t):
            _call("gkoc_ccsr_row_scan_" + tn + "_" + in_, gexec.stream, n, *da.dev, out, 1)
        else:
            _call("gkoc_csr_row_wise_absolute_sum_" + tn + "_" + in_, gexec.stream, n, da.dev[0], da.dev[2], out)
        sync()
        got = out.get()
        assert _tail_ok(got, n) and da.unchanged()
        got = got[:n]
        assert np.all(got.imag == 0) and not np.any(np.signbit(got.imag))
        ref, plain = cr.row_abs_sum(br.hp(t), A[0], A[2]), cr.row_abs_sum(br.plain(t), A[0], A[2])
        if integers:
            assert np.array_equal(got.real.astype(np.longdouble), ref)          # exact in every order
        ok, ratio = br.rule_r(got.real, ref, plain, t)
        assert ok, ratio
        if not integers:
            STATS[("row sums", tn)] = max(STATS.get(("row sums", tn), 0.0), ratio)


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", ["c128", "c64"])
def test_row_scan_diagonal(gexec, tn, in_):
    """mode 0: out[r] = the FIRST stored entry with column r; rows without one keep what out held"""
    t, it = br.TYPES[tn], IT[in_]
    rng = np.random.default_rng(43)
    rows = [[0, 3], [0, 2], [2, 2, 5], [], [1, 4, 4, 4], [5], [0, 1, 2, 3, 4, 5, 6], [0, 6]]
    ptrs = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    cols = np.array([c for r in rows for c in r], np.int64)
    vals = cr.random_values(rng, len(cols), t)
    n = len(rows)
    before = np.full(n + 2, CANARY, t)
    before[:n] = cr.random_values(rng, n, t)
    da, out = DevCsr(gexec, it, ptrs, cols, vals), Dev(gexec, before)
    _call("gkoc_ccsr_row_scan_" + tn + "_" + in_, gexec.stream, n, *da.dev, out, 0)
    sync()
    got = out.get()
    want = cr.extract_diagonal(ptrs, cols, vals, before[:n])
    assert same_bits(got[:n], want) and _tail_ok(got, n) and da.unchanged()
    assert same_bits(want[[1, 3, 7]], before[[1, 3, 7]]) and want[2] == vals[4] and want[4] == vals[8]


def test_row_scan_argument_checks(gexec):
    from ginkgo_amd._lib import GkoError
    out = Dev(gexec, np.full(4, CANARY, np.complex128))
    da = DevCsr(gexec, np.int32, [0, 1, 2], [0, 1], np.ones(2, np.complex128))
    for mode in (2, -1):
        with pytest.raises(GkoError):
            _call("gkoc_ccsr_row_scan_c128_i32", gexec.stream, 2, *da.dev, out, mode)
    _call("gkoc_ccsr_row_scan_c128_i32", gexec.stream, 0, *da.dev, out, 1)
    _call("gkoc_csr_row_wise_absolute_sum_f64_i32", gexec.stream, 0, da.dev[0], da.dev[2], out)
    sync()
    assert np.all(out.get() == CANARY)


def test_row_sums_rows_beyond_the_grid_cap(gexec):
    """the GKOC_FOR2 style (capped grid, grid-stride loop): one entry per row"""
    n = _grid_cap_rows() + 257
    vals = (np.arange(n) % 9 - 4).astype(np.float32)
    da = DevCsr(gexec, np.int32, np.arange(n + 1), np.arange(n), vals)
    out = _out(gexec, n, np.float32)
    _call("gkoc_csr_row_wise_absolute_sum_f32_i32", gexec.stream, n, da.dev[0], da.dev[2], out)
    sync()
    got = out.get()
    assert _tail_ok(got, n) and np.array_equal(got[:n], np.abs(vals)), np.flatnonzero(got[:n] != np.abs(vals))[:4]


# ------------------------------------------------------------------------------------ Diagonal
def _diag(rng, n, t):
    """entries away from zero, both branches of the complex reciprocal (|re| >= |im| and the opposite)"""
    d = cr.random_values(rng, n, t)
    d = d + np.where(d.real < 0, -1, 1).astype(t)
    if br.is_complex(t):
        d[1::2] = d[1::2] * t(1j)
    return d.astype(t)


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("rows,cols", [(1, 1), (17, 5), (300, 33), (0, 4), (4, 0)])
def test_diagonal_apply_to_dense(gexec, tn, rows, cols):
    t = br.TYPES[tn]
    rng = np.random.default_rng(rows * 50 + cols)
    b = cr.random_values(rng, rows * cols, t).reshape(rows, cols)
    dl, dr = _diag(rng, rows, t), _diag(rng, cols, t)
    fb = padded(b, cols + 2)
    cases = [("gkoc_diagonal_apply_to_dense_", dl, (0,), cr.diag_apply_dense(br.plain(t), dl, b)),
             ("gkoc_diagonal_apply_to_dense_", dl, (1,), cr.diag_apply_dense(br.plain(t), dl, b, True)),
             ("gkoc_diagonal_right_apply_to_dense_", dr, (), cr.diag_right_apply_dense(br.plain(t), dr, b))]
    for name, diag, extra, want in cases:
        fc = padded(np.full((rows, cols), np.nan, t), cols + 3)
        dd, db, dc = Dev(gexec, diag), Dev(gexec, fb), Dev(gexec, fc)
        _call(name + tn, gexec.stream, rows, cols, dd, db, cols + 2, dc, cols + 3, *extra)
        sync()
        got = dc.get()
        assert np.all(got[:, cols:] == t(CANARY)) and same_bits(db.get(), fb) and same_bits(dd.get(), diag)
        assert same_bits(got[:, :cols], want), (name, extra)


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_diagonal_apply_to_csr(gexec, tn, in_):
    """the values of a Csr in place: rows by diag[row] (or its reciprocal), entries by diag[column]; rows of
    0, 1, 63, 64, 65 and 200 entries for the wave-per-row kernel"""
    t, it = br.TYPES[tn], IT[in_]
    rng = np.random.default_rng(47)
    lengths = [0, 1, 63, 64, 65, 200, 0, 3] + [int(k) for k in rng.integers(0, 9, 300)]
    n = len(lengths)
    ptrs = np.concatenate([[0], np.cumsum(lengths)])
    cols = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lengths]).astype(np.int64)
    nnz = len(cols)
    vals = cr.random_values(rng, nnz, t)
    diag = _diag(rng, n, t)
    plain = br.plain(t)
    for name, args, want in (
            ("gkoc_diagonal_apply_to_csr_", lambda dp, dc, dd, dv: (n, dd, dp, dv, 0),
             cr.diag_apply_csr(plain, diag, ptrs, vals)),
            ("gkoc_diagonal_apply_to_csr_", lambda dp, dc, dd, dv: (n, dd, dp, dv, 1),
             cr.diag_apply_csr(plain, diag, ptrs, vals, True)),
            ("gkoc_diagonal_right_apply_to_csr_", lambda dp, dc, dd, dv: (nnz, dd, dc, dv),
             cr.diag_right_apply_csr(plain, diag, cols, vals))):
        v = np.concatenate([vals, np.full(3, CANARY, t)])
        dp, dc, dd, dv = Dev(gexec, ptrs.astype(it)), Dev(gexec, cols.astype(it)), Dev(gexec, diag), Dev(gexec, v)
        _call(name + tn + "_" + in_, gexec.stream, *args(dp, dc, dd, dv))
        sync()
        got = dv.get()
        assert _tail_ok(got, nnz) and same_bits(got[:nnz], want), name
        assert same_bits(dp.get(), ptrs.astype(it)) and same_bits(dc.get(), cols.astype(it))
        assert same_bits(dd.get(), diag)
    _call("gkoc_diagonal_apply_to_csr_" + tn + "_" + in_, gexec.stream, 0, dd, dp, dv, 0)       # no rows, no entries
    _call("gkoc_diagonal_right_apply_to_csr_" + tn + "_" + in_, gexec.stream, 0, dd, dc, dv)
    sync()
    assert same_bits(dv.get(), got)


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("n", [0, 1, 257, 1000])
def test_diagonal_convert_to_csr(gexec, tn, in_, n):
    t, it = br.TYPES[tn], IT[in_]
    diag = cr.random_values(np.random.default_rng(n), n, t)
    dd = Dev(gexec, diag)
    dp, dc, dv = _out(gexec, n + 1, it, fill=-5), _out(gexec, n, it, fill=-5), _out(gexec, n, t)
    _call("gkoc_diagonal_convert_to_csr_" + tn + "_" + in_, gexec.stream, n, dd, dp, dc, dv)
    sync()
    wp, wc, wv = cr.diag_to_csr(diag, it)
    gp, gc, gv = dp.get(), dc.get(), dv.get()
    assert _tail_ok(gp, n + 1) and _tail_ok(gc, n) and _tail_ok(gv, n) and same_bits(dd.get(), diag)
    assert same_bits(gp[:n + 1], wp) and same_bits(gc[:n], wc) and same_bits(gv[:n], wv)
    assert gp[0] == 0                                    # n = 0: row_ptrs[0] = 0 and nothing else


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_diagonal_fill_in_matrix_data(gexec, tn, in_):
    """triplets in any order, at most one per diagonal position; off-diagonal ones are ignored, positions
    without a triplet keep what diag held"""
    t, it = br.TYPES[tn], IT[in_]
    rng = np.random.default_rng(53)
    n = 400
    on = rng.choice(n, 250, replace=False)
    rows = np.concatenate([on, rng.integers(0, n, 600)])
    cols = np.concatenate([on, rng.integers(0, n, 600)])
    off = np.arange(len(rows)) >= 250
    cols[off & (rows == cols)] = (cols[off & (rows == cols)] + 1) % n           # the random ones: off the diagonal
    order = rng.permutation(len(rows))
    rows, cols = rows[order], cols[order]
    vals = cr.random_values(rng, len(rows), t)
    before = np.concatenate([cr.random_values(rng, n, t), np.full(2, CANARY, t)])
    dr, dc, dv, dd = Dev(gexec, rows.astype(it)), Dev(gexec, cols.astype(it)), Dev(gexec, vals), Dev(gexec, before)
    _call("gkoc_diagonal_fill_in_matrix_data_" + tn + "_" + in_, gexec.stream, len(rows), dr, dc, dv, dd)
    sync()
    got = dd.get()
    want = cr.diag_fill(rows, cols, vals, before[:n])
    assert _tail_ok(got, n) and same_bits(got[:n], want)
    assert np.count_nonzero(want != before[:n]) == 250
    assert same_bits(dr.get(), rows.astype(it)) and same_bits(dc.get(), cols.astype(it)) and same_bits(dv.get(), vals)
    _call("gkoc_diagonal_fill_in_matrix_data_" + tn + "_" + in_, gexec.stream, 0, dr, dc, dv, dd)
    sync()
    assert same_bits(dd.get(), got)


def test_diagonal_right_apply_to_csr_beyond_the_grid_cap(gexec):
    """the GKOC_FOR style of misc.hip (capped grid, grid-stride loop): one thread per entry"""
    nnz = _grid_cap_rows() + 257
    cols = (np.arange(nnz) % 5).astype(np.int32)
    vals = (np.arange(nnz) % 7 - 3).astype(np.float64)
    diag = np.array([2, -1, 3, 4, -2], np.float64)
    dv = Dev(gexec, np.concatenate([vals, [CANARY] * 3]))
    _call("gkoc_diagonal_right_apply_to_csr_f64_i32", gexec.stream, nnz, Dev(gexec, diag), Dev(gexec, cols), dv)
    sync()
    got = dv.get()
    want = vals * diag[cols]
    assert _tail_ok(got, nnz) and np.array_equal(got[:nnz], want), np.flatnonzero(got[:nnz] != want)[:4]


# --------------------------------------------------------------------------------- SparsityCsr
@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("n", [0, 1, 700])
def test_sparsity_csr_remove_diagonal(gexec, in_, n):
    """count, the caller's scan (diagonal_element_prefix_sum), remove"""
    it = IT[in_]
    rng = np.random.default_rng(59 + n)
    p, c = cr.random_pattern(rng, n, max(n, 1), 0.02 if n > 1 else 1.1, (5,) if n > 5 else ())
    rows = [c[p[r]:p[r + 1]].tolist() for r in range(n)]
    if n > 20:
        rows[3], rows[4], rows[6] = [3], [1, 4, 4, 9], [r for r in rows[6] if r != 6]   # only / twice / no diagonal
        rows[n - 1] = [0, n - 1]
    ptrs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = np.array([x for r in rows for x in r], np.int64)
    da = DevCsr(gexec, it, ptrs, cols)
    counts = _out(gexec, n + 1, it, fill=-5, tail=2)
    _call("gkoc_sparsity_csr_count_diagonal_" + in_, gexec.stream, n, *da.dev, counts)
    sync()
    got = counts.get()
    want = cr.count_diagonal(ptrs, cols)
    assert _tail_ok(got, n + 1) and np.array_equal(got[:n + 1], want)
    _call("gkoc_prefix_sum_nonnegative_" + in_, gexec.stream, counts, n + 1)
    sync()
    prefix = counts.get()[:n + 1]
    assert np.array_equal(prefix, np.concatenate([[0], np.cumsum(want[:n])]))
    wp, wi = cr.remove_diagonal(ptrs, cols, prefix)
    ap, ai = _out(gexec, n + 1, it, fill=-5), _out(gexec, len(wi), it, fill=-5)
    _call("gkoc_sparsity_csr_remove_diagonal_" + in_, gexec.stream, n, *da.dev, counts, ap, ai)
    sync()
    gp, gi = ap.get(), ai.get()
    assert _tail_ok(gp, n + 1) and _tail_ok(gi, len(wi)) and da.unchanged()
    assert np.array_equal(gp[:n + 1], wp) and np.array_equal(gi[:len(wi)], wi)
    if n > 20:
        assert want[3] == 1 and want[4] == 2 and want[5] == 0 and want[6] == 0
        assert gp[4] == gp[3] and list(gi[gp[4]:gp[5]]) == [1, 9]


def test_print_tables():
    print("\nlargest observed |kernel - ref| / (eps max|ref|)")
    print("| entry point | " + " | ".join(TN) + " |")
    for name in sorted({k[0] for k in STATS}):
        print("| " + name + " | " + " | ".join("%.2f" % STATS.get((name, tn), float("nan")) for tn in TN) + " |")
