"""The ELL and SELL-P products through gkoc_ell_[advanced_]spmv_* and gkoc_sellp_[advanced_]spmv_* in float,
double and both complex types with both index types, at the smallest shapes that select every branch of
the launchers of csrc/formats.hip (the list of branches and what reaches them: docs/binding_kernel_tests.md,
"ELL and SELL-P products and set-up").  The matrices, operand layouts and scalars come from
tests/format_spmv_refs.py, whose CPU test checks that the case lists cover what they promise.

Real types: bit for bit against the plain restatement, and against the plain-C oracle.  Complex types: rule R
against the long-double value, sized by the plain restatement; the largest |kernel - ref| / (eps max|ref|)
and whether the plain restatement's bits were met are recorded (util.record_perf, `pytest -s`).
After every call every input is read back and compared bit for bit, and c is cut from a padded array whose
padding (and the element in front of a c that starts one element in) must keep the canary."""
import functools

import numpy as np
import pytest

import binding_refs as br
import format_spmv_refs as fr
from binding_gpu import CANARY, Dev, canaries_ok, grid_cap_rows, padded, raises_invalid, same_bits
from binding_gpu import call as _call
from test_csr_spmv_branches_gpu import KEY_MULTI_CHUNK, tuned
from util import record_perf

pytestmark = pytest.mark.gpu

TN = {np.float64: "f64", np.float32: "f32", np.complex128: "c128", np.complex64: "c64"}
IN = {np.int32: "i32", np.int64: "i64"}
REAL = (np.float64, np.float32)
COMPLEX = (np.complex128, np.complex64)
INDEX = (np.int32, np.int64)


class Strided:
    """rows x cols values inside a rows x ld padded array that starts `off` elements into its buffer"""

    def __init__(self, gexec, a, ld, off=0):
        self.rows, self.cols, self.ld, self.off = a.shape[0], a.shape[1], ld, off
        self.host = np.concatenate((np.full(off, CANARY, a.dtype), padded(a, ld).reshape(-1)))
        self.dev = Dev(gexec, self.host)
        self.ptr = self.dev.at(off)
        self.address = self.dev.t.data_ptr() + off * a.dtype.itemsize

    def unchanged(self):
        return same_bits(self.dev.get(), self.host)

    def result(self):
        """the values, after checking the canaries around them"""
        got = self.dev.get()
        body = got[self.off:].reshape(self.rows, self.ld)
        assert np.all(got[:self.off] == got.dtype.type(CANARY)), "written in front of c"
        assert canaries_ok(body, self.cols), "written into the padding columns of c"
        return body[:, :self.cols].copy()


class DevMatrix:
    """an ELL (kind 'ell': k, stride, cols, vals) or SELL-P ('sellp': slice_size, sets, lens, cols, vals)
    matrix on the device with the host arrays it was made from"""

    def __init__(self, gexec, kind, n_rows, n_cols, head, arrays):
        self.kind, self.n_rows, self.n_cols, self.head = kind, n_rows, n_cols, head
        self.host = list(arrays)
        self.dev = [Dev(gexec, a) for a in arrays]
        self.t, self.it = arrays[-1].dtype.type, arrays[-2].dtype.type

    def unchanged(self):
        return all(same_bits(d.get(), h) for d, h in zip(self.dev, self.host))

    def product(self, b, **kw):
        if self.kind == "ell":
            return fr.ell_product(self.t, self.n_rows, *self.head, *self.host, b, **kw)
        return fr.sellp_product(self.t, self.n_rows, *self.head, *self.host, b, **kw)

    def oracle(self, oracle, b, scal, c):
        fn = oracle.ell_spmv if self.kind == "ell" else oracle.sellp_spmv
        args = (self.n_rows, *self.head, *self.host, b)
        return fn(*args) if scal is None else fn(*args, scal[0], scal[1], c)


def ell_matrix(gexec, t, it, rows, n_cols, k, stride, pad_value=None):
    cols, vals = fr.ell_build(rows, k, stride, t, it)
    if pad_value is not None:
        vals[cols < 0] = pad_value
    return DevMatrix(gexec, "ell", len(rows), n_cols, (k, stride), (cols, vals))


def sellp_matrix(gexec, t, it, rows, n_cols, slice_size, stride_factor, pad_value=None):
    sets, lens, cols, vals = fr.sellp_build(rows, slice_size, stride_factor, t, it)
    if pad_value is not None:
        vals[cols < 0] = pad_value
    return DevMatrix(gexec, "sellp", len(rows), n_cols, (slice_size,), (sets, lens, cols, vals))


def launch(gexec, m, scal, db, dc, nrhs, dalpha=None, dbeta=None, n_rows=None):
    """(entry point, arguments) of the product in the plain (scal is None) or the advanced form"""
    name = f"gkoc_{m.kind}_{'advanced_' if scal is not None else ''}spmv_{TN[m.t]}_{IN[m.it]}"
    head = (gexec.stream, m.n_rows if n_rows is None else n_rows, m.n_cols) + m.head
    if scal is None:
        return name, head + tuple(m.dev) + (db.ptr, db.ld, dc.ptr, dc.ld, nrhs)
    return name, head + (dalpha,) + tuple(m.dev) + (db.ptr, db.ld, dbeta, dc.ptr, dc.ld, nrhs)


def run(gexec, m, layout, scal, b, c0):
    """one product; returns (kernel result, Strided b, Strided c) after the checks every call gets"""
    nrhs, ldb, ldc, boff, coff = layout
    t = m.t
    nan_c = scal is None or scal[1] == 0
    db = Strided(gexec, b, ldb, boff)
    dc = Strided(gexec, np.full((m.n_rows, nrhs), np.nan, t) if nan_c else c0, ldc, coff)
    scalars = [] if scal is None else [np.array([s], t) for s in scal]
    dscal = [Dev(gexec, s) for s in scalars]
    name, args = launch(gexec, m, scal, db, dc, nrhs, *dscal)
    _call(name, *args)
    got = dc.result()
    assert m.unchanged() and db.unchanged(), "an input changed"
    assert all(same_bits(d.get(), h) for d, h in zip(dscal, scalars)), "alpha / beta changed"
    return got, db, dc


def operands(rng, t, m, nrhs):
    return fr.values(rng, (m.n_cols, nrhs), t), fr.values(rng, (m.n_rows, nrhs), t)


def check_real(gexec, oracle, m, layout, want_branch, scal, rng, what):
    nrhs = layout[0]
    b, c0 = operands(rng, m.t, m, nrhs)
    got, db, dc = run(gexec, m, layout, scal, b, c0)
    branch = fr.branch_of(m.n_cols, nrhs, layout[1], layout[2], db.address, dc.address, np.dtype(m.t).itemsize)
    assert branch == want_branch, (what, branch)
    kw = {} if scal is None else dict(alpha=scal[0], beta=scal[1], c=None if scal[1] == 0 else c0)
    _, plain = m.product(b, **kw)
    assert not np.any(np.isnan(got)), what
    assert same_bits(got, plain), (what, float(np.max(np.abs(got - plain))))
    assert np.array_equal(got, m.oracle(oracle, b, scal, c0)), what


# ------------------------------------------------------------------------------------ real types
@pytest.mark.parametrize("it", INDEX)
@pytest.mark.parametrize("t", REAL)
def test_ell_every_branch(gexec, oracle, t, it):
    """every operand layout of fr.LAYOUTS (one-column kernel with and without unit stride, lane = row with 2 /
    4 / 8 columns, fragments of 4 / 8 with partial lanes and chunks, refusal of the fragments for odd strides
    and for a b or c one element off) at every row count, k = 0, 1, 7, 8, 9, 16, 17, 25 (the pipelined row
    loop's chunk edges), stride = n_rows and n_rows + 5, rows of 0 .. k entries, a padding slot in front"""
    rng = np.random.default_rng(100)
    for li, n, n_cols, k, stride, family, si in fr.ell_cases():
        layout, want = fr.LAYOUTS[li]
        m = ell_matrix(gexec, t, it, fr.ell_rows(rng, t, n, n_cols, k, family), n_cols, k, stride)
        check_real(gexec, oracle, m, layout, want, fr.REAL_SCALARS[si], rng, (layout, n, n_cols, k, stride, family, si))


@pytest.mark.parametrize("it", INDEX)
@pytest.mark.parametrize("t", REAL)
def test_sellp_every_branch(gexec, oracle, t, it):
    """the same layouts on SELL-P with slice sizes 64, 32, 2, 1 (several slices of different length inside one
    wave: maxlen > nlen), 100 and 128 (slices that do not divide or exceed the wave), row lengths cycling
    through 0, 1, 7, 8, 9, 15, 16, 17, 25, and whole slices emptied in front, in the middle and at the end.
    A trailing empty slice that shares its wave with a stored one is the shape whose lanes used to load past
    the end of col_idxs / values in the fragment kernel: at least one such case per slice size 1, 2, 32 must
    have run on a fragment layout."""
    rng = np.random.default_rng(200)
    shape_seen = set()
    for li, n, n_cols, si_, family, si in fr.sellp_cases():
        layout, want = fr.LAYOUTS[li]
        ss, sf = fr.SLICES[si_]
        m = sellp_matrix(gexec, t, it, fr.sellp_rows(rng, t, n, n_cols, ss, family), n_cols, ss, sf)
        check_real(gexec, oracle, m, layout, want, fr.REAL_SCALARS[si], rng, (layout, n, n_cols, ss, sf, family, si))
        if want.startswith("frag") and fr.trailing_empty_slice_in_shared_wave(ss, m.host[1]):
            shape_seen.add(ss)
    assert shape_seen >= {1, 2, 32}, shape_seen


# ------------------------------------------------------------------------------------ complex types
def check_complex(gexec, m, layout, scal, rng, what, seen):
    nrhs = layout[0]
    b, c0 = operands(rng, m.t, m, nrhs)
    got, _, _ = run(gexec, m, layout, scal, b, c0)
    kw = {} if scal is None else dict(alpha=scal[0], beta=scal[1], c=None if scal[1] == 0 else c0)
    ref, plain = m.product(b, **kw)
    assert not np.any(np.isnan(got)), what
    ok, ratio = br.rule_r(got, ref, plain, m.t)
    seen["ratio"] = max(seen.get("ratio", 0.0), ratio)
    seen["bit_equal"] = seen.get("bit_equal", True) and same_bits(got, plain)
    assert ok, (what, ratio)


@pytest.fixture
def seen(request):
    s = {}
    yield s
    if s:
        record_perf("format_spmv", test=request.node.name, **s)
        print(f"\n[format_spmv] {request.node.name}: {s}", end="")


@pytest.mark.parametrize("it", INDEX)
@pytest.mark.parametrize("t", COMPLEX)
def test_complex_products(gexec, seen, t, it):
    """the one path of complex_formats.hip: layouts (1,1,1), (3,4,5), (8,8,8), every row count, ELL with every
    k and SELL-P with every slice size, the plain form, (0.5 - 2i, -1 + 0.5i) and beta = 0 over a NaN c"""
    rng = np.random.default_rng(300)
    i = 0
    for layout in fr.COMPLEX_LAYOUTS:
        for n in fr.ROWS:
            n_cols, scal = fr.COLS[i % 3], fr.COMPLEX_SCALARS[i % 3]
            k = fr.ELL_K[i % len(fr.ELL_K)]
            family = ("cycle", "padfront")[(i // 2) % 2]
            m = ell_matrix(gexec, t, it, fr.ell_rows(rng, t, n, n_cols, k, family), n_cols, k, n + 5 * (i % 2))
            check_complex(gexec, m, layout, scal, rng, ("ell", layout, n, n_cols, k, family, scal), seen)
            ss, sf = fr.SLICES[i % len(fr.SLICES)]
            family = ("cycle", "empties")[(i // 3) % 2]
            m = sellp_matrix(gexec, t, it, fr.sellp_rows(rng, t, n, n_cols, ss, family), n_cols, ss, sf)
            check_complex(gexec, m, layout, fr.COMPLEX_SCALARS[(i + 1) % 3], rng, ("sellp", layout, n, n_cols, ss, sf, family),
                          seen)
            i += 1


def test_complex_beyond_the_grid_cap(gexec, seen):
    """2 * grid_cap_rows() + 257 rows x 2 columns, one stored entry per row, c64 / i32: the complex launchers
    start at most 8 * max_stream_blocks blocks, so the last rows are reached only by the grid-stride loop;
    ELL (k = 1) and SELL-P (slice size 64: every slice has length 1, which makes the two layouts the same
    arrays).  Every row is compared: a row is one textbook product, each part two rounded products and one
    rounded sum, so its error is below 3 sqrt(2) (eps / 2) |v| |b| < 2.2 eps |ref|; the per-row bound is rule
    R's 8 eps |ref|."""
    t, it = np.complex64, np.int32
    n = 2 * grid_cap_rows() + 257
    rng = np.random.default_rng(400)
    cols, vals = rng.integers(0, 2, n).astype(it), fr.values(rng, n, t)
    b = fr.values(rng, (2, 1), t)
    ns = (n + 63) // 64
    sets, lens = np.arange(ns + 1, dtype=np.uint64), np.ones(ns, np.uint64)
    pad = ns * 64 - n
    scols, svals = np.concatenate((cols, np.full(pad, -1, it))), np.concatenate((vals, np.zeros(pad, t)))
    for m in (DevMatrix(gexec, "ell", n, 2, (1, n), (cols, vals)),
              DevMatrix(gexec, "sellp", n, 2, (64,), (sets, lens, scols, svals))):
        got, _, _ = run(gexec, m, (1, 1, 1, 0, 0), None, b, None)
        ref, plain = m.product(b)
        ok, ratio = br.rule_r(got, ref, plain, t)
        seen["ratio"] = max(seen.get("ratio", 0.0), ratio)
        seen["bit_equal"] = seen.get("bit_equal", True) and same_bits(got, plain)
        assert ok and not np.any(np.isnan(got)), (m.kind, ratio)
        wrong = np.flatnonzero(np.abs(got - ref)[:, 0] > 8 * br.eps_of(t) * np.abs(ref)[:, 0])
        assert wrong.size == 0, (m.kind, wrong[:5])


# ------------------------------------------------------------------------------------ padding
def _leak_rows(rng, t, n_rows, n_cols, k):
    """no real entry in column 0; one padding slot at a changing place of every row"""
    rows = []
    for r in range(n_rows):
        slots = fr.entries(rng, t, n_cols, r % k, low=1)
        slots.insert(r % (len(slots) + 1), (fr.PAD, np.dtype(t).type(np.nan)))
        rows.append(slots)
    return rows


@pytest.mark.parametrize("t", REAL + COMPLEX)
def test_padding_values_and_row_zero_of_b_do_not_reach_c(gexec, oracle, t):
    """NaN in the value of every padding slot and in row 0 of b, which no real entry refers to: a slot counts
    by its column alone, so every kernel returns the reference's bits (rule R for the complex ones) and no NaN.
    One-column kernel with and without unit stride, lane = row with 2, 4 and 8 columns, fragments of 4 and 8 -
    whose padding slots do gather row 0 of b - and the complex kernels"""
    rng = np.random.default_rng(500)
    it, n, n_cols, k = np.int32, 129, 37, 10
    rows = _leak_rows(rng, t, n, n_cols, k)
    nan = np.dtype(t).type(np.nan)
    mats = (ell_matrix(gexec, t, it, rows, n_cols, k, n + 5, pad_value=nan),
            sellp_matrix(gexec, t, it, rows, n_cols, 32, 2, pad_value=nan),
            sellp_matrix(gexec, t, it, rows, n_cols, 2, 2, pad_value=nan))
    if br.is_complex(t):
        layouts = [(lay, None) for lay in fr.COMPLEX_LAYOUTS]
        scalars = fr.COMPLEX_SCALARS[:2]
    else:
        want = ("one unit", "one strided", "row 2", "frag 4", "row 4", "frag 8", "row 8")
        layouts = [next((lay, w) for lay, w in fr.LAYOUTS if w == name) for name in want]
        scalars = fr.REAL_SCALARS[:2]
    for m in mats:
        assert np.all(np.isnan(m.host[-1][m.host[-2] < 0])) and not np.any(m.host[-2] == 0)
        for layout, want in layouts:
            for scal in scalars:
                b, c0 = operands(rng, t, m, layout[0])
                b[0] = nan
                got, db, dc = run(gexec, m, layout, scal, b, c0)
                kw = {} if scal is None else dict(alpha=scal[0], beta=scal[1], c=c0)
                ref, plain = m.product(b, **kw)
                assert not np.any(np.isnan(got)) and not np.any(np.isnan(plain)), (m.kind, layout, scal)
                if br.is_complex(t):
                    assert br.rule_r(got, ref, plain, t)[0], (m.kind, layout, scal)
                else:
                    assert fr.branch_of(n_cols, layout[0], layout[1], layout[2], db.address, dc.address,
                                        np.dtype(t).itemsize) == want
                    assert same_bits(got, plain), (m.kind, layout, scal)


# ------------------------------------------------------------------------------------ wave order
@functools.lru_cache(maxsize=None)
def _wave_rows(t):
    rng = np.random.default_rng(600)
    return fr.sellp_rows(rng, t, 4871, 300, 64, "cycle")


@pytest.mark.parametrize("t", REAL)
def test_multi_column_wave_order_key(gexec, t):
    """GKOC_TUNE_MULTI_XCD_CHUNK_ROWS = 0, 512 and 1024 on 4871 rows = 19 full blocks and a tail: with 512 the
    first 16 blocks are permuted and the rest keep their order (1024 needs 32 blocks and permutes none; 256
    would be the identity).  Lane = row with two columns, fragments of four and of eight; ELL, SELL-P 64 and
    32.  Whatever the order of the blocks, the bits are the reference's"""
    rng = np.random.default_rng(601)
    rows, n_cols, it = _wave_rows(t), 300, np.int32
    mats = (ell_matrix(gexec, t, it, rows, n_cols, 25, 4871 + 5), sellp_matrix(gexec, t, it, rows, n_cols, 64, 1),
            sellp_matrix(gexec, t, it, rows, n_cols, 32, 2))
    for m in mats:
        for nrhs in (2, 4, 8):
            layout = (nrhs, nrhs, nrhs, 0, 0)
            b, c0 = operands(rng, t, m, nrhs)
            _, plain = m.product(b, alpha=0.7, beta=-1.3, c=c0)
            default, db, dc = run(gexec, m, layout, (0.7, -1.3), b, c0)
            assert fr.branch_of(n_cols, nrhs, nrhs, nrhs, db.address, dc.address, np.dtype(t).itemsize) == \
                {2: "row 2", 4: "frag 4", 8: "frag 8"}[nrhs]
            assert same_bits(default, plain), (m.kind, m.head, nrhs)
            for value in (0, 512, 1024):
                with tuned((KEY_MULTI_CHUNK, value)):
                    got, _, _ = run(gexec, m, layout, (0.7, -1.3), b, c0)
                assert same_bits(got, default), (m.kind, m.head, nrhs, value)


# ------------------------------------------------------------------------------------ refused and empty calls
@pytest.mark.parametrize("t", REAL + COMPLEX)
def test_refused_calls_leave_c_alone(gexec, t):
    """what the launchers refuse before any launch: an ELL stride below n_rows, a negative k, slice size 0,
    the advanced forms without alpha or without beta"""
    rng = np.random.default_rng(700)
    it, n, n_cols, nrhs = np.int32, 65, 37, 4
    rows = fr.ell_rows(rng, t, n, n_cols, 7, "cycle")
    ell, sellp = ell_matrix(gexec, t, it, rows, n_cols, 7, n), sellp_matrix(gexec, t, it, rows, n_cols, 64, 1)
    b, c0 = operands(rng, t, ell, nrhs)
    one = Dev(gexec, np.ones(1, t))

    def refused(m, scal, dalpha=None, dbeta=None, **change):
        db, dc = Strided(gexec, b, nrhs), Strided(gexec, c0, nrhs + 2)
        name, args = launch(gexec, m, scal, db, dc, nrhs, dalpha, dbeta)
        args = list(args)
        for pos, v in change.items():
            args[int(pos[1:])] = v
        assert raises_invalid(name, *args), (name, change)
        assert same_bits(dc.result(), c0) and m.unchanged()

    refused(ell, None, a4=n - 1)            # stride
    refused(ell, None, a3=-1)               # k
    refused(sellp, None, a3=0)              # slice size
    refused(ell, (1, 1), one, one, a4=n - 1)
    refused(ell, (1, 1), one, one, a3=-1)
    refused(sellp, (1, 1), one, one, a3=0)
    for m in (ell, sellp):
        refused(m, (1, 1), None, one)
        refused(m, (1, 1), one, None)


@pytest.mark.parametrize("t", REAL + COMPLEX)
def test_empty_calls(gexec, t):
    """n_rows = 0 and nrhs = 0 return OK and write nothing; a matrix without columns (n_cols = 0, every slot
    padding, a b without rows) gives +0 or beta * c on layouts that would otherwise select the fragments -
    the launchers keep such a call on the lane = row kernel, which loads nothing for a padding slot"""
    rng = np.random.default_rng(800)
    it, n, n_cols = np.int32, 65, 37
    rows = fr.ell_rows(rng, t, n, n_cols, 7, "cycle")
    scal = fr.COMPLEX_SCALARS[1] if br.is_complex(t) else fr.REAL_SCALARS[1]
    for m in (ell_matrix(gexec, t, it, rows, n_cols, 7, n), sellp_matrix(gexec, t, it, rows, n_cols, 64, 1)):
        for sc in (None, scal):
            dscal = [] if sc is None else [Dev(gexec, np.array([s], t)) for s in sc]
            for n_rows, nrhs in ((0, 4), (n, 0)):
                b, c0 = operands(rng, t, m, 4)
                db, dc = Strided(gexec, b, 4), Strided(gexec, c0, 6)
                name, args = launch(gexec, m, sc, db, dc, nrhs, *dscal, n_rows=n_rows)
                _call(name, *args)
                assert same_bits(dc.result(), c0) and m.unchanged()
    # no columns
    empty_rows = [[(fr.PAD, np.dtype(t).type(1.5))] * (r % 4) for r in range(n)]
    for m in (ell_matrix(gexec, t, it, empty_rows, 0, 3, n), sellp_matrix(gexec, t, it, empty_rows, 0, 32, 1)):
        for layout in ((1, 1, 1, 0, 0), (4, 4, 4, 0, 0), (8, 8, 8, 0, 0)):
            b, c0 = operands(rng, t, m, layout[0])
            assert b.shape[0] == 0
            for sc in (None, scal):
                got, db, dc = run(gexec, m, layout, sc, b, c0)
                if not br.is_complex(t) and layout[0] > 1:
                    assert fr.branch_of(0, layout[0], layout[1], layout[2], db.address, dc.address,
                                        np.dtype(t).itemsize).startswith("row")
                _, plain = m.product(b, **({} if sc is None else dict(alpha=sc[0], beta=sc[1], c=c0)))
                assert same_bits(got, plain), (m.kind, layout, sc)
                if sc is None:
                    assert same_bits(got, np.zeros_like(got))
