"""The entry points that build ELL and SELL-P matrices on the device, called directly: gkoc_compute_max_row_nnz_*,
gkoc_sellp_compute_slice_sets_*, gkoc_convert_ptrs_to_sizes_*, gkoc_convert_idxs_to_ptrs_* with its two
mixed-width forms, gkoc_fill_seq_array_*, gkoc_aos_to_soa_* and gkoc_csr_convert_to_ell_* /
gkoc_csr_convert_to_sellp_* in all four value types.  Everything here is exact: indices are compared as
numbers, values bit for bit (random bit patterns with NaN payloads and -0.0 - the kernels only move them).
Outputs are followed by canaries, inputs are read back, and what an operation does not define must keep its
fill: rows n_rows .. stride of ELL, and the rows a partial last SELL-P slice has room for beyond n_rows.
The restatements are those of tests/format_spmv_refs.py."""
import ctypes as C

import numpy as np
import pytest

import format_spmv_refs as fr
from binding_gpu import Dev, grid_cap_rows, same_bits
from binding_gpu import call as _call

pytestmark = pytest.mark.gpu

TN = {np.float64: "f64", np.float32: "f32", np.complex128: "c128", np.complex64: "c64"}
IN = {np.int32: "i32", np.int64: "i64"}
VALUE = (np.float64, np.float32, np.complex128, np.complex64)
INDEX = (np.int32, np.int64)
FILL, TAIL = 77, 123456789


def stream_rows():
    """256 * max_stream_blocks: what the capped set-up launchers cover with one pass of their grid"""
    return grid_cap_rows() // 4


class Out:
    """n entries FILL followed by three TAIL entries, any integer dtype"""

    def __init__(self, gexec, n, dtype):
        self.n = n
        a = np.full(n + 3, FILL, dtype)
        a[n:] = TAIL
        self.dev = Dev(gexec, a)
        self._as_parameter_ = self.dev._as_parameter_

    def get(self, defined=None):
        """the first `defined` entries (all n by default); the others must hold FILL, the tail TAIL"""
        got = self.dev.get()
        k = self.n if defined is None else defined
        assert np.all(got[self.n:] == TAIL), "written behind the output"
        assert np.all(got[k:self.n] == FILL), "written beyond what the operation defines"
        return got[:k]


def bit_patterns(rng, n, t):
    """n values of type t with random bits; some -0.0, some NaNs with a payload"""
    t = np.dtype(t)
    words = rng.integers(0, 2 ** 64, n * t.itemsize // 8 + 1, dtype=np.uint64)
    v = words.view(np.uint8)[:n * t.itemsize].view(t).copy()
    if n > 3:
        parts = v.view(np.float32 if t in (np.float32, np.complex64) else np.float64)
        parts[1] = -0.0
        parts[2] = np.nan
        parts[2:3].view(np.uint32 if parts.dtype == np.float32 else np.uint64)[0] |= 0x1234
    return v


# ------------------------------------------------------------------------------------ row statistics
@pytest.mark.parametrize("it", INDEX)
def test_compute_max_row_nnz(gexec, it):
    """rows 0 (answer 0), 1, 255, 256, 257; 256 * max_stream_blocks + 257 rows - more than the capped grid
    covers in one pass - with the maximum in the last row, then in row 0; all rows empty"""
    rng = np.random.default_rng(1)
    big = stream_rows() + 257
    cases = [np.zeros(0, int)] + [rng.integers(0, 9, n) for n in (1, 255, 256, 257)] + [np.zeros(300, int)]
    for where in (big - 1, 0):
        lengths = rng.integers(0, 9, big)
        lengths[where] = 11
        cases.append(lengths)
    for lengths in cases:
        ptrs = np.concatenate(([0], np.cumsum(lengths))).astype(it)
        dp = Dev(gexec, ptrs)
        res = C.c_int64(-5)
        _call("gkoc_compute_max_row_nnz_" + IN[it], gexec.stream, len(lengths), dp, C.byref(res))
        want = int(lengths.max()) if len(lengths) else 0
        assert res.value == want, len(lengths)
        if len(lengths) < 1000:
            assert fr.compute_max_row_nnz(ptrs) == want
        assert same_bits(dp.get(), ptrs)


@pytest.mark.parametrize("it", INDEX)
def test_sellp_compute_slice_sets(gexec, it):
    """the six (slice size, stride factor) pairs of the products and (200, 1) - a wave striding over a slice
    wider than 64 rows -; rows 0 (slice_sets[0] = 0 and nothing else), 1, 63, 64, 65, 1000, so that last slices
    are partial; lengths that are multiples of the stride factor and lengths one above"""
    rng = np.random.default_rng(2)
    for ss, sf in fr.SLICES + ((200, 1),):
        for n in (0, 1, 63, 64, 65, 1000):
            for family in ("multiples", "one above", "random"):
                lengths = rng.integers(0, 6, n) * sf + (family == "one above") if family != "random" \
                    else rng.integers(0, 20, n)
                ptrs = np.concatenate(([0], np.cumsum(lengths))).astype(it)
                ns = (n + ss - 1) // ss
                dp, sets, lens = Dev(gexec, ptrs), Out(gexec, ns + 1, np.uint64), Out(gexec, ns, np.uint64)
                _call("gkoc_sellp_compute_slice_sets_" + IN[it], gexec.stream, n, ss, sf, dp, sets, lens)
                want_sets, want_lens = fr.sellp_compute_slice_sets(ptrs, ss, sf)
                assert np.array_equal(sets.get(), want_sets) and np.array_equal(lens.get(), want_lens), (ss, sf, n)
                assert same_bits(dp.get(), ptrs)
                if family == "multiples" and n:
                    assert np.array_equal(want_lens, [lengths[s * ss:(s + 1) * ss].max() for s in range(ns)])
                if n == 0:
                    assert want_sets.tolist() == [0]


SIZES = (0, 1, 255, 256, 257, 100003)


@pytest.mark.parametrize("it", INDEX)
def test_convert_ptrs_to_sizes_and_fill_seq_array(gexec, it):
    rng = np.random.default_rng(3)
    for n in SIZES:
        ptrs = np.concatenate(([0], np.cumsum(rng.integers(0, 9, n)))).astype(it)
        dp, sizes = Dev(gexec, ptrs), Out(gexec, n, np.uint64)
        _call("gkoc_convert_ptrs_to_sizes_" + IN[it], gexec.stream, n, dp, sizes)
        assert np.array_equal(sizes.get(), fr.convert_ptrs_to_sizes(ptrs)) and same_bits(dp.get(), ptrs)
        seq = Out(gexec, n, it)
        _call("gkoc_fill_seq_array_" + IN[it], gexec.stream, seq, n)
        assert np.array_equal(seq.get(), np.arange(n))
    # more entries than one pass of the capped grid of fill_seq_array covers
    n = stream_rows() + 257
    seq = Out(gexec, n, it)
    _call("gkoc_fill_seq_array_" + IN[it], gexec.stream, seq, n)
    assert np.array_equal(seq.get(), np.arange(n))


def _index_lists(rng, n):
    """sorted row indices of n rows: runs of equal indices, gaps of 1, 8, 9, 1000 and n - 1 empty rows,
    nothing stored, and entries in the last row only"""
    yield "nothing stored", np.zeros(0, np.int64)
    if n == 0:
        return
    yield "last row only", np.full(5, n - 1)
    yield "first and last row", np.array([0, 0, 0, n - 1])[:4 if n > 1 else 3]
    yield "runs", np.sort(rng.integers(0, n, 3 * min(n, 2000)))
    rows, r = [], 0
    for gap in (1, 8, 9, 1000, 1, 9, 8):
        rows += [r] * 3
        r += gap + 1
    yield "gaps", np.array([v for v in rows if v < n])


@pytest.mark.parametrize("it,pt,name", [(np.int32, np.int32, "i32"), (np.int64, np.int64, "i64"),
                                        (np.int32, np.int64, "i32_i64"), (np.int64, np.int32, "i64_i32")])
def test_convert_idxs_to_ptrs(gexec, it, pt, name):
    rng = np.random.default_rng(4)
    for n in SIZES:
        for what, idxs in _index_lists(rng, n):
            idxs = idxs.astype(it)
            di, ptrs = Dev(gexec, idxs), Out(gexec, n + 1, pt)
            _call("gkoc_convert_idxs_to_ptrs_" + name, gexec.stream, len(idxs), di, n, ptrs)
            want = fr.convert_idxs_to_ptrs(idxs, n, pt)
            assert np.array_equal(ptrs.get(), want), (n, what)
            assert same_bits(di.get(), idxs)
            if what == "nothing stored":
                assert not want.any()


# ------------------------------------------------------------------------------------ triplets
ENTRY_BYTES = {(np.float64, np.int32): 16, (np.float64, np.int64): 24, (np.float32, np.int32): 12,
               (np.float32, np.int64): 24, (np.complex128, np.int32): 24, (np.complex128, np.int64): 32,
               (np.complex64, np.int32): 16, (np.complex64, np.int64): 24}


@pytest.mark.parametrize("it", INDEX)
@pytest.mark.parametrize("t", VALUE)
def test_aos_to_soa(gexec, t, it):
    """the C layout of { I row; I column; T value; } as a numpy structured dtype with C alignment (float with
    64-bit indices ends in four bytes of padding); 0, 1, 257 and 256 * max_stream_blocks + 257 entries"""
    rng = np.random.default_rng(5)
    entry = np.dtype({"names": ["row", "column", "value"], "formats": [it, it, t]}, align=True)
    assert entry.itemsize == ENTRY_BYTES[(t, it)]
    for n in (0, 1, 257, stream_rows() + 257):
        e = np.zeros(n, entry)
        e.view(np.uint8)[:] = 0xa5                                    # the padding bytes too
        e["row"], e["column"] = rng.integers(0, 2 ** 31 - 1, n), rng.integers(0, 2 ** 31 - 1, n)
        e["value"] = bit_patterns(rng, n, t)
        de = Dev(gexec, e.view(np.uint8))
        rows, cols = Out(gexec, n, it), Out(gexec, n, it)
        vals = Dev(gexec, np.concatenate((np.zeros(n, t), np.full(3, 5.5, t))))
        _call(f"gkoc_aos_to_soa_{TN[t]}_{IN[it]}", gexec.stream, n, de, rows, cols, vals)
        assert np.array_equal(rows.get(), e["row"]) and np.array_equal(cols.get(), e["column"])
        got = vals.get()
        assert same_bits(got[:n], np.ascontiguousarray(e["value"])) and np.all(got[n:] == t(5.5))
        assert same_bits(de.get(), e.view(np.uint8))


# ------------------------------------------------------------------------------------ conversions
def _conversion_cases(rng):
    """(name, row lengths): rows 1, 63, 64, 65, 200 with empty rows in front, inside and at the end, and 200
    rows whose second 64-row group holds exactly 2048 entries (staged through LDS) and whose third holds 2049
    (the direct loop)"""
    for n in (1, 63, 64, 65, 200):
        lengths = rng.integers(0, 12, n)
        lengths[[0, n // 2, n - 1]] = 0
        yield f"rows {n}", lengths
    lengths = rng.integers(0, 12, 200)
    lengths[64:192] = 32
    lengths[150] = 33
    lengths[199] = 0
    yield "stage cap", lengths


def _value_buffers(gexec, t, it, n, fill_value=-3.25):
    fc, fv = np.full(n + 3, -7, it), np.full(n + 3, fill_value, t)
    return fc, fv, Dev(gexec, fc), Dev(gexec, fv)


@pytest.mark.parametrize("it", INDEX)
@pytest.mark.parametrize("t", VALUE)
def test_csr_convert_to_ell(gexec, t, it):
    """k = the longest row with stride = n_rows, and k + 2 with stride = n_rows + 5, whose rows n_rows .. stride
    keep their fill; padding is (-1, +0)"""
    rng = np.random.default_rng(6)
    for name, lengths in _conversion_cases(rng):
        n = len(lengths)
        ptrs, cols, vals = fr.random_csr(rng, t, it, lengths, 500)
        vals = bit_patterns(rng, len(vals), t)
        if name == "stage cap":
            assert ptrs[128] - ptrs[64] == 2048 and ptrs[192] - ptrs[128] == 2049
        dev = [Dev(gexec, a) for a in (ptrs, cols, vals)]
        for k, stride in ((int(lengths.max()), n), (int(lengths.max()) + 2, n + 5)):
            fc, fv, dc, dv = _value_buffers(gexec, t, it, k * stride)
            _call(f"gkoc_csr_convert_to_ell_{TN[t]}_{IN[it]}", gexec.stream, n, *dev, k, stride, dc, dv)
            wc, wv = fr.csr_convert_to_ell(ptrs, cols, vals, k, stride, fc, fv)
            assert np.array_equal(dc.get(), wc) and same_bits(dv.get(), wv), (name, k, stride)
            if stride > n and k:
                assert np.all(wc[:k * stride].reshape(k, stride)[:, n:] == -7)
            assert all(same_bits(d.get(), h) for d, h in zip(dev, (ptrs, cols, vals)))


@pytest.mark.parametrize("it", INDEX)
@pytest.mark.parametrize("t", VALUE)
def test_csr_convert_to_sellp(gexec, t, it):
    """slice size 64 (the staged kernel), 32, 2 and 100 (lane walks its row) on the slice sets of the
    restatement; the rows a partial last slice has room for beyond n_rows keep their fill, as in the reference"""
    rng = np.random.default_rng(7)
    for name, lengths in _conversion_cases(rng):
        n = len(lengths)
        ptrs, cols, vals = fr.random_csr(rng, t, it, lengths, 500)
        vals = bit_patterns(rng, len(vals), t)
        dev = [Dev(gexec, a) for a in (ptrs, cols, vals)]
        for ss, sf in ((64, 1), (32, 2), (2, 2), (100, 3)):
            sets, _ = fr.sellp_compute_slice_sets(ptrs, ss, sf)
            total = int(sets[-1]) * ss
            fc, fv, dc, dv = _value_buffers(gexec, t, it, total)
            ds = Dev(gexec, sets)
            _call(f"gkoc_csr_convert_to_sellp_{TN[t]}_{IN[it]}", gexec.stream, n, ss, *dev, ds, dc, dv)
            wc, wv = fr.csr_convert_to_sellp(ptrs, cols, vals, ss, sets, fc, fv)
            assert np.array_equal(dc.get(), wc) and same_bits(dv.get(), wv), (name, ss, sf)
            assert all(same_bits(d.get(), h) for d, h in zip(dev + [ds], (ptrs, cols, vals, sets)))
            if n % ss and int(sets[-1]) > int(sets[-2]):
                assert np.any(wc[:total] == -7), "a partial last slice keeps the fill of the rows it does not have"
