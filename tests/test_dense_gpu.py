"""Dense kernels that only the C++ binding calls, through the C ABI against numpy: dense::simple_apply /
apply (csrc/dense_gemm.hip), the precision conversions, compute_norm1 / compute_mean and their complex
forms, components::reduce_add_array and components::prefix_sum_nonnegative (csrc/scan.hpp).

The product's contract is the reference's left-to-right sum with multiply and add rounded separately
(binding_refs.gemm in the value type): bit equality, for the complex types with the textbook product.  The
tree reductions are exact on small integers and within the header's 450 eps sum|terms| on random input."""
import ctypes as C

import numpy as np
import pytest

import binding_refs as br
from binding_gpu import CANARY, Dev, padded, same_bits, sync

pytestmark = pytest.mark.gpu

TN = ["f64", "f32", "c128", "c64"]
GEMM_SHAPES = [(1, 1, 1), (16, 16, 16), (17, 15, 33), (5, 1, 1000), (1, 7, 0), (100, 3, 50), (33, 65, 17)]


def _rand(rng, shape, t):
    v = rng.uniform(-1, 1, shape)
    return (v + 1j * rng.uniform(-1, 1, shape)).astype(t) if br.is_complex(t) else v.astype(t)


def _call(name, *args):
    from ginkgo_amd._lib import call
    call(name, *args)


def _pad_ok(full, cols):
    return np.all(full[:, cols:] == full.dtype.type(CANARY))


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_simple_apply(gexec, tn, m, n, k):
    t = br.TYPES[tn]
    rng = np.random.default_rng(m * 1000 + n * 10 + k)
    a, b = _rand(rng, (m, k), t), _rand(rng, (k, n), t)
    c0 = np.full((m, n), np.nan, t)                                # overwritten, never read
    for pad in (0, 3):
        fa, fb, fc = padded(a, k + pad), padded(b, n + pad), padded(c0, n + pad)
        da, db, dc = Dev(gexec, fa), Dev(gexec, fb), Dev(gexec, fc)
        _call("gkoc_dense_simple_apply_" + tn, gexec.stream, m, n, k, da, k + pad, db, n + pad, dc, n + pad)
        sync()
        got = dc.get()
        assert _pad_ok(got, n) and same_bits(da.get(), fa) and same_bits(db.get(), fb)
        want = br.gemm(br.plain(t), a, b)
        assert np.array_equal(got[:, :n], want), np.max(np.abs(got[:, :n] - want))
        ok, _ = br.rule_r(got[:, :n], br.gemm(br.hp(t), a, b), want, t)
        assert ok


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
@pytest.mark.parametrize("alpha,beta", [(1, 0), (-0.5, 2), (0.75, 0)])
def test_apply(gexec, tn, m, n, k, alpha, beta):
    """c = alpha a b + beta c; beta = 0 does not read c (NaN in, no NaN out); k = 0 gives beta c"""
    t = br.TYPES[tn]
    rng = np.random.default_rng(m * 1000 + n * 10 + k + 1)
    a, b, c = _rand(rng, (m, k), t), _rand(rng, (k, n), t), _rand(rng, (m, n), t)
    if br.is_complex(t):
        alpha, beta = alpha * (1 - 0.5j), beta * (0.5 + 1j)
    if beta == 0:
        c[:] = np.nan
    pad = 3
    fa, fb, fc = padded(a, k + pad), padded(b, n + pad), padded(c, n + pad)
    da, db, dc = Dev(gexec, fa), Dev(gexec, fb), Dev(gexec, fc)
    dal, dbe = Dev(gexec, np.array([alpha], t)), Dev(gexec, np.array([beta], t))
    _call("gkoc_dense_apply_" + tn, gexec.stream, m, n, k, dal, da, k + pad, db, n + pad, dbe, dc, n + pad)
    sync()
    got = dc.get()
    assert _pad_ok(got, n)
    want = br.gemm(br.plain(t), a, b, c, alpha, beta)
    assert np.all(np.isfinite(got[:, :n]))
    assert np.array_equal(got[:, :n], want), np.max(np.abs(got[:, :n] - want))
    if k == 0:
        assert np.array_equal(got[:, :n], np.zeros((m, n), t) if beta == 0 else want)
    if beta != 0:
        ok, _ = br.rule_r(got[:, :n], br.gemm(br.hp(t), a, b, c, alpha, beta), want, t)
        assert ok


@pytest.mark.parametrize("tn", TN)
def test_gemm_argument_checks_return_before_a_launch(gexec, tn):
    from ginkgo_amd._lib import GkoError, NotSupported
    t = br.TYPES[tn]
    buf = np.full((4, 8), CANARY, t)
    da, db, dc = Dev(gexec, buf), Dev(gexec, buf), Dev(gexec, buf)
    one = Dev(gexec, np.ones(1, t))
    with pytest.raises(GkoError):                                       # lda < k
        _call("gkoc_dense_simple_apply_" + tn, gexec.stream, 4, 4, 6, da, 5, db, 8, dc, 8)
    with pytest.raises(GkoError):                                       # ldc < n
        _call("gkoc_dense_apply_" + tn, gexec.stream, 4, 4, 4, one, da, 8, db, 8, one, dc, 3)
    with pytest.raises(GkoError):
        _call("gkoc_dense_simple_apply_" + tn, gexec.stream, -1, 4, 4, da, 8, db, 8, dc, 8)
    with pytest.raises(NotSupported):                                   # more than 65535 row tiles
        _call("gkoc_dense_simple_apply_" + tn, gexec.stream, 65536 * 16, 1, 1, da, 1, db, 1, dc, 1)
    sync()
    assert same_bits(dc.get(), buf) and same_bits(da.get(), buf)
    _call("gkoc_dense_simple_apply_" + tn, gexec.stream, 0, 4, 4, da, 8, db, 8, dc, 8)      # empty: fine
    sync()
    assert same_bits(dc.get(), buf)


@pytest.mark.parametrize("rows,cols", [(1, 1), (257, 3), (1000, 7), (0, 3)])
def test_convert_precision(gexec, rows, cols):
    rng = np.random.default_rng(rows)
    x64 = rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(-40, 40, (rows, cols))   # some overflow f32
    if rows:
        x64[0, 0] = np.float64(np.float32(1.0)) + 2.0 ** -24        # a tie: rounds to even
    fx = padded(x64, cols + 2)
    fy = np.full((rows, cols + 5), CANARY, np.float32)
    dx, dy = Dev(gexec, fx), Dev(gexec, fy)
    _call("gkoc_dense_convert_f64_f32", gexec.stream, rows, cols, dx, cols + 2, dy, cols + 5)
    sync()
    got = dy.get()
    with np.errstate(over="ignore"):
        assert same_bits(got[:, :cols], x64.astype(np.float32)) and _pad_ok(got, cols)
    x32 = rng.standard_normal((rows, cols)).astype(np.float32)
    dx, dy = Dev(gexec, padded(x32, cols + 1)), Dev(gexec, np.full((rows, cols + 4), CANARY, np.float64))
    _call("gkoc_dense_convert_f32_f64", gexec.stream, rows, cols, dx, cols + 1, dy, cols + 4)
    sync()
    got = dy.get()
    assert same_bits(got[:, :cols], x32.astype(np.float64)) and _pad_ok(got, cols)


@pytest.mark.parametrize("tn", ["c128", "c64"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (257, 3), (70, 33)])
def test_complex_convert_modes(gexec, tn, rows, cols):
    """gkoc_cdense_convert: make_complex, get_real, get_imag, conj_transpose - copies, bit for bit"""
    t = br.TYPES[tn]
    rt = br.real_of(t)
    rng = np.random.default_rng(rows)
    z, x = _rand(rng, (rows, cols), t), _rand(rng, (rows, cols), rt)
    for mode, src, want in ((0, x, x.astype(t)), (1, z, z.real.astype(rt)), (2, z, z.imag.astype(rt)),
                            (3, z, np.conj(z.T))):
        din = Dev(gexec, padded(src, cols + 2))
        dout = Dev(gexec, np.full((want.shape[0], want.shape[1] + 3), CANARY, want.dtype))
        _call("gkoc_cdense_convert_" + tn, gexec.stream, rows, cols, din, cols + 2, dout, want.shape[1] + 3, mode)
        sync()
        got = dout.get()
        assert same_bits(got[:, :want.shape[1]], np.ascontiguousarray(want)), mode
        assert _pad_ok(got, want.shape[1])


RED_ROWS = [1, 63, 64, 65, 1025, 100003]


def _norm1_mean(gexec, tn, x, ld):
    """(norm1, mean[, sum]) per column of x through the entry points of the value type"""
    from ginkgo_amd._lib import lib
    t = br.TYPES[tn]
    rows, cols = x.shape
    dx = Dev(gexec, padded(x, ld))
    rt = br.real_of(t)
    dn, dm = Dev(gexec, np.full(cols + 1, CANARY, rt)), Dev(gexec, np.full(cols + 1, CANARY, t))
    if br.is_complex(t):
        ds = Dev(gexec, np.full(cols + 1, CANARY, t))
        _call("gkoc_cdense_compute_norm1_" + tn, gexec.stream, rows, cols, dx, ld, dn)
        _call("gkoc_cdense_compute_mean_" + tn, gexec.stream, rows, cols, dx, ld, dm)
        _call("gkoc_cdense_compute_sum_" + tn, gexec.stream, rows, cols, dx, ld, ds)
    else:
        nbytes = lib().gkoc_reduction_workspace_bytes(C.c_int64(rows), C.c_int64(cols), C.c_size_t(x.itemsize))
        work = Dev(gexec, np.zeros(nbytes + 64, np.uint8))
        _call("gkoc_dense_compute_norm1_" + tn, gexec.stream, rows, cols, dx, ld, dn, work, C.c_size_t(nbytes))
        _call("gkoc_dense_compute_mean_" + tn, gexec.stream, rows, cols, dx, ld, dm)
    sync()
    n1, mean = dn.get(), dm.get()
    assert n1[cols] == rt(CANARY) and mean[cols] == t(CANARY)
    out = [n1[:cols], mean[:cols]]
    if br.is_complex(t):
        s = ds.get()
        assert s[cols] == t(CANARY)
        out.append(s[:cols])
    return out


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("rows", RED_ROWS)
@pytest.mark.parametrize("cols", [1, 3])
def test_norm1_mean_exact_on_small_integers(gexec, tn, rows, cols):
    """integer entries (complex: each on one axis, so |z| is an integer too) with column sums below 2^24:
    norm1 and the sum are the same in every summation order, the mean is that sum divided once by rows"""
    t = br.TYPES[tn]
    rt = br.real_of(t)
    rng = np.random.default_rng(rows + cols)
    re = rng.integers(-4, 5, (rows, cols)).astype(np.float64)
    x = re.astype(t)
    if br.is_complex(t):
        x = np.where(rng.integers(0, 2, (rows, cols)).astype(bool), 1j * re, re).astype(t)
    wide = x.astype(np.clongdouble if br.is_complex(t) else np.longdouble)
    total = np.sum(wide, axis=0)
    for ld in (cols, cols + 3):
        got = _norm1_mean(gexec, tn, x, ld)
        assert np.array_equal(got[0].astype(np.longdouble), np.sum(np.abs(wide), axis=0))
        if br.is_complex(t):
            assert np.array_equal(got[2].astype(wide.dtype), total)
            assert np.array_equal(got[1].real, total.real.astype(rt) / rt(rows))
            assert np.array_equal(got[1].imag, total.imag.astype(rt) / rt(rows))
        else:
            assert np.array_equal(got[1], total.astype(rt) / rt(rows))


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("rows,cols", [(0, 3), (2048, 1), (2049, 3), (524289, 1), (5, 0), (0, 0)])
def test_norm1_mean_launcher_edges(gexec, tn, rows, cols):
    """the two-stage column reductions at the edges of their launcher: no rows (zeros, and a mean of zero,
    not 0 / 0), no columns (nothing written), one block per column and its first split (2048 | 2049 rows),
    and one row past the cap of 256 blocks of 2048 rows.  The data of
    test_norm1_mean_exact_on_small_integers: |entries| <= 4, so column sums stay below 524289 * 4 < 2^24
    and are exact in every summation order"""
    t = br.TYPES[tn]
    rt = br.real_of(t)
    rng = np.random.default_rng(rows + cols)
    re = rng.integers(-4, 5, (rows, cols)).astype(np.float64)
    x = re.astype(t)
    if br.is_complex(t):
        x = np.where(rng.integers(0, 2, (rows, cols)).astype(bool), 1j * re, re).astype(t)
    wide = x.astype(np.clongdouble if br.is_complex(t) else np.longdouble)
    total = np.sum(wide, axis=0)
    for ld in (cols, cols + 1):
        got = _norm1_mean(gexec, tn, x, ld)        # (asserts the canary after the last column)
        assert all(g.shape == (cols,) for g in got)
        assert np.array_equal(got[0].astype(np.longdouble), np.sum(np.abs(wide), axis=0))
        if br.is_complex(t):
            assert np.array_equal(got[2].astype(wide.dtype), total)
        if rows == 0:
            assert all(same_bits(g, np.zeros(cols, g.dtype)) for g in got)
            assert not np.any(np.isnan(got[1]))
        elif br.is_complex(t):
            assert np.array_equal(got[1].real, total.real.astype(rt) / rt(rows))
            assert np.array_equal(got[1].imag, total.imag.astype(rt) / rt(rows))
        else:
            assert np.array_equal(got[1], total.astype(rt) / rt(rows))


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 3), (65, 1), (1025, 3), (100003, 3), (100003, 1)])
def test_norm1_mean_random(gexec, tn, rows, cols):
    """the header's contract for the tree reductions: |err| <= 450 eps sum|terms|"""
    t = br.TYPES[tn]
    x = _rand(np.random.default_rng(rows * 7 + cols), (rows, cols), t)
    wide = x.astype(np.clongdouble if br.is_complex(t) else np.longdouble)
    budget = 450 * br.eps_of(t) * np.sum(np.abs(wide), axis=0)
    got = _norm1_mean(gexec, tn, x, cols + 2)
    assert np.all(np.abs(got[0] - np.sum(np.abs(wide), axis=0)) <= budget)
    assert np.all(np.abs(got[1] - np.sum(wide, axis=0) / rows) <= budget / rows)
    if br.is_complex(t):
        assert np.all(np.abs(got[2] - np.sum(wide, axis=0)) <= budget)


@pytest.mark.parametrize("tn", ["f64", "f32"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (65, 3), (1025, 1), (100003, 3)])
def test_dot_norm2_contract(gexec, tn, rows, cols):
    """the contract include/gko_cdna4.h states for the deterministic tree reductions of dense::compute_dot /
    compute_norm2: |err| <= 450 eps sum|x_i y_i| (1e-13 in double)"""
    from ginkgo_amd._lib import lib
    t = br.TYPES[tn]
    rng = np.random.default_rng(rows + cols)
    x, y = _rand(rng, (rows, cols), t), _rand(rng, (rows, cols), t)
    dx, dy = Dev(gexec, padded(x, cols + 3)), Dev(gexec, padded(y, cols + 1))
    dd, dn = Dev(gexec, np.full(cols + 1, CANARY, t)), Dev(gexec, np.full(cols + 1, CANARY, t))
    nbytes = lib().gkoc_reduction_workspace_bytes(C.c_int64(rows), C.c_int64(cols), C.c_size_t(x.itemsize))
    work = Dev(gexec, np.zeros(nbytes + 64, np.uint8))
    _call("gkoc_dense_compute_dot_" + tn, gexec.stream, rows, cols, dx, cols + 3, dy, cols + 1, dd, work,
          C.c_size_t(nbytes))
    _call("gkoc_dense_compute_norm2_" + tn, gexec.stream, rows, cols, dx, cols + 3, dn, work, C.c_size_t(nbytes))
    sync()
    dot, nrm = dd.get(), dn.get()
    assert dot[cols] == t(CANARY) and nrm[cols] == t(CANARY)
    xl, yl = x.astype(np.longdouble), y.astype(np.longdouble)
    eps = br.eps_of(t)
    assert np.all(np.abs(dot[:cols] - np.sum(xl * yl, axis=0)) <= 450 * eps * np.sum(np.abs(xl * yl), axis=0))
    want = np.sqrt(np.sum(xl * xl, axis=0))
    assert np.all(np.abs(nrm[:cols] - want) <= 450 * eps * want)


SCAN_N = [0, 1, 2, 255, 256, 257, 65537, 1000003]
INT = {"i32": np.int32, "i64": np.int64, "u64": np.uint64}


@pytest.mark.parametrize("tn", ["f64", "f32", "i32", "i64", "u64"])
@pytest.mark.parametrize("n", SCAN_N)
def test_reduce_add_array(gexec, tn, n):
    """val[0] += sum(arr): small integers, so exact in every order, on top of a non-zero start"""
    t = {**br.TYPES, **INT}[tn]
    rng = np.random.default_rng(n)
    arr = rng.integers(0 if tn == "u64" else -3, 4, n).astype(t)
    val = np.array([11, 5], t)
    darr, dval = Dev(gexec, arr), Dev(gexec, val)
    _call("gkoc_reduce_add_array_" + tn, gexec.stream, n, darr, dval)
    sync()
    got = dval.get()
    assert got[0] == t(11 + int(arr.astype(np.int64).sum())) and got[1] == 5
    assert same_bits(darr.get(), arr)


@pytest.mark.parametrize("tn", list(INT))
@pytest.mark.parametrize("n", SCAN_N)
@pytest.mark.parametrize("checked", [False, True])
def test_prefix_sum_nonnegative(gexec, tn, n, checked):
    """in-place exclusive scan: entry i becomes the sum of the entries before it, the last entry's own value
    does not matter"""
    t = INT[tn]
    rng = np.random.default_rng(n + 1)
    counts = rng.integers(0, 1000, n + 2).astype(t)
    if n:
        counts[n - 1] = 123456                                      # ignored
    want = counts.copy()
    want[:n] = np.concatenate([[0], np.cumsum(counts[:max(n - 1, 0)].astype(np.int64))])[:n].astype(t)
    d = Dev(gexec, counts)
    _call("gkoc_prefix_sum_nonnegative_" + ("checked_" if checked else "") + tn, gexec.stream, d, n)
    sync()
    assert np.array_equal(d.get(), want)                            # the two entries behind n untouched


def test_prefix_sum_checked_overflow_boundary(gexec):
    """The overflow check follows Ginkgo's reference as csrc/scan.hpp records it
    (reference/components/prefix_sum_kernels.cpp): entries 0 .. n-2 are added and OverflowError is thrown when
    one of those additions would pass the type's maximum; the last entry is replaced by zero before it is
    added, so its value can never overflow the scan.  Largest stored sum 2^31 - 1: fine, exactly; one more:
    GKOC_E_OVERFLOW, input unchanged."""
    from ginkgo_amd._lib import GkoError
    big = 2 ** 31 - 1
    for n in (3, 70000):
        counts = np.zeros(n, np.int32)
        counts[0], counts[n - 2] = big - 1000, 1000
        counts[n - 1] = big                                         # the last entry is not summed
        d = Dev(gexec, counts)
        _call("gkoc_prefix_sum_nonnegative_checked_i32", gexec.stream, d, n)
        sync()
        got = d.get()
        assert got[n - 1] == big and got[0] == 0 and got[1] == big - 1000 and got[n - 2] == big - 1000
        over = counts.copy()
        over[n - 2] = 1001
        d = Dev(gexec, over)
        with pytest.raises(GkoError, match="-6|overflow"):
            _call("gkoc_prefix_sum_nonnegative_checked_i32", gexec.stream, d, n)
        sync()
        assert np.array_equal(d.get(), over)
    # 64 bits: a sum past 2^63 - 1 in int64, past 2^64 - 1 in uint64
    for tn, top in (("i64", 2 ** 63 - 1), ("u64", 2 ** 64 - 1)):
        t = INT[tn]
        ok = np.array([top - 5, 5, 7], t)
        d = Dev(gexec, ok)
        _call("gkoc_prefix_sum_nonnegative_checked_" + tn, gexec.stream, d, 3)
        sync()
        assert [int(v) for v in d.get()] == [0, top - 5, top]
        d = Dev(gexec, np.array([top - 5, 6, 0], t))
        with pytest.raises(GkoError):
            _call("gkoc_prefix_sum_nonnegative_checked_" + tn, gexec.stream, d, 3)
