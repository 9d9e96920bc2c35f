"""tests/value_kernel_refs.py against independent formulations, without a GPU: numpy's own complex arithmetic
on well-scaled input, dense fancy indexing for the gathers and fill-ins, scipy.sparse for the Ell / Sellp
diagonals, the Coo product and Dense -> Csr, dense per-block transposes for the Jacobi storage, and - before any
device is involved - the quotient sweep: plain Smith passes it on every point, the unscaled conjugate form
does not."""
import numpy as np
import pytest
import scipy.sparse as sp

import binding_refs as br
import csr_struct_refs as cr
import value_kernel_refs as vr

CTN = ["c128", "c64"]


def _close(a, b, t, k=8):
    a, b = np.asarray(a, np.clongdouble), np.asarray(b, np.clongdouble)
    return np.all(np.abs(a - b) <= k * br.eps_of(t) * np.maximum(np.abs(b), 1e-300))


# ------------------------------------------------------------------------------------ the quotient
@pytest.mark.parametrize("tn", CTN)
def test_sweep_reaches_the_edges_of_the_type(tn):
    t = br.TYPES[tn]
    a, b = vr.quotient_sweep(tn)
    fi = np.finfo(br.real_of(t))
    assert np.all(np.isfinite(b.real) & np.isfinite(b.imag)) and np.all(np.abs(a) > 0.5) and np.all(np.abs(a) < 1.5)
    mod = np.abs(b.astype(np.clongdouble))
    assert np.all((b.real == 0) | (np.abs(b.real) >= fi.tiny)) and np.all((b.imag == 0) | (np.abs(b.imag) >= fi.tiny))
    sq = mod * mod
    assert np.any(sq < np.longdouble(fi.smallest_subnormal) / 2), "no divisor whose squared modulus underflows to zero"
    assert np.any((sq > fi.smallest_subnormal) & (sq < fi.tiny)), "none whose squared modulus is subnormal"
    assert np.any(sq > np.longdouble(fi.max)), "none whose squared modulus overflows"
    assert np.any(np.abs(b.real) >= np.abs(b.imag)) and np.any(np.abs(b.real) < np.abs(b.imag))
    q = np.abs(vr.smith(br.hp(t), a, b))
    assert np.all((q > np.longdouble(fi.tiny) * 2) & (q < np.longdouble(fi.max) / 2)), "every point is representable"


@pytest.mark.parametrize("tn", CTN)
def test_plain_smith_passes_the_sweep(tn):
    t = br.TYPES[tn]
    a, b = vr.quotient_sweep(tn)
    got = vr.smith(br.plain(t), a, b)
    assert got.dtype == t
    ok, bad, worst = vr.quotient_check(got, a, b, t)
    assert ok, (bad, a[bad], b[bad], got[bad])
    # and it is a good quotient, not merely finite: a few eps of the long-double value at every point
    ref = vr.smith(br.hp(t), a, b)
    assert np.all(np.abs(got.astype(np.clongdouble) - ref) <= 6 * br.eps_of(t) * np.abs(ref)), worst


@pytest.mark.parametrize("tn", CTN)
def test_unscaled_quotient_fails_the_sweep(tn):
    """the teeth of the sweep: the conjugate form gives inf / NaN / a wrong value where |b|^2 leaves the range"""
    t = br.TYPES[tn]
    a, b = vr.quotient_sweep(tn)
    got = vr.unscaled_quotient(br.plain(t), a, b)
    ok, bad, _ = vr.quotient_check(got, a, b, t)
    assert not ok
    per_exponent = len(a) // len(vr.SWEEP_EXPONENTS[tn])
    failing = set()
    for i in range(len(a)):
        if not vr.quotient_check(got[i:i + 1], a[i:i + 1], b[i:i + 1], t)[0]:
            failing.add(vr.SWEEP_EXPONENTS[tn][i // per_exponent])
    e = vr.SWEEP_EXPONENTS[tn]
    assert {e[0], e[1], e[-2], e[-1]} <= failing and 0 not in failing and e[3] not in failing, failing
    # where the squared modulus is in range both forms agree to rounding
    mid = slice(4 * per_exponent, 5 * per_exponent)
    assert _close(got[mid], vr.smith(br.plain(t), a, b)[mid], t)


@pytest.mark.parametrize("tn", CTN)
def test_smith_against_numpy_on_well_scaled_input(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(3)
    a, b = cr.random_values(rng, 500, t), cr.random_values(rng, 500, t) + t(1.5)
    assert _close(vr.smith(br.plain(t), a, b), a.astype(np.complex128) / b.astype(np.complex128), t)
    assert _close(vr.smith(br.hp(t), a, b), a.astype(np.complex128) / b.astype(np.complex128), np.complex128)
    one = np.ones(500, t)
    assert br_same(vr.smith(br.plain(t), one, b), cr.reciprocal(br.plain(t), b))
    assert br_same(vr.invert_diagonal(br.plain(t), b), cr.reciprocal(br.plain(t), b))


def br_same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------- Dense BLAS-1
@pytest.mark.parametrize("real_scalar", [False, True])
@pytest.mark.parametrize("alpha_cols", [1, 3])
@pytest.mark.parametrize("tn", CTN)
def test_axpy_against_numpy(tn, alpha_cols, real_scalar):
    t = br.TYPES[tn]
    rng = np.random.default_rng(5)
    x, y = cr.random_values(rng, 60, t).reshape(20, 3), cr.random_values(rng, 60, t).reshape(20, 3)
    al = (rng.uniform(1, 2, alpha_cols).astype(br.real_of(t)) if real_scalar
          else cr.random_values(rng, alpha_cols, t) + t(1.5))
    w = np.complex128
    aw, xw, yw = al.astype(np.float64 if real_scalar else w).reshape(1, -1), x.astype(w), y.astype(w)
    want = {vr.SCALE: yw * aw, vr.INV_SCALE: yw / aw, vr.ADD_SCALED: yw + xw * aw, vr.SUB_SCALED: yw - xw * aw}
    for op, wv in want.items():
        for ar in (br.plain(t), br.hp(t)):
            got = vr.axpy(ar, op, al, x, y, real_scalar)
            assert got.shape == y.shape and got.dtype == ar.wt
            assert np.all(np.abs(got.astype(np.clongdouble) - wv) <= 8 * br.eps_of(t) * 8), (op, ar.name)


def test_axpy_plain_is_the_textbook_product():
    """an input on which the fused and the separately rounded products differ in float"""
    t = np.complex64
    y = np.array([[1 + 2 ** -12 + 1j * (1 - 2 ** -12)]], t)
    a = np.array([1 + 2 ** -12 - 1j * (1 + 2 ** -11)], t)
    got = vr.axpy(br.plain(t), vr.SCALE, a, None, y, False)[0, 0]
    f = np.float32
    re = f(f(y[0, 0].real * a[0].real) - f(y[0, 0].imag * a[0].imag))
    im = f(f(y[0, 0].real * a[0].imag) + f(y[0, 0].imag * a[0].real))
    assert got.real == re and got.imag == im


@pytest.mark.parametrize("tn", CTN)
@pytest.mark.parametrize("rows", [1, 257, 100003])
def test_squared_norm2(tn, rows):
    t = br.TYPES[tn]
    x = cr.random_values(np.random.default_rng(rows), rows * 2, t).reshape(rows, 2)
    ref = vr.squared_norm2(br.hp(t), x)
    assert ref.dtype == np.longdouble
    assert np.allclose(ref.astype(np.float64), np.linalg.norm(x.astype(np.complex128), axis=0) ** 2, rtol=1e-12)
    pl = vr.squared_norm2(br.plain(t), x)
    assert pl.dtype == br.real_of(t)
    assert np.all(np.abs(pl - ref) <= rows * br.eps_of(t) * ref)
    d = vr.squared_norm2_depth(rows)
    assert d >= 17 and (rows > 1 or d == 18) and vr.squared_norm2_depth(100003) == 8 + 8 + 1 + 8
    assert vr.squared_norm2_depth(2 ** 22) == 64 + 8 + 1 + 8


@pytest.mark.parametrize("tn", CTN)
def test_absolute(tn):
    t = br.TYPES[tn]
    rt = br.real_of(t)
    e = vr.edge_reals(rt)
    e = e[np.isfinite(e)]
    x = (e[:, None] + 1j * e[None, :]).astype(t).reshape(-1, 1)
    ref = vr.absolute(br.hp(t), x)
    assert np.all(np.isfinite(ref)) and np.all(ref[(x.real != 0) | (x.imag != 0)] > 0)
    exact = np.sqrt(x.real.astype(np.longdouble) ** 2 + x.imag.astype(np.longdouble) ** 2)    # no overflow in long double
    assert np.all(np.abs(ref - exact) <= 4 * np.finfo(np.longdouble).eps * exact)
    assert vr.absolute(br.hp(t), np.array([[3 + 4j]], t))[0, 0] == 5


# -------------------------------------------------------------------------------- counts, gathers
@pytest.mark.parametrize("tn", CTN)
def test_count_and_to_csr_against_scipy(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(11)
    x = np.where(rng.uniform(size=(40, 17)) < 0.3, cr.random_values(rng, 40 * 17, t).reshape(40, 17), 0).astype(t)
    x[3, 4], x[5, 6], x[7, :] = t(complex(-0.0, 0.0)), t(complex(0.0, -0.0)), 0
    x[2, 2] = t(complex(0.0, 2.0))
    m = sp.csr_matrix(x.astype(np.complex128))
    m.eliminate_zeros()
    ptrs, cols, vals = vr.dense_to_csr(x)
    assert np.array_equal(ptrs, m.indptr) and np.array_equal(cols, m.indices) and np.array_equal(vals, m.data.astype(t))
    assert np.array_equal(vr.count_nonzeros_per_row(x), np.diff(m.indptr))
    assert not vr.is_nonzero(x[3, 4]) and not vr.is_nonzero(x[5, 6]) and vr.is_nonzero(x[2, 2])
    assert vr.is_nonzero(t(complex(np.nan, 0))) and vr.is_nonzero(t(complex(0, np.nan)))


def test_gather_and_fill_in_against_fancy_indexing():
    rng = np.random.default_rng(13)
    orig = vr.random_bits(rng, 50 * 4, np.complex128).reshape(50, 4)
    rows = np.array([3, 3, 49, 0, 17, 3])
    assert br_same(vr.row_gather(rows, orig), orig[rows])
    pos = rng.choice(50 * 4, 70, replace=False)
    r, c = pos // 4, pos % 4
    vals = vr.random_bits(rng, 70, np.complex128)
    out0 = np.full((50, 4), -777.25, np.complex128)
    want = out0.copy()
    want[r, c] = vals
    got = vr.fill_in_matrix_data(r, c, vals, out0)
    assert br_same(got, want) and np.count_nonzero(got.view(np.uint64) != out0.view(np.uint64)) > 0
    assert np.all(out0 == -777.25)


@pytest.mark.parametrize("tn", CTN)
@pytest.mark.parametrize("shape", [(5, 5), (7, 3), (3, 7)])
def test_add_scaled_identity_real(tn, shape):
    t = br.TYPES[tn]
    m = cr.random_values(np.random.default_rng(17), shape[0] * shape[1], t).reshape(shape)
    for ar in (br.plain(t), br.hp(t)):
        got = vr.add_scaled_identity_real(ar, 0.75, -1.5, m)
        want = -1.5 * m.astype(np.complex128) + 0.75 * np.eye(*shape)
        assert np.all(np.abs(got.astype(np.complex128) - want) <= 4 * br.eps_of(t) * 4)
    assert np.count_nonzero(np.eye(*shape)) == min(shape)


# --------------------------------------------------------------------------------------- Csr / Coo
@pytest.mark.parametrize("tn", CTN)
def test_csr_scale_against_scipy(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(19)
    p, c = cr.random_pattern(rng, 30, 30, 0.2, (4,))
    v = cr.random_values(rng, len(c), t)
    d = cr.random_values(rng, 30, t) + t(1.5)
    a = sp.csr_matrix((v.astype(np.complex128), c, p), shape=(30, 30))
    dw = d.astype(np.complex128)
    want = {0: sp.diags(dw) @ a, 1: sp.diags(1 / dw) @ a, 2: a @ sp.diags(dw)}
    for mode, w in want.items():
        w = sp.csr_matrix(w)
        w.sort_indices()
        for ar in (br.plain(t), br.hp(t)):
            got = vr.csr_scale_by_diagonal(ar, p, c, d, mode, v)
            assert _close(got, w.data, t, 16), mode


@pytest.mark.parametrize("tn", CTN)
def test_coo_spmv2_against_scipy(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(23)
    nnz = 400
    rows, cols = rng.integers(0, 20, nnz), rng.integers(0, 15, nnz)
    rows[:50], cols[:50] = 7, 3                          # duplicates of one position
    vals = cr.random_values(rng, nnz, t)
    b, c0 = cr.random_values(rng, 45, t).reshape(15, 3), cr.random_values(rng, 60, t).reshape(20, 3)
    alpha = t(0.5 - 2j)
    a = sp.coo_matrix((vals.astype(np.complex128), (rows, cols)), shape=(20, 15))
    for al in (None, alpha):
        c, m, S = vr.coo_spmv2(rows, cols, vals, b, c0, al)
        want = c0.astype(np.complex128) + (1 if al is None else complex(al)) * (a @ b.astype(np.complex128))
        assert np.all(np.abs(c.astype(np.complex128) - want) <= 1e-13 * S.astype(np.float64))
        assert np.array_equal(m[:, 0], np.bincount(rows, minlength=20)) and m[7, 0] >= 50
        c2, m2, S2 = vr.coo_spmv2_fast(rows, cols, vals, b, c0, al)
        assert np.array_equal(m, m2) and np.all(np.abs(c - c2) <= 1e-17 * S) and np.all(np.abs(S - S2) <= 1e-17 * S)
        assert np.all(S >= np.abs(c) * (1 - 1e-15))


# ------------------------------------------------------------------------------------- Ell / Sellp
def _rows_with_diagonals(rng, n, t):
    """rows of 0 .. 6 entries with distinct columns, some without a diagonal; values never zero"""
    rows = []
    for r in range(n):
        k = int(rng.integers(0, 7))
        cols = set(rng.choice(n, min(k, n), replace=False).tolist())
        if r % 3 == 0:
            cols.discard(r)
        elif k:
            cols.add(r)
        cols = sorted(cols) if r % 2 else sorted(cols, reverse=True)
        rows.append([(c, v) for c, v in zip(cols, cr.random_values(rng, len(cols), t) + t(2))])
    return rows


def _scipy_of(rows, n):
    r = [i for i, e in enumerate(rows) for _ in e]
    c = [c for e in rows for c, _ in e]
    v = [complex(v) for e in rows for _, v in e]
    return sp.csr_matrix((v, (r, c)), shape=(n, n))


@pytest.mark.parametrize("tn", ["f64", "c64"])
@pytest.mark.parametrize("n", [1, 70, 131])
def test_ell_and_sellp_diagonals_against_scipy(tn, n):
    t = br.TYPES[tn]
    rng = np.random.default_rng(n)
    rows = _rows_with_diagonals(rng, n, t)
    want = _scipy_of(rows, n).diagonal()
    want = (want if br.is_complex(t) else want.real).astype(t)
    fill = t(-777.25)
    has = np.array([any(c == r for c, _ in e) for r, e in enumerate(rows)])
    want = np.where(has, want, fill)
    ell_k = max(len(e) for e in rows) + 1
    cols, vals = vr.ell_from_rows(rows, n + 5, ell_k, t, np.int32)
    assert br_same(vr.ell_extract_diagonal(n, ell_k, n + 5, cols, vals, np.full(n, fill, t)), want)
    for ss in (32, 64):
        sets, sc, sv = vr.sellp_from_rows(rows, ss, t, np.int64)
        assert len(sets) == -(-n // ss) + 1 and len(sc) == int(sets[-1]) * ss
        assert br_same(vr.sellp_extract_diagonal(n, ss, sets, sc, sv, np.full(n, fill, t)), want)
        assert np.count_nonzero(sc >= 0) == sum(len(e) for e in rows)


def test_extract_diagonal_takes_the_first_slot_with_the_rows_column_whatever_its_value():
    t = np.float64
    rows = [[(0, 0.0), (0, 5.0)], [(0, 1.0)], [(2, -0.0), (1, 3.0), (2, 7.0)]]
    cols, vals = vr.ell_from_rows(rows, 4, 3, t, np.int32)
    got = vr.ell_extract_diagonal(3, 3, 4, cols, vals, np.full(3, 9.0))
    assert got[0] == 0 and got[1] == 9 and got[2] == 0 and np.signbit(got[2])
    assert cols[1 + 1 * 4] == -1 and vals[1 + 1 * 4] == 0                    # padding: column -1, never a match


def test_ell_copy():
    rng = np.random.default_rng(29)
    n, k, ss, ds = 9, 3, 11, 14
    sc, sv = rng.integers(0, 9, ss * k).astype(np.int32), rng.uniform(size=ss * k)
    dc, dv = vr.ell_copy(n, k, ss, sc, sv, ds, np.full(ds * k, -5, np.int32), np.full(ds * k, -777.25))
    assert np.array_equal(dc.reshape(k, ds)[:, :n], sc.reshape(k, ss)[:, :n])
    assert np.array_equal(dv.reshape(k, ds)[:, :n], sv.reshape(k, ss)[:, :n])
    assert np.all(dc.reshape(k, ds)[:, n:] == -5) and np.all(dv.reshape(k, ds)[:, n:] == -777.25)


# ------------------------------------------------------------------------------------------ Jacobi
@pytest.mark.parametrize("max_bs", [1, 5, 32])
def test_jacobi_transpose_against_dense_blocks(max_bs):
    from ginkgo_amd.preconditioner import compute_storage_scheme
    rng = np.random.default_rng(max_bs)
    scheme = compute_storage_scheme(max_bs)
    sizes = np.concatenate([[max_bs, 1], rng.integers(1, max_bs + 1, 37)])
    ptrs = np.concatenate([[0], np.cumsum(sizes)])
    total = vr.block_storage_size(scheme, len(sizes))
    assert total % int(scheme.group_offset) == 0 and total >= max_bs * max_bs * len(sizes)
    blocks = cr.random_values(rng, total, np.complex128)
    fill = np.full(total, -777.25, np.complex128)
    for conj in (0, 1):
        out = vr.jacobi_transpose(scheme, ptrs, blocks, conj, fill)
        for a, b in zip(vr.jacobi_blocks_dense(scheme, ptrs, blocks), vr.jacobi_blocks_dense(scheme, ptrs, out)):
            assert br_same(b, np.ascontiguousarray(a.conj().T if conj else a.T))
        touched = out != fill
        assert np.count_nonzero(touched) == int(np.sum(sizes ** 2))
        back = vr.jacobi_transpose(scheme, ptrs, out, conj, fill)
        assert br_same(back[touched], blocks[touched]) and np.all(back[~touched] == -777.25)
    starts = [vr.block_start(scheme, b) for b in range(len(sizes))]
    assert len(set(starts)) == len(starts) and max(starts) < total


def test_initialize_precisions():
    assert vr.initialize_precisions([7], 4).tolist() == [7, 7, 7, 7]
    assert vr.initialize_precisions([1, 2, 3], 7).tolist() == [1, 2, 3, 1, 2, 3, 1]
    assert vr.initialize_precisions([1, 2, 3, 4, 5], 3).tolist() == [1, 2, 3]
    assert vr.initialize_precisions([1, 2], 0).size == 0


@pytest.mark.parametrize("tn", CTN)
def test_scalar_apply_and_invert(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(31)
    d, b, x0 = cr.random_values(rng, 12, t), cr.random_values(rng, 36, t).reshape(12, 3), \
        cr.random_values(rng, 36, t).reshape(12, 3)
    w = np.complex128
    al, be = t(0.5 + 1j), t(-2 + 0.25j)
    for ar in (br.plain(t), br.hp(t)):
        assert _close(vr.scalar_apply(ar, d, b), b.astype(w) * d.astype(w)[:, None], t)
        assert np.all(np.abs(vr.scalar_apply(ar, d, b, al, be, x0).astype(w)
                             - (complex(be) * x0.astype(w) + complex(al) * b.astype(w) * d.astype(w)[:, None]))
                      <= 16 * br.eps_of(t) * 4)
    z = np.array([0, complex(-0.0, 0.0), complex(0.0, -0.0), 2j, 4], t)
    inv = vr.invert_diagonal(br.plain(t), z)
    assert br_same(inv[:3], np.ones(3, t)) and inv[3] == t(-0.5j) and inv[4] == t(0.25)


# -------------------------------------------------------------------------------- array components
@pytest.mark.parametrize("tn", CTN)
def test_conj_array(tn):
    t = br.TYPES[tn]
    x = vr.random_bits(np.random.default_rng(37), 300, t)
    got = vr.conj_array(x)
    fin = np.isfinite(x.real) & np.isfinite(x.imag)
    assert np.array_equal(got[fin], np.conj(x[fin]))
    rt = br.real_of(t)
    u = np.uint32 if rt == np.float32 else np.uint64
    gb, xb = got.view(u).reshape(-1, 2), x.view(u).reshape(-1, 2)
    top = u(1) << u(np.dtype(u).itemsize * 8 - 1)
    assert np.array_equal(gb[:, 0], xb[:, 0]) and np.array_equal(gb[:, 1] ^ top, xb[:, 1])
    assert br_same(vr.conj_array(got), x)


def test_random_bits_holds_the_special_values():
    x = vr.random_bits(np.random.default_rng(41), 4000, np.float32)
    assert np.isnan(x).sum() > 1 and np.signbit(x[1]) and x[1] == 0 and np.isinf(x[2])
    nan_bits = x[np.isnan(x)].view(np.uint32) & 0x7fffff
    assert len(set(nan_bits.tolist())) > 1, "NaN payloads differ"


def test_table_builders_agree_with_the_row_builders():
    rng = np.random.default_rng(43)
    n, w = 150, 4
    length = rng.integers(0, w + 1, n)
    C = rng.integers(0, n, (n, w))
    C[np.arange(w)[None, :] >= length[:, None]] = -1
    V = rng.uniform(1, 2, (n, w))
    rows = [[(int(C[r, k]), V[r, k]) for k in range(length[r])] for r in range(n)]
    ec, ev = vr.ell_from_table(C, V, n + 2, np.int32)
    rc, rv = vr.ell_from_rows(rows, n + 2, w, np.float64, np.int32)
    assert br_same(ec, rc) and br_same(ev, rv)
    for ss in (32, 64):
        a, b = vr.sellp_from_table(C, V, ss, np.int64), vr.sellp_from_rows(rows, ss, np.float64, np.int64)
        assert all(br_same(x, y) for x, y in zip(a, b))
