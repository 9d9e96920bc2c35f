"""The complex Dense BLAS-1 and conversions (gkoc_cdense_*, csrc/complex_blas.hip), the real Dense helpers
gkoc_dense_absolute_*, gkoc_dense_fill_in_matrix_data_*, gkoc_dense_add_scaled_identity_real_* and the scalar
Jacobi on complex values (gkoc_cjacobi_invert_diagonal_*, gkoc_cjacobi_scalar_apply_*) through the C ABI
against tests/value_kernel_refs.py.

Products and sums are bit-identical to the plain restatement (textbook complex product, every real operation
rounded on its own).  The three users of the complex quotient - cjacobi_invert_diagonal, ccsr_scale_by_diagonal
mode 1, cdense_inv_scale with a complex scalar - are swept over the range of the type
(test_quotient_sweep_*): finite wherever the long-double quotient is a normal number, and within rule R, sized
by plain Smith, of it.  squared_norm2: (depth + 3) eps sum, depth = the additions on the longest path of the
two-level tree (value_kernel_refs.squared_norm2_depth), exact on small integers.  Moduli: hypot within 2 ulp.
Counts, conversions, gathers and fill-ins are exact and bit for bit.  Inputs are read back and compared bit
for bit, outputs are pre-filled with NaN and followed by canaries or sit in padded operands.  After the last
test the file prints the largest observed |kernel - ref| / (eps max|ref|) (pytest -s)."""
import numpy as np
import pytest

import binding_refs as br
import csr_struct_refs as cr
import value_kernel_refs as vr
from binding_gpu import CANARY, Dev, DevCsr, call as _call, canaries_ok, grid_cap_rows as _grid_cap_rows, \
    head_of, out_buf as _out, padded, raises_invalid, same_bits, sync, tail_ok as _tail_ok

pytestmark = pytest.mark.gpu

TN = ["c128", "c64"]
IT = {"i32": np.int32, "i64": np.int64}
SIZES = [0, 1, 255, 256, 257, 2049, 100003]
OPS = {vr.SCALE: "gkoc_cdense_scale_", vr.INV_SCALE: "gkoc_cdense_inv_scale_", vr.ADD_SCALED: "gkoc_cdense_add_scaled_",
       vr.SUB_SCALED: "gkoc_cdense_sub_scaled_"}
STATS = {}


def _stat(name, tn, ratio):
    STATS[(name, tn)] = max(STATS.get((name, tn), 0.0), ratio)


def _scalars(rng, k, t, real_scalar):
    """k scalars away from zero, both branches of the quotient"""
    if real_scalar:
        return (rng.uniform(0.5, 2, k) * rng.choice([-1, 1], k)).astype(br.real_of(t))
    a = cr.random_values(rng, k, t)
    a = a + np.where(a.real < 0, -1, 1).astype(t)
    a[1::2] = a[1::2] * t(1j)
    return a.astype(t)


# ------------------------------------------------------------------ scale, inv_scale, add_scaled, sub_scaled
@pytest.mark.parametrize("alpha_cols", ["one", "cols"])
@pytest.mark.parametrize("real_scalar", [0, 1])
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("tn", TN)
def test_axpy(gexec, tn, op, real_scalar, alpha_cols):
    t = br.TYPES[tn]
    cols = 3
    for rows in SIZES:
        rng = np.random.default_rng(rows + 7 * op)
        x, y = (cr.random_values(rng, rows * cols, t).reshape(rows, cols) for _ in range(2))
        alpha = _scalars(rng, 1 if alpha_cols == "one" else cols, t, real_scalar)
        fx, fy = padded(x, cols + 2), padded(y, cols + 3)
        dx, dy, da = Dev(gexec, fx), Dev(gexec, fy), Dev(gexec, alpha)
        args = (gexec.stream, rows, cols, da, len(alpha), real_scalar)
        if op in (vr.SCALE, vr.INV_SCALE):
            _call(OPS[op] + tn, *args, dy, cols + 3)
        else:
            _call(OPS[op] + tn, *args, dx, cols + 2, dy, cols + 3)
        sync()
        got = dy.get()
        assert canaries_ok(got, cols) and same_bits(dx.get(), fx) and same_bits(da.get(), alpha)
        got = got[:, :cols]
        want = vr.axpy(br.plain(t), op, alpha, x, y, bool(real_scalar))
        if op == vr.INV_SCALE and not real_scalar:
            ok, ratio = br.rule_r(got, vr.axpy(br.hp(t), op, alpha, x, y, False), want, t)
            assert ok, (rows, ratio)
            _stat("cdense_inv_scale, complex scalar", tn, ratio)
            STATS[("  ... entries that differ from plain Smith", tn)] = \
                STATS.get(("  ... entries that differ from plain Smith", tn), 0) + int(np.count_nonzero(got != want))
        else:
            assert same_bits(got, want), (rows, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:4])


def test_axpy_special_scalars_and_argument_checks(gexec):
    """scaling by an exact zero multiplies like by any value (NaN * 0 stays NaN, -1 * 0 = -0); a NULL alpha or
    an alpha_cols that is neither 1 nor cols is refused before the launch"""
    t = np.complex64
    y = np.array([[1 - 2j, complex(np.nan, 1)], [complex(-1, 0), 3j]], t)
    dy, da = Dev(gexec, padded(y, 4)), Dev(gexec, np.zeros(1, t))
    _call("gkoc_cdense_scale_c64", gexec.stream, 2, 2, da, 1, 0, dy, 4)
    sync()
    got = dy.get()
    assert canaries_ok(got, 2)
    assert np.isnan(got[0, 1].real) and np.isnan(got[0, 1].imag) and got[0, 0] == 0 and got[1, 1] == 0
    assert got[1, 0] == 0 and np.signbit(got[1, 0].real) and not np.signbit(got[1, 0].imag)   # (-0 - 0, -0 + 0)
    before = dy.get()
    assert raises_invalid("gkoc_cdense_scale_c64", gexec.stream, 2, 2, da, 3, 0, dy, 4)
    assert raises_invalid("gkoc_cdense_add_scaled_c64", gexec.stream, 2, 2, None, 1, 0, dy, 4, dy, 4)
    sync()
    assert same_bits(dy.get(), before)


def test_scale_beyond_the_grid_cap(gexec):
    """the GKOC_FOR2 / grid_of style of complex_blas.hip (capped grid, grid-stride loop)"""
    n = _grid_cap_rows() + 257
    y = ((np.arange(n) % 9 - 4) + 1j * (np.arange(n) % 5 - 2)).astype(np.complex64).reshape(n, 1)
    dy = Dev(gexec, np.concatenate([y.reshape(-1), np.full(3, CANARY, np.complex64)]))
    _call("gkoc_cdense_scale_c64", gexec.stream, n, 1, Dev(gexec, np.array([-2], np.float32)), 1, 1, dy, 1)
    sync()
    got = dy.get()
    want = (-2 * y).reshape(-1)
    assert _tail_ok(got, n) and np.array_equal(got[:n], want), np.flatnonzero(got[:n] != want)[:4]


# ---------------------------------------------------------------------------------------- the quotient
@pytest.mark.parametrize("tn", TN)
def test_quotient_sweep_invert_diagonal(gexec, tn):
    t = br.TYPES[tn]
    _, b = vr.quotient_sweep(tn)
    dd, out = Dev(gexec, b), _out(gexec, len(b), t)
    _call("gkoc_cjacobi_invert_diagonal_" + tn, gexec.stream, len(b), dd, out)
    sync()
    got = out.get()
    assert _tail_ok(got, len(b)) and same_bits(dd.get(), b)
    ok, bad, ratio = vr.quotient_check(got[:len(b)], np.ones(len(b), t), b, t)
    assert ok, "first wrong element: 1 / %r = %r, long double %r" % (
        b[bad], got[bad], vr.smith(br.hp(t), np.ones(1, t), b[bad:bad + 1])[0])
    _stat("quotient sweep: cjacobi_invert_diagonal", tn, ratio)


@pytest.mark.parametrize("tn", TN)
def test_quotient_sweep_inv_scale(gexec, tn):
    """one column per divisor, three rows of numerators of modulus about 1"""
    t = br.TYPES[tn]
    a, b = vr.quotient_sweep(tn)
    cols = len(b)
    y = np.stack([a, np.roll(a, 1), np.conj(a)]).astype(t)
    fy = padded(y, cols + 3)
    dy, da = Dev(gexec, fy), Dev(gexec, b)
    _call("gkoc_cdense_inv_scale_" + tn, gexec.stream, 3, cols, da, cols, 0, dy, cols + 3)
    sync()
    got = dy.get()
    assert canaries_ok(got, cols) and same_bits(da.get(), b)
    bb = np.broadcast_to(b, y.shape)
    ok, bad, ratio = vr.quotient_check(got[:, :cols], y, bb, t)
    assert ok, "first wrong element: %r / %r = %r, long double %r" % (
        y.reshape(-1)[bad], bb.reshape(-1)[bad], got[:, :cols].reshape(-1)[bad],
        vr.smith(br.hp(t), y, bb).reshape(-1)[bad])
    _stat("quotient sweep: cdense_inv_scale", tn, ratio)


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_quotient_sweep_csr_scale_by_inverse_diagonal(gexec, tn, in_):
    """mode 1 of gkoc_ccsr_scale_by_diagonal: vals[k] *= 1 / diag[row], two entries of modulus about 1 per row"""
    t, it = br.TYPES[tn], IT[in_]
    a, b = vr.quotient_sweep(tn)
    n = len(b)
    ptrs, cols = np.arange(0, 2 * n + 1, 2), np.tile([0, 1], n)
    vals = np.stack([a, np.conj(np.roll(a, 2))], axis=1).reshape(-1).astype(t)
    da = DevCsr(gexec, it, ptrs, cols)
    dd, dv = Dev(gexec, b), Dev(gexec, np.concatenate([vals, np.full(3, CANARY, t)]))
    _call("gkoc_ccsr_scale_by_diagonal_" + tn + "_" + in_, gexec.stream, n, *da.dev, dd, 1, dv)
    sync()
    got = dv.get()
    assert _tail_ok(got, 2 * n) and da.unchanged() and same_bits(dd.get(), b)
    ref = vr.csr_scale_by_diagonal(br.hp(t), ptrs, cols, b, 1, vals)
    pl = vr.csr_scale_by_diagonal(br.plain(t), ptrs, cols, b, 1, vals)
    ok, bad, ratio = vr.entrywise_check(got[:2 * n], ref, pl, t)
    assert ok, "first wrong element: %r * (1 / %r) = %r, long double %r" % (vals[bad], b[bad // 2], got[bad], ref[bad])
    _stat("quotient sweep: ccsr_scale_by_diagonal mode 1", tn, ratio)


# ------------------------------------------------------------------------------------- scalar Jacobi
@pytest.mark.parametrize("tn", TN)
def test_cjacobi_invert_diagonal(gexec, tn):
    """1 / d; a zero entry (both parts zero, either sign) inverts as one: (1, +0) bit for bit"""
    t = br.TYPES[tn]
    for n in SIZES:
        rng = np.random.default_rng(n + 3)
        d = _scalars(rng, n, t, False)
        zeros = np.array([0, complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)], t)
        where = np.arange(0, n, 7)[:40]
        d[where] = zeros[np.arange(len(where)) % 4]
        dd, out = Dev(gexec, d), _out(gexec, n, t)
        _call("gkoc_cjacobi_invert_diagonal_" + tn, gexec.stream, n, dd, out)
        sync()
        got = head_of(out, n, n, fill=np.nan)
        assert same_bits(dd.get(), d)
        assert same_bits(got[where], np.ones(len(where), t)), "the zero-diagonal substitute"
        want = vr.invert_diagonal(br.plain(t), d)
        ok, bad, ratio = vr.entrywise_check(got, vr.invert_diagonal(br.hp(t), d), want, t)
        assert ok, (n, bad)
        _stat("cjacobi_invert_diagonal", tn, ratio)
        STATS[("  ... entries that differ from plain Smith", tn)] = \
            STATS.get(("  ... entries that differ from plain Smith", tn), 0) + int(np.count_nonzero(got != want))


@pytest.mark.parametrize("advanced", [0, 1])
@pytest.mark.parametrize("tn", TN)
def test_cjacobi_scalar_apply(gexec, tn, advanced):
    t = br.TYPES[tn]
    for rows, cols in [(0, 3), (3, 0), (1, 1), (255, 2), (256, 1), (257, 3), (2049, 2), (100003, 1)]:
        rng = np.random.default_rng(rows + cols)
        d = cr.random_values(rng, rows, t)
        b, x0 = (cr.random_values(rng, rows * cols, t).reshape(rows, cols) for _ in range(2))
        fb = padded(b, cols + 2)
        fx = padded(x0 if advanced else np.full((rows, cols), np.nan, t), cols + 3)
        al, be = np.array([0.75 - 1.25j], t), np.array([-0.5 + 2j], t)
        dd, db, dx, dal, dbe = (Dev(gexec, z) for z in (d, fb, fx, al, be))
        _call("gkoc_cjacobi_scalar_apply_" + tn, gexec.stream, rows, cols, dd, dal if advanced else None, db, cols + 2,
              dbe if advanced else None, dx, cols + 3)
        sync()
        got = dx.get()
        assert canaries_ok(got, cols) and same_bits(db.get(), fb) and same_bits(dd.get(), d)
        assert same_bits(dal.get(), al) and same_bits(dbe.get(), be)
        want = vr.scalar_apply(br.plain(t), d, b, al[0], be[0], x0) if advanced else vr.scalar_apply(br.plain(t), d, b)
        assert same_bits(got[:, :cols], want.reshape(rows, cols)), (rows, cols)
    assert raises_invalid("gkoc_cjacobi_scalar_apply_" + tn, gexec.stream, 1, 1, dd, dal, db, 3, None, dx, 4)


# ----------------------------------------------------------------------------------- squared_norm2
@pytest.mark.parametrize("tn", TN)
def test_squared_norm2(gexec, tn):
    t, rt = br.TYPES[tn], br.real_of(br.TYPES[tn])
    cols = 3
    for rows in SIZES + [600001]:
        for integers in (True, False):
            rng = np.random.default_rng(rows)
            x = (rng.integers(-3, 4, (rows, cols)) + 1j * rng.integers(-3, 4, (rows, cols))).astype(t) if integers \
                else cr.random_values(rng, rows * cols, t).reshape(rows, cols)
            fx = padded(x, cols + 2)
            dx, out = Dev(gexec, fx), _out(gexec, cols, rt)
            _call("gkoc_cdense_compute_squared_norm2_" + tn, gexec.stream, rows, cols, dx, cols + 2, out)
            sync()
            got = head_of(out, cols, cols, fill=np.nan)
            assert same_bits(dx.get(), fx)
            ref = vr.squared_norm2(br.hp(t), x)
            if rows == 0:
                assert same_bits(got, np.zeros(cols, rt))
            if integers:
                assert np.array_equal(got.astype(np.longdouble), ref), rows          # exact in every order
            bound = (vr.squared_norm2_depth(max(rows, 1)) + 3) * br.eps_of(t) * ref
            err = np.abs(got.astype(np.longdouble) - ref)
            print("squared_norm2", tn, rows, "err / (eps sum) =", float(np.max(err / (br.eps_of(t) * np.maximum(ref, 1)))),
                  "bound", vr.squared_norm2_depth(max(rows, 1)) + 3)
            assert np.all(err <= bound), (rows, err, bound)
            if rows and not integers:
                _stat("cdense_compute_squared_norm2 (of eps sum)", tn, float(np.max(err / (br.eps_of(t) * ref))))
    out = _out(gexec, 2, rt)
    _call("gkoc_cdense_compute_squared_norm2_" + tn, gexec.stream, 5, 0, dx, 5, out)        # no columns: nothing
    sync()
    head_of(out, 2, 0, fill=np.nan)
    assert raises_invalid("gkoc_cdense_compute_squared_norm2_" + tn, gexec.stream, -1, 2, dx, 5, out)


# --------------------------------------------------------------------------------- dot, conj dot
@pytest.mark.parametrize("rows,cols", [(0, 3), (2048, 1), (2049, 3), (524289, 1), (5, 0), (0, 0)])
@pytest.mark.parametrize("conjugate_x", [0, 1])
@pytest.mark.parametrize("tn", TN)
def test_compute_dot_launcher_edges(gexec, tn, conjugate_x, rows, cols):
    """x . y and conj(x) . y per column at the edges of the two-stage launcher: no rows (zeros), no columns
    (nothing written), one block per column and its first split, one row past the cap of 256 blocks of 2048
    rows.  Gaussian integers in [-3, 3]: both parts of every product are integers of modulus <= 18, every
    partial sum stays below 524289 * 18 < 2^24, so the result is exact in every summation order"""
    t = br.TYPES[tn]
    rng = np.random.default_rng(rows + cols)
    x, y = [(rng.integers(-3, 4, (rows, cols)) + 1j * rng.integers(-3, 4, (rows, cols))).astype(t) for _ in range(2)]
    fx, fy = padded(x, cols + 2), padded(y, cols + 1)
    dx, dy, out = Dev(gexec, fx), Dev(gexec, fy), _out(gexec, cols, t)
    _call("gkoc_cdense_compute_dot_" + tn, gexec.stream, rows, cols, dx, cols + 2, dy, cols + 1, out, conjugate_x)
    sync()
    got = head_of(out, cols, cols, fill=np.nan)
    assert same_bits(dx.get(), fx) and same_bits(dy.get(), fy)
    wx, wy = x.astype(np.complex128), y.astype(np.complex128)
    assert np.array_equal(got.astype(np.complex128), np.sum((np.conj(wx) if conjugate_x else wx) * wy, axis=0))
    if rows == 0:
        assert same_bits(got, np.zeros(cols, t))


# ------------------------------------------------------------------------------------------ moduli
def _within_ulps(got, ref, k):
    """|got - ref| <= k ulp of the type at ref (subnormal results: k times the smallest subnormal)"""
    rounded = ref.astype(got.dtype)
    return np.abs(got.astype(np.longdouble) - ref) <= k * np.spacing(np.abs(rounded)).astype(np.longdouble)


def _modulus_cases(t):
    rt = br.real_of(t)
    e = vr.edge_reals(rt)
    e = e[np.isfinite(e)]
    grid = (e[:, None] + 1j * e[None, :]).astype(t).reshape(-1)
    rnd = cr.random_values(np.random.default_rng(5), 100003 * 2 - len(grid) % 2, t)
    x = np.concatenate([grid, rnd])
    return x[:len(x) // 2 * 2].reshape(-1, 2)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tn", TN)
def test_cdense_absolute(gexec, tn, mode):
    """hypot: 2 ulp of the long-double modulus; moduli at the overflow and underflow edges of the type stay finite
    and non-zero; mode 0 leaves the imaginary parts +0"""
    t, rt = br.TYPES[tn], br.real_of(br.TYPES[tn])
    allx = _modulus_cases(t)
    fi = np.finfo(rt)
    for rows in [0, 1, 255, 256, 257, 2049, len(allx)]:
        x = allx[:rows]
        fx, fo = padded(x, 4), padded(np.full((rows, 2), np.nan, rt), 5)
        dx, do = Dev(gexec, fx), Dev(gexec, fo)
        _call("gkoc_cdense_absolute_" + tn, gexec.stream, rows, 2, dx, 4, do if mode else None, 5 if mode else 0, mode)
        sync()
        gx, go = dx.get(), do.get()
        ref = vr.absolute(br.hp(t), x)
        if mode == 0:
            assert canaries_ok(gx, 2) and same_bits(go, fo)
            got = gx[:, :2].real.copy()
            assert same_bits(gx[:, :2].imag.copy(), np.zeros((rows, 2), rt)), "imaginary parts are +0"
        else:
            assert canaries_ok(go, 2) and same_bits(gx, fx)
            got = go[:, :2]
        inrange = ref <= np.longdouble(fi.max)
        assert np.all(_within_ulps(got, ref, 2)[inrange]), rows
        assert np.all(np.isfinite(got[inrange])) and np.all(np.isinf(got[~inrange]))
        assert np.all(got[(x.real != 0) | (x.imag != 0)] > 0), "a non-zero value has a non-zero modulus"
        if rows:
            ulps = np.abs(got.astype(np.longdouble) - ref)[inrange] / np.spacing(np.abs(ref.astype(rt)))[inrange]
            _stat("cdense_absolute (ulp)", tn, float(np.max(ulps)))
    assert raises_invalid("gkoc_cdense_absolute_" + tn, gexec.stream, 1, 1, dx, 4, do, 5, 2)


@pytest.mark.parametrize("tn", ["f64", "f32"])
def test_dense_absolute(gexec, tn):
    """real values: the magnitude bit for bit (no rounding is involved); NaN stays NaN"""
    t = br.TYPES[tn]
    rng = np.random.default_rng(9)
    base = np.concatenate([vr.edge_reals(t), rng.uniform(-1, 1, 100003 * 2).astype(t)])
    for rows, ldx, ldy in [(0, 2, 2), (1, 2, 2), (255, 2, 2), (256, 2, 5), (257, 4, 2), (2049, 2, 2), (100003, 2, 2),
                           (100003, 3, 4)]:
        x = base[:rows * 2].reshape(rows, 2)
        fx, fy = padded(x, ldx), padded(np.full((rows, 2), np.nan, t), ldy)
        dx, dy = Dev(gexec, fx), Dev(gexec, fy)
        _call("gkoc_dense_absolute_" + tn, gexec.stream, rows, 2, dx, ldx, dy, ldy)
        sync()
        got = dy.get()
        assert canaries_ok(got, 2) and same_bits(dx.get(), fx)
        got = got[:, :2]
        nan = np.isnan(x)
        assert np.array_equal(np.isnan(got), nan)
        assert same_bits(np.where(nan | (x == 0), 0, got).astype(t), np.where(nan | (x == 0), 0, np.abs(x)).astype(t))
        assert np.all(got[x == 0] == 0)
    x = base[:600].reshape(300, 2).copy()                                  # x == y: inplace_absolute_dense
    dx = Dev(gexec, x)
    _call("gkoc_dense_absolute_" + tn, gexec.stream, 300, 2, dx, 2, dx, 2)
    sync()
    keep = ~np.isnan(x)
    assert np.array_equal(dx.get()[keep], np.abs(x)[keep])


def test_dense_absolute_beyond_the_grid_cap(gexec):
    """launch_elementwise (elementwise.hpp): the flat vector kernel and, with a stride, the general kernel"""
    n = _grid_cap_rows() * 2 + 257
    x = (np.arange(n) % 11 - 5).astype(np.float32)
    for ld in (1, 2):
        fx = np.full((n, ld), CANARY, np.float32)
        fx[:, 0] = x
        dx, dy = Dev(gexec, fx), Dev(gexec, np.full((n, ld), CANARY, np.float32))
        _call("gkoc_dense_absolute_f32", gexec.stream, n, 1, dx, ld, dy, ld)
        sync()
        got = dy.get()
        assert np.all(got[:, 1:] == np.float32(CANARY))
        assert np.array_equal(got[:, 0], np.abs(x)), np.flatnonzero(got[:, 0] != np.abs(x))[:4]


# ------------------------------------------------------------------------- counts and Dense -> Csr
def _sparse_dense(rng, rows, cols, t):
    x = np.where(rng.uniform(size=(rows, cols)) < 0.35, cr.random_values(rng, rows * cols, t).reshape(rows, cols), 0)
    x = x.astype(t)
    special = [complex(-0.0, 0.0), complex(0.0, -0.0), complex(np.nan, 0), complex(0, np.nan), complex(0, 1e-30),
               complex(-0.0, -0.0)]
    for i, v in enumerate(special):
        if rows:
            x[(3 * i) % rows, (5 * i) % cols] = v
    if rows > 9:
        x[9, :] = 0
    return x


@pytest.mark.parametrize("tn", TN)
def test_count_nonzeros_and_to_csr(gexec, tn):
    """-0.0 + 0i and 0 - 0i count as zero, a NaN as non-zero; the kept values bit for bit in row-major order"""
    t = br.TYPES[tn]
    cols = 17
    for rows in [0, 1, 255, 256, 257, 2049, 100003]:
        x = _sparse_dense(np.random.default_rng(rows), rows, cols, t)
        fx = padded(x, cols + 2)
        dx = Dev(gexec, fx)
        ptrs, wc, wv = vr.dense_to_csr(x)
        for ob, ct in ((4, np.int32), (8, np.int64)):
            out = _out(gexec, rows, ct, fill=-5)
            _call("gkoc_cdense_count_nonzeros_per_row_" + tn, gexec.stream, rows, cols, dx, cols + 2, out, ob)
            sync()
            assert np.array_equal(head_of(out, rows, rows, fill=-5), vr.count_nonzeros_per_row(x).astype(ct))
        assert raises_invalid("gkoc_cdense_count_nonzeros_per_row_" + tn, gexec.stream, rows, cols, dx, cols + 2, out, 2)
        sync()
        assert np.array_equal(out.get()[:rows], vr.count_nonzeros_per_row(x)), "refused call left the output alone"
        for in_, it in IT.items():
            dp = Dev(gexec, ptrs.astype(it))
            oc, ov = _out(gexec, len(wc), it, fill=-5), _out(gexec, len(wc), t)
            _call("gkoc_cdense_to_csr_" + tn + "_" + in_, gexec.stream, rows, cols, dx, cols + 2, dp, oc, ov)
            sync()
            assert np.array_equal(head_of(oc, len(wc), len(wc), fill=-5), wc.astype(it))
            assert same_bits(head_of(ov, len(wc), len(wc), fill=np.nan), wv)
            assert same_bits(dp.get(), ptrs.astype(it))
        assert same_bits(dx.get(), fx)
        if rows > 20:
            c = vr.count_nonzeros_per_row(x)
            assert c[9] == 0 and np.isnan(wv).any() and not np.any((wv.real == 0) & (wv.imag == 0))


# --------------------------------------------------------------------------- gathers and fill-ins
@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_row_gather(gexec, tn, in_):
    """copies of random bit patterns (NaN payloads, -0.0); repeated rows"""
    t, it = br.TYPES[tn], IT[in_]
    cols, n_orig = 3, 5000
    rng = np.random.default_rng(17)
    orig = vr.random_bits(rng, n_orig * (cols + 2), t).reshape(n_orig, cols + 2)
    do = Dev(gexec, orig)
    for n in SIZES:
        rows = rng.integers(0, n_orig, n)
        rows[:min(n, 6)] = [4999, 0, 7, 7, 7, 4999][:min(n, 6)]
        dr = Dev(gexec, rows.astype(it))
        fg = padded(np.full((n, cols), np.nan, t), cols + 3)
        dg = Dev(gexec, fg)
        _call("gkoc_cdense_row_gather_" + tn + "_" + in_, gexec.stream, n, cols, dr, do, cols + 2, dg, cols + 3)
        sync()
        got = dg.get()
        assert canaries_ok(got, cols) and same_bits(dr.get(), rows.astype(it))
        assert same_bits(got[:, :cols], vr.row_gather(rows, orig[:, :cols])), n
    assert same_bits(do.get(), orig)


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", ["c128", "c64", "f64", "f32"])
def test_fill_in_matrix_data(gexec, tn, in_):
    """gkoc_cdense_fill_in_matrix_data_* / gkoc_dense_fill_in_matrix_data_*: out(row, col) = value for triplets
    with distinct positions inside the matrix; every other entry of the target and its padding keep the fill"""
    t, it = br.TYPES[tn], IT[in_]
    name = ("gkoc_cdense_" if br.is_complex(t) else "gkoc_dense_") + "fill_in_matrix_data_" + tn + "_" + in_
    rng = np.random.default_rng(19)
    R, Cc, ld = 700, 300, 303
    for nnz in SIZES:
        pos = rng.choice(R * Cc, nnz, replace=False)
        r, c = pos // Cc, pos % Cc
        assert nnz == 0 or (r.max() < R and c.max() < Cc and r.min() >= 0 and c.min() >= 0)
        vals = vr.random_bits(rng, nnz, t)
        target = padded(np.full((R, Cc), 3.5, t), ld)
        dr, dc, dv, dt = Dev(gexec, r.astype(it)), Dev(gexec, c.astype(it)), Dev(gexec, vals), Dev(gexec, target)
        _call(name, gexec.stream, nnz, dr, dc, dv, dt, ld)
        sync()
        assert same_bits(dt.get(), vr.fill_in_matrix_data(r, c, vals, target)), nnz
        assert same_bits(dr.get(), r.astype(it)) and same_bits(dc.get(), c.astype(it)) and same_bits(dv.get(), vals)


@pytest.mark.parametrize("tn", TN)
def test_add_scaled_identity_real(gexec, tn):
    """m = beta m + alpha I with real scalars: (re beta, im beta), re + alpha on the min(rows, cols) diagonal
    entries - bit-identical to the plain restatement"""
    t, rt = br.TYPES[tn], br.real_of(br.TYPES[tn])
    for rows, cols in [(0, 3), (3, 0), (1, 1), (5, 5), (7, 3), (3, 7), (257, 300), (300, 257), (2049, 5), (100003, 2)]:
        rng = np.random.default_rng(rows * 3 + cols)
        m = cr.random_values(rng, rows * cols, t).reshape(rows, cols)
        fm = padded(m, cols + 2)
        al, be = np.array([0.8125], rt), np.array([-1.7], rt)
        dm, dal, dbe = Dev(gexec, fm), Dev(gexec, al), Dev(gexec, be)
        _call("gkoc_dense_add_scaled_identity_real_" + tn, gexec.stream, rows, cols, dal, dbe, dm, cols + 2)
        sync()
        got = dm.get()
        assert canaries_ok(got, cols) and same_bits(dal.get(), al) and same_bits(dbe.get(), be)
        want = vr.add_scaled_identity_real(br.plain(t), al[0], be[0], m)
        assert same_bits(got[:, :cols], want), (rows, cols)
    assert raises_invalid("gkoc_dense_add_scaled_identity_real_" + tn, gexec.stream, 2, 5, dal, dbe, dm, 4)


@pytest.fixture(scope="module", autouse=True)
def _print_tables():
    """after the last test of this file: the figures its tests gathered (pytest -s)"""
    yield
    if not STATS:
        return
    print("\nlargest observed |kernel - ref| / (eps max|ref|) (rows marked otherwise: that unit)")
    print("| entry point | " + " | ".join(TN) + " |")
    for name in sorted({k[0] for k in STATS}, key=lambda s: s.strip(" .")):
        print("| " + name + " | " + " | ".join("%.2f" % STATS.get((name, tn), float("nan")) for tn in TN) + " |")
