"""The array components and the fused criterion through the C ABI: gkoc_fill_array_{f64,f32,c128,c64,i32,i64},
gkoc_fill_array_small, gkoc_convert_precision_*, gkoc_conj_array_*, gkoc_narrow_i64_to_i32 and
gkoc_x_residual_norm_then_cg_step_1_*.

Fills, conjugation and narrowing move bits: compared bit for bit, NaN payloads included (the fill value travels
by value with its bits intact, binding_gpu.by_value).  Precision conversion equals numpy's astype, which rounds
to nearest even.  The fused criterion must leave exactly what gkoc_residual_norm_* / gkoc_implicit_residual_norm_*
followed by gkoc_cg_step_1_* leave on the same input: both host answers, stop_status, the flag bytes and p.
Every output is followed by canaries; inputs are read back and compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import binding_refs as br
import value_kernel_refs as vr
from binding_gpu import CANARY, Dev, by_value, call as _call, grid_cap_rows as _grid_cap_rows, raises_invalid, \
    same_bits, sync

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 2049, 100003]
FILL_TYPES = {"f64": np.float64, "f32": np.float32, "c128": np.complex128, "c64": np.complex64, "i32": np.int32,
              "i64": np.int64}


def _framed(n, t, inside, frame=5):
    """`frame` canaries, n entries `inside`, `frame` canaries: (array, slice of the n entries)"""
    t = np.dtype(t)
    can = t.type(CANARY) if t.kind in "fc" else t.type(-77)
    a = np.full(n + 2 * frame, can, t)
    a[frame:frame + n] = inside
    return a, slice(frame, frame + n)


def _nan_with_payload(t, payload, negative=False):
    """a quiet NaN of the real type t with the given payload bits"""
    if t == np.float32:
        return np.array([0x7fc00000 | payload | (0x80000000 if negative else 0)], np.uint32).view(np.float32)[0]
    return np.array([0x7ff8000000000000 | payload | (0x8000000000000000 if negative else 0)], np.uint64).view(np.float64)[0]


def _fill_values(tn):
    t = FILL_TYPES[tn]
    if np.dtype(t).kind == "i":
        ii = np.iinfo(t)
        return [t(0), t(-1), t(ii.max), t(ii.min), t(123456789)]
    rt = br.real_of(t)
    reals = [rt(1.5), rt(-0.0), rt(np.inf), np.finfo(rt).smallest_subnormal, _nan_with_payload(rt, 0x1234),
             _nan_with_payload(rt, 0x2bcd, True)]
    if br.is_complex(t):
        out = []
        for i, re in enumerate(reals):
            v = np.zeros(1, t)
            v.real, v.imag = re, reals[(i + 2) % len(reals)]
            out.append(v[0])
        return out
    return reals


@pytest.mark.parametrize("tn", list(FILL_TYPES))
def test_fill_array(gexec, tn):
    t = FILL_TYPES[tn]
    for n in SIZES:
        for k, value in enumerate(_fill_values(tn)):
            if n > 3000 and k > 1:
                continue
            buf, inside = _framed(n, t, 7)
            d = Dev(gexec, buf)
            _call("gkoc_fill_array_" + tn, gexec.stream, d.at(inside.start), n, by_value(value))
            sync()
            want = buf.copy()
            want[inside] = value
            assert same_bits(want[inside], np.full(n, value, t))
            assert same_bits(d.get(), want), (n, value)


@pytest.mark.parametrize("tn", ["f32", "c64", "i32"])
def test_fill_array_beyond_the_grid_cap(gexec, tn):
    """the max_stream_blocks forms of dense.hip (real values: gkoc_dense_fill_*, complex pairs) and formats.hip
    (indices)"""
    t = FILL_TYPES[tn]
    n = _grid_cap_rows() + 257
    buf, inside = _framed(n, t, 7)
    d = Dev(gexec, buf)
    value = _fill_values(tn)[-1]
    _call("gkoc_fill_array_" + tn, gexec.stream, d.at(inside.start), n, by_value(value))
    sync()
    want = buf.copy()
    want[inside] = value
    assert same_bits(d.get(), want)


@pytest.mark.parametrize("elem_bytes", [1, 2, 4])
def test_fill_array_small(gexec, elem_bytes):
    """only the low elem_bytes bytes of the pattern are used"""
    t = {1: np.uint8, 2: np.uint16, 4: np.uint32}[elem_bytes]
    for n in SIZES:
        for pattern in (0xA1B2C3D4, 0x00000001, 0xFFFFFF00):
            buf = np.full(n + 10, 0x5E5E5E5E & np.iinfo(t).max, t)
            d = Dev(gexec, buf)
            _call("gkoc_fill_array_small", gexec.stream, d.at(5), n, elem_bytes, C.c_uint32(pattern))
            sync()
            want = buf.copy()
            want[5:5 + n] = pattern & np.iinfo(t).max
            assert np.array_equal(d.get(), want), (n, hex(pattern))
    before = d.get()
    for bad in (3, 0, 8):
        assert raises_invalid("gkoc_fill_array_small", gexec.stream, d, 4, bad, C.c_uint32(1))
    sync()
    assert np.array_equal(d.get(), before)


def test_fill_array_small_beyond_the_grid_cap(gexec):
    """the grid_of style of misc.hip, on bytes"""
    n = _grid_cap_rows() + 257
    d = Dev(gexec, np.full(n + 10, 0x5E, np.uint8))
    _call("gkoc_fill_array_small", gexec.stream, d.at(5), n, 1, C.c_uint32(0x1C7))
    sync()
    got = d.get()
    assert np.all(got[:5] == 0x5E) and np.all(got[5 + n:] == 0x5E) and np.all(got[5:5 + n] == 0xC7)


# ------------------------------------------------------------------------------ precision conversion
def _conversion_inputs(rng, src, n):
    """values the narrowing can trip on: halfway cases of round to nearest even, the float subnormal range,
    values that overflow to inf, NaN, signed zeros - then random bit patterns"""
    f = np.finfo(np.float32)
    special = np.array([0.0, -0.0, 1.0, 1 + 2.0 ** -24, 1 + 2.0 ** -23 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50,
                        -(1 + 3 * 2.0 ** -24), float(f.max), float(f.max) * (1 + 2.0 ** -25), float(f.max) * (1 + 2.0 ** -24),
                        -float(f.max) * 1.5, 1e300, float(f.tiny), float(f.tiny) / 3, 2.0 ** -149, 2.0 ** -150,
                        2.0 ** -150 * (1 + 2.0 ** -30), -2.0 ** -151, 3 * 2.0 ** -150, 1e-320, np.inf, -np.inf, np.nan])
    with np.errstate(all="ignore"):
        x = np.concatenate([special.astype(src), vr.random_bits(rng, n, src)])[:n]
    return x


@pytest.mark.parametrize("direction", ["f64_f32", "f32_f64"])
def test_convert_precision(gexec, direction):
    src, dst = (np.float64, np.float32) if direction == "f64_f32" else (np.float32, np.float64)
    rng = np.random.default_rng(89)
    for n in SIZES:
        x = _conversion_inputs(rng, src, n)
        buf, inside = _framed(n, dst, np.nan)
        dx, do = Dev(gexec, x), Dev(gexec, buf)
        _call("gkoc_convert_precision_" + direction, gexec.stream, n, dx, do.at(inside.start))
        sync()
        got = do.get()
        with np.errstate(all="ignore"):
            want = x.astype(dst)
        assert same_bits(got[:inside.start], buf[:inside.start]) and same_bits(got[inside.stop:], buf[inside.stop:])
        assert same_bits(dx.get(), x)
        g = got[inside]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(g), nan)
        assert same_bits(np.where(nan, 0, g).astype(dst), np.where(nan, 0, want).astype(dst)), \
            (n, x[~nan][np.flatnonzero(g[~nan] != want[~nan])[:4]])
        if n > 30 and direction == "f64_f32":
            assert np.isinf(want).sum() >= 4 and np.count_nonzero((want != 0) & (np.abs(want) < np.finfo(dst).tiny)) >= 4
            assert np.signbit(g[1]) and g[1] == 0 and g[3] == 1 and g[4] == dst(1 + 2.0 ** -22)


def test_convert_precision_beyond_the_grid_cap(gexec):
    """the grid_of style of misc.hip"""
    n = _grid_cap_rows() + 257
    x = (np.arange(n) % 1001 - 500).astype(np.float32) / 8
    buf, inside = _framed(n, np.float64, np.nan)
    do = Dev(gexec, buf)
    _call("gkoc_convert_precision_f32_f64", gexec.stream, n, Dev(gexec, x), do.at(inside.start))
    sync()
    got = do.get()
    assert same_bits(got[:inside.start], buf[:inside.start]) and same_bits(got[inside.stop:], buf[inside.stop:])
    assert np.array_equal(got[inside], x.astype(np.float64)), np.flatnonzero(got[inside] != x)[:4]


# ----------------------------------------------------------------------------- conj, narrow
@pytest.mark.parametrize("tn", ["c128", "c64"])
def test_conj_array(gexec, tn):
    """the real part untouched, the sign bit of the imaginary part flipped - also for 0 and NaN"""
    t = br.TYPES[tn]
    rng = np.random.default_rng(97)
    rt = br.real_of(t)
    for n in SIZES:
        x = vr.random_bits(rng, n, t)
        if n > 8:
            x[5], x[6] = complex(1.0, 0.0), complex(1.0, -0.0)
            x[7:9].real = 2.0
            x[7:9].imag = [_nan_with_payload(rt, 0x155), _nan_with_payload(rt, 0x2aa, True)]
        buf, inside = _framed(n, t, x)
        d = Dev(gexec, buf)
        _call("gkoc_conj_array_" + tn, gexec.stream, n, d.at(inside.start))
        sync()
        want = buf.copy()
        want[inside] = vr.conj_array(x)
        assert same_bits(d.get(), want), n
        if n > 8:
            assert np.signbit(want[inside][5].imag) and not np.signbit(want[inside][6].imag)
    assert raises_invalid("gkoc_conj_array_" + tn, gexec.stream, 4, None)


def test_conj_array_beyond_the_grid_cap(gexec):
    """the max_stream_blocks form of mixed_precision.hip"""
    n = _grid_cap_rows() + 257
    x = ((np.arange(n) % 7 - 3) + 1j * (np.arange(n) % 5 - 2)).astype(np.complex64)
    buf, inside = _framed(n, np.complex64, x)
    d = Dev(gexec, buf)
    _call("gkoc_conj_array_c64", gexec.stream, n, d.at(inside.start))
    sync()
    want = buf.copy()
    want[inside] = vr.conj_array(x)
    assert same_bits(d.get(), want)


def test_narrow_i64_to_i32(gexec):
    """exact on values within the int32 range, the ends included"""
    rng = np.random.default_rng(101)
    for n in SIZES + [_grid_cap_rows() + 257]:
        x = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64)
        x[:min(n, 4)] = [2 ** 31 - 1, -2 ** 31, 0, -1][:min(n, 4)]
        buf, inside = _framed(n, np.int32, -5)
        dx, do = Dev(gexec, x), Dev(gexec, buf)
        _call("gkoc_narrow_i64_to_i32", gexec.stream, n, dx, do.at(inside.start))
        sync()
        want = buf.copy()
        want[inside] = x.astype(np.int32)
        assert np.array_equal(want[inside].astype(np.int64), x)
        assert np.array_equal(do.get(), want) and np.array_equal(dx.get(), x), n
    assert raises_invalid("gkoc_narrow_i64_to_i32", gexec.stream, 4, None, do)


# --------------------------------------------------------------------- criterion, then cg::step_1
def _step_1(p, z, rho, prev_rho, stop):
    """cg::step_1 of one column: p = z + (rho / prev_rho) p, p = z when prev_rho is 0; nothing when stopped"""
    if stop & 0x3f:
        return p.copy()
    if prev_rho == 0:
        return z.copy()
    return (z + (rho / prev_rho) * p).astype(p.dtype)


FUSED_CASES = {
    # name: (tau, orig_tau, goal, stop before, rho, prev_rho)
    "converges on this call": (1e-9, 2.0, 1e-6, 0, 3.0, 2.0),
    "does not converge": (1e-3, 2.0, 1e-6, 0, 3.0, 2.0),
    "does not converge, prev_rho = 0": (1e-3, 2.0, 1e-6, 0, 3.0, 0.0),
    "had stopped before": (1e-3, 2.0, 1e-6, 0x03, 3.0, 2.0),
    "tau exactly at the goal": (0.5, 2.0, 0.25, 0, -1.5, 0.75),
}


@pytest.mark.parametrize("set_finalized", [0, 1])
@pytest.mark.parametrize("implicit", [0, 1])
@pytest.mark.parametrize("tn", ["f64", "f32"])
def test_criterion_then_cg_step_1(gexec, tn, implicit, set_finalized):
    """the fused call against the criterion followed by gkoc_cg_step_1_* on copies of the same input"""
    t = br.TYPES[tn]
    crit = "gkoc_implicit_residual_norm_" if implicit else "gkoc_residual_norm_"
    for name, (tau, orig, goal, stop0, rho, prev) in FUSED_CASES.items():
        for rows in (0, 1, 257, 100003):
            rng = np.random.default_rng(rows + 103)
            if implicit:
                tau_in = t(tau) ** 2 * (-1 if name == "does not converge" else 1)      # sqrt(|tau|) is compared
            else:
                tau_in = t(tau)
            z, p0 = rng.uniform(-1, 1, rows).astype(t), rng.uniform(-1, 1, rows).astype(t)
            pbuf, inside = _framed(rows, t, p0)
            ins = [np.array([tau_in], t), np.array([orig], t), z, np.array([rho], t), np.array([prev], t)]
            results = []
            for fused in (0, 1):
                dtau, dorig, dz, drho, dprev = (Dev(gexec, a) for a in ins)
                dstop = Dev(gexec, np.array([stop0, 0x55, 0x55, 0x55], np.uint8))
                dflags = Dev(gexec, np.array([0x77, 0x77, 0x77, 0x77], np.uint8))
                dp = Dev(gexec, pbuf)
                allc, chg = C.c_int(-9), C.c_int(-9)
                if fused:
                    _call("gkoc_x_residual_norm_then_cg_step_1_" + tn, gexec.stream, dtau, dorig, by_value(t(goal)),
                          C.c_uint8(5), C.c_int(set_finalized), C.c_int(implicit), dstop, dflags, C.byref(allc),
                          C.byref(chg), rows, dp.at(inside.start), dz, drho, dprev)
                else:
                    _call(crit + tn, gexec.stream, 1, dtau, dorig, by_value(t(goal)), C.c_uint8(5),
                          C.c_int(set_finalized), dstop, dflags, C.byref(allc), C.byref(chg))
                    _call("gkoc_cg_step_1_" + tn, gexec.stream, rows, 1, dp.at(inside.start), 1, dz, 1, drho, dprev, dstop)
                sync()
                for d, a in zip((dtau, dorig, dz, drho, dprev), ins):
                    assert same_bits(d.get(), a), "an input changed"
                results.append((allc.value, chg.value, dstop.get(), dflags.get(), dp.get()))
            sep, fus = results
            assert fus[0] == sep[0] and fus[1] == sep[1], (name, rows, "host answers", sep[:2], fus[:2])
            assert np.array_equal(fus[2], sep[2]) and np.array_equal(fus[3], sep[3]), (name, rows, sep[2:4], fus[2:4])
            assert same_bits(fus[4], sep[4]), (name, rows, "p")
            # and what both must be
            converges = name in ("converges on this call", "tau exactly at the goal")
            stop_after = int(fus[2][0])
            if converges:
                assert stop_after == (0x80 | 5 | (0x40 if set_finalized else 0)) and fus[0] == 1 and fus[1] == 1
            elif stop0:
                assert stop_after == stop0 and fus[0] == 1 and fus[1] == 0
            else:
                assert stop_after == 0 and fus[0] == 0 and fus[1] == 0
            assert np.all(fus[2][1:] == 0x55)
            want = pbuf.copy()
            want[inside] = _step_1(p0, z, t(rho), t(prev), stop_after)
            assert same_bits(fus[4], want), (name, rows)
            if converges or stop0:
                assert same_bits(fus[4], pbuf), "a stopped column keeps p"
    for bad in range(4):
        args = [gexec.stream, dtau, dorig, by_value(t(goal)), C.c_uint8(5), C.c_int(0), C.c_int(0), dstop, dflags,
                C.byref(allc), C.byref(chg), 4, dp, dz, drho, dprev]
        args[12 + bad] = None
        assert raises_invalid("gkoc_x_residual_norm_then_cg_step_1_" + tn, *args)
