"""numpy restatements of the kernels that only the C++ binding calls: idr::{initialize, step_1, step_2,
step_3, compute_omega}, cb_gmres::{restart, arnoldi, solve_krylov} with its storage accessors, and the
dense product (arithmetic of Ginkgo's reference kernels, operand layouts of include/gko_cdna4.h).

Every operation is written once, parametrised by an `Arith(wt, dot)`: the working dtype and the inner
product `dot(a, b) = sum a_i b_i` (no conjugate; callers conjugate).  Two instances matter:

* `hp(T)`: np.longdouble / np.clongdouble, numpy sums - the high-precision reference, the expected value.
* `plain(T)`: the kernel's value type, left-to-right sums - the plain same-precision restatement.  It is
  never an expected value; it sizes tolerances (rule R, `rule_r`): a kernel may miss the reference by four
  times what the plain restatement misses it by, plus 8 eps of the largest reference entry.

Arrays are tight 2-d numpy arrays (the tests cut strided views themselves); nothing here touches a GPU.
tests/test_binding_refs_cpu.py checks these functions against independent formulations."""
import numpy as np

STOPPED = 0x41          # stopping_status with an id set: has_stopped()

REAL_OF = {np.dtype(np.float64): np.float64, np.dtype(np.float32): np.float32,
           np.dtype(np.complex128): np.float64, np.dtype(np.complex64): np.float32}
TYPES = {"f64": np.float64, "f32": np.float32, "c128": np.complex128, "c64": np.complex64}


def is_complex(t):
    return np.dtype(t).kind == "c"


def real_of(t):
    return REAL_OF[np.dtype(t)]


def eps_of(t):
    return float(np.finfo(real_of(t)).eps)


class Arith:
    def __init__(self, wt, dot, name):
        self.wt, self.dot, self.name = wt, dot, name
        self.rt = np.longdouble if wt in (np.longdouble, np.clongdouble) else real_of(wt)

    def a(self, x):
        return np.array(x, dtype=self.wt)

    def cdot(self, a, b):
        """<a, b> = sum a conj(b)"""
        return self.dot(a, np.conj(b))

    def norm(self, a):
        return np.sqrt(self.rt(np.real(self.dot(a, np.conj(a)))))


def _seq_dot(wt):
    def dot(a, b):
        t = (a * b).astype(wt)
        return np.cumsum(t, dtype=wt)[-1] if t.size else wt(0)     # cumsum adds left to right
    return dot


def hp(t):
    wt = np.clongdouble if is_complex(t) else np.longdouble
    return Arith(wt, lambda a, b: wt(np.sum(a * b)) if a.size else wt(0), "hp")


def plain(t):
    wt = np.dtype(t).type
    return Arith(wt, _seq_dot(wt), "plain")


def rule_r(kernel, ref, plain_v, t, extra=0.0):
    """rule R: |kernel - ref| <= 4 max|plain - ref| + 8 eps(T) max|ref| (+ extra); returns
    (ok, largest |kernel - ref| / (eps max|ref|)) for one output array"""
    ref = np.asarray(ref)
    k = np.asarray(kernel).astype(ref.dtype)
    p = np.asarray(plain_v).astype(ref.dtype)
    if ref.size == 0:
        return True, 0.0
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(k - ref)))
    bound = 4 * float(np.max(np.abs(p - ref))) + 8 * eps_of(t) * scale + extra
    return err <= bound, err / (eps_of(t) * scale) if scale > 0 else err


class Exact:
    """watches the intermediates of an exact case: all (Gaussian) integers of magnitude below 2^24, so the
    operation gives the same values in float and double in any summation order"""

    def __init__(self):
        self.largest = 0.0

    def see(self, v):
        v = np.atleast_1d(np.asarray(v))
        assert np.all(np.isfinite(v)), "non-finite intermediate in an exact case"
        assert np.all(v.real == np.round(v.real)) and np.all(v.imag == np.round(v.imag)), \
            "non-integral intermediate in an exact case"
        if v.size:
            self.largest = max(self.largest, float(np.max(np.abs(v.real))), float(np.max(np.abs(v.imag))))
        assert self.largest < 2 ** 24, self.largest


class _NoWatch:
    def see(self, v):
        pass


def _div(a, b):
    """a / b for scalars; by a complex b with zero imaginary part component-wise, as Smith's quotient gives
    it (numpy multiplies by a rounded reciprocal there, which is not exact on integers)"""
    if np.iscomplexobj(b) and b.imag == 0:
        a = np.asarray(a)
        return a.dtype.type(a.real / b.real) + a.dtype.type(1j) * (a.imag / b.real) if np.iscomplexobj(a) \
            else a / b.real
    return a / b


def div_by_real(v, r):
    """complex or real v / real r, component-wise (what the kernels do; numpy would form a complex quotient)"""
    v = np.asarray(v)
    if np.iscomplexobj(v):
        out = np.empty(v.shape, v.dtype)
        out.real, out.imag = v.real / r, v.imag / r
        return out
    return v / r


def _active(stop, i):
    return stop is None or not (int(stop[i]) & 0x3f)


# ------------------------------------------------------------------------------------------------ IDR
def idr_initialize(ar, p, s, nrhs):
    """m (s x s nrhs), orthonormalised p (s x n), stop (nrhs)"""
    p = ar.a(p).copy()
    m = np.zeros((s, s * nrhs), ar.wt)
    for r in range(s):
        for i in range(nrhs):
            m[r, r * nrhs + i] = 1
    for r in range(p.shape[0]):
        for i in range(r):
            d = ar.cdot(p[r], p[i])
            p[r] = p[r] - d * p[i]
        p[r] = p[r] / ar.norm(p[r])
    return m, p, np.zeros(nrhs, np.uint8)


def idr_step_1(ar, k, m, f, residual, g, c, v, stop=None, watch=None):
    w = watch or _NoWatch()
    m, f, residual, g = (ar.a(z) for z in (m, f, residual, g))
    c, v = ar.a(c).copy(), ar.a(v).copy()
    s, nrhs = f.shape
    for i in range(nrhs):
        if not _active(stop, i):
            continue
        for row in range(s):
            temp = f[row, i]
            for col in range(row):
                temp = temp - m[row, col * nrhs + i] * c[col, i]
                w.see(temp)
            c[row, i] = _div(temp, m[row, row * nrhs + i])
            w.see(c[row, i])
        temp = residual[:, i].copy()
        for j in range(k, s):
            temp = temp - c[j, i] * g[:, j * nrhs + i]
            w.see(temp)
        v[:, i] = temp
    return c, v


def idr_step_2(ar, k, omega, pv, c, u, stop=None, watch=None):
    w = watch or _NoWatch()
    omega, pv, c = (ar.a(z) for z in (omega, pv, c))
    u = ar.a(u).copy()
    s, nrhs = c.shape
    for i in range(nrhs):
        if not _active(stop, i):
            continue
        temp = omega[i] * pv[:, i]
        w.see(temp)
        for j in range(k, s):
            temp = temp + c[j, i] * u[:, j * nrhs + i]
            w.see(temp)
        u[:, k * nrhs + i] = temp
    return u


def idr_step_3(ar, k, p, g, g_k, u, m, f, residual, x, stop=None, watch=None):
    """returns dict(g, g_k, u, m, f, residual, x)"""
    w = watch or _NoWatch()
    p = ar.a(p)
    g, g_k, u, m, f, residual, x = (ar.a(z).copy() for z in (g, g_k, u, m, f, residual, x))
    s, nrhs = f.shape
    for i in range(nrhs):
        if not _active(stop, i):
            continue
        for j in range(k):
            alpha = _div(ar.dot(p[j], g_k[:, i]), m[j, j * nrhs + i])
            w.see(alpha)
            g_k[:, i] = g_k[:, i] - alpha * g[:, j * nrhs + i]
            u[:, k * nrhs + i] = u[:, k * nrhs + i] - alpha * u[:, j * nrhs + i]
            w.see(g_k[:, i])
            w.see(u[:, k * nrhs + i])
        g[:, k * nrhs + i] = g_k[:, i]
        for j in range(k, s):
            m[j, k * nrhs + i] = ar.dot(p[j], g[:, k * nrhs + i])
            w.see(m[j, k * nrhs + i])
        beta = _div(f[k, i], m[k, k * nrhs + i])
        w.see(beta)
        residual[:, i] = residual[:, i] - beta * g[:, k * nrhs + i]
        x[:, i] = x[:, i] + beta * u[:, k * nrhs + i]
        w.see(residual[:, i])
        w.see(x[:, i])
        if k + 1 < s:
            f[k, i] = 0
            for j in range(k + 1, s):
                f[j, i] = f[j, i] - beta * m[j, k * nrhs + i]
                w.see(f[j, i])
    return dict(g=g, g_k=g_k, u=u, m=m, f=f, residual=residual, x=x)


def idr_compute_omega(ar, kappa, tht, residual_norm, omega, stop=None):
    tht, omega = ar.a(tht), ar.a(omega).copy()
    rn = np.array(residual_norm, dtype=ar.rt)
    kappa = ar.rt(kappa)
    for i in range(omega.shape[0]):
        if not _active(stop, i):
            continue
        thr = omega[i]
        omega[i] = omega[i] / tht[i]
        absrho = np.abs(thr / (np.sqrt(ar.rt(np.real(tht[i]))) * rn[i]))
        if absrho < kappa:
            omega[i] = omega[i] * (kappa / absrho)
    return omega


def idr_exact_step3_case(rng, t, n, s, k, nrhs):
    """integer-valued inputs of step_3 with beta = 3: rows of p hold six entries +-1, one of them on an edge
    row of the two-level reduction; returns the inputs (value type t) and the long-double result, whose
    intermediates the reference itself checks to be integral and small"""
    cx = is_complex(t)

    def ints(shape, lo=-2, hi=3):
        v = rng.integers(lo, hi, shape).astype(np.float64)
        return (v + 1j * rng.integers(lo, hi, shape)).astype(t) if cx else v.astype(t)
    edges = [r for r in (0, 255, 256, 1023, 1024, n - 1025, n - 2, n - 1) if 0 <= r < n]
    p = np.zeros((s, n), t)
    for j in range(s):
        rows = rng.choice(n, min(5, n), replace=False)
        p[j, rows] = rng.choice([-1, 1], rows.size)
        p[j, edges[(j + k) % len(edges)]] = 1
    g, u, g_k = ints((n, s * nrhs)), ints((n, s * nrhs)), ints((n, nrhs))
    residual, x = ints((n, nrhs)), ints((n, nrhs))
    m = np.zeros((s, s * nrhs), t)
    for j in range(s):
        m[j, j * nrhs:(j + 1) * nrhs] = 1
    f = ints((s, nrhs), -3, 4)
    with np.errstate(all="ignore"):          # (m_kk may still be zero here)
        ref = idr_step_3(hp(t), k, p, g, g_k, u, m, f, residual, x)
    # m_kk must be a non-zero REAL integer (a complex quotient by a + 0 i is exact in every implementation):
    # shift g_k on a row that only p_k touches, which moves m_kk and none of the alphas
    own = np.flatnonzero((p[k] != 0) & (np.count_nonzero(p[:k], axis=0) == 0))
    if own.size:
        for i in range(nrhs):
            mkk = ref["m"][k, k * nrhs + i]
            delta = -1j * mkk.imag + (1 if mkk.real == 0 else 0)
            g_k[own[0], i] += t(p[k, own[0]] * delta) if cx else t(p[k, own[0]].real * delta.real)
    ref = idr_step_3(hp(t), k, p, g, g_k, u, m, f, residual, x)
    mkk = ref["m"][k, k * nrhs:(k + 1) * nrhs]
    assert np.all(mkk.imag == 0) and np.all(mkk.real != 0), "exact case: m_kk is not a non-zero real integer"
    f[k] = (3 * mkk).astype(t)
    watch = Exact()
    ref = idr_step_3(hp(t), k, p, g, g_k, u, m, f, residual, x, watch=watch)
    return dict(p=p, g=g, g_k=g_k, u=u, m=m, f=f, residual=residual, x=x), ref, watch.largest


def idr_rounding_case(rng, t, n, s, k, nrhs):
    """well-conditioned random inputs of the three steps: orthonormal rows of p, 0.5 <= |m_jj| <= 2"""
    cx = is_complex(t)

    def rnd(shape):
        v = rng.standard_normal(shape)
        return (v + 1j * rng.standard_normal(shape)).astype(t) if cx else v.astype(t)
    q, _ = np.linalg.qr(rnd((n, s)).astype(np.complex128 if cx else np.float64))
    p = np.conj(q.T).copy()                      # rows orthonormal; p g = (p q) L = L (no conjugate in the dots)
    low = np.eye(s) + 0.3 * np.tril(rng.standard_normal((s, s)), -1)
    g1 = q @ low                                 # <p_j, g_j> = 1, <p_j, g_b> = 0 for b > j
    g = np.repeat(g1, nrhs, axis=1) + 0.01 * rnd((n, s * nrhs)) / np.sqrt(n)
    g_k = q[:, k][:, None] + rnd((n, nrhs)) / np.sqrt(n) + q[:, :k] @ rnd((k, nrhs))
    u = rnd((n, s * nrhs))
    m = np.zeros((s, s * nrhs), np.complex128 if cx else np.float64)
    for i in range(nrhs):
        for a in range(s):
            for b in range(a + 1):
                m[a, b * nrhs + i] = p[a] @ g[:, b * nrhs + i]
    d = dict(p=p, g=g, g_k=g_k, u=u, m=m, f=rnd((s, nrhs)), residual=rnd((n, nrhs)), x=rnd((n, nrhs)),
             c=rnd((s, nrhs)), v=rnd((n, nrhs)), omega=rnd((nrhs,)), pv=rnd((n, nrhs)))
    return {key: np.ascontiguousarray(v).astype(t) for key, v in d.items()}


# ------------------------------------------------------------------------------- CB-GMRES: storage
KEEP, F32, F16, I64, I32, I16 = range(6)
KIND_NAMES = {KEEP: "keep", F32: "f32", F16: "f16", I64: "i64", I32: "i32", I16: "i16"}
_INT_OF = {I64: np.int64, I32: np.int32, I16: np.int16}


def f32_to_half(x):
    """gko::half from float: round to nearest even, results below the normal half range -> signed zero"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    small = np.abs(x) < np.float32(2.0 ** -14)
    return np.where(small, np.copysign(np.float16(0), x).astype(np.float16), h).astype(np.float16)


def half_to_f32(h):
    """subnormal halves read as signed zero"""
    h = np.asarray(h, np.float16)
    bits = h.view(np.uint16)
    sub = (bits & 0x7c00) == 0
    return np.where(sub, np.copysign(np.float32(0), h.astype(np.float32)), h.astype(np.float32)).astype(np.float32)


def f32_to_half_bits_by_hand(x):
    """the same conversion written on the bit patterns (the independent formulation of the CPU test)"""
    f = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    sign = (f >> 16) & 0x8000
    e = (f >> 23) & 0xff
    m = f & 0x7fffff
    res = sign | ((np.maximum(e, 113) - 112) << 10) | (m >> 13)
    tail = m & 0x1fff
    res = res + ((tail > 0x1000) | ((tail == 0x1000) & ((res & 1) == 1))).astype(np.uint64)
    res = np.where(e >= 143, sign | 0x7c00, res)
    res = np.where(e <= 112, sign, res)
    res = np.where(e == 0xff, sign | 0x7c00 | np.where(m != 0, 0x3ff, 0).astype(np.uint64), res)
    return res.astype(np.uint16)


def storage_dtype(kind, t):
    if kind == KEEP:
        return np.dtype(t).type
    if kind == F32:
        return np.complex64 if is_complex(t) else np.float32
    if kind == F16:
        return np.float16
    return _INT_OF[kind]


def correction(kind):
    return 2.0 / float(np.iinfo(_INT_OF[kind]).max) if kind >= I64 else 1.0


def quantum(kind, t, scalar=None):
    """what one rounding or truncation of a stored entry can move it by, relative to entries of size one"""
    if kind >= I64:
        return float(abs(scalar))
    return float(np.finfo(real_of(t) if kind == KEEP else (np.float32 if kind == F32 else np.float16)).eps)


def store(kind, t, v, scalar=None):
    """value -> storage; v in any working type (the division of the integer kinds is done in v's type)"""
    v = np.asarray(v)
    if kind == KEEP:
        return v.astype(t)
    if kind == F32:
        return v.astype(np.complex64 if is_complex(t) else np.float32)
    if kind == F16:
        return f32_to_half(v.astype(np.float32))
    q = np.trunc(v / np.asarray(scalar, v.dtype))
    return q.astype(_INT_OF[kind])


def load(kind, st, wt, scalar=None):
    if kind == F16:
        return half_to_f32(st).astype(wt)
    if kind >= I64:
        return st.astype(wt) * np.asarray(scalar, wt)
    return st.astype(wt)


# ------------------------------------------------------------------------------ CB-GMRES: the steps
class CbGmres:
    """state of one CB-GMRES cycle in the arithmetic `ar`, basis stored through `kind` for value type t.
    bases: (krylov_dim + 1, rows, nrhs) storage values, scalars (krylov_dim + 1, nrhs), hess[it] the rotated
    Hessenberg column of step it ((it + 2) x nrhs), hess_raw[it] the same before the rotations."""

    def __init__(self, ar, t, kind, rows, nrhs, krylov_dim, rounds=3):
        self.ar, self.t, self.kind, self.rounds = ar, t, kind, rounds
        self.rows, self.nrhs, self.kd = rows, nrhs, krylov_dim
        self.bases = np.zeros((krylov_dim + 1, rows, nrhs), storage_dtype(kind, t))
        self.scalars = np.ones((krylov_dim + 1, nrhs), ar.rt)
        self.gsin = np.zeros((krylov_dim, nrhs), ar.wt)
        self.gcos = np.zeros((krylov_dim, nrhs), ar.wt)
        self.rnc = np.zeros((krylov_dim + 1, nrhs), ar.wt)
        self.residual_norm = np.zeros(nrhs, ar.rt)
        self.an = np.zeros((3, nrhs), ar.rt)
        self.fin = np.zeros(nrhs, np.uint64)
        self.hess, self.hess_raw = {}, {}
        self.rounds_taken = np.zeros(nrhs, int)

    def basis(self, k, c):
        return load(self.kind, self.bases[k, :, c], self.ar.wt, self.scalars[k, c])

    def sync_from(self, bases, scalars, gsin, gcos, rnc, fin):
        """take over a state (another run's or the kernel's): the stored basis bit for bit, the rest converted
        to this arithmetic - so that the next step starts from identical inputs"""
        self.bases[:] = bases
        if scalars is not None:
            self.scalars[:] = scalars
        self.gsin[:], self.gcos[:], self.rnc[:] = gsin, gcos, rnc
        self.fin[:] = fin

    def restart(self, residual):
        ar, corr = self.ar, correction(self.kind)
        residual = ar.a(residual)
        nxt = np.zeros((self.rows, self.nrhs), ar.wt)
        self.bases[:] = 0
        self.rnc[:] = 0
        self.scalars[:] = ar.rt(corr)
        for c in range(self.nrhs):
            rn = ar.norm(residual[:, c])
            self.residual_norm[c] = rn
            self.rnc[0, c] = rn
            if self.kind >= I64:
                self.an[2, c] = np.max(np.abs(residual[:, c])) if self.rows else 0
                self.scalars[0, c] = self.an[2, c] / rn * ar.rt(corr)
            nxt[:, c] = div_by_real(residual[:, c], rn)
            self.bases[0, :, c] = store(self.kind, self.t, nxt[:, c], self.scalars[0, c])
        self.fin[:] = 0
        return nxt

    def arnoldi(self, it, nxt, stop=None):
        ar = self.ar
        nxt = ar.a(nxt).copy()
        eta = ar.rt(1) / np.sqrt(ar.rt(2))
        h = np.zeros((it + 2, self.nrhs), ar.wt)
        for c in range(self.nrhs):
            if not _active(stop, c):
                continue
            self.fin[c] += 1
            v = nxt[:, c]
            bs = [self.basis(k, c) for k in range(it + 1)]
            an0 = eta * ar.norm(v)
            for k in range(it + 1):
                h[k, c] = ar.cdot(v, bs[k])
            for k in range(it + 1):
                v = v - h[k, c] * bs[k]
            an1, an2 = ar.norm(v), (np.max(np.abs(v)) if v.size else ar.rt(0))
            rounds = 1
            while an1 < an0 and rounds < self.rounds:
                an0 = eta * an1
                b = [ar.cdot(v, bs[k]) for k in range(it + 1)]
                for k in range(it + 1):
                    v = v - b[k] * bs[k]
                    h[k, c] = h[k, c] + b[k]
                an1, an2 = ar.norm(v), np.max(np.abs(v))
                rounds += 1
            self.rounds_taken[c] = rounds
            self.an[:, c] = (an0, an1, an2)
            if self.kind >= I64:
                self.scalars[it + 1, c] = an2 / an1 * ar.rt(correction(self.kind))
            h[it + 1, c] = an1
            v = div_by_real(v, an1)
            nxt[:, c] = v
            self.bases[it + 1, :, c] = store(self.kind, self.t, v, self.scalars[it + 1, c])
        self.hess_raw[it] = h.copy()
        self.hess[it] = self.givens(it, h, stop)
        return nxt

    def givens(self, it, h, stop=None):
        ar = self.ar
        h = h.copy()
        for c in range(self.nrhs):
            if not _active(stop, c):
                continue
            for j in range(it):
                cs, sn = self.gcos[j, c], self.gsin[j, c]
                hj, hj1 = h[j, c], h[j + 1, c]
                h[j, c] = cs * hj + sn * hj1
                h[j + 1, c] = -np.conj(sn) * hj + np.conj(cs) * hj1
            this_h, next_h = h[it, c], h[it + 1, c]
            if this_h == 0:
                cs, sn = ar.wt(0), ar.wt(1)
            else:
                scale = np.abs(this_h) + np.abs(next_h)
                a, b = np.abs(this_h / scale), np.abs(next_h / scale)
                hyp = scale * np.sqrt(a * a + b * b)
                cs, sn = np.conj(this_h) / hyp, np.conj(next_h) / hyp
            self.gcos[it, c], self.gsin[it, c] = cs, sn
            h[it, c] = cs * this_h + sn * next_h
            h[it + 1, c] = 0
            r = self.rnc[it, c]
            self.rnc[it + 1, c] = -np.conj(sn) * r
            self.rnc[it, c] = cs * r
            self.residual_norm[c] = np.abs(self.rnc[it + 1, c])
        return h

    def solve_krylov(self, fin=None):
        """y (krylov_dim x nrhs) and before_preconditioner (rows x nrhs) from the rotated Hessenberg columns"""
        ar = self.ar
        fin = self.fin if fin is None else fin
        y = np.zeros((self.kd, self.nrhs), ar.wt)
        out = np.zeros((self.rows, self.nrhs), ar.wt)
        for c in range(self.nrhs):
            mm = int(fin[c])
            for i in range(mm - 1, -1, -1):
                temp = self.rnc[i, c]
                for j in range(i + 1, mm):
                    temp = temp - self.hess[j][i, c] * y[j, c]
                y[i, c] = temp / self.hess[i][i, c]
            for k in range(mm):
                out[:, c] = out[:, c] + self.basis(k, c) * y[k, c]
        return y, out


def unrotate(col, gcos, gsin, it):
    """the Hessenberg column of step `it` before its Givens rotations, from the rotated column ((it + 2)
    entries, the last one zero) and the rotations 0 .. it"""
    h = np.array(col).copy()
    for j in range(it, -1, -1):
        cs, sn = gcos[j], gsin[j]
        a, b = h[j], h[j + 1]
        h[j] = np.conj(cs) * a - sn * b
        h[j + 1] = np.conj(sn) * a + cs * b
    return h


def solve_upper(ar, h, rhs):
    """back substitution on an upper triangular h (mm x mm), left to right in the row"""
    h, rhs = ar.a(h), ar.a(rhs)
    mm = rhs.shape[0]
    y = np.zeros(mm, ar.wt)
    for i in range(mm - 1, -1, -1):
        temp = rhs[i]
        for j in range(i + 1, mm):
            temp = temp - h[i, j] * y[j]
        y[i] = temp / h[i, i]
    return y


# ----------------------------------------------------------------------------------------------- GEMM
def _mul(ar, x, y):
    """x * y; complex value types: the textbook product, every real operation rounded on its own"""
    if np.iscomplexobj(x) and ar.wt not in (np.clongdouble,):
        x, y = np.asarray(x, ar.wt), np.asarray(y, ar.wt)
        re = (x.real * y.real).astype(ar.rt) - (x.imag * y.imag).astype(ar.rt)
        im = (x.real * y.imag).astype(ar.rt) + (x.imag * y.real).astype(ar.rt)
        out = np.empty(np.broadcast(x, y).shape, ar.wt)
        out.real, out.imag = re, im
        return out
    return (x * y).astype(ar.wt)


def gemm(ar, a, b, c=None, alpha=None, beta=None):
    """c = a b (alpha is None) or (beta c if beta != 0 else 0) + sum_k (alpha a) b: terms added left to right,
    multiply and add rounded separately"""
    a, b = ar.a(a), ar.a(b)
    mm, kk = a.shape
    nn = b.shape[1]
    if alpha is None:
        out = np.zeros((mm, nn), ar.wt)
    else:
        alpha, beta = ar.wt(alpha), ar.wt(beta)
        out = _mul(ar, ar.a(c), beta) if beta != 0 else np.zeros((mm, nn), ar.wt)
        a = _mul(ar, alpha, a)
    for k in range(kk):
        out = (out + _mul(ar, a[:, k:k + 1], b[k:k + 1, :])).astype(ar.wt)
    return out


# ------------------------------------------------------------------------------------ whole solvers
def idr_solve(ar, matvec, b, p, s, tol, max_iters, kappa=0.7):
    """IDR(s) as core/solver/idr.cpp drives the five kernels (identity preconditioner, no smoothing), one
    right-hand side; p: the shadow vectors handed to initialize (deterministic).  Returns x and the number
    of iterations after which ||b - A x|| <= tol ||b|| held (recurrence residual), or max_iters"""
    b = ar.a(b).reshape(-1, 1)
    n = b.shape[0]
    m, p, stop = idr_initialize(ar, p, s, 1)
    x = np.zeros((n, 1), ar.wt)
    r = b.copy()
    g, u = np.zeros((n, s), ar.wt), np.zeros((n, s), ar.wt)
    c, v = np.zeros((s, 1), ar.wt), np.zeros((n, 1), ar.wt)
    omega = np.ones(1, ar.wt)
    bn = ar.norm(b[:, 0])
    iters = 0
    while iters < max_iters:
        f = np.array([[ar.dot(p[j], r[:, 0])] for j in range(s)], ar.wt)
        for k in range(s):
            c, v = idr_step_1(ar, k, m, f, r, g, c, v)
            u = idr_step_2(ar, k, omega, v, c, u)
            g_k = matvec(u[:, k]).reshape(-1, 1)
            o = idr_step_3(ar, k, p, g, g_k, u, m, f, r, x)
            g, u, m, f, r, x = o["g"], o["u"], o["m"], o["f"], o["residual"], o["x"]
            iters += 1
            if ar.norm(r[:, 0]) <= tol * bn:
                return x[:, 0], iters
        t = matvec(r[:, 0])
        omega = np.array([ar.cdot(r[:, 0], t)], ar.wt)        # t^H r
        tht = np.array([ar.cdot(t, t)], ar.wt)
        omega = idr_compute_omega(ar, kappa, tht, [ar.norm(r[:, 0])], omega)
        x[:, 0] = x[:, 0] + omega[0] * r[:, 0]
        r[:, 0] = r[:, 0] - omega[0] * t
        iters += 1
        if ar.norm(r[:, 0]) <= tol * bn:
            return x[:, 0], iters
    return x[:, 0], iters


def cb_gmres_solve(ar, t, kind, matvec, b, krylov_dim, tol, max_cycles):
    """CB-GMRES(krylov_dim), one right-hand side, identity preconditioner.  Stops when the true residual
    (computed in `ar` at the end of a cycle, or the recurrence's estimate inside one, then confirmed)
    reaches tol ||b||; returns x, iterations, the smallest relative true residual seen at a cycle's end"""
    b = ar.a(b)
    n = b.shape[0]
    x = np.zeros(n, ar.wt)
    bn = ar.norm(b)
    iters, best = 0, float("inf")
    for _ in range(max_cycles):
        r = b - matvec(x)
        rel = float(ar.norm(r) / bn)
        best = min(best, rel)
        if rel <= tol:
            break
        st = CbGmres(ar, t, kind, n, 1, krylov_dim)
        nxt = st.restart(r.reshape(-1, 1))
        for it in range(krylov_dim):
            nxt = st.arnoldi(it, matvec(nxt[:, 0]).reshape(-1, 1))
            iters += 1
            if float(st.residual_norm[0] / bn) <= tol:
                break
        _, dx = st.solve_krylov()
        x = x + dx[:, 0]
    else:
        r = b - matvec(x)
        best = min(best, float(ar.norm(r) / bn))
    return x, iters, best


def model_matrices(grid=12):
    """the 3-d 7-point stencil on grid^3 points and a nonsymmetric convection-diffusion variant of it
    (scipy CSR, float64)"""
    import scipy.sparse as sp
    e = np.ones(grid)
    d1 = sp.diags([-e[:-1], 2 * e, -e[:-1]], [-1, 0, 1])
    c1 = sp.diags([-e[:-1], e[:-1]], [-1, 1])
    eye = sp.identity(grid)
    lap = sp.kron(sp.kron(d1, eye), eye) + sp.kron(sp.kron(eye, d1), eye) + sp.kron(sp.kron(eye, eye), d1)
    conv = sp.kron(sp.kron(c1, eye), eye) + 0.5 * sp.kron(sp.kron(eye, c1), eye)
    return {"stencil7": sp.csr_matrix(lap), "convdiff": sp.csr_matrix(lap + 0.4 * conv)}


# ------------------------------------------------------------------- properties of a CB-GMRES state
def _wide(t):
    return np.clongdouble if is_complex(t) else np.longdouble


def decompressed(st, k, c):
    return load(st.kind, st.bases[k, :, c], _wide(st.t), np.longdouble(st.scalars[k, c]))


def orth_defect(st, new, c):
    """max_j |<basis_j, basis_new>|, j < new, of the decompressed basis (long double)"""
    v = decompressed(st, new, c)
    return max(float(np.abs(np.sum(decompressed(st, j, c) * np.conj(v)))) for j in range(new))


def norm_defect(st, new, c):
    v = decompressed(st, new, c)
    return abs(float(np.sqrt(np.sum(np.abs(v) ** 2))) - 1.0)


def reorth_case(rng, t, rows, nb):
    """nb orthonormal basis vectors (nb x rows, value type t) and a next_krylov = sum_k a_k basis_k + 1e-6 w
    with w a unit vector orthogonal to them: one Gram-Schmidt round leaves a result that is far from
    orthogonal, so the kernel has to take the second round"""
    cx = is_complex(t)
    z = rng.standard_normal((rows, nb + 1))
    if cx:
        z = z + 1j * rng.standard_normal((rows, nb + 1))
    q, _ = np.linalg.qr(z)
    a = rng.uniform(0.5, 1.5, nb)
    nxt = q[:, :nb] @ a + 1e-6 * q[:, nb]
    return np.ascontiguousarray(q[:, :nb].T).astype(t), nxt.astype(t)
