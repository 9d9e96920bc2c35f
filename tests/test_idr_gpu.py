"""idr::{initialize, step_1, step_2, step_3, compute_omega} (csrc/idr.hip) through the C ABI against the
numpy references of binding_refs.py, for double, float, complex<double>, complex<float>.

Exact cases: integer-valued inputs whose every intermediate is a small (Gaussian) integer - the long-double
reference checks that itself - so the kernel must return the same numbers, bit for bit, whatever its
summation order; each row of p has an entry on an edge row of the two-level reduction (0, 255, 256, 1023,
1024, n-1025, n-2, n-1), so a dropped tail or chunk boundary changes an integer.  Rounding cases: well
conditioned random inputs, rule R (binding_refs.rule_r): |kernel - ref| <= 4 max|plain - ref| + 8 eps
max|ref| per output array, `plain` being the left-to-right restatement in the value type.  The largest
observed |kernel - ref| / (eps max|ref|) per kernel and type is printed by the last test."""
import ctypes as C

import numpy as np
import pytest

import binding_refs as br
from binding_gpu import CANARY, Dev, padded, same_bits, sync

pytestmark = pytest.mark.gpu

TN = ["f64", "f32", "c128", "c64"]
RATIOS = {}


def _call(name, *args):
    from ginkgo_amd._lib import call
    call(name, *args)


def _note(kernel, tn, ratio):
    RATIOS[(kernel, tn)] = max(RATIOS.get((kernel, tn), 0.0), ratio)


def _real(tn, v):
    return C.c_double(v) if tn in ("f64", "c128") else C.c_float(v)


class Bufs:
    """the operands of one call on the device: 2-d arrays with row stride cols + pad (canary in the padding),
    1-d arrays as they are"""

    def __init__(self, gexec, pad, **arrs):
        self.pad, self.cols, self.dev = pad, {}, {}
        for name, a in arrs.items():
            if a.ndim == 2:
                self.cols[name] = a.shape[1]
                a = padded(a, a.shape[1] + pad)
            self.dev[name] = Dev(gexec, a)

    def __getitem__(self, name):
        return self.dev[name]

    def ld(self, name):
        return self.cols[name] + self.pad

    def get(self, name):
        full = self.dev[name].get()
        if name not in self.cols:
            return full
        assert np.all(full[:, self.cols[name]:] == full.dtype.type(CANARY)), name + ": padding overwritten"
        return np.ascontiguousarray(full[:, :self.cols[name]])


def _step_1(gexec, tn, k, d, stop, pad):
    b = Bufs(gexec, pad, m=d["m"], f=d["f"], residual=d["residual"], g=d["g"], c=d["c"], v=d["v"], stop=stop)
    s, nrhs = d["f"].shape
    _call("gkoc_idr_step_1_" + tn, gexec.stream, d["g"].shape[0], nrhs, s, k, b["m"], b.ld("m"), b["f"],
          b.ld("f"), b["residual"], b.ld("residual"), b["g"], b.ld("g"), b["c"], b.ld("c"), b["v"], b.ld("v"),
          b["stop"])
    sync()
    for name in ("m", "f", "residual", "g"):
        assert same_bits(b.get(name), d[name]), name + " is an input"
    return dict(c=b.get("c"), v=b.get("v"))


def _step_2(gexec, tn, k, d, stop, pad):
    b = Bufs(gexec, pad, omega=d["omega"], pv=d["pv"], c=d["c"], u=d["u"], stop=stop)
    s, nrhs = d["c"].shape
    _call("gkoc_idr_step_2_" + tn, gexec.stream, d["u"].shape[0], nrhs, s, k, b["omega"], b["pv"], b.ld("pv"),
          b["c"], b.ld("c"), b["u"], b.ld("u"), b["stop"])
    sync()
    return dict(u=b.get("u"))


S3 = ("g", "g_k", "u", "m", "f", "residual", "x")


def _step_3(gexec, tn, k, d, stop, pad):
    b = Bufs(gexec, pad, p=d["p"], stop=stop, **{name: d[name] for name in S3})
    s, nrhs = d["f"].shape
    _call("gkoc_idr_step_3_" + tn, gexec.stream, d["g"].shape[0], nrhs, s, k, b["p"], b.ld("p"), b["g"],
          b.ld("g"), b["g_k"], b.ld("g_k"), b["u"], b.ld("u"), b["m"], b.ld("m"), b["f"], b.ld("f"),
          b["residual"], b.ld("residual"), b["x"], b.ld("x"), b["stop"])
    sync()
    assert same_bits(b.get("p"), d["p"])
    return {name: b.get(name) for name in S3}


def _ints(rng, t, shape, lo=-2, hi=3):
    v = rng.integers(lo, hi, shape).astype(np.float64)
    return (v + 1j * rng.integers(lo, hi, shape)).astype(t) if br.is_complex(t) else v.astype(t)


def _exact_inputs(rng, t, n, s, k, nrhs):
    """step_3's exact case plus integer inputs for step_1 (unit lower triangular m1) and step_2"""
    case, ref3, largest = br.idr_exact_step3_case(rng, t, n, s, k, nrhs)
    m1 = np.zeros((s, s * nrhs), t)
    for i in range(nrhs):
        low = np.tril(rng.integers(-1, 2, (s, s)), -1) + np.eye(s)
        m1[:, i::nrhs] = low
    d1 = dict(m=m1, f=_ints(rng, t, (s, nrhs)), residual=case["residual"], g=case["g"],
              c=_ints(rng, t, (s, nrhs)), v=_ints(rng, t, (n, nrhs)))
    w1 = br.Exact()
    c, v = br.idr_step_1(br.hp(t), k, d1["m"], d1["f"], d1["residual"], d1["g"], d1["c"], d1["v"], watch=w1)
    d2 = dict(omega=_ints(rng, t, (nrhs,), 1, 4), pv=_ints(rng, t, (n, nrhs)), c=c.astype(t), u=case["u"])
    w2 = br.Exact()
    u = br.idr_step_2(br.hp(t), k, d2["omega"], d2["pv"], d2["c"], d2["u"], watch=w2)
    print(f"exact case n={n} s={s} k={k} nrhs={nrhs}: largest intermediate step_1 {w1.largest:g} "
          f"step_2 {w2.largest:g} step_3 {largest:g}")
    return d1, dict(c=c, v=v), d2, dict(u=u), case, ref3


EXACT = ([(1000, 4, k, 3, 3) for k in range(4)] + [(1025, 8, k, 1, 0) for k in (0, 3, 7)] +
         [(1, 1, 0, 1, 3), (1, 1, 0, 3, 0), (255, 1, 0, 3, 0), (256, 2, 0, 1, 3), (257, 2, 1, 3, 3),
          (1024, 2, 1, 1, 0), (4096 * 4 + 3, 4, 2, 3, 0), (4096 * 4 + 3, 8, 5, 1, 3), (300001, 4, 3, 3, 3)])


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("n,s,k,nrhs,pad", EXACT)
def test_steps_exact(gexec, tn, n, s, k, nrhs, pad):
    t = br.TYPES[tn]
    rng = np.random.default_rng(n * 100 + s * 10 + k)
    d1, r1, d2, r2, d3, r3 = _exact_inputs(rng, t, n, s, k, nrhs)
    stop = np.zeros(nrhs, np.uint8)
    for got, ref in ((_step_1(gexec, tn, k, d1, stop, pad), r1), (_step_2(gexec, tn, k, d2, stop, pad), r2),
                     (_step_3(gexec, tn, k, d3, stop, pad), r3)):
        for name, want in ref.items():
            assert np.array_equal(got[name].astype(want.dtype), want), name


@pytest.mark.parametrize("tn", TN)
def test_step_3_exact_past_the_partials(gexec, tn):
    """n = 1024 * 1024 + 5: more than 1024 partials of 1024 rows, stage 1 of the dots starts to stride"""
    t = br.TYPES[tn]
    n, s, k, nrhs = 1024 * 1024 + 5, 2, 1, 1
    case, ref, largest = br.idr_exact_step3_case(np.random.default_rng(9), t, n, s, k, nrhs)
    print(f"exact case n={n}: largest intermediate {largest:g}")
    got = _step_3(gexec, tn, k, case, np.zeros(nrhs, np.uint8), 0)
    for name, want in ref.items():
        assert np.array_equal(got[name].astype(want.dtype), want), name


ROUNDING = [(1, 1, 0, 1, 0), (255, 2, 1, 3, 3), (256, 4, 0, 1, 0), (257, 4, 3, 3, 3), (1000, 8, 7, 3, 0),
            (1000, 1, 0, 3, 3), (4096 * 4 + 3, 8, 4, 1, 3), (20011, 4, 2, 3, 0)]


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("n,s,k,nrhs,pad", ROUNDING)
def test_steps_rounding(gexec, tn, n, s, k, nrhs, pad):
    t = br.TYPES[tn]
    d = br.idr_rounding_case(np.random.default_rng(n + s + k), t, n, s, k, nrhs)
    stop = np.zeros(nrhs, np.uint8)
    hp, pl = br.hp(t), br.plain(t)
    runs = []
    got = _step_1(gexec, tn, k, d, stop, pad)
    a1 = (k, d["m"], d["f"], d["residual"], d["g"], d["c"], d["v"])
    runs.append(("step_1", got, dict(zip("cv", br.idr_step_1(hp, *a1))), dict(zip("cv", br.idr_step_1(pl, *a1)))))
    got = _step_2(gexec, tn, k, d, stop, pad)
    a2 = (k, d["omega"], d["pv"], d["c"], d["u"])
    runs.append(("step_2", got, dict(u=br.idr_step_2(hp, *a2)), dict(u=br.idr_step_2(pl, *a2))))
    got = _step_3(gexec, tn, k, d, stop, pad)
    a3 = (k,) + tuple(d[name] for name in ("p",) + S3)
    runs.append(("step_3", got, br.idr_step_3(hp, *a3), br.idr_step_3(pl, *a3)))
    for kernel, got, ref, plain_v in runs:
        for name in ref:
            ok, ratio = br.rule_r(got[name], ref[name], plain_v[name], t)
            _note(kernel, tn, ratio)
            assert ok, (kernel, name, ratio)


def _poison(d, names, nrhs, col):
    """NaN in everything that belongs to right-hand side `col`"""
    out = {}
    for name, a in d.items():
        a = a.copy()
        if name in names:
            if a.ndim == 1:
                a[col] = np.nan
            else:
                a[:, col::nrhs] = np.nan
        out[name] = a
    return out


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("n,s,k", [(1000, 4, 2), (257, 2, 1)])
def test_stopped_column_is_untouched(gexec, tn, n, s, k):
    """status 0x41 on the middle column, NaN in all of that column's inputs: every output keeps that column
    bit for bit; the neighbours are the exact case's integers"""
    t = br.TYPES[tn]
    nrhs = 3
    rng = np.random.default_rng(n + k)
    d1, r1, d2, r2, d3, r3 = _exact_inputs(rng, t, n, s, k, nrhs)
    stop = np.array([0, br.STOPPED, 0], np.uint8)
    for fn, d, ref, cols in ((_step_1, d1, r1, ("m", "f", "residual", "g", "c", "v")),
                             (_step_2, d2, r2, ("omega", "pv", "c", "u")), (_step_3, d3, r3, S3)):
        dn = _poison(d, cols, nrhs, 1)
        got = fn(gexec, tn, k, dn, stop, 3)
        for name, want in ref.items():
            g = got[name]
            assert same_bits(g[:, 1::nrhs], dn[name][:, 1::nrhs]), name + ": stopped column written"
            for col in (0, 2):
                assert np.array_equal(g[:, col::nrhs].astype(want.dtype), want[:, col::nrhs]), name


def _initialize(gexec, tn, nrhs, s, n, p, deterministic, pad):
    t = br.TYPES[tn]
    b = Bufs(gexec, pad, m=np.full((s, s * nrhs), CANARY, t), p=p,
             stop=np.full(nrhs + 2, 0xee, np.uint8))
    _call("gkoc_idr_initialize_" + tn, gexec.stream, nrhs, s, b["m"], b.ld("m"), n, b["p"], b.ld("p"),
          deterministic, b["stop"])
    sync()
    return b.get("m"), b.get("p"), b.get("stop")


def _gram_defect(p):
    w = p.astype(np.clongdouble)
    return float(np.max(np.abs(w @ np.conj(w).T - np.eye(p.shape[0]))))


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("n,s,nrhs,pad", [(1, 1, 1, 0), (255, 2, 3, 3), (257, 4, 1, 0), (1000, 8, 3, 3),
                                          (4096 * 4 + 3, 4, 3, 0), (300001, 2, 1, 3)])
def test_initialize_deterministic(gexec, tn, n, s, nrhs, pad):
    t = br.TYPES[tn]
    rng = np.random.default_rng(n + s)
    p0 = rng.standard_normal((s, n))
    p0 = (p0 + 1j * rng.standard_normal((s, n))).astype(t) if br.is_complex(t) else p0.astype(t)
    m, p, stop = _initialize(gexec, tn, nrhs, s, n, p0, 1, pad)
    wm, wp, _ = br.idr_initialize(br.hp(t), p0, s, nrhs)
    _, pp, _ = br.idr_initialize(br.plain(t), p0, s, nrhs)
    assert np.array_equal(m.astype(wm.dtype), wm)
    assert np.all(stop[:nrhs] == 0) and np.all(stop[nrhs:] == 0xee)
    ok, ratio = br.rule_r(p, wp, pp, t)
    _note("initialize", tn, ratio)
    assert ok, ratio
    assert _gram_defect(p) <= 4 * _gram_defect(pp) + 8 * br.eps_of(t)


@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("n,s", [(257, 4), (20011, 8)])
def test_initialize_random(gexec, tn, n, s):
    """deterministic = 0: the shadow vectors are drawn by the kernel; rows orthonormal by rule R against the
    plain Gram-Schmidt's own defect on Gaussian rows of that n; two calls draw different vectors"""
    t = br.TYPES[tn]
    canary = np.full((s, n), CANARY, t)
    m, p1, stop = _initialize(gexec, tn, 1, s, n, canary, 0, 3)
    _, p2, _ = _initialize(gexec, tn, 1, s, n, canary, 0, 3)
    assert np.all(np.isfinite(p1)) and not np.array_equal(p1, p2)
    rng = np.random.default_rng(n)
    g = rng.standard_normal((s, n))
    g = (g + 1j * rng.standard_normal((s, n))).astype(t) if br.is_complex(t) else g.astype(t)
    _, pp, _ = br.idr_initialize(br.plain(t), g, s, 1)
    for p in (p1, p2):
        assert _gram_defect(p) <= 4 * _gram_defect(pp) + 8 * br.eps_of(t), (_gram_defect(p), _gram_defect(pp))
    if br.is_complex(t):
        assert np.any(p1.imag != 0)
    assert np.array_equal(m, np.eye(s, dtype=t)) and stop[0] == 0


@pytest.mark.parametrize("tn", TN)
def test_initialize_empty_dimensions(gexec, tn):
    t = br.TYPES[tn]
    p0 = np.full((4, 50), CANARY, t)
    # s = 0: returns 0, writes nothing
    b = Bufs(gexec, 3, m=p0, p=p0, stop=np.full(8, 0xee, np.uint8))
    _call("gkoc_idr_initialize_" + tn, gexec.stream, 3, 0, b["m"], b.ld("m"), 50, b["p"], b.ld("p"), 1, b["stop"])
    sync()
    assert same_bits(b.get("m"), p0) and same_bits(b.get("p"), p0) and np.all(b.get("stop") == 0xee)
    # n = 0: m and stop are still set, p is not touched
    b = Bufs(gexec, 3, m=np.full((4, 8), CANARY, t), p=p0, stop=np.full(8, 0xee, np.uint8))
    _call("gkoc_idr_initialize_" + tn, gexec.stream, 2, 4, b["m"], b.ld("m"), 0, b["p"], b.ld("p"), 1, b["stop"])
    sync()
    wm, _, _ = br.idr_initialize(br.hp(t), np.zeros((4, 0), t), 4, 2)
    assert np.array_equal(b.get("m").astype(wm.dtype), wm) and same_bits(b.get("p"), p0)
    assert np.all(b.get("stop")[:2] == 0) and np.all(b.get("stop")[2:] == 0xee)
    # nrhs = 0 with s > 0: the reference's loops over the right-hand sides are empty; m (s x 0) and stop get
    # nothing, the call succeeds
    rng = np.random.default_rng(0)
    pr = rng.standard_normal((4, 50)).astype(t)
    b = Bufs(gexec, 3, m=np.full((4, 2), CANARY, t), p=pr, stop=np.full(8, 0xee, np.uint8))
    _call("gkoc_idr_initialize_" + tn, gexec.stream, 0, 4, b["m"], b.ld("m") , 50, b["p"], b.ld("p"), 1, b["stop"])
    sync()
    assert np.all(b.get("stop") == 0xee) and np.all(b.get("m") == t(CANARY))
    _, wp, _ = br.idr_initialize(br.hp(t), pr, 4, 0)
    _, pp, _ = br.idr_initialize(br.plain(t), pr, 4, 0)
    ok, ratio = br.rule_r(b.get("p"), wp, pp, t)
    assert ok, ratio


@pytest.mark.parametrize("tn", TN)
def test_compute_omega(gexec, tn):
    """both branches of the kappa test, a tht with zero imaginary part, a stopped column (NaN inputs,
    untouched), and tht = 0: the kernel sets omega = 0 there - that is this backend's guard against the
    division by zero, not the reference's arithmetic (which gives NaN), so only 'finite and zero' is asserted"""
    t = br.TYPES[tn]
    rt = br.real_of(t)
    cx = br.is_complex(t)
    tht = np.array([4.0, 4.0, np.nan, 2.5, 0.0, 9.0], t)
    omega = np.array([1.0, 3.9, np.nan, -1.25, 1.0, 0.3], t)
    if cx:
        omega = (omega * (0.6 + 0.8j)).astype(t)
        tht[5] = 9.0 + 0.5j
    rn = np.array([1.0, 1.0, np.nan, 0.5, 1.0, 2.0], rt)
    stop = np.array([0, 0, br.STOPPED, 0, 0, 0], np.uint8)
    kappa = 0.7
    d_tht, d_rn, d_om, d_stop = (Dev(gexec, a) for a in (tht, rn, omega, stop))
    _call("gkoc_idr_compute_omega_" + tn, gexec.stream, 6, _real(tn, kappa), d_tht, d_rn, d_om, d_stop)
    sync()
    got = d_om.get()
    assert same_bits(got[2:3], omega[2:3])
    assert np.isfinite(got[4]) and got[4] == 0
    live = [0, 1, 3, 5]
    with np.errstate(all="ignore"):
        ref = br.idr_compute_omega(br.hp(t), rt(kappa), tht, rn, omega, stop)
        pl = br.idr_compute_omega(br.plain(t), rt(kappa), tht, rn, omega, stop)
    absrho = np.abs(omega[live].astype(np.complex128) / (np.sqrt(tht[live].real.astype(np.float64)) * rn[live]))
    assert (absrho < kappa).tolist() == [True, False, False, True]          # both branches are taken
    ok, ratio = br.rule_r(got[live], ref[live], pl[live], t)
    _note("compute_omega", tn, ratio)
    assert ok, ratio
    assert same_bits(d_tht.get(), tht) and same_bits(d_rn.get(), rn)


# ------------------------------------------------------------------------------------------ end to end
def _idr_on_device(gexec, tn, a_sp, b, p0, s, limit, tol, kappa=0.7):
    """Ginkgo's IDR(s) loop (core/solver/idr.cpp, identity preconditioner) over the five entry points,
    Csr.apply, the dense product (f = P r) and the dense dot / norm kernels; stops when the TRUE residual,
    computed in numpy from x, is below tol ||b||.  Returns (x, iterations, relative true residual)"""
    import torch
    import ginkgo_amd as g
    from ginkgo_amd._lib import lib
    t = br.TYPES[tn]
    cx = br.is_complex(t)
    n = a_sp.shape[0]
    tt = torch.complex128 if cx else torch.float64
    a = g.Csr.from_scipy(gexec, a_sp)
    dev = gexec.device

    def vec(cols=1):
        return torch.zeros((n, cols), dtype=tt, device=dev)

    def spmv(src, dst):
        if cx:      # a real matrix on (re, im) pairs: two real right-hand sides
            a.apply(g.Dense(gexec, torch.view_as_real(src[:, 0])), g.Dense(gexec, torch.view_as_real(dst[:, 0])))
        else:
            a.apply(g.Dense(gexec, src), g.Dense(gexec, dst))

    x, r, v, t_, g_k = vec(), vec(), vec(), vec(), vec()
    r.copy_(torch.from_numpy(b.reshape(-1, 1).astype(t)))
    gm, u = vec(s), vec(s)
    p = torch.from_numpy(np.ascontiguousarray(p0.astype(t))).to(dev)
    m = torch.zeros((s, s), dtype=tt, device=dev)
    f, c = torch.zeros((s, 1), dtype=tt, device=dev), torch.zeros((s, 1), dtype=tt, device=dev)
    omega = torch.ones(1, dtype=tt, device=dev)
    tht = torch.zeros(1, dtype=tt, device=dev)
    rnorm = torch.zeros(1, dtype=torch.float64, device=dev)
    stop = torch.zeros(1, dtype=torch.uint8, device=dev)
    nbytes = lib().gkoc_reduction_workspace_bytes(C.c_int64(n), C.c_int64(1), C.c_size_t(16))
    work = torch.zeros(nbytes + 64, dtype=torch.uint8, device=dev)
    st = gexec.stream
    _call("gkoc_idr_initialize_" + tn, st, 1, s, m, s, n, p, n, 1, stop)
    bn = np.linalg.norm(b)

    def true_res():
        torch.cuda.synchronize()
        return float(np.linalg.norm(b - a_sp @ x.cpu().numpy()[:, 0]) / bn)

    iters = 0
    while iters < limit:
        _call("gkoc_dense_simple_apply_" + tn, st, s, 1, n, p, n, r, 1, f, 1)
        for k in range(s):
            _call("gkoc_idr_step_1_" + tn, st, n, 1, s, k, m, s, f, 1, r, 1, gm, s, c, 1, v, 1, stop)
            _call("gkoc_idr_step_2_" + tn, st, n, 1, s, k, omega, v, 1, c, 1, u, s, stop)
            uk = u[:, k:k + 1].contiguous()
            spmv(uk, g_k)
            _call("gkoc_idr_step_3_" + tn, st, n, 1, s, k, p, n, gm, s, g_k, 1, u, s, m, s, f, 1, r, 1, x, 1, stop)
            iters += 1
            res = true_res()
            if res <= tol or iters >= limit:
                return x.cpu().numpy()[:, 0], iters, res
        spmv(r, t_)
        if cx:
            _call("gkoc_cdense_compute_dot_" + tn, st, n, 1, t_, 1, r, 1, omega, 1)        # t^H r
            _call("gkoc_cdense_compute_dot_" + tn, st, n, 1, t_, 1, t_, 1, tht, 1)
        else:
            _call("gkoc_dense_compute_dot_" + tn, st, n, 1, t_, 1, r, 1, omega, work, C.c_size_t(nbytes))
            _call("gkoc_dense_compute_dot_" + tn, st, n, 1, t_, 1, t_, 1, tht, work, C.c_size_t(nbytes))
        _call("gkoc_dense_compute_norm2_" + tn, st, n, 1, r, 1, rnorm, work, C.c_size_t(nbytes))
        _call("gkoc_idr_compute_omega_" + tn, st, 1, C.c_double(kappa), tht, rnorm, omega, stop)
        x += omega * r
        r -= omega * t_
        iters += 1
        res = true_res()
        if res <= tol:
            break
    return x.cpu().numpy()[:, 0], iters, res


@pytest.mark.parametrize("tn", ["f64", "c128"])
@pytest.mark.parametrize("matrix", ["stencil7", "convdiff"])
@pytest.mark.parametrize("s", [1, 4])
def test_idr_end_to_end(gexec, tn, matrix, s):
    """true residual <= 1e-9 within the iteration count of the long-double reference loop (same shadow
    vectors, deterministic) + 20 %, at least 5 more"""
    t = br.TYPES[tn]
    a_sp = br.model_matrices(12)[matrix]
    n = a_sp.shape[0]
    rng = np.random.default_rng(21)
    b = rng.uniform(-1, 1, n)
    if br.is_complex(t):
        b = b + 1j * rng.uniform(-1, 1, n)
    p0 = rng.standard_normal((s, n))
    hp = br.hp(t)
    dense = a_sp.toarray().astype(np.longdouble)
    _, ref_iters = br.idr_solve(hp, lambda w: dense @ w, b, p0, s, 1e-9, 3000)
    assert ref_iters < 3000
    limit = max(int(np.ceil(1.2 * ref_iters)), ref_iters + 5)
    x, iters, res = _idr_on_device(gexec, tn, a_sp, b, p0, s, limit, 1e-9)
    print(f"IDR({s}) {matrix} {tn}: {iters} iterations (reference {ref_iters}, limit {limit}), "
          f"true residual {res:.3e}")
    assert res <= 1e-9 and iters <= limit
    assert np.linalg.norm(b - a_sp @ x) / np.linalg.norm(b) <= 1e-9


def test_zz_print_ratios():
    """the table of the largest |kernel - ref| / (eps max|ref|) seen by the rounding cases of this run"""
    for (kernel, tn), ratio in sorted(RATIOS.items()):
        print(f"idr ratio {kernel:14s} {tn:5s} {ratio:8.2f}")
