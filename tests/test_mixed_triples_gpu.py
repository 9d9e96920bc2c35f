"""The mixed-precision products of csrc/mixed_precision.hip through the C ABI: gkoc_csr_spmv_mixed_*,
gkoc_ell_spmv_mixed_* in every (matrix, input, output) value-type triple and gkoc_dense_row_gather_mixed_* in its
four direction pairs, at the edge shapes of the two plain kernels, against tests/mixed_refs.py (checked on the
CPU by tests/test_mixed_refs_cpu.py).

Acceptance.  Real non-uniform triples: bit-identical to the oracle.  Complex non-uniform triples: per output entry
|got - ref| <= (m + 8) eps(AT) S + eps(OT) |ref| against the long-double value (mixed_refs.bound; derivation in its
docstring), equality on Gaussian integers, exactly 1 on the cancellation row (and on [2^30 + 1, -2^30] . 1 when the
matrix type is wide: the values must reach the arithmetic as stored); the number of entries whose bits
differ from the plain restatement is counted per triple and format and printed after the last test (pytest -s) -
reported, not asserted.  Uniform triples and (f32, f64, f64): bit-identical to the tuned entry points they are
routed to.  Row gather: the plain form equals numpy's astype bit for bit, the advanced form the restatement bit
for bit (real) or within 8 eps(AT) (|alpha||orig| + |beta||out|) + eps(OT) |ref| (complex).

Every input is read back and compared bit for bit; value outputs start as NaN; b and c are cut out of padded
arrays with ldb = nrhs + 2 and ldc = nrhs + 3 whose padding must keep its canary."""
import ctypes as C
import functools

import numpy as np
import pytest

import binding_refs as br
import mixed_refs as mr
from binding_gpu import CANARY, Dev, call as _call, canaries_ok, grid_cap_rows, out_buf, padded, raises_invalid, \
    same_bits, sync, tail_ok

pytestmark = pytest.mark.gpu

IT = {"i32": np.int32, "i64": np.int64}
FMTS = ("csr", "ell")
NRHS = (1, 3)
DIFFERS = {}            # (format, triple) -> [entries whose bits differ from the plain restatement, entries compared]
GATHER_DIFFERS = {}


@functools.lru_cache(maxsize=None)
def _case(fmt, name, triple, nrhs, kind):
    """inputs and reference of one call, computed once and shared by the index types"""
    x = mr.spmv_inputs(fmt, name, triple, nrhs, kind)
    p = x.reference()
    for a in (x.vals, x.cols, x.b, x.c, p.ref, p.plain, p.S, p.m):
        a.setflags(write=False)
    return x, p


def _codes(triple):
    return [C.c_int(mr.CODE[t]) for t in triple]


class Call:
    """the device operands of one call of gkoc_{csr,ell}_spmv_mixed_*; c starts from c0 (None: NaN)"""

    def __init__(self, gexec, x, in_, c0=None):
        self.x, self.in_, self.gexec = x, in_, gexec
        it, nrhs = IT[in_], x.nrhs
        ot = mr.dt(x.triple[2])
        self.host = [x.cols.astype(it), x.vals, padded(x.b, nrhs + 2)]
        if x.fmt == "csr":
            self.host.append(x.ptrs.astype(it))
        if x.alpha is not None:
            self.host += [np.array([x.alpha]), np.array([x.beta])]
        self.dev = [Dev(gexec, h) for h in self.host]
        self.c0 = padded(np.full((x.n_rows, nrhs), np.nan, ot) if c0 is None else c0, nrhs + 3)
        self.dc = Dev(gexec, self.c0)

    def args(self, triple=None):
        x, d = self.x, self.dev
        al, be = (d[-2], d[-1]) if x.alpha is not None else (None, None)
        head = (self.gexec.stream, *_codes(triple or x.triple), x.n_rows, x.n_cols)
        tail = (d[1], d[2], x.nrhs + 2, be, self.dc, x.nrhs + 3, x.nrhs)
        if x.fmt == "csr":
            return ("gkoc_csr_spmv_mixed_" + self.in_, *head, al, d[3], d[0], *tail)
        return ("gkoc_ell_spmv_mixed_" + self.in_, *head, x.k, x.stride, al, d[0], *tail)

    def run(self):
        _call(*self.args())
        sync()
        return self.result()

    def result(self):
        got = self.dc.get()
        assert canaries_ok(got, self.x.nrhs), (self.x.name, "padding of c written")
        for d, h in zip(self.dev, self.host):
            assert same_bits(d.get(), h), (self.x.name, "an input changed")
        return got[:, :self.x.nrhs]


def _parts_that_differ(got, plain):
    """real and imaginary parts of a complex result whose bits are not the plain restatement's"""
    bits = {8: np.uint32, 16: np.uint64}[got.dtype.itemsize]
    return int(np.count_nonzero(np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(plain).view(bits)))


def _accept(x, p, got, oracle, in_):
    """the acceptance of one call's result (see the module docstring)"""
    tag = (x.fmt, x.name, mr.tid(x.triple), x.nrhs, x.kind, in_)
    ot = mr.dt(x.triple[2])
    assert got.dtype == ot and got.shape == (x.n_rows, x.nrhs)
    if x.kind == "beta_zero_over_nan_c":
        assert np.all(np.isfinite(got)), tag
    if x.name == "cancellation_row":
        assert np.all(got == mr.cancellation_want(ot)), (tag, got)
    if x.name == "wide_matrix_values_survive":
        assert np.all(got == mr.survive_want(x.triple[0], ot)), (tag, got)
    if x.kind == "integers":
        assert np.array_equal(got.astype(p.ref.dtype), p.ref), tag
    if x.triple[0] in mr.REAL:
        adv = dict(alpha=x.alpha, beta=x.beta, c=x.c) if x.alpha is not None else {}
        it = IT[in_]
        if x.fmt == "csr":
            want = oracle.csr_spmv_mixed(x.ptrs.astype(it), x.cols.astype(it), x.vals, x.b, ot, **adv)
        else:
            want = oracle.ell_spmv_mixed(x.n_rows, x.k, x.stride, x.cols.astype(it), x.vals, x.b, ot, **adv)
        assert same_bits(got, want.reshape(got.shape)), (tag, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:4])
        return
    at = np.complex128
    err, tol = np.abs(got.astype(np.clongdouble) - p.ref), mr.bound(p, at, ot)
    some = tol > 0
    if some.any():
        print("bound | %s %s %s nrhs %d %s %s | used %.3f" % (*tag[:3], x.nrhs, x.kind, in_,
                                                             float(np.max(err[some] / tol[some]))))
    assert np.all(err <= tol), (tag, np.argwhere(err > tol)[:4])
    count = DIFFERS.setdefault((x.fmt, x.triple), [0, 0])
    count[0] += _parts_that_differ(got, p.plain)
    count[1] += 2 * got.size


def _families(fmt):
    return list(mr.CSR_FAMILIES if fmt == "csr" else mr.ELL_FAMILIES) + ["n_cols_0_empty_matrix"]


# ------------------------------------------------------------------------------- the two plain kernels
CASES = [(f, n) for f in FMTS for n in _families(f)]


@pytest.mark.parametrize("triple", mr.PLAIN, ids=mr.tid)
@pytest.mark.parametrize("fmt,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_plain_kernels_at_their_edges(gexec, oracle, fmt, name, triple):
    """one case family of mixed_refs.CSR_FAMILIES / ELL_FAMILIES (named by the edge it sits on) in one triple: both
    index types, nrhs 1 and 3, plain and advanced form, beta == 0 over a c full of NaN, alpha == 0, Gaussian
    integers"""
    for in_ in IT:
        for nrhs in NRHS:
            for kind in mr.kinds_of(name):
                x, p = _case(fmt, name, triple, nrhs, kind)
                got = Call(gexec, x, in_, None if kind == "plain" else x.c).run()
                _accept(x, p, got, oracle, in_)


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("triple", [("f64", "f32", "f32"), ("c64", "c128", "c64")], ids=mr.tid)
@pytest.mark.parametrize("fmt", FMTS)
def test_empty_dimensions_leave_the_output_alone(gexec, fmt, triple, in_):
    """n_rows = 0 and nrhs = 0: nothing to write - a c holding canaries keeps every bit; n_cols = 0 with an
    empty matrix is a product like any other (zeros, or beta c) and is part of the test above"""
    ot = mr.dt(triple[2])
    for kind in ("plain", "advanced"):
        x, _ = _case(fmt, "n_rows_0", triple, 3, kind)
        c = Call(gexec, x, in_)
        c.c0 = np.full((4, 6), CANARY, ot)
        c.dc = Dev(gexec, c.c0)
        _call(*c.args())
        sync()
        assert same_bits(c.dc.get(), c.c0)
        name = "rows_65_last_segment_of_one_row" if fmt == "csr" else "rows_257"
        x, _ = _case(fmt, name, triple, 0, kind)
        c = Call(gexec, x, in_)
        c.c0 = np.full((x.n_rows, 3), CANARY, ot)
        c.dc = Dev(gexec, c.c0)
        _call(*c.args())
        sync()
        assert same_bits(c.dc.get(), c.c0)


# ----------------------------------------------------------------------------------------- routing
def _direct(c, tn):
    """the same call on the tuned entry point that spmv_mixed routes it to (operands of Call c)"""
    x, d, s = c.x, c.dev, c.gexec.stream
    adv = x.alpha is not None
    al, be = (d[-2], d[-1]) if adv else (None, None)
    ldb, ldc, suf = x.nrhs + 2, x.nrhs + 3, tn + "_" + c.in_
    if x.fmt == "csr" and tn in mr.CPLX:
        return ("gkoc_ccsr_spmv_" + suf, s, x.n_rows, x.nrhs, d[3], d[0], d[1], al, d[2], ldb, be, c.dc, ldc)
    if x.fmt == "csr":
        mid = (al,) if adv else ()
        last = (be,) if adv else ()
        return ("gkoc_csr_" + ("advanced_" if adv else "") + "spmv_" + suf, s, x.n_rows, x.n_cols, *mid, d[3], d[0], d[1],
                d[2], ldb, *last, c.dc, ldc, x.nrhs)
    mid = (al,) if adv else ()
    last = (be,) if adv else ()
    return ("gkoc_ell_" + ("advanced_" if adv else "") + "spmv_" + suf, s, x.n_rows, x.n_cols, x.k, x.stride, *mid, d[0],
            d[1], d[2], ldb, *last, c.dc, ldc, x.nrhs)


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("triple", mr.TUNED, ids=mr.tid)
@pytest.mark.parametrize("fmt", FMTS)
def test_uniform_triples_are_routed_to_the_tuned_entry_points(gexec, fmt, triple, in_):
    """the routing, not the tuned kernels: bit-identical to gkoc_csr_spmv_* / gkoc_ccsr_spmv_* / gkoc_ell_spmv_* /
    *_f32_f64_* called directly on copies of the same input, at the smallest shapes"""
    names = ("rows_1", "rows_65_last_segment_of_one_row") if fmt == "csr" else ("rows_1", "rows_257", "k_0")
    tn = "f32_f64" if triple == ("f32", "f64", "f64") else triple[0]
    for name in names:
        for nrhs in NRHS:
            for kind in ("plain", "advanced"):
                x, p = _case(fmt, name, triple, nrhs, kind)
                c0 = None if kind == "plain" else x.c
                got = Call(gexec, x, in_, c0).run()
                d = Call(gexec, x, in_, c0)
                if tn == "f32_f64" and kind == "advanced":          # the direct entry takes alpha as a double
                    d.host[-2] = d.host[-2].astype(np.float64)
                    d.dev[-2] = Dev(gexec, d.host[-2])
                _call(*_direct(d, tn))
                sync()
                assert same_bits(got, d.result()), (fmt, name, triple, nrhs, kind)
                ot = mr.dt(triple[2])
                tol = mr.bound(p, mr.widest(*[mr.dt(t) for t in triple]), ot)       # and it is the product
                assert np.all(np.abs(got.astype(p.ref.dtype) - p.ref) <= tol + 8 * br.eps_of(ot) * p.S)


# -------------------------------------------------------------------------------------- row gather
PAIRS = [("f64", "f32"), ("f32", "f64"), ("c128", "c64"), ("c64", "c128")]
N_ORIG = 300


def _gather_source(vt, cols):
    """N_ORIG x cols: -0.0, NaN, values that overflow when narrowed, the float subnormal range, ties, then random"""
    t = mr.dt(vt)
    if cols == 0:
        return np.zeros((N_ORIG, 0), t)
    s = mr.special_sources(t)
    rnd = mr.values(np.random.default_rng(11), N_ORIG * cols - len(s), t, spread=True)
    return np.concatenate([s, rnd]).reshape(N_ORIG, cols)


def _gather_rows(n, seed):
    rows = np.random.default_rng(seed).integers(0, N_ORIG, n)
    rows[:min(n, 6)] = [N_ORIG - 1, 0, 7, 7, 7, N_ORIG - 1][:min(n, 6)]    # the last row, repeated rows
    return rows


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("vt,ot", PAIRS)
def test_row_gather_plain_form_is_astype(gexec, vt, ot, in_):
    to = mr.dt(ot)
    for cols in (3, 0):
        orig = _gather_source(vt, cols)
        fo = padded(orig, cols + 2)
        do = Dev(gexec, fo)
        for n in (0, 1, 255, 256, 257, 2049):
            rows = _gather_rows(n, n).astype(IT[in_])
            dr = Dev(gexec, rows)
            fg = padded(np.full((n, cols), np.nan, to), cols + 3)
            dg = Dev(gexec, fg)
            _call("gkoc_dense_row_gather_mixed_" + in_, gexec.stream, C.c_int(mr.CODE[vt]), C.c_int(mr.CODE[ot]), n, cols,
                  None, dr, do, cols + 2, None, dg, cols + 3)
            sync()
            got = dg.get()
            assert canaries_ok(got, cols) and same_bits(dr.get(), rows) and same_bits(do.get(), fo)
            want = mr.row_gather(orig, rows, to).plain
            assert same_bits(got[:, :cols], want), (n, cols, np.argwhere(got[:, :cols] != want)[:4])


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("vt,ot", PAIRS)
def test_row_gather_advanced_form(gexec, vt, ot, in_):
    tv, to = mr.dt(vt), mr.dt(ot)
    at = mr.widest(tv, to)
    cols = 3
    orig = mr.values(np.random.default_rng(13), (N_ORIG, cols), tv, spread=True)
    fo = padded(orig, cols + 2)
    do = Dev(gexec, fo)
    alpha, beta = mr.scalars(tv, tv)
    sc = [np.array([alpha]), np.array([beta])]
    dal, dbe = (Dev(gexec, z) for z in sc)
    for n in (0, 1, 255, 256, 257, 2049):
        rows = _gather_rows(n, n + 1).astype(IT[in_])
        out0 = mr.values(np.random.default_rng(n), (n, cols), to)
        dr, dg = Dev(gexec, rows), Dev(gexec, padded(out0, cols + 3))
        _call("gkoc_dense_row_gather_mixed_" + in_, gexec.stream, C.c_int(mr.CODE[vt]), C.c_int(mr.CODE[ot]), n, cols,
              dal, dr, do, cols + 2, dbe, dg, cols + 3)
        sync()
        got = dg.get()
        assert canaries_ok(got, cols) and same_bits(dr.get(), rows) and same_bits(do.get(), fo)
        assert same_bits(dal.get(), sc[0]) and same_bits(dbe.get(), sc[1])
        got = got[:, :cols]
        g = mr.row_gather(orig, rows, to, alpha, beta, out0)
        if vt in mr.REAL:
            assert same_bits(got, g.plain), (n, np.argwhere(got != g.plain)[:4])
        else:
            err = np.abs(got.astype(np.clongdouble) - g.ref)
            assert np.all(err <= mr.gather_bound(g, at, to)), (n, np.argwhere(err > mr.gather_bound(g, at, to))[:4])
            count = GATHER_DIFFERS.setdefault((vt, ot), [0, 0])
            count[0] += _parts_that_differ(got, g.plain)
            count[1] += 2 * got.size


def test_row_gather_beyond_the_grid_cap(gexec):
    """launch_row_gather_mixed caps its grid at max_stream_blocks blocks and loops: grid_cap_rows() + 257 rows of
    one column, f32 -> f64, every row compared"""
    n = grid_cap_rows() + 257
    orig = (np.arange(N_ORIG) * 0.37 - 50).astype(np.float32).reshape(N_ORIG, 1)
    rows = (np.arange(n, dtype=np.int64) * 7919 % N_ORIG).astype(np.int32)
    do, dr = Dev(gexec, orig), Dev(gexec, rows)
    dg = out_buf(gexec, n, np.float64)
    _call("gkoc_dense_row_gather_mixed_i32", gexec.stream, C.c_int(1), C.c_int(0), n, 1, None, dr, do, 1, None, dg, 1)
    sync()
    got = dg.get()
    want = orig[rows, 0].astype(np.float64)
    assert tail_ok(got, n) and same_bits(got[:n], want), np.flatnonzero(got[:n] != want)[:4]


# ------------------------------------------------------------------------------------------ guards
def _not_supported(name, *args):
    from ginkgo_amd._lib import NotSupported
    with pytest.raises(NotSupported):
        _call(name, *args)
    return True


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("fmt", FMTS)
def test_spmv_refused_before_any_launch(gexec, fmt, in_):
    """the guards of spmv_mixed that come before any launch (and before the routing, or on a non-uniform triple):
    GKOC_E_INVALID for a type code of -1 or 4, alpha without beta and the reverse, a negative dimension,
    ldc < nrhs, ldb < nrhs with n_cols > 0, Ell stride < n_rows, Ell k < 0 and a NULL c; GKOC_E_NOT_SUPPORTED for
    real and complex types in one call.  The output keeps its bits, and the same operands then give the product"""
    triple = ("f64", "f32", "f64")
    x, p = _case(fmt, "rows_65_last_segment_of_one_row" if fmt == "csr" else "rows_257", triple, 3, "advanced")
    c = Call(gexec, x, in_, x.c)
    name, *good = c.args()
    pos = {"mt": 1, "it": 2, "ot": 3, "n_rows": 4, "n_cols": 5}
    if fmt == "csr":
        pos.update(alpha=6, ldb=11, beta=12, c=13, ldc=14, nrhs=15)
    else:
        pos.update(k=6, stride=7, alpha=8, ldb=12, beta=13, c=14, ldc=15, nrhs=16)
    assert good[pos["ldb"]] == 5 and good[pos["ldc"]] == 6 and good[pos["nrhs"]] == 3 and good[pos["c"]] is c.dc

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[pos[k]] = v
        return a
    for code in (-1, 4):
        for which in ("mt", "it", "ot"):
            assert raises_invalid(name, *bad(**{which: C.c_int(code)})), (which, code)
    assert raises_invalid(name, *bad(alpha=None)) and raises_invalid(name, *bad(beta=None))
    assert raises_invalid(name, *bad(n_rows=-1)) and raises_invalid(name, *bad(n_cols=-1))
    assert raises_invalid(name, *bad(nrhs=-1))
    assert raises_invalid(name, *bad(ldc=2)) and raises_invalid(name, *bad(ldb=2))
    assert raises_invalid(name, *bad(c=None))
    if fmt == "ell":
        assert raises_invalid(name, *bad(stride=x.n_rows - 1)) and raises_invalid(name, *bad(k=-1))
    for codes in ((0, 2, 0), (3, 3, 1), (1, 0, 2)):
        assert _not_supported(name, *bad(mt=C.c_int(codes[0]), it=C.c_int(codes[1]), ot=C.c_int(codes[2])))
    sync()
    assert same_bits(c.dc.get(), c.c0), "a refused call wrote to c"
    got = c.run()
    assert np.all(np.abs(got - p.ref) <= mr.bound(p, np.float64, np.float64))
    # ldb < nrhs is accepted when there are no columns to read
    x0, p0 = _case(fmt, "n_cols_0_empty_matrix", triple, 3, "advanced")
    c = Call(gexec, x0, in_, x0.c)
    a = list(c.args())
    a[1 + pos["ldb"]] = 0
    _call(*a)
    sync()
    assert same_bits(c.result(), p0.plain)


@pytest.mark.parametrize("in_", list(IT))
def test_row_gather_refused_before_any_launch(gexec, in_):
    """GKOC_E_INVALID: a type code of -1 or 4, vt == ot, alpha without beta and the reverse, a negative dimension,
    ld_orig < cols, ld_out < cols, a NULL pointer; GKOC_E_NOT_SUPPORTED: real and complex in one gather"""
    name = "gkoc_dense_row_gather_mixed_" + in_
    orig = mr.values(np.random.default_rng(1), (9, 3), np.float64)
    rows = np.array([8, 0, 3, 3], IT[in_])
    do, dr, dsc = Dev(gexec, orig), Dev(gexec, rows), Dev(gexec, np.array([0.5]))
    out0 = padded(np.full((4, 3), np.nan, np.float32), 6)
    dg = Dev(gexec, out0)
    good = [gexec.stream, C.c_int(0), C.c_int(1), 4, 3, None, dr, do, 3, None, dg, 6]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[dict(vt=1, ot=2, n=3, cols=4, alpha=5, rows=6, orig=7, ld_orig=8, beta=9, out=10, ld_out=11)[k]] = v
        return a
    for code in (-1, 4):
        assert raises_invalid(name, *bad(vt=C.c_int(code))) and raises_invalid(name, *bad(ot=C.c_int(code)))
    assert raises_invalid(name, *bad(ot=C.c_int(0))) and raises_invalid(name, *bad(vt=C.c_int(3), ot=C.c_int(3)))
    assert raises_invalid(name, *bad(alpha=dsc)) and raises_invalid(name, *bad(beta=dsc))
    assert raises_invalid(name, *bad(n=-1)) and raises_invalid(name, *bad(cols=-1))
    assert raises_invalid(name, *bad(ld_orig=2)) and raises_invalid(name, *bad(ld_out=2))
    assert raises_invalid(name, *bad(rows=None)) and raises_invalid(name, *bad(orig=None))
    assert raises_invalid(name, *bad(out=None))
    assert _not_supported(name, *bad(ot=C.c_int(3))) and _not_supported(name, *bad(vt=C.c_int(2)))
    sync()
    assert same_bits(dg.get(), out0), "a refused call wrote to out"
    _call(name, *good)
    sync()
    assert same_bits(dg.get()[:, :3], orig[rows].astype(np.float32)) and canaries_ok(dg.get(), 3)


# ----------------------------------------------------------------------------------- Python mirror
def _torch_of(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("triple", [("c64", "c128", "c64"), ("c128", "c64", "c128")], ids=mr.tid)
@pytest.mark.parametrize("fmt", FMTS)
def test_python_classes_give_the_bits_of_the_abi_call(gexec, fmt, triple):
    """Csr.apply / Ell.apply with complex non-uniform operands; a scalar given in the other precision is converted
    to the matrix' type (alpha) or the output's (beta)"""
    import ginkgo_amd as g
    name = "rows_129" if fmt == "csr" else "padding_in_the_middle_of_a_row"
    mt, ot = mr.dt(triple[0]), mr.dt(triple[2])
    other = {np.complex64: np.complex128, np.complex128: np.complex64}
    for kind in ("plain", "advanced"):
        x = mr.spmv_inputs(fmt, name, triple, 3, kind)
        if kind == "advanced":                           # scalars that both precisions hold
            x.alpha, x.beta = mt(-1.75 + 0.625j), ot(0.25 - 1.125j)
        p = x.reference()
        want = Call(gexec, x, "i32", None if kind == "plain" else x.c).run()
        if fmt == "csr":
            a = g.Csr.from_arrays(gexec, (x.n_rows, x.n_cols), x.ptrs.astype(np.int32), x.cols.astype(np.int32),
                                  x.vals.copy())
        else:
            a = g.Ell(gexec, (x.n_rows, x.n_cols), gexec.to_device(x.vals.copy()),
                      gexec.to_device(x.cols.astype(np.int32)), x.k, x.stride)
        db = g.Dense.from_numpy(gexec, x.b.copy())
        dc = g.Dense.from_numpy(gexec, np.full((x.n_rows, 3), np.nan, ot) if kind == "plain" else x.c.copy())
        if kind == "plain":
            a.apply(db, dc)
            assert same_bits(dc.to_numpy(), want)
            continue
        # given in the other precision: a narrow scalar is widened; a wide one that the narrow type cannot hold
        # must arrive rounded to it
        al_given = np.array([[x.alpha]]).astype(other[mt]) if mt is np.complex128 else \
            np.array([[np.complex128(x.alpha) + (1 + 1j) * 2.0 ** -30]])
        be_given = np.array([[x.beta]]).astype(other[ot]) if ot is np.complex128 else \
            np.array([[np.complex128(x.beta) + (1 - 1j) * 2.0 ** -30]])
        assert al_given.dtype == other[mt] and be_given.dtype == other[ot]
        assert al_given.astype(mt)[0, 0] == x.alpha and be_given.astype(ot)[0, 0] == x.beta
        a.apply(g.Dense.from_numpy(gexec, al_given), db, g.Dense.from_numpy(gexec, be_given), dc)
        assert same_bits(dc.to_numpy(), want), kind
        err = np.abs(want.astype(np.clongdouble) - p.ref)
        assert np.all(err <= mr.bound(p, np.complex128, ot))


def test_python_row_gather_c128_to_c64_with_int64_indices(gexec):
    import ginkgo_amd as g
    import torch
    orig = _gather_source("c128", 3)
    rows = _gather_rows(257, 2).astype(np.int64)
    d = g.Dense.from_numpy(gexec, orig)
    out = g.Dense.create(gexec, (257, 3), torch.complex64)
    d.row_gather(gexec.to_device(rows), out)
    assert same_bits(out.to_numpy(), mr.row_gather(orig, rows, np.complex64).plain)


def test_python_real_complex_mix_raises_not_supported(gexec):
    import ginkgo_amd as g
    import torch
    from ginkgo_amd._lib import NotSupported
    x, _ = _case("csr", "rows_1", ("c64", "c128", "c64"), 1, "plain")
    a = g.Csr.from_arrays(gexec, (x.n_rows, x.n_cols), x.ptrs.astype(np.int32), x.cols.astype(np.int32), x.vals.copy())
    e = g.Ell(gexec, (1, x.n_cols), gexec.to_device(x.vals[:1].copy()), gexec.to_device(np.zeros(1, np.int32)), 1, 1)
    db = g.Dense.from_numpy(gexec, np.ones((x.n_cols, 1), np.float64))
    for op in (a, e):
        dc = g.Dense.from_numpy(gexec, np.full((1, 1), np.nan, np.complex64))
        with pytest.raises(NotSupported):
            op.apply(db, dc)
        assert np.all(np.isnan(dc.to_numpy().real))
    d = g.Dense.from_numpy(gexec, np.ones((4, 2), np.float64))
    out = g.Dense.create(gexec, (2, 2), torch.complex64)
    with pytest.raises(NotSupported):
        d.row_gather(gexec.to_device(np.array([0, 3], np.int32)), out)


# ------------------------------------------------------------------------------------------- table
@pytest.fixture(scope="module", autouse=True)
def _print_tables():
    """after the last test of this file: entries whose bits differ from the plain restatement (pytest -s)"""
    yield
    if not DIFFERS and not GATHER_DIFFERS:
        return
    print("\nparts (real and imaginary) of complex results whose bits differ from the plain restatement / parts compared")
    print("| triple (matrix-input-output) | csr | ell |")
    for t in mr.PLAIN_CPLX:
        print("| " + mr.tid(t) + " | " + " | ".join("%d / %d" % tuple(DIFFERS.get((f, t), (0, 0))) for f in FMTS) + " |")
    for pair, (bad, n) in sorted(GATHER_DIFFERS.items()):
        print("| advanced row gather %s -> %s | %d / %d |" % (*pair, bad, n))
