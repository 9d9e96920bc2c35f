"""The GMRES kernels of csrc/gmres.hip through the C ABI, in all four value types, at the smallest shapes that
select each of their paths, against the numpy references of tests/gmres_refs.py (checked on their own by
tests/test_gmres_refs_cpu.py).

Every vector operand has a leading dimension of its own and is cut from a padded array whose padding must keep its
canary; value outputs start as NaN and flat arrays are followed by canaries; every input is read back and compared
bit for bit; every call runs twice from the same inputs and must give the same bits.

Acceptance.  initialize, restart, multi_axpy, multi_sub_scaled, the w of mgs_step and solve_krylov: bit-identical
to the plain restatement (for complex types with the textbook product and Smith's quotient of
csrc/complex_type.hpp), started from the kernel's own state where there is one.  hessenberg_qr: bit-identical for
real types; for complex types the replayed rows are bit-identical and what follows the modulus (hypot: rounded
differently by the device's and the host's math libraries) obeys rule R against long double.  Independently of
the restatements, the y of a whole sweep solves the least-squares problem min || beta e_1 - H y || as a long-double
Householder solver does, and the last residual norm is its residual.  multi_dot and the h_next of mgs_step: within
(depth + c) eps sum |terms| of the long-double sum (gmres_refs.multi_dot_depth / mgs_step_depth / term_roundings),
and exactly equal on integer-valued inputs.

Every rule-R ratio and every fraction of a depth bound is printed by the case that observes it, before it is
asserted (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest

import binding_refs as br
import gmres_refs as gr
from binding_gpu import CANARY, Dev, call, canaries_ok, grid_cap_rows, padded, same_bits, sync

pytestmark = pytest.mark.gpu

TYPES = ("f64", "f32", "c128", "c64")
BYTE_CANARY, WORD_CANARY = 0x5a, 0x5a5a5a5a


def _note(kind, what, tn, v):
    """one line per observed figure: kind "ratio" is |kernel - ref| / (eps max |ref|) of a rule-R output, kind
    "bound" the fraction of a depth bound that a dot used"""
    print(f"{kind:5s} | {what} | {tn} | {float(v):.3f}")


def _wide(t):
    return np.clongdouble if br.is_complex(t) else np.longdouble


class Mat:
    """a rows x cols operand with leading dimension cols + pad inside a padded device array"""

    def __init__(self, gexec, a, pad):
        a = np.asarray(a)
        self.cols, self.ld = a.shape[1], a.shape[1] + pad
        self.host = padded(a, self.ld)
        self.dev = Dev(gexec, self.host)
        self._as_parameter_ = self.dev._as_parameter_

    def row(self, i):
        return self.dev.at(i * self.ld)

    def get(self):
        full = self.dev.get()
        assert canaries_ok(full, self.cols), "padding overwritten"
        return np.ascontiguousarray(full[:, :self.cols])

    def unchanged(self):
        return same_bits(self.dev.get(), self.host)


class Flat:
    """a flat device array followed by three canaries"""

    def __init__(self, gexec, a):
        a = np.ascontiguousarray(a).reshape(-1)
        self.n = a.shape[0]
        self.canary = a.dtype.type({1: BYTE_CANARY, 8: WORD_CANARY}[a.dtype.itemsize]) if a.dtype.kind == "u" \
            else a.dtype.type(CANARY)
        self.host = np.concatenate([a, np.full(3, self.canary, a.dtype)])
        self.dev = Dev(gexec, self.host)
        self._as_parameter_ = self.dev._as_parameter_

    def get(self):
        full = self.dev.get()
        assert np.all(full[self.n:] == self.canary), "written behind the end"
        return full[:self.n]

    def unchanged(self):
        return same_bits(self.dev.get(), self.host)


def nans(shape, t):
    return np.full(shape, np.nan, t)


def same_bits_or_nan(a, b):
    """bit for bit, except that where both hold a NaN its sign and payload are free (the host and the device
    propagate them differently); parts of complex values one by one"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    rt = br.real_of(a.dtype)
    ra, rb = a.reshape(-1).view(rt), b.reshape(-1).view(rt)
    both = np.isnan(ra) & np.isnan(rb)
    return same_bits(np.where(both, rt(0), ra), np.where(both, rt(0), rb))


def twice(run):
    """run() builds its operands, calls the kernel and returns the outputs as a tuple of arrays: two runs from
    the same inputs must agree bit for bit"""
    first, second = run(), run()
    assert all(same_bits(a, b) for a, b in zip(first, second)), "two runs differ"
    return first


def flat_basis(basis):
    return basis.reshape(-1, basis.shape[2])


def _stops(nrhs):
    stop = np.zeros(nrhs, np.uint8)
    if nrhs >= 3:
        stop[1], stop[2] = gr.STOPPED, gr.FINALIZED
    return stop


# ------------------------------------------------------------------------------ element-wise kernels
def check_initialize(gexec, tn, rows, nrhs, kd):
    t = br.TYPES[tn]
    b = gr.rand(np.random.default_rng([1, rows, nrhs]), (rows, nrhs), t)
    if rows:
        b[0, 0] = -0.0

    def run():
        db, res = Mat(gexec, b, 1), Mat(gexec, nans((rows, nrhs), t), 2)
        gs, gc = Mat(gexec, nans((kd, nrhs), t), 3), Mat(gexec, nans((kd, nrhs), t), 1)
        stop = Flat(gexec, np.full(nrhs, 0xff, np.uint8))
        call("gkoc_common_gmres_initialize_" + tn, gexec.stream, rows, nrhs, db, db.ld, res, res.ld, gs, gs.ld,
             gc, gc.ld, kd, stop)
        sync()
        assert db.unchanged()
        return res.get(), gs.get(), gc.get(), stop.get()
    got = twice(run)
    assert all(same_bits(g, r) for g, r in zip(got, gr.initialize(b, kd))), ("initialize", tn, rows, nrhs)


def check_restart(gexec, tn, rows, nrhs, kd):
    t = br.TYPES[tn]
    rng = np.random.default_rng([2, rows, nrhs])
    residual = gr.rand(rng, (rows, nrhs), t)
    norm = rng.uniform(0.5, 2, nrhs).astype(br.real_of(t))

    def run():
        res, dn = Mat(gexec, residual, 2), Flat(gexec, norm)
        rnc = Mat(gexec, nans((kd + 1, nrhs), t), 3)
        kry = Mat(gexec, nans(((kd + 1) * rows, nrhs), t), 1)
        fin = Flat(gexec, np.full(nrhs, 99, np.uint64))
        call("gkoc_gmres_restart_" + tn, gexec.stream, rows, nrhs, res, res.ld, dn, rnc, kry, kry.ld, fin)
        sync()
        assert res.unchanged() and dn.unchanged()
        return kry.get(), rnc.get(), fin.get()
    kry, rnc, fin = twice(run)
    k0, rnc0, fin0 = gr.restart(br.plain(t), residual, norm)
    assert same_bits(kry[:rows], k0) and same_bits(kry[rows:], nans((kd * rows, nrhs), t)), ("restart", tn, rows, nrhs)
    assert same_bits(rnc[0], rnc0) and same_bits(rnc[1:], nans((kd, nrhs), t)) and same_bits(fin, fin0)


def check_multi_axpy(gexec, tn, rows, nrhs, kd, fin, stop):
    t = br.TYPES[tn]
    rng = np.random.default_rng([3, rows, nrhs, kd])
    basis, y = gr.rand(rng, (kd + 1, rows, nrhs), t), gr.rand(rng, (kd, nrhs), t)
    fin, stop = np.asarray(fin, np.uint64), np.asarray(stop, np.uint8)
    assert fin.max(initial=0) <= kd
    out0 = nans((rows, nrhs), t)

    def run():
        kry, dy, out = Mat(gexec, flat_basis(basis), 1), Mat(gexec, y, 2), Mat(gexec, out0, 3)
        dfin, dstop = Flat(gexec, fin), Flat(gexec, stop)
        call("gkoc_gmres_multi_axpy_" + tn, gexec.stream, rows, nrhs, kry, kry.ld, dy, dy.ld, out, out.ld, dfin,
             dstop)
        sync()
        assert kry.unchanged() and dy.unchanged() and dfin.unchanged()
        return out.get(), dstop.get()
    out, after = twice(run)
    ref, ref_stop = gr.multi_axpy(br.plain(t), basis, y, fin, stop, out0)
    assert same_bits(out, ref), ("multi_axpy", tn, rows, nrhs, _first_diff(out, ref))
    assert same_bits(after, ref_stop)
    for k in np.flatnonzero(stop & 0x40):
        assert np.all(np.isnan(out[:, k].real))                      # a finalized column keeps its NaN


def check_multi_sub_scaled(gexec, tn, rows, nrhs, num, edit=None):
    t = br.TYPES[tn]
    rng = np.random.default_rng([4, rows, nrhs, num])
    basis, h, w0 = gr.rand(rng, (num, rows, nrhs), t), gr.rand(rng, (num, nrhs), t), gr.rand(rng, (rows, nrhs), t)
    if edit:
        edit(basis, h, w0)

    def run():
        kry, dh, w = Mat(gexec, flat_basis(basis), 1), Mat(gexec, h, 3), Mat(gexec, w0, 2)
        call("gkoc_x_gmres_multi_sub_scaled_" + tn, gexec.stream, rows, nrhs, num, kry, kry.ld, dh, dh.ld, w, w.ld)
        sync()
        assert kry.unchanged() and dh.unchanged()
        return (w.get(),)
    got, = twice(run)
    ref = gr.multi_sub_scaled(br.plain(t), basis, h, w0)
    assert same_bits_or_nan(got, ref), ("multi_sub_scaled", tn, rows, nrhs, num, _first_diff(got, ref))
    return got, w0


def _first_diff(got, ref):
    bad = np.flatnonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))).reshape(-1))
    if not bad.size:
        return "differs in the sign of a zero only"
    i = int(bad[0])
    return f"first wrong element {i}: {got.reshape(-1)[i]!r}, expected {ref.reshape(-1)[i]!r}"


def _fins(nrhs, kd):
    return np.array([(kd, 1, 0, 2, 3)[k % 5] for k in range(nrhs)], np.uint64).clip(0, kd)


@pytest.mark.parametrize("tn", TYPES)
@pytest.mark.parametrize("rows", (0, 1, 255, 256, 257, 2049, 100003))
def test_elementwise_shapes(gexec, tn, rows):
    """gaps 1, 7, 8: restart, initialize, multi_axpy and multi_sub_scaled with one column (the paths that skip
    idx / cols) and with 2, 3 and 5"""
    kd = 3
    for nrhs in (1, 2, 3, 5):
        check_initialize(gexec, tn, rows, nrhs, kd)
        check_restart(gexec, tn, rows, nrhs, kd)
        check_multi_axpy(gexec, tn, rows, nrhs, kd, _fins(nrhs, kd), _stops(nrhs))
        check_multi_sub_scaled(gexec, tn, rows, nrhs, 3)


@pytest.mark.parametrize("tn", TYPES)
@pytest.mark.parametrize("rows,nrhs", ((2097409, 1), (699137, 3)))
def test_elementwise_beyond_the_grid_cap(gexec, tn, rows, nrhs):
    """gap 6: rows * nrhs just above the 8192 blocks x 256 threads of stream_blocks: every thread takes a second
    trip of its stride loop for the first 257 (or 259) elements; every element is compared"""
    assert 0 < rows * nrhs - grid_cap_rows() < 512
    kd = 2
    check_initialize(gexec, tn, rows, nrhs, kd)
    check_restart(gexec, tn, rows, nrhs, kd)
    check_multi_axpy(gexec, tn, rows, nrhs, kd, np.full(nrhs, kd, np.uint64), np.zeros(nrhs, np.uint8))
    check_multi_sub_scaled(gexec, tn, rows, nrhs, 2)


@pytest.mark.parametrize("tn", TYPES)
def test_multi_axpy_trip_counts(gexec, tn):
    """gap 2: the by-4 loop and its tail with the counts 0, 1, 3, 4, 5, 7, 8 mixed over the columns of one
    call, and each of them alone at one column; running, stopped and finalized columns"""
    counts = (0, 1, 3, 4, 5, 7, 8)
    stop = np.array([0, gr.STOPPED, 0, 0, gr.FINALIZED, 0, gr.STOPPED], np.uint8)
    check_multi_axpy(gexec, tn, 257, 7, 8, counts, stop)
    for c in counts:
        check_multi_axpy(gexec, tn, 257, 1, 8, [c], [0])
    check_multi_axpy(gexec, tn, 257, 1, 8, [5], [gr.STOPPED])
    check_multi_axpy(gexec, tn, 257, 1, 8, [5], [gr.FINALIZED])


@pytest.mark.parametrize("tn", TYPES)
def test_multi_axpy_finalize_second_block(gexec, tn):
    """gap 5 (gmres_finalize_kernel): 257 columns, so that column 256 belongs to the second block"""
    nrhs = 257
    stop = np.zeros(nrhs, np.uint8)
    stop[[1, 255, 256]] = gr.STOPPED
    stop[[2, 254]] = gr.FINALIZED
    check_multi_axpy(gexec, tn, 3, nrhs, 3, _fins(nrhs, 3), stop)
    check_multi_axpy(gexec, tn, 0, nrhs, 3, _fins(nrhs, 3), stop)          # no rows: only the finalize launch


@pytest.mark.parametrize("tn", TYPES)
def test_multi_sub_scaled_trip_counts(gexec, tn):
    """gap 2: num = 1, 3, 4, 5, 8, 9 terms at one and at three columns"""
    for num in (1, 3, 4, 5, 8, 9):
        for nrhs in (1, 3):
            check_multi_sub_scaled(gexec, tn, 257, nrhs, num)


@pytest.mark.parametrize("tn", TYPES)
def test_multi_sub_scaled_zero_h(gexec, tn):
    """gap 1: a zero h in the unrolled part (d = 1) and in the tail (d = 8).  One column: the term is skipped, a
    NaN and a -0.0 product of that basis vector do not reach w.  Three columns: the term 0 * v is subtracted -
    the NaN reaches w and a w of -0.0 becomes +0.0 (pinned: include/gko_cdna4.h says so)"""
    t = br.TYPES[tn]

    def edit(basis, h, w0):
        for d in (1, 8):
            h[d] = 0
            basis[d, 0] = np.nan
            basis[d, 1] = -1.0
        w0[1] = -0.0
    got, w0 = check_multi_sub_scaled(gexec, tn, 257, 1, 9, edit)
    assert not np.isnan(got[0, 0])
    rng = np.random.default_rng([4, 257, 1, 9])
    basis, h = gr.rand(rng, (9, 257, 1), t), gr.rand(rng, (9, 1), t)
    keep = [d for d in range(9) if d not in (1, 8)]
    without = gr.multi_sub_scaled(br.plain(t), basis[keep], h[keep], w0)
    assert same_bits(got, without)                     # exactly as if the two terms were not there
    got, _ = check_multi_sub_scaled(gexec, tn, 257, 3, 9, edit)
    assert np.all(np.isnan(got[0].real)) and not np.any(np.isnan(got[1:].real))

    def only_zero(basis, h, w0):
        h[0] = 0
        basis[0, 1] = -1.0
        w0[1] = -0.0
    got, _ = check_multi_sub_scaled(gexec, tn, 257, 1, 1, only_zero)
    assert np.all(np.signbit(got[1].real))             # skipped: -0.0 stays
    got, _ = check_multi_sub_scaled(gexec, tn, 257, 3, 1, only_zero)
    assert not np.any(np.signbit(got[1].real))         # -0.0 - (0 * -1.0) = -0.0 - -0.0 = +0.0


# ------------------------------------------------------------------------------------------ multi_dot
def _need_multi_dot(rows, nrhs, num, t):
    from ginkgo_amd._lib import lib
    fn = lib().gkoc_gmres_multi_dot_workspace_bytes
    fn.restype = C.c_size_t
    return int(fn(C.c_int64(rows), C.c_int64(nrhs), C.c_int64(num), C.c_size_t(np.dtype(t).itemsize)))


def _status(name, *args):
    """the status a refused call returns (0 if it was not refused)"""
    import re
    from ginkgo_amd._lib import GkoError
    try:
        call(name, *args)
    except GkoError as e:
        return int(re.search(r"failed with status (-?\d+):", str(e)).group(1))
    return 0


def run_multi_dot(gexec, tn, basis, nxt, short=0):
    t = br.TYPES[tn]
    num, rows, nrhs = basis.shape
    wb = _need_multi_dot(rows, nrhs, num, t)
    kry, dn = Mat(gexec, flat_basis(basis), 2), Mat(gexec, nxt, 1)
    hcol = Mat(gexec, nans((num + 1, nrhs), t), 3)
    work = Flat(gexec, np.zeros(wb, np.uint8))
    args = (gexec.stream, rows, nrhs, num, kry, kry.ld, dn, dn.ld, hcol, hcol.ld, work, C.c_size_t(wb - short))
    if short:
        assert _status("gkoc_gmres_multi_dot_" + tn, *args) == -3           # GKOC_E_WORKSPACE
    else:
        call("gkoc_gmres_multi_dot_" + tn, *args)
    sync()
    work.get()
    assert kry.unchanged() and dn.unchanged()
    got = hcol.get()
    assert same_bits(got[num], nans(nrhs, t)), "row num_dots of hessenberg_col was written"
    return got[:num]


def check_multi_dot(gexec, tn, rows, num, nrhs, exact=False):
    t = br.TYPES[tn]
    basis, nxt = gr.multi_dot_case(tn, rows, num, nrhs, exact)
    got, = twice(lambda: (run_multi_dot(gexec, tn, basis, nxt),))
    ref, s = gr.multi_dot(br.hp(t), basis, nxt)
    if rows == 0:
        assert same_bits(got, np.zeros((num, nrhs), t))
    elif exact:
        assert np.array_equal(got, ref.astype(t)), ("multi_dot exact", tn, rows, num, nrhs)
    else:
        bound = gr.dot_bound(t, gr.multi_dot_depth(rows), s)
        err = np.abs(got.astype(_wide(t)) - ref)
        _note("bound", f"multi_dot rows {rows} num {num} nrhs {nrhs}", tn, np.max(err / bound))
        assert np.all(err <= bound), ("multi_dot", tn, rows, num, nrhs, float(np.max(err / bound)))


@pytest.mark.parametrize("tn", TYPES)
@pytest.mark.parametrize("rows", gr.MULTI_DOT_ROWS)
def test_multi_dot(gexec, tn, rows):
    """gap 3: no rows (the memset), the chunk boundary 1023 / 1024 / 1025, several chunks, and 258 chunks - the
    second trip of stage 2; 1, 3 and 8 dots, 1 and 3 columns"""
    for num in (1, 3, 8):
        for nrhs in (1, 3):
            check_multi_dot(gexec, tn, rows, num, nrhs)
    if gr.needs_exact(tn, rows) or rows in (1025, 100003):
        check_multi_dot(gexec, tn, rows, 3, 1, exact=True)


# ------------------------------------------------------------------------------------------- mgs_step
ALIGNED = 4                  # element offset of a vector inside its buffer: 4 elements are 16 bytes or more


def _need_x(n, t):
    from ginkgo_amd._lib import lib
    return int(lib().gkoc_x_workspace_bytes(C.c_int64(n), C.c_size_t(np.dtype(t).itemsize)))


def _vec(gexec, v, off):
    a = np.full(v.shape[0] + 8, CANARY, v.dtype)
    a[off:off + v.shape[0]] = v
    return Dev(gexec, a), a


def run_mgs(gexec, tn, w, v, h, vn, offs=(ALIGNED,) * 3, short=0, rows=None, null_h_next=False):
    """returns (w after, h_next) ; with short / rows / null_h_next the refused call's status instead of h_next"""
    t = br.TYPES[tn]
    n = w.shape[0]
    wb = _need_x(n, t)
    (dw, hw), (dv, hv), (dvn, hvn) = (_vec(gexec, z, o) for z, o in zip((w, v, vn), offs))
    dh, hn = Flat(gexec, np.array([h], t)), Flat(gexec, nans(1, t))
    work = Flat(gexec, np.zeros(wb, np.uint8))
    args = (gexec.stream, n if rows is None else rows, dw.at(offs[0]), dv.at(offs[1]), dh, dvn.at(offs[2]),
            None if null_h_next else hn, work, C.c_size_t(wb - short))
    status = _status("gkoc_x_gmres_mgs_step_" + tn, *args)
    sync()
    work.get()
    assert same_bits(dv.get(), hv) and same_bits(dvn.get(), hvn) and dh.unchanged()
    full = dw.get()
    hw[offs[0]:offs[0] + n] = full[offs[0]:offs[0] + n]
    assert same_bits(full, hw), "written around w"
    return full[offs[0]:offs[0] + n].copy(), (hn.get()[0] if status == 0 else (status, hn.get()[0]))


def check_mgs(gexec, tn, n, zero_h, offs=(ALIGNED,) * 3, exact=False):
    t = br.TYPES[tn]
    w, v, h, vn = gr.mgs_case(tn, n, zero_h, exact)
    got_w, got_h = twice(lambda: run_mgs(gexec, tn, w, v, h, vn, offs))
    ref_w = gr.mgs_step(br.plain(t), w, v, h, vn)[0]
    assert same_bits(got_w, ref_w), ("mgs_step w", tn, n, offs, _first_diff(got_w, ref_w))
    if zero_h:
        assert same_bits(got_w, w)
    terms = np.conj(vn.astype(_wide(t))) * got_w                  # the dot of the kernel's own, rounded w
    ref = np.sum(terms) if n else _wide(t)(0)
    if n == 0:
        assert same_bits(np.array([got_h]), np.zeros(1, t))
    elif exact:
        assert got_h == t(ref), ("mgs_step exact", tn, n, got_h, ref)
    else:
        vec_ok = all((o * np.dtype(t).itemsize) % 16 == 0 for o in offs)
        bound = gr.dot_bound(t, gr.mgs_step_depth(n, gr.vec_width(t), vec_ok), np.sum(np.abs(terms)))
        err = abs(_wide(t)(got_h) - ref)
        _note("bound", f"mgs_step n {n} offsets {offs} zero_h {zero_h}", tn, err / bound)
        assert err <= bound, ("mgs_step h_next", tn, n, offs, float(err / bound))


MGS_CASES = [(tn, n) for tn in TYPES for n in gr.MGS_ROWS if n <= gr.SINGLE_TEETH_LIMIT or tn in gr.MGS_BIG_TYPES]


@pytest.mark.parametrize("tn,n", MGS_CASES)
def test_mgs_step(gexec, tn, n):
    """gap 4: all three vectors aligned and each one in turn one element further (vec_ok false, except for c128,
    whose elements are 16 bytes), the scalar tail n % W, h_cur zero (noop) and non-zero, and 4 196 353 rows, where
    the cap of 2048 blocks binds"""
    if n > gr.SINGLE_TEETH_LIMIT:
        check_mgs(gexec, tn, n, False)
        if gr.needs_exact(tn, n):
            check_mgs(gexec, tn, n, False, exact=True)
        return
    for zero_h in (False, True):
        check_mgs(gexec, tn, n, zero_h)
        for k in range(3):
            offs = tuple(ALIGNED + (1 if j == k else 0) for j in range(3))
            check_mgs(gexec, tn, n, zero_h, offs)
    if n in (5, 2047, 100003):
        check_mgs(gexec, tn, n, False, exact=True)
        check_mgs(gexec, tn, n, False, (ALIGNED + 1, ALIGNED, ALIGNED), exact=True)


# ------------------------------------------------------------------------ hessenberg_qr, solve_krylov
class Sweep:
    """the operands of hessenberg_qr and solve_krylov on the device, every one with its own leading dimension"""

    def __init__(self, gexec, tn, kd, nrhs, beta):
        self.gexec, self.tn, self.kd, self.nrhs = gexec, tn, kd, nrhs
        t = self.t = br.TYPES[tn]
        self.gsin, self.gcos = Mat(gexec, nans((kd, nrhs), t), 1), Mat(gexec, nans((kd, nrhs), t), 2)
        rnc = nans((kd + 1, nrhs), t)
        rnc[0] = beta
        self.rnc = Mat(gexec, rnc, 3)
        self.rn = Flat(gexec, beta.astype(br.real_of(t)))
        self.hess = Mat(gexec, nans((kd, (kd + 1) * nrhs), t), 2)
        self.fin = Flat(gexec, np.zeros(nrhs, np.uint64))

    def state(self):
        return dict(gsin=self.gsin.get(), gcos=self.gcos.get(), rn=self.rn.get(), rnc=self.rnc.get(),
                    hess=self.hess.get().reshape(self.kd, self.kd + 1, self.nrhs), fin=self.fin.get())

    def put_column(self, it, hcol):
        full = self.hess.get()
        full[it, :(it + 2) * self.nrhs] = hcol.reshape(-1)
        self.hess = Mat(self.gexec, full, 2)

    def qr(self, it, stop):
        dstop = Flat(self.gexec, stop)
        call("gkoc_common_gmres_hessenberg_qr_" + self.tn, self.gexec.stream, self.nrhs, self.gsin, self.gsin.ld,
             self.gcos, self.gcos.ld, self.rn, self.rnc, self.rnc.ld, self.hess.row(it), self.nrhs, it, self.fin,
             dstop)
        sync()
        assert dstop.unchanged()

    def solve(self, stop):
        y, dstop = Mat(self.gexec, nans((self.kd, self.nrhs), self.t), 4), Flat(self.gexec, stop)
        inputs = (self.rnc, self.hess, self.fin)
        before = [z.dev.get() for z in inputs]
        call("gkoc_common_gmres_solve_krylov_" + self.tn, self.gexec.stream, self.nrhs, self.rnc, self.rnc.ld,
             self.hess, self.hess.ld, y, y.ld, self.fin, dstop)
        sync()
        assert dstop.unchanged() and all(same_bits(z.dev.get(), b) for z, b in zip(inputs, before))
        return y.get()


def run_sweep(gexec, tn, kd, nrhs, hraw, beta, stopped_col, finalized_col):
    """a full sweep on the device; every step is compared with the restatements started from the device's own
    state before it.  Returns the final state with y"""
    t = br.TYPES[tn]
    cx = br.is_complex(t)
    sw = Sweep(gexec, tn, kd, nrhs, beta)
    for it in range(kd):
        stop = np.zeros(nrhs, np.uint8)
        if stopped_col is not None and it >= 2:
            stop[stopped_col] = gr.STOPPED
        sw.put_column(it, hraw[it])
        before = sw.state()
        sw.qr(it, stop)
        after = sw.state()
        names = ("gsin", "gcos", "rn", "rnc", "hcol", "fin")
        args = (before["gsin"], before["gcos"], before["rn"], before["rnc"], hraw[it], it, before["fin"], stop)
        plain = dict(zip(names, gr.hessenberg_qr(br.plain(t), *args)))
        got = dict(after, hcol=after["hess"][it, :it + 2])
        if stopped_col is not None and it >= 2:                # the stopped column keeps its bits and its count
            for name in ("gsin", "gcos", "rnc"):
                assert same_bits(after[name][:, stopped_col], before[name][:, stopped_col])
            assert after["fin"][stopped_col] == 2 and same_bits(after["rn"][stopped_col], before["rn"][stopped_col])
            assert same_bits(got["hcol"][:, stopped_col], hraw[it][:, stopped_col])
        if cx:
            # what follows the modulus: rule R against long double from the same state; the rest bit for bit
            hp = dict(zip(names, gr.hessenberg_qr(br.hp(t), *args)))
            act = stop == 0
            for name, rows in (("gsin", [it]), ("gcos", [it]), ("rnc", [it, it + 1]), ("hcol", [it])):
                for r in rows:
                    ok, ratio = br.rule_r(got[name][r, act], hp[name][r, act], plain[name][r, act], t)
                    _note("ratio", "hessenberg_qr " + name, tn, ratio)
                    assert ok, ("hessenberg_qr", name, tn, kd, nrhs, it, ratio)
                    plain[name][r, act] = got[name][r, act]
            ok, ratio = br.rule_r(got["rn"][act], hp["rn"][act], plain["rn"][act], t)
            _note("ratio", "hessenberg_qr residual_norm", tn, ratio)
            assert ok, ("hessenberg_qr residual_norm", tn, kd, nrhs, it, ratio)
            plain["rn"][act] = got["rn"][act]
            assert not got["hcol"][it + 1, act].any()                    # the rotated sub-diagonal: exactly zero
        for name in names:
            assert same_bits(got[name], plain[name]), \
                ("hessenberg_qr", name, tn, kd, nrhs, it, _first_diff(got[name], plain[name]))
        assert same_bits(after["hess"][it + 1:], before["hess"][it + 1:]) and \
            same_bits(after["hess"][:it], before["hess"][:it])
    stop = np.zeros(nrhs, np.uint8)
    if finalized_col is not None:
        stop[finalized_col] = gr.FINALIZED
    st = sw.state()
    y = sw.solve(stop)
    assert same_bits(sw.solve(stop), y), "two runs differ"
    ref = gr.solve_krylov(br.plain(t), st["rnc"], st["hess"], st["fin"], stop, nans((kd, nrhs), t))
    assert same_bits(y, ref), ("solve_krylov", tn, kd, nrhs, _first_diff(y, ref))
    if finalized_col is not None:
        assert np.all(np.isnan(y[:, finalized_col].real))
    return dict(st, y=y)


SWEEP_CASES = [(kd, nrhs) for kd in (1, 2, 7) for nrhs in (1, 5, 257)]


@pytest.mark.parametrize("tn", TYPES)
@pytest.mark.parametrize("kd,nrhs", SWEEP_CASES)
def test_hessenberg_qr_and_solve_krylov(gexec, tn, kd, nrhs):
    """gaps 5, 7, 8: a full sweep iter = 0 .. kd - 1 and the back substitution, with a zero pivot, a column
    stopped from iteration 2 on, a finalized column in solve_krylov, and a column index of 256"""
    t = br.TYPES[tn]
    zp = (min(1, kd - 1), 0)
    stopped = nrhs - 1 if (nrhs > 1 and kd > 2) else None
    finalized = 2 if nrhs > 2 else None
    hraw, beta = gr.hessenberg_case(100 * kd + nrhs, t, kd, nrhs, zero_pivot=zp)
    first = run_sweep(gexec, tn, kd, nrhs, hraw, beta, stopped, finalized)
    second = run_sweep(gexec, tn, kd, nrhs, hraw, beta, stopped, finalized)
    assert all(same_bits(first[k], second[k]) for k in first), "two sweeps differ"
    assert first["gcos"][zp[0], zp[1]] == 0 and first["gsin"][zp[0], zp[1]] == 1        # the zero-pivot branch
    cs = np.abs(first["gcos"].astype(_wide(t))) ** 2 + np.abs(first["gsin"].astype(_wide(t))) ** 2
    free = gr.sweep(br.plain(t), hraw, beta, stop_from={stopped: 2} if stopped is not None else None)
    cols = range(nrhs) if nrhs <= 5 else (0, 1, 3, 255, 256)
    for k in cols:
        m = int(first["fin"][k])
        assert m == (2 if k == stopped else kd)
        assert np.all(np.abs(cs[:m, k] - 1) <= 8 * br.eps_of(t))
        if k == finalized:
            continue
        e1 = np.zeros(m + 1, np.longdouble)
        e1[0] = beta[k]
        y, res = gr.lstsq_hp(gr.dense_hessenberg(hraw, k)[:m + 1, :m], e1)
        ok, ratio = br.rule_r(first["y"][:m, k], y, free["y"][:m, k], t)
        if float(np.max(np.abs(y))) > br.eps_of(t) * float(beta[k]):      # (a solution that is zero has no scale)
            _note("ratio", "sweep y vs lstsq", tn, ratio)
        assert ok, ("least squares y", tn, kd, nrhs, k, ratio)
        if k != stopped:
            ok, ratio = br.rule_r(first["rn"][k:k + 1], np.array([res]), free["rn"][k:k + 1], t)
            _note("ratio", "sweep residual_norm vs lstsq", tn, ratio)
            assert ok, ("least squares residual", tn, kd, nrhs, k, ratio)


# --------------------------------------------------------------------------------- refused arguments
@pytest.mark.parametrize("tn", TYPES)
def test_refused_before_any_launch(gexec, tn):
    """what the entry points refuse before they launch anything: a workspace one byte short (GKOC_E_WORKSPACE),
    rows < 0 and a null h_next of mgs_step (GKOC_E_INVALID).  The outputs keep their bits, and a valid call
    afterwards still gives the right answer"""
    t = br.TYPES[tn]
    basis, nxt = gr.multi_dot_case(tn, 1025, 3, 3)
    got = run_multi_dot(gexec, tn, basis, nxt, short=1)
    assert same_bits(got, nans((3, 3), t))
    check_multi_dot(gexec, tn, 1025, 3, 3)
    w, v, h, vn = gr.mgs_case(tn, 2047)
    for kw, status in ((dict(short=1), -3), (dict(rows=-1), -1), (dict(null_h_next=True), -1)):
        got_w, (got_status, h_next) = run_mgs(gexec, tn, w, v, h, vn, **kw)
        assert got_status == status and same_bits(got_w, w) and same_bits(np.array([h_next]), nans(1, t)), kw
    check_mgs(gexec, tn, 2047, False)

