"""The block-Jacobi kernels of csrc/jacobi.hip through the C ABI, at the smallest shapes that select each branch of
their launchers, against the numpy restatement of tests/jacobi_refs.py (checked on its own by
tests/test_jacobi_refs_cpu.py, which also asserts the pivot margins and zero pivots of the inputs used here).

Every value output starts as NaN and is followed by canaries; strided operands are cut from padded arrays whose
padding must survive; every input is read back and compared bit for bit.  The condition that selects a branch is
restated in Python (jacobi_refs.apply_branch, wide_group_layout, ...) and asserted from the scheme and the arguments
of the case, addresses included.

Acceptance.  find_blocks: exact.  generate: real types bit-identical to the plain restatement, storage outside the
blocks untouched; complex types bit-identical where that holds, else rule R against the long-double inverse with the
same pivots (binding_refs.rule_r) - which of the two held is printed by the last test.  Products: bit-identical to
the restatement on every branch (real types: sum = x beta, sum += (alpha m) b in column order; other types: sum = 0,
sum += m b, alpha sum + beta x), except the matrix-core kernel: |x - hp| <= (bs + 2) eps sum_c |alpha m_c b_c| +
eps |beta x| per entry.  Reduced storage: stored bytes and products bit for bit.  Fused kernels: vectors
bit-identical, each reduced scalar within (depth + 1) eps sum |terms| of the long-double sum over the kernel's own
vectors (jacobi_refs.fused_dot_depth), equal on integer-valued inputs.

Figures (rule-R ratios, fractions of bounds) are printed by the last test (pytest -s)."""
import ctypes as C
import re

import numpy as np
import pytest

import binding_refs as br
import jacobi_refs as jr
import value_kernel_refs as vr
from binding_gpu import CANARY, Dev, DevCsr, call, padded, same_bits, sync

pytestmark = pytest.mark.gpu

REAL, CPLX = ("f64", "f32"), ("c128", "c64")
TYPES = REAL + CPLX
IT = {"i32": np.int32, "i64": np.int64}
INVALID, NOT_SUPPORTED, WORKSPACE = -1, -2, -3
TUNE_XCD_MAP, TUNE_LANES = 1, 15
SENTINEL = -99
FIGURES = {}            # what the last test prints: name -> largest observed figure
HELD = {}               # complex generate: (type, max_block_size) -> "bits" or "rule R"


def _figure(name, v):
    FIGURES[name] = max(FIGURES.get(name, 0.0), float(v))


def _status(fn):
    from ginkgo_amd._lib import NotSupported
    try:
        fn()
    except NotSupported:
        return NOT_SUPPORTED
    except Exception as e:          # ginkgo_amd._lib.GkoError
        m = re.search(r"failed with status (-?\d+):", str(e))
        return int(m.group(1)) if m else None
    return 0


def _scheme(sc):
    from ginkgo_amd._lib import JacobiScheme
    return JacobiScheme(*sc.as_tuple())


def _nan(shape, t):
    return np.full(shape, np.nan, t) if not br.is_complex(t) else np.full(shape, complex(np.nan, np.nan), t)


class Vec:
    """a rows x cols operand with leading dimension ld, `shift` elements behind a 16-byte-aligned address, inside a
    device array that holds canaries in front of it, in its padding and behind it"""

    def __init__(self, gexec, a, ld=None, shift=0):
        a = np.asarray(a)
        self.rows, self.cols = a.shape
        self.ld, self.shift = max(self.cols, 1) if ld is None else ld, shift
        fill = np.full(3, CANARY, a.dtype)
        self.host = np.concatenate([np.full(shift, CANARY, a.dtype), padded(a, self.ld).reshape(-1), fill])
        self.dev = Dev(gexec, self.host)
        self.ptr = self.dev.at(shift)

    def get(self):
        full = self.dev.get()
        keep = np.ones(full.shape, bool)
        body = keep[self.shift:self.shift + self.rows * self.ld].reshape(self.rows, self.ld)
        body[:, :self.cols] = False
        assert same_bits(full[keep], self.host[keep]), "a canary around an operand was overwritten"
        inner = full[self.shift:self.shift + self.rows * self.ld].reshape(self.rows, self.ld)
        return np.ascontiguousarray(inner[:, :self.cols])

    def unchanged(self):
        return same_bits(self.dev.get(), self.host)


class Flat:
    """a flat device array followed by three canaries"""

    def __init__(self, gexec, a):
        a = np.ascontiguousarray(a).reshape(-1)
        self.n = a.shape[0]
        canary = 0x5a if a.dtype.kind == "u" else CANARY
        self.host = np.concatenate([a, np.full(3, canary, a.dtype)])
        self.dev = Dev(gexec, self.host)
        self._as_parameter_ = self.dev._as_parameter_

    def get(self):
        full = self.dev.get()
        assert same_bits(full[self.n:], self.host[self.n:]), "written behind the end"
        return full[:self.n]

    def unchanged(self):
        return same_bits(self.dev.get(), self.host)


class Blk:
    """the preconditioner of a case on the device: block pointers in index type itn, block storage, precisions"""

    def __init__(self, gexec, itn, a, blocks=None, prec=None):
        self.a, self.itn = a, itn
        self.ptrs = Flat(gexec, a["block_ptrs"].astype(IT[itn]))
        self.blocks = Flat(gexec, a["blocks"] if blocks is None else blocks)
        self.prec = None if prec is None else Flat(gexec, np.asarray(prec, np.uint8))
        self.sc, self.nb, self.mbs = _scheme(a["scheme"]), int(a["num_blocks"]), C.c_uint32(a["max_block_size"])

    def head(self, gexec):
        return gexec.stream, self.nb, self.mbs, self.sc, self.ptrs, self.blocks

    def unchanged(self):
        return self.ptrs.unchanged() and self.blocks.unchanged() and (self.prec is None or self.prec.unchanged())


def run_apply(gexec, tn, blk, b, kind="plain", adv=None, x0=None, ldb=None, ldx=None, shift_b=0, shift_x=0,
              prec=None, expect=None, nrhs=None):
    """one product through gkoc_jacobi_simple_apply / apply (kind plain), apply_stored_f64 (stored: prec = the byte)
    or apply_adaptive (adaptive: blk.prec); adv = (alpha, beta).  x starts as NaN unless x0 is given.  expect: the
    branch of launch_apply the case must select.  Returns x"""
    t = br.TYPES[tn]
    b = np.asarray(b)
    nrhs = b.shape[1] if nrhs is None else nrhs
    bv = Vec(gexec, b, ldb, shift_b)
    xv = Vec(gexec, _nan(b.shape, t) if x0 is None else x0, ldx, shift_x)
    if expect is not None:
        got = jr.apply_branch(blk.a["scheme"], np.dtype(t).itemsize, nrhs, bv.ld, xv.ld, bv.ptr.value, xv.ptr.value)
        assert got == expect, (got, expect)
    al = be = None
    if adv is not None:
        al, be = Flat(gexec, np.array([adv[0]], t)), Flat(gexec, np.array([adv[1]], t))
    tail = (bv.ptr, bv.ld, be, xv.ptr, xv.ld, nrhs)
    if kind == "plain" and adv is None:
        call(f"gkoc_jacobi_simple_apply_{tn}_{blk.itn}", *blk.head(gexec), bv.ptr, bv.ld, xv.ptr, xv.ld, nrhs)
    elif kind == "plain":
        call(f"gkoc_jacobi_apply_{tn}_{blk.itn}", *blk.head(gexec), al, *tail)
    elif kind == "stored":
        call(f"gkoc_jacobi_apply_stored_f64_{blk.itn}", *blk.head(gexec), C.c_uint8(prec), al, *tail)
    else:
        call(f"gkoc_jacobi_apply_adaptive_{tn}_{blk.itn}", *blk.head(gexec), blk.prec, al, *tail)
    sync()
    assert bv.unchanged() and blk.unchanged(), "an input of the product was written"
    assert al is None or (al.unchanged() and be.unchanged())
    return xv.get()


def tune_get(key):
    from ginkgo_amd._lib import lib
    v = C.c_int64(0)
    assert lib().gkoc_tune_get(C.c_int(key), C.byref(v)) == 0
    return v.value


def tune_set(key, value):
    from ginkgo_amd._lib import lib
    assert lib().gkoc_tune_set(C.c_int(key), C.c_int64(value)) == 0


# --------------------------------------------------------------------------------------------- find_blocks
def run_find_blocks(gexec, tn, itn, rp, cols, max_bs):
    n = len(rp) - 1
    csr = DevCsr(gexec, IT[itn], rp, cols if len(cols) else np.zeros(1, np.int64))
    out = Flat(gexec, np.full(n + 1, SENTINEL, IT[itn]))
    nb = C.c_int64(-5)
    call(f"gkoc_jacobi_find_blocks_{tn}_{itn}", gexec.stream, n, csr.dev[0], csr.dev[1], C.c_uint32(max_bs),
         C.byref(nb), out)
    sync()
    assert csr.unchanged()
    return nb.value, out.get()


@pytest.mark.parametrize("itn", ("i32", "i64"))
def test_find_blocks(gexec, itn):
    """n 0 .. 100 003 x max_block_size 1 .. 64 x the four patterns: the block pointers of the restatement, the entries
    behind num_blocks + 1 keep their fill.  The chain pattern with max_block_size 1 at 100 003 rows is the longest
    chain mark_chain doubles its way along"""
    for i, n in enumerate((0, 1, 255, 256, 257, 100003)):
        for max_bs in (1, 2, 13, 32, 64):
            for kind in jr.PATTERNS:
                rp, cols = jr.pattern(kind, n, max_bs)
                want = jr.find_blocks(rp, cols, max_bs)
                tn = TYPES[(i + max_bs) % 4]             # the four value-type names share one body
                nb, got = run_find_blocks(gexec, tn, itn, rp, cols, max_bs)
                assert nb == len(want) - 1, (n, max_bs, kind, nb)
                assert np.array_equal(got[:nb + 1], want), (n, max_bs, kind)
                assert np.all(got[nb + 1:] == SENTINEL), (n, max_bs, kind, "written behind num_blocks + 1")
                if kind == "same" and n > max_bs:
                    assert np.all(np.diff(want)[:-1] == max_bs)
                if kind == "chain" and max_bs == 1:
                    assert nb == n


@pytest.mark.parametrize("itn", ("i32", "i64"))
def test_find_blocks_refusals(gexec, itn):
    """max_block_size 0 and 65: GKOC_E_NOT_SUPPORTED, neither num_blocks nor block_ptrs written"""
    rp, cols = jr.pattern("same", 9, 4)
    for max_bs in (0, 65):
        csr = DevCsr(gexec, IT[itn], rp, cols)
        out = Flat(gexec, np.full(10, SENTINEL, IT[itn]))
        nb = C.c_int64(-5)
        assert _status(lambda: call(f"gkoc_jacobi_find_blocks_f64_{itn}", gexec.stream, 9, csr.dev[0], csr.dev[1],
                                    C.c_uint32(max_bs), C.byref(nb), out)) == NOT_SUPPORTED
        sync()
        assert nb.value == -5 and out.unchanged() and csr.unchanged()


# ------------------------------------------------------------------------------------------------ generate
_REFS = {}


def generate_refs(tn, max_bs):
    """(plain storage over a NaN fill, its runs, long-double storage with the same pivots), computed once"""
    key = (tn, max_bs)
    if key not in _REFS:
        t = br.TYPES[tn]
        c = jr.generate_case(tn, max_bs)
        size = jr.storage_size(c["scheme"], len(c["block_ptrs"]) - 1)
        args = (c["row_ptrs"], c["cols"], c["vals"], c["scheme"], c["block_ptrs"])
        pl, runs = jr.generate(br.plain(t), *args, _nan(size, t))
        hp, _ = jr.generate(br.hp(t), *args, np.zeros(size), pivots=[r["pivots"] for r in runs])
        _REFS[key] = (pl, runs, hp)
    return _REFS[key]


def run_generate(gexec, tn, itn, c, max_bs, conditioning=None):
    t = br.TYPES[tn]
    nb = len(c["block_ptrs"]) - 1
    size = jr.storage_size(c["scheme"], nb)
    csr = DevCsr(gexec, IT[itn], c["row_ptrs"], c["cols"], c["vals"])
    ptrs = Flat(gexec, c["block_ptrs"].astype(IT[itn]))
    out = Flat(gexec, _nan(size, t))
    call(f"gkoc_jacobi_generate_{tn}_{itn}", gexec.stream, c["n"], *csr.dev, nb, C.c_uint32(max_bs), _scheme(c["scheme"]),
         ptrs, out, conditioning)
    sync()
    assert csr.unchanged() and ptrs.unchanged(), "an input of generate was written"
    return out


@pytest.mark.parametrize("itn", ("i32", "i64"))
@pytest.mark.parametrize("tn", TYPES)
def test_generate(gexec, tn, itn):
    """max_block_size 1 .. 64 (complex: 32): per_wave k + 1 blocks of mixed sizes in one wave, a zero leading entry,
    exact ties, exactly singular blocks (stored half transformed, as the restatement leaves them), entries outside
    the blocks, unsorted columns, missing entries; the padding of the storage groups keeps its NaN fill"""
    t = br.TYPES[tn]
    sizes = jr.GENERATE_SIZES[tn]
    for max_bs in (sizes if itn == "i32" else (1, 8, 13, sizes[-1])):
        c = jr.generate_case(tn, max_bs)
        pl, runs, hp = generate_refs(tn, max_bs)
        got = run_generate(gexec, tn, itn, c, max_bs).get()
        mask = jr.entry_mask(c["scheme"], c["block_ptrs"], got.shape[0])
        assert same_bits(got[~mask], pl[~mask]), (tn, max_bs, "the padding of the storage was written")
        if not br.is_complex(t):
            assert same_bits(got, pl), (tn, max_bs, int(np.flatnonzero(got.view(np.uint8) != pl.view(np.uint8))[0]))
            continue
        # the singular and the zero-lead blocks hold small dyadic numbers, exact in any arithmetic: the values of the
        # restatement's (half-transformed) block; the sign of a zero part is left to rule R's side of the promise
        for b, name in enumerate(c["names"]):
            if name in ("singular", "zero_lead"):
                for _, _, idx in jr.block_entries(c["scheme"], c["block_ptrs"][b:b + 2] - c["block_ptrs"][b]):
                    at = idx.reshape(-1) + vr.block_start(c["scheme"], b)
                    assert np.array_equal(got[at], pl[at]), (tn, max_bs, b, name)
        if same_bits(got, pl):
            HELD[tn, max_bs] = "bits"
            continue
        # complex<double>: the header promises the restatement's bits
        assert tn != "c128", (tn, max_bs, int(np.flatnonzero(got.view(np.uint8) != pl.view(np.uint8))[0]))
        HELD[tn, max_bs] = "rule R"
        _figure(f"generate {tn} entries that differ from the plain restatement in value", np.count_nonzero(got[mask] != pl[mask]))
        ok, ratio = br.rule_r(got[mask], hp[mask], pl[mask], t)
        _figure(f"generate {tn} inverse blocks, rule R", ratio)
        assert ok, (tn, max_bs, ratio)


@pytest.mark.parametrize("tn", TYPES)
def test_generate_refusals(gexec, tn):
    """a conditioning array, and complex blocks of 33 rows: GKOC_E_NOT_SUPPORTED, the storage keeps its fill"""
    t = br.TYPES[tn]
    c = jr.generate_case(tn, 4)
    nb = len(c["block_ptrs"]) - 1
    cond = Flat(gexec, _nan(nb, t))
    csr = DevCsr(gexec, np.int32, c["row_ptrs"], c["cols"], c["vals"])
    ptrs = Flat(gexec, c["block_ptrs"].astype(np.int32))
    out = Flat(gexec, _nan(jr.storage_size(c["scheme"], nb), t))
    for max_bs, sc, cnd in ((4, c["scheme"], cond),) + (((33, jr.storage_scheme(33), None),) if br.is_complex(t) else ()):
        assert _status(lambda: call(f"gkoc_jacobi_generate_{tn}_i32", gexec.stream, c["n"], *csr.dev, nb,
                                    C.c_uint32(max_bs), _scheme(sc), ptrs, out, cnd)) == NOT_SUPPORTED
    sync()
    assert out.unchanged() and cond.unchanged() and csr.unchanged()


# ------------------------------------------------------------- simple_apply / apply, real types (launch_apply)
def check_products(gexec, tn, blk, a, expect=None, ref=jr.apply_tuned, what="", **layout):
    """x = M b, x = beta x + alpha M b, and beta = 0 over a NaN x, each bit-identical to the restatement"""
    t = br.TYPES[tn]
    pl = br.plain(t)
    args = (a["scheme"], a["block_ptrs"], blk.blocks_seen if hasattr(blk, "blocks_seen") else a["blocks"], a["b"])
    kw = dict(expect=expect, **layout)
    got = run_apply(gexec, tn, blk, a["b"], **kw)
    assert same_bits(got, ref(pl, *args)), (what, tn, "x = M b")
    al, be = a["alpha"][0], a["beta"][0]
    got = run_apply(gexec, tn, blk, a["b"], adv=(al, be), x0=a["x0"], **kw)
    assert same_bits(got, ref(pl, *args, al, be, a["x0"])), (what, tn, "x = beta x + alpha M b")
    got = run_apply(gexec, tn, blk, a["b"], adv=(al, t(0)), **kw)
    assert same_bits(got, ref(pl, *args, al, t(0), a["x0"])), (what, tn, "beta = 0 over a NaN x")


def group_counts(bo, value_size):
    """block counts of the one-column cases: one partly filled group; 4 GPW groups (one workgroup), one more, one
    fewer; three groups (odd: the second group of a GPW = 2 wave stays empty)"""
    gs = 64 // bo
    gpw = jr.groups_per_wave(bo, value_size)
    return [max(1, gs - 1), 4 * gpw * gs, (4 * gpw + 1) * gs, (4 * gpw - 1) * gs, 3 * gs - (1 if gs > 1 else 0)]


@pytest.mark.parametrize("bo", (1, 2, 4, 8, 16))
@pytest.mark.parametrize("tn", REAL)
def test_apply_one_column(gexec, tn, bo):
    """jacobi_apply_fixed_kernel<BO, GPW>: every group count of `group_counts`, the last block shorter than
    block_offset; and one column with ldb = 3, ldx = 2, which drops to the general kernel"""
    vs = np.dtype(br.TYPES[tn]).itemsize
    for i, nb in enumerate(group_counts(bo, vs)):
        a = jr.apply_case(tn, bo, nb, 1)
        assert jr.wide_group_layout(a["scheme"]) and (bo == 1 or np.diff(a["block_ptrs"])[-1] < bo)
        blk = Blk(gexec, ("i32", "i64")[i % 2], a)
        check_products(gexec, tn, blk, a, expect=("fixed", None), what=f"bo {bo}, {nb} blocks")
    check_products(gexec, tn, blk, a, expect=("general", None), ldb=3, ldx=2, what=f"bo {bo}, strided column")


@pytest.mark.parametrize("tn", REAL)
def test_apply_several_columns_wide(gexec, tn):
    """jacobi_apply_fixed_multi_kernel: 2, 3, 4 columns (PC = 4), 5, 7, 8 (PC = 8), 9 and 17 at block_offset 4 and 16
    (several passes and a tail pass); even strides on an aligned base (pairs), the same strides one element on, odd
    strides; two workgroups, the last group partly filled"""
    cases = [(8, k) for k in (2, 3, 4, 5, 7, 8)] + [(bo, k) for bo in (4, 16) for k in (9, 17)] + [(1, 3), (2, 5)]
    if tn == "f32":
        cases += [(8, 9), (8, 17)]                  # no matrix-core kernel in float
    for i, (bo, nrhs) in enumerate(cases):
        nb = 5 * (64 // bo) - 1
        a = jr.apply_case(tn, bo, nb, nrhs)
        blk = Blk(gexec, ("i32", "i64")[i % 2], a)
        name = "multi4" if nrhs <= 4 else "multi8"
        even = nrhs + 2 - nrhs % 2
        for ldb, ldx, shift, pairs in ((even, even + 2, 0, True), (even, even + 2, 1, False), (nrhs + 1 - nrhs % 2, even + 1, 0, False)):
            check_products(gexec, tn, blk, a, expect=(name, pairs), ldb=ldb, ldx=ldx, shift_b=shift, shift_x=shift,
                           what=f"bo {bo}, {nrhs} columns, ld {ldb} / {ldx}, shift {shift}")
    # x alone off the pair alignment
    check_products(gexec, tn, blk, a, expect=(name, False), ldb=even, ldx=even, shift_x=1, what="x shifted")


@pytest.mark.parametrize("max_bs", (3, 5, 13, 32, 64))
@pytest.mark.parametrize("tn", REAL)
def test_apply_general_layouts(gexec, tn, max_bs):
    """jacobi_apply_kernel on the schemes that are not wide: one column and three strided ones; five groups"""
    sc = jr.storage_scheme(max_bs)
    assert not jr.wide_group_layout(sc)
    for itn, nrhs, ld in (("i32", 1, 1), ("i64", 3, 5)):
        a = jr.apply_case(tn, max_bs, 4 * sc.group_size + 1, nrhs)
        check_products(gexec, tn, Blk(gexec, itn, a), a, expect=("general", None), ldb=ld, ldx=ld + 1,
                       what=f"max_block_size {max_bs}, {nrhs} columns")


def test_apply_matrix_core_branch(gexec):
    """jacobi_apply_mfma_kernel (f64, block_offset 8, from nine columns): 9, 16, 17, 33 columns, the last group partly
    filled; per entry |x - hp| <= (bs + 2) eps sum_c |alpha m_c b_c| + eps |beta x|"""
    t, eps = np.float64, br.eps_of(np.float64)
    for i, nrhs in enumerate((9, 16, 17, 33)):
        a = jr.apply_case("f64", 8, 5 * 8 - 3, nrhs)
        blk = Blk(gexec, ("i32", "i64")[i % 2], a)
        args = (a["scheme"], a["block_ptrs"], a["blocks"], a["b"])
        bs = np.repeat(np.diff(a["block_ptrs"]), np.diff(a["block_ptrs"]))[:, None].astype(np.longdouble)
        for adv, x0, beta_x in ((None, None, 0.0), ((a["alpha"][0], a["beta"][0]), a["x0"], np.abs(a["beta"][0] * a["x0"])),
                                ((a["alpha"][0], t(0)), None, 0.0)):
            got = run_apply(gexec, "f64", blk, a["b"], adv=adv, x0=x0, ldb=nrhs + 1, ldx=nrhs + 2, expect=("mfma", None))
            al = None if adv is None else adv[0]
            hp = jr.apply_tuned(br.hp(t), *args, *(() if adv is None else (adv[0], adv[1], a["x0"])))
            bound = (bs + 2) * eps * jr.apply_abs_sum(*args, alpha=al) + eps * beta_x
            err = np.abs(got.astype(np.longdouble) - hp)
            _figure("matrix-core product, fraction of the per-entry bound", np.max(err / bound))
            assert np.all(err <= bound), (nrhs, adv, float(np.max(err / bound)))


@pytest.mark.parametrize("tn", REAL)
def test_apply_special_arguments(gexec, tn):
    """num_blocks = 0 and nrhs = 0 write nothing; max_block_size > block_offset: GKOC_E_INVALID; a scheme wider than a
    wavefront: GKOC_E_NOT_SUPPORTED; b == x: GKOC_E_INVALID (b and x must not overlap).  Nothing is written"""
    t = br.TYPES[tn]
    a = jr.apply_case(tn, 8, 11, 2)
    blk = Blk(gexec, "i32", a)
    bv, xv = Vec(gexec, a["b"], 3), Vec(gexec, _nan(a["b"].shape, t), 4)
    al, be = Flat(gexec, a["alpha"]), Flat(gexec, a["beta"])
    wide = jr.Scheme(8, 8 * 128, 4)
    assert (wide.block_offset << wide.group_power) > 64

    def simple(nb=blk.nb, mbs=8, sc=a["scheme"], b=bv.ptr, x=xv.ptr, nrhs=2):
        return _status(lambda: call(f"gkoc_jacobi_simple_apply_{tn}_i32", gexec.stream, nb, C.c_uint32(mbs), _scheme(sc),
                                    blk.ptrs, blk.blocks, b, 3, x, 4, nrhs))

    def advanced(nb=blk.nb, mbs=8, sc=a["scheme"], b=bv.ptr, x=xv.ptr, nrhs=2):
        return _status(lambda: call(f"gkoc_jacobi_apply_{tn}_i32", gexec.stream, nb, C.c_uint32(mbs), _scheme(sc),
                                    blk.ptrs, blk.blocks, al, b, 3, be, x, 4, nrhs))
    for fn in (simple, advanced):
        assert fn(nb=0) == 0 and fn(nrhs=0) == 0
        assert fn(mbs=9) == INVALID and fn(sc=wide) == NOT_SUPPORTED
        assert fn(b=xv.ptr) == INVALID, "b == x is refused"
    sync()
    assert bv.unchanged() and xv.unchanged() and blk.unchanged()


@pytest.mark.parametrize("tn", REAL)
def test_apply_xcd_map_is_a_bijection(gexec, tn):
    """GKOC_TUNE_JACOBI_XCD_MAP on and off at 2048 and 2051 workgroups (1 048 576 and 1 050 112 single-row blocks,
    block_offset 1, one column): both settings give the restatement's bits for every row"""
    import torch
    t = br.TYPES[tn]
    old = tune_get(TUNE_XCD_MAP)
    try:
        for nb, wgs in ((1048576, 2048), (1050112, 2051)):
            a = jr.apply_case(tn, 1, nb, 1, uniform=True)
            assert jr.fixed_workgroups(a["scheme"], nb, np.dtype(t).itemsize) == wgs
            blk = Blk(gexec, "i32" if wgs == 2048 else "i64", a)
            want = jr.apply_tuned(br.plain(t), a["scheme"], a["block_ptrs"], a["blocks"], a["b"])
            adv = jr.apply_tuned(br.plain(t), a["scheme"], a["block_ptrs"], a["blocks"], a["b"], a["alpha"][0],
                                 a["beta"][0], a["x0"])
            for tune in (1, 0):
                tune_set(TUNE_XCD_MAP, tune)
                assert jr.xcd_map_applies(wgs, tune) == bool(tune)
                got = run_apply(gexec, tn, blk, a["b"], expect=("fixed", None))
                assert same_bits(got, want), (tn, nb, tune, int(np.flatnonzero(got != want)[0]))
                got = run_apply(gexec, tn, blk, a["b"], adv=(a["alpha"][0], a["beta"][0]), x0=a["x0"])
                assert same_bits(got, adv), (tn, nb, tune)
            del blk
    finally:
        tune_set(TUNE_XCD_MAP, old)
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ apply_stored_f64, convert_storage_f64
@pytest.mark.parametrize("bo", (1, 2, 4, 8, 16))
@pytest.mark.parametrize("prec", jr.PRECISIONS)
def test_stored_precisions(gexec, prec, bo):
    """convert_storage narrows every group in place (values below and above the half range included): the bytes of
    the restatement; both products on the stored blocks bit for bit; three groups (the second group of the last wave
    stays empty)"""
    sc = jr.storage_scheme(bo)
    nb = 3 * sc.group_size - (1 if sc.group_size > 1 else 0)
    # launch_convert_storage and launch_apply_stored need the wide layout; launch_apply_stored_fixed takes two groups
    # per wave at every block_offset (16 included), so three groups are one workgroup whose second wave is half empty
    assert jr.wide_group_layout(sc) and jr.num_groups(sc, nb) == 3
    assert jr.fixed_workgroups(sc, nb, 8, gpw=2) == 1 and jr.adaptive_branch(sc, 1, 1, 1) == "fixed"
    a = jr.apply_case("f64", bo, nb, 1, fill=-777.25)
    edge = a["blocks"].copy()
    edge[::7] *= 1e-6
    edge[3::11] *= 3e5
    a["blocks"][::7] *= 1e-6                                   # products: finite after the conversion
    for itn, src in (("i32", a["blocks"]), ("i64", edge)):
        dev = Flat(gexec, src)
        call("gkoc_jacobi_convert_storage_f64", gexec.stream, nb, _scheme(sc), dev, C.c_uint8(prec))
        sync()
        stored = dev.get()
        assert same_bits(stored, jr.convert_storage(sc, nb, src, prec)), (prec, bo)
    blk = Blk(gexec, "i32" if bo < 4 else "i64", a, blocks=jr.convert_storage(sc, nb, a["blocks"], prec))
    blk.blocks_seen = jr.widen_storage(sc, nb, blk.blocks.host[:-3], np.full(jr.num_groups(sc, nb), prec))
    check_products(gexec, "f64", blk, a, kind="stored", prec=prec, what=f"prec {prec:#x}, bo {bo}")


@pytest.mark.parametrize("itn", ("i32", "i64"))
def test_stored_special_arguments(gexec, itn):
    """an unknown precision: GKOC_E_NOT_SUPPORTED from both entry points; precision 0 is gkoc_jacobi_apply; with a
    reduced precision nrhs = 2 (and a stride) is refused before anything is launched - x keeps its NaN, the canary
    behind it survives; b == x: GKOC_E_INVALID"""
    a = jr.apply_case("f64", 8, 11, 2, fill=-777.25)
    sc = a["scheme"]
    blk = Blk(gexec, itn, a, blocks=jr.convert_storage(sc, 11, a["blocks"], 0x01))
    assert _status(lambda: call("gkoc_jacobi_convert_storage_f64", gexec.stream, 11, _scheme(sc), blk.blocks,
                                C.c_uint8(0x03))) == NOT_SUPPORTED
    b1 = a["b"][:, :1]
    # nrhs = 2 with unit strides: the second column would start one entry on, its last entry is the canary behind x
    bv, xv = Vec(gexec, b1, 1), Vec(gexec, _nan(b1.shape, np.float64), 1)
    bs, xs = Vec(gexec, b1, 2), Vec(gexec, _nan(b1.shape, np.float64), 2)

    def stored(prec, b, ldb, x, ldx, nrhs):
        return _status(lambda: call(f"gkoc_jacobi_apply_stored_f64_{itn}", *blk.head(gexec), C.c_uint8(prec), None, b, ldb,
                                    None, x, ldx, nrhs))
    assert stored(0x03, bv.ptr, 1, xv.ptr, 1, 1) == NOT_SUPPORTED
    assert stored(0x01, bv.ptr, 1, xv.ptr, 1, 2) == NOT_SUPPORTED, "nrhs = 2 with unit strides is refused"
    assert stored(0x01, bs.ptr, 2, xs.ptr, 2, 1) == NOT_SUPPORTED
    assert stored(0x01, bv.ptr, 1, bv.ptr, 1, 1) == INVALID
    sync()
    assert xv.unchanged() and xs.unchanged() and bv.unchanged() and blk.unchanged(), "a refused call wrote"
    full = Blk(gexec, itn, a)
    got = run_apply(gexec, "f64", full, a["b"], kind="stored", prec=0, adv=(a["alpha"][0], a["beta"][0]), x0=a["x0"])
    assert same_bits(got, run_apply(gexec, "f64", full, a["b"], adv=(a["alpha"][0], a["beta"][0]), x0=a["x0"]))
    assert same_bits(got, jr.apply_tuned(br.plain(np.float64), sc, a["block_ptrs"], a["blocks"], a["b"], a["alpha"][0],
                                         a["beta"][0], a["x0"]))


# ---------------------------------------------------------------------------------------- apply_adaptive_f64
@pytest.mark.parametrize("itn", ("i32", "i64"))
@pytest.mark.parametrize("max_bs", (8, 13))
def test_adaptive_f64(gexec, max_bs, itn):
    """one precision per storage group, all six of them: block_offset 8 (wide: the fixed kernel with PREC = -1 for one
    column, the STORED general kernel for three strided ones) and 13 (general)"""
    sc = jr.storage_scheme(max_bs)
    gp = np.array([0x00, 0x01, 0x02, 0x10, 0x11, 0x20, 0x01])
    nb = len(gp) * sc.group_size - 1
    for nrhs, ld in ((1, 1), (3, 4)):
        a = jr.apply_case("f64", max_bs, nb, nrhs, fill=-777.25)
        assert jr.adaptive_branch(sc, nrhs, ld, ld + 1 if nrhs > 1 else 1) == \
            ("fixed" if max_bs == 8 and nrhs == 1 else "general")
        stored = jr.convert_groups(sc, nb, a["blocks"], gp)
        blk = Blk(gexec, itn, a, blocks=stored, prec=np.repeat(gp, sc.group_size)[:nb])
        blk.blocks_seen = jr.widen_storage(sc, nb, stored, gp)
        check_products(gexec, "f64", blk, a, kind="adaptive", ldb=ld, ldx=ld + 1 if nrhs > 1 else 1,
                       what=f"adaptive, max_block_size {max_bs}, {nrhs} columns")


# ------------------------------------------------------------------------------------------ the any-type path
@pytest.mark.parametrize("rows_kernel", (False, True), ids=("lanes", "thread_per_row"))
@pytest.mark.parametrize("tn", ("f32",) + CPLX)
def test_any_type_products(gexec, tn, rows_kernel):
    """gkoc_jacobi_{simple_apply,apply}_{c64,c128} and gkoc_jacobi_apply_adaptive_{f32,c64,c128}: every SUB of
    launch_apply_lanes_any (max_block_size 1, 2, 3, 8, 13, 32), a group count that leaves the last wave partly filled,
    one column and three strided ones, full storage and one precision per group; against the restatement (float: the
    reference's bits; complex: the textbook product).  thread_per_row: GKOC_TUNE_JACOBI_LANES = 1"""
    t = br.TYPES[tn]
    vs = np.dtype(t).itemsize
    old = tune_get(TUNE_LANES)
    tune_set(TUNE_LANES, 1 if rows_kernel else 0)
    try:
        for i, max_bs in enumerate((1, 2, 3, 8, 13, 32)):
            sc = jr.storage_scheme(max_bs)
            assert jr.any_branch(sc, 1 if rows_kernel else 0) == ("rows" if rows_kernel else "lanes")
            groups = 4 * jr.lanes_groups_per_wave(sc, vs) + 1
            nb = groups * sc.group_size - (1 if sc.group_size > 1 else 0)
            itn = ("i32", "i64")[i % 2]
            gp = np.resize([0x00, 0x02, 0x10, 0x01, 0x11, 0x20], groups)
            for nrhs, ldb, ldx in ((1, 1, 1), (3, 4, 5)):
                a = jr.apply_case(tn, max_bs, nb, nrhs, fill=-777.25)
                if br.is_complex(t):
                    check_products(gexec, tn, Blk(gexec, itn, a), a, ref=jr.apply_any, ldb=ldb, ldx=ldx,
                                   what=f"full storage, max_block_size {max_bs}")
                stored = jr.convert_groups(sc, nb, a["blocks"], gp)
                blk = Blk(gexec, itn, a, blocks=stored, prec=np.repeat(gp, sc.group_size)[:nb])
                blk.blocks_seen = jr.widen_storage(sc, nb, stored, gp)
                check_products(gexec, tn, blk, a, ref=jr.apply_any, kind="adaptive", ldb=ldb, ldx=ldx,
                               what=f"adaptive, max_block_size {max_bs}")
    finally:
        tune_set(TUNE_LANES, old)


@pytest.mark.parametrize("tn", CPLX)
def test_any_type_refuses_overlap(gexec, tn):
    """b == x: GKOC_E_INVALID from the complex products and the adaptive ones, on either kernel; nothing written"""
    a = jr.apply_case(tn, 13, 9, 1)
    blk = Blk(gexec, "i32", a, prec=np.zeros(9, np.uint8))
    xv = Vec(gexec, a["b"], 1)
    old = tune_get(TUNE_LANES)
    try:
        for tune in (0, 1):
            tune_set(TUNE_LANES, tune)
            assert _status(lambda: call(f"gkoc_jacobi_simple_apply_{tn}_i32", *blk.head(gexec), xv.ptr, 1, xv.ptr, 1, 1)) \
                == INVALID
            assert _status(lambda: call(f"gkoc_jacobi_apply_adaptive_{tn}_i32", *blk.head(gexec), blk.prec, None, xv.ptr,
                                        1, None, xv.ptr, 1, 1)) == INVALID
    finally:
        tune_set(TUNE_LANES, old)
    f = jr.apply_case("f64", 8, 9, 1)
    fb = Blk(gexec, "i32", f, prec=np.zeros(9, np.uint8))
    fx = Vec(gexec, f["b"], 1)
    assert _status(lambda: call("gkoc_jacobi_apply_adaptive_f64_i32", *fb.head(gexec), fb.prec, None, fx.ptr, 1, None,
                                fx.ptr, 1, 1)) == INVALID
    sync()
    assert xv.unchanged() and fx.unchanged()


# --------------------------------------------------------------------------------------------- transposes
@pytest.mark.parametrize("itn", ("i32", "i64"))
@pytest.mark.parametrize("tn", REAL)
def test_transpose(gexec, tn, itn):
    """gkoc_jacobi_transpose_{f64,f32}: blocks of 1 to 32 rows, the whole storage against
    value_kernel_refs.jacobi_transpose over a NaN fill; applied twice it is the identity.  f64 with a precision array:
    the entries move as raw words of their group's type.  f32 with one: refused"""
    t = br.TYPES[tn]
    for max_bs in (1, 5, 13, 32):
        sc = jr.storage_scheme(max_bs)
        nb = 3 * sc.group_size + 1
        a = jr.apply_case(tn, max_bs, nb, 1, fill=-777.25)
        blk = Blk(gexec, itn, a)
        out = Flat(gexec, _nan(a["blocks"].shape, t))
        call(f"gkoc_jacobi_transpose_{tn}_{itn}", *blk.head(gexec), None, out)
        sync()
        got = out.get()
        assert same_bits(got, vr.jacobi_transpose(sc, a["block_ptrs"], a["blocks"], False, _nan(a["blocks"].shape, t)))
        back = Flat(gexec, a["blocks"])
        call(f"gkoc_jacobi_transpose_{tn}_{itn}", gexec.stream, nb, blk.mbs, blk.sc, blk.ptrs, out, None, back)
        sync()
        assert same_bits(back.get(), a["blocks"]) and blk.unchanged()
        gp = np.array([0x02, 0x00, 0x10, 0x20])
        bp = np.repeat(gp, sc.group_size)[:nb]
        if tn == "f64":
            stored = jr.convert_groups(sc, nb, a["blocks"], gp)
            sblk = Blk(gexec, itn, a, blocks=stored, prec=bp)
            out = Flat(gexec, np.full(stored.shape, -3.5))
            call(f"gkoc_jacobi_transpose_f64_{itn}", *sblk.head(gexec), sblk.prec, out)
            sync()
            assert same_bits(out.get(), jr.transpose_stored(sc, a["block_ptrs"], stored, bp, np.full(stored.shape, -3.5)))
            assert sblk.unchanged()
        else:
            pr = Flat(gexec, bp.astype(np.uint8))
            assert _status(lambda: call(f"gkoc_jacobi_transpose_f32_{itn}", *blk.head(gexec), pr, out)) == NOT_SUPPORTED


# ------------------------------------------------------------------------------------------ fused kernels
def work_bytes(n, t):
    from ginkgo_amd._lib import lib
    got = lib().gkoc_x_workspace_bytes(C.c_int64(n), C.c_size_t(np.dtype(t).itemsize))
    assert got == jr.fused_workspace_bytes(n, np.dtype(t).itemsize)
    return got


def run_apply_dot(gexec, tn, blk, r, wbytes=None):
    t = br.TYPES[tn]
    n = r.shape[0]
    b, x, dot = Flat(gexec, r), Flat(gexec, _nan(n, t)), Flat(gexec, _nan(1, t))
    work = Flat(gexec, np.zeros(work_bytes(n, t), np.uint8))
    call(f"gkoc_x_jacobi_simple_apply_dot_{tn}_{blk.itn}", gexec.stream, blk.nb, n, blk.mbs, blk.sc, blk.ptrs, blk.blocks,
         b, x, dot, work, C.c_size_t(work_bytes(n, t) if wbytes is None else wbytes))
    sync()
    work.get()
    assert b.unchanged() and blk.unchanged()
    return x.get(), dot.get()[0]


def run_step2(gexec, tn, blk, v, take_sqrt=0, wbytes=None):
    t = br.TYPES[tn]
    n = v["x"].shape[0]
    d = {k: Flat(gexec, v[k]) for k in ("x", "r", "p", "q", "beta", "rho", "stop_status")}
    z, rho_out, nrm = Flat(gexec, _nan(n, t)), Flat(gexec, _nan(1, t)), Flat(gexec, _nan(1, t))
    work = Flat(gexec, np.zeros(work_bytes(n, t), np.uint8))
    call(f"gkoc_x_cg_step_2_jacobi_apply_{tn}_{blk.itn}", gexec.stream, blk.nb, n, blk.mbs, blk.sc, blk.ptrs, blk.blocks,
         d["x"], d["r"], d["p"], d["q"], d["beta"], d["rho"], d["stop_status"], z, rho_out, nrm, C.c_int(take_sqrt), work,
         C.c_size_t(work_bytes(n, t) if wbytes is None else wbytes))
    sync()
    work.get()
    assert all(d[k].unchanged() for k in ("p", "q", "beta", "rho", "stop_status")) and blk.unchanged()
    return dict(x=d["x"].get(), r=d["r"].get(), z=z.get()), rho_out.get()[0], nrm.get()[0]


PIPE_VECS = ("x", "r", "z", "w", "p", "q", "f", "g", "m", "n")


def run_pipe(gexec, tn, blk, v, wbytes=None, alias_beta=False):
    t = br.TYPES[tn]
    n = v["x"].shape[0]
    d = {k: Flat(gexec, v[k]) for k in PIPE_VECS + ("prev_rho", "rho", "delta", "beta_in", "beta_out", "stop_status")}
    out3 = Flat(gexec, _nan(3, t))
    work = Flat(gexec, np.zeros(work_bytes(n, t), np.uint8))
    call(f"gkoc_x_pipe_cg_steps_jacobi_{tn}_{blk.itn}", gexec.stream, blk.nb, n, blk.mbs, blk.sc, blk.ptrs, blk.blocks,
         *[d[k] for k in PIPE_VECS], d["prev_rho"], d["rho"], d["delta"], d["beta_in"],
         d["beta_in"] if alias_beta else d["beta_out"], d["stop_status"], out3, work,
         C.c_size_t(work_bytes(n, t) if wbytes is None else wbytes), None)
    sync()
    work.get()
    assert all(d[k].unchanged() for k in ("n", "prev_rho", "rho", "delta", "beta_in", "stop_status")) and blk.unchanged()
    out = {k: d[k].get() for k in PIPE_VECS[:-1]}
    out["beta_out"] = d["beta_out"].get()
    return out, out3.get()


def check_sums(tn, got, pairs, depth, what, exact=False):
    t = br.TYPES[tn]
    hp, sums = jr.dots_hp(pairs)
    got = np.asarray(got, t).astype(np.longdouble)
    if exact:
        br.Exact().see(sums)
        assert np.array_equal(got, hp), (what, tn, got, hp)
        return
    bound = (depth + 1) * br.eps_of(t) * sums
    err = np.abs(got - hp)
    _figure(f"fused sums {tn}, fraction of the depth bound", np.max(err / bound))
    assert np.all(err <= bound), (what, tn, got, hp)


def check_fused(gexec, tn, itn, a, exact=False, what=""):
    """the three fused kernels on one case: vectors bit-identical to the restatement, sums within the depth bound (or
    equal), <r, z> of step_2 + apply with the bits of apply_dot on the same r"""
    t = br.TYPES[tn]
    vs = np.dtype(t).itemsize
    pl = br.plain(t)
    blk = Blk(gexec, itn, a)
    blkargs = (a["scheme"], a["block_ptrs"], a["blocks"])
    v = a["vec"]
    depth = jr.fused_dot_depth(a["scheme"], blk.nb, vs)
    # step_2 + apply
    got, rho, nrm = run_step2(gexec, tn, blk, v)
    ref = jr.step2_apply(pl, *blkargs, v)
    for k in ("x", "r", "z"):
        assert same_bits(got[k], ref[k]), (what, tn, "step_2 + apply", k)
    check_sums(tn, [rho, nrm], [(got["r"], got["z"]), (got["r"], got["r"])], depth, what + " step_2 + apply", exact)
    _, rho2, nrm2 = run_step2(gexec, tn, blk, v, take_sqrt=1)
    assert same_bits(np.array(rho2), np.array(rho)) and abs(float(nrm2) ** 2 - float(nrm)) <= 4 * br.eps_of(t) * float(nrm)
    # apply + dot on the r that step_2 left
    x, dot = run_apply_dot(gexec, tn, blk, got["r"])
    assert same_bits(x, got["z"]) and same_bits(x, jr.apply_dot(pl, *blkargs, got["r"]))
    assert same_bits(np.array(dot), np.array(rho)), (what, tn, "<r, z> differs between step_2 + apply and apply_dot")
    # PipeCg
    out, out3 = run_pipe(gexec, tn, blk, v)
    ref = jr.pipe_steps(pl, *blkargs, v)
    for k in PIPE_VECS[:-1] + ("beta_out",):
        assert same_bits(out[k], np.asarray(ref[k]).reshape(-1)), (what, tn, "pipe steps", k)
    check_sums(tn, out3, [(out["r"], out["z"]), (out["w"], out["z"]), (out["r"], out["r"])],
               jr.fused_dot_depth(a["scheme"], blk.nb, vs, rows_fold=True), what + " pipe steps", exact)
    return got, out


@pytest.mark.parametrize("bo", (1, 2, 4, 8, 16))
@pytest.mark.parametrize("tn", REAL)
def test_fused_shapes(gexec, tn, bo):
    """block_offset 1 .. 16: one single-row block, one workgroup (4 GPW full groups), two workgroups with a partly
    filled last one; both index types"""
    vs = np.dtype(br.TYPES[tn]).itemsize
    gs, gpw = 64 // bo, jr.groups_per_wave(bo, vs)
    for i, nb in enumerate((1, 4 * gpw * gs, (4 * gpw + 2) * gs - (1 if gs > 1 else 0))):
        a = jr.fused_case(tn, bo, nb, last=1 if nb == 1 else None)
        assert nb > 1 or a["n"] == 1
        assert jr.fixed_workgroups(a["scheme"], nb, vs) == (1, 1, 2)[i]
        check_fused(gexec, tn, ("i32", "i64")[(i + bo) % 2], a, what=f"bo {bo}, {nb} blocks")


@pytest.mark.parametrize("tn", REAL)
def test_fused_states_and_exact_sums(gexec, tn):
    """beta = 0 and a stopped column leave the vectors and sum the old ones; the PipeCg kernel also with prev_rho = 0
    and beta' = 0 -> delta; integer-valued inputs give the exact sums"""
    for bo, nb in ((8, 19), (16, 21)):
        for state in ("beta0", "stopped", "prev0", "delta"):
            a = jr.fused_case(tn, bo, nb, state=state)
            v = a["vec"]
            got, out = check_fused(gexec, tn, "i32", a, what=state)
            if state in ("beta0", "stopped"):
                assert same_bits(got["x"], v["x"]) and same_bits(got["r"], v["r"])
                assert all(same_bits(out[k], v[k]) for k in ("x", "r", "z", "w")), (state, "step_1 is a no-op")
            if state == "stopped":
                assert all(same_bits(out[k], v[k]) for k in "pqfg") and same_bits(out["beta_out"], v["beta_in"])
            if state == "delta":
                assert same_bits(out["beta_out"], v["delta"])
        check_fused(gexec, tn, "i64", jr.fused_case(tn, bo, nb, exact=True), exact=True, what="exact")


class FusedBufs:
    """every operand of the three fused kernels in buffers the test keeps, so that a refused call can be followed by
    a look at all of them: the vectors (z of step_2 + apply and x of apply_dot start as NaN), the scalars, the
    results rho_out / norm_out / dot / out3 (NaN) and the workspace"""

    def __init__(self, gexec, tn, n, v=None):
        t = br.TYPES[tn]
        self.tn, self.n, self.t = tn, n, t
        src = v if v is not None else {}
        self.vec = {k: Flat(gexec, src.get(k, np.ones(n, t))) for k in PIPE_VECS}
        self.zx = Flat(gexec, _nan(n, t))
        self.sc = {k: Flat(gexec, src.get(k, np.ones(1, t)))
                   for k in ("beta", "rho", "prev_rho", "delta", "beta_in", "beta_out")}
        self.stop = Flat(gexec, np.zeros(1, np.uint8))
        self.res = Flat(gexec, _nan(6, t))              # rho_out, norm_out, dot, out3
        self.wb = work_bytes(n, t)
        self.work = Flat(gexec, np.zeros(self.wb, np.uint8))

    def everything(self):
        return list(self.vec.values()) + list(self.sc.values()) + [self.zx, self.stop, self.res, self.work]

    def apply_dot(self, gexec, head, itn, wbytes=None, in_place=False):
        return _status(lambda: call(f"gkoc_x_jacobi_simple_apply_dot_{self.tn}_{itn}", *head, self.vec["r"],
                                    self.vec["r"] if in_place else self.zx, self.res.dev.at(2), self.work,
                                    C.c_size_t(self.wb if wbytes is None else wbytes)))

    def step2(self, gexec, head, itn, wbytes=None):
        v, s = self.vec, self.sc
        return _status(lambda: call(f"gkoc_x_cg_step_2_jacobi_apply_{self.tn}_{itn}", *head, v["x"], v["r"], v["p"], v["q"],
                                    s["beta"], s["rho"], self.stop, self.zx, self.res.dev.at(0), self.res.dev.at(1),
                                    C.c_int(0), self.work, C.c_size_t(self.wb if wbytes is None else wbytes)))

    def pipe(self, gexec, head, itn, wbytes=None, alias_beta=False):
        s = self.sc
        return _status(lambda: call(f"gkoc_x_pipe_cg_steps_jacobi_{self.tn}_{itn}", *head,
                                    *[self.vec[k] for k in PIPE_VECS], s["prev_rho"], s["rho"], s["delta"], s["beta_in"],
                                    s["beta_in"] if alias_beta else s["beta_out"], self.stop, self.res.dev.at(3), self.work,
                                    C.c_size_t(self.wb if wbytes is None else wbytes), None))


@pytest.mark.parametrize("tn", REAL)
def test_fused_refusals(gexec, tn):
    """a scheme that is not wide: GKOC_E_NOT_SUPPORTED; a workspace one byte short: GKOC_E_WORKSPACE; beta_in ==
    beta_out: GKOC_E_INVALID; b == x of apply_dot: GKOC_E_INVALID; so many single-row blocks under a max_block_size 16
    scheme that the partial sums do not fit - 65 536 in double, 131 072 in float, 4096 workgroups either way:
    gkoc_x_cg_step_2_jacobi_apply_fits answers 0 and both step kernels return GKOC_E_WORKSPACE.  After every refused
    call every vector, scalar, result and the workspace is read back: nothing was written"""
    import torch
    from ginkgo_amd._lib import lib
    t = br.TYPES[tn]
    vs = np.dtype(t).itemsize

    def intact(bufs, blk=None):
        sync()
        assert all(f.unchanged() for f in bufs.everything()) and (blk is None or blk.unchanged()), "a refused call wrote"
        return True

    a = jr.fused_case(tn, 8, 19)
    blk = Blk(gexec, "i32", a)
    bufs = FusedBufs(gexec, tn, a["n"], a["vec"])
    head = (gexec.stream, blk.nb, a["n"], blk.mbs, blk.sc, blk.ptrs, blk.blocks)
    assert bufs.apply_dot(gexec, head, "i32", wbytes=bufs.wb - 1) == WORKSPACE and intact(bufs, blk)
    assert bufs.step2(gexec, head, "i32", wbytes=bufs.wb - 1) == WORKSPACE and intact(bufs, blk)
    assert bufs.pipe(gexec, head, "i32", wbytes=bufs.wb - 1) == WORKSPACE and intact(bufs, blk)
    assert bufs.pipe(gexec, head, "i32", alias_beta=True) == INVALID and intact(bufs, blk)
    assert bufs.apply_dot(gexec, head, "i32", in_place=True) == INVALID and intact(bufs, blk)
    n13 = jr.fused_case(tn, 13, 9)
    b13 = Blk(gexec, "i64", n13)
    assert not jr.wide_group_layout(n13["scheme"])
    bufs13 = FusedBufs(gexec, tn, n13["n"], n13["vec"])
    head13 = (gexec.stream, b13.nb, n13["n"], b13.mbs, b13.sc, b13.ptrs, b13.blocks)
    for fn in (bufs13.apply_dot, bufs13.step2, bufs13.pipe):
        assert fn(gexec, head13, "i64") == NOT_SUPPORTED and intact(bufs13, b13)
    check_fused(gexec, tn, "i32", a, what="after the refusals")
    # too many workgroups for the workspace
    n = 65536 * 8 // vs
    sc = jr.storage_scheme(16)
    assert jr.fixed_workgroups(sc, n, vs) == 4096 and not jr.step2_apply_fits(sc, n, n, vs)
    assert 3 * 4096 > jr.fused_workspace_bytes(n, vs) // vs
    assert lib().gkoc_x_cg_step_2_jacobi_apply_fits(C.c_int64(n), C.c_int64(n), _scheme(sc), C.c_size_t(vs)) == 0
    # 65 536 blocks in float: GPW = 2 makes 2048 workgroups of them, which fit
    assert lib().gkoc_x_cg_step_2_jacobi_apply_fits(C.c_int64(65536), C.c_int64(65536), _scheme(sc), C.c_size_t(vs)) == \
        int(jr.step2_apply_fits(sc, 65536, 65536, vs)) == int(tn == "f32")
    assert lib().gkoc_x_cg_step_2_jacobi_apply_fits(C.c_int64(19), C.c_int64(a["n"]), _scheme(a["scheme"]), C.c_size_t(vs)) == 1
    assert lib().gkoc_x_cg_step_2_jacobi_apply_fits(C.c_int64(9), C.c_int64(n13["n"]), _scheme(n13["scheme"]), C.c_size_t(vs)) == 0
    ptrs = Flat(gexec, np.arange(n + 1, dtype=np.int32))
    blocks = torch.ones(jr.storage_size(sc, n), dtype=torch.float64 if tn == "f64" else torch.float32,
                        device=gexec.device)                                       # 134 MB, never read
    big = FusedBufs(gexec, tn, n)
    bighead = (gexec.stream, n, n, C.c_uint32(16), _scheme(sc), ptrs, blocks)
    assert big.step2(gexec, bighead, "i32") == WORKSPACE and intact(big)
    assert big.pipe(gexec, bighead, "i32") == WORKSPACE and intact(big)
    assert ptrs.unchanged()
    del blocks
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------- observed figures, last
def test_zz_observed_figures():
    """prints what the tests above observed (pytest -s): per rule-R output the largest |kernel - ref| / (eps max|ref|),
    the largest fraction of the matrix-core and depth bounds, and for the complex inverse blocks which acceptance held"""
    print()
    for name in sorted(FIGURES):
        print(f"figure | {name} | {FIGURES[name]:.3f}")
    for tn in CPLX:
        held = {m: h for (t_, m), h in HELD.items() if t_ == tn}
        print(f"held   | generate {tn} | " + ", ".join(f"{m}: {held[m]}" for m in sorted(held)))
    assert all(h in ("bits", "rule R") for h in HELD.values())
