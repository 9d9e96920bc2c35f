"""cb_gmres::{restart, arnoldi, solve_krylov} (csrc/cb_gmres.hip, cb_gmres_complex.hip) through the C ABI
against the numpy references of binding_refs.py, for every value type / storage kind pair and for the
layouts that select each code path: one right-hand side with unit strides (four rows per lane; basis
vectors k >= 1 start misaligned when st0 = rows is not a multiple of four, aligned when st0 is rounded up -
then restart zeroes the basis with its kernel instead of a memset and the padding keeps its canary), one
right-hand side with stride 2 and three right-hand sides (the strided path).

The storage conversions are emulated bit for bit on the host (binding_refs.store / load), so what the
kernel stores is compared for equality with store(the kernel's own next_krylov).  Sums are compared by rule
R (binding_refs.rule_r) with the long-double reference and the plain restatement started from the kernel's
own state at every step (identical inputs: the stored basis bit for bit).  Properties of the basis
(norm, orthogonality, Arnoldi relation) are compared with the same property of the plain restatement running
freely through the same emulated storage, maxima over a cycle.

The last test prints the largest observed error ratios of the run."""
import numpy as np
import pytest

import binding_refs as br
from binding_gpu import CANARY, Dev, same_bits, sync

pytestmark = pytest.mark.gpu

PAIRS = ([("f64", k) for k in (br.KEEP, br.F32, br.F16, br.I64, br.I32, br.I16)] +
         [("f32", k) for k in (br.KEEP, br.F16, br.I32, br.I16)] +
         [("c128", br.KEEP), ("c128", br.F32), ("c64", br.KEEP)])
REJECTED = ([("f32", br.F32), ("f32", br.I64)] + [("c128", k) for k in (br.F16, br.I64, br.I32, br.I16)] +
            [("c64", k) for k in (br.F32, br.F16, br.I64, br.I32, br.I16)])
# name: (nrhs, st1, ldn, aligned st0)
LAYOUTS = {"unit": (1, 1, 1, False), "unit_aligned": (1, 1, 1, True), "stride2": (1, 2, 2, False),
           "three": (3, 3, 3, False), "three_padded": (3, 5, 4, True)}
FILL = 0x5a
RATIOS = {}


def _ids(p):
    return f"{p[0]}-{br.KIND_NAMES[p[1]]}"


def _call(name, *args):
    from ginkgo_amd._lib import call
    call(name, *args)


def _note(what, tn, kind, ratio):
    key = (what, tn, br.KIND_NAMES[kind])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def _rand(rng, shape, t):
    v = rng.uniform(-1, 1, shape)
    return (v + 1j * rng.uniform(-1, 1, shape)).astype(t) if br.is_complex(t) else v.astype(t)


def _operator(v):
    """a fixed nonsymmetric banded operator on the rows of v (any dtype), the 'A' of the Arnoldi tests"""
    w = 2.5 * v
    w[1:] -= v[:-1]
    w[:-1] -= 0.4 * v[1:]
    if v.shape[0] > 7:
        w[7:] += 0.3 * v[:-7]
    return w


class State:
    """the operands of the three entry points on the device"""

    def __init__(self, gexec, tn, kind, rows, kd, layout, with_buffer=True, pad_small=0):
        self.gexec, self.tn, self.kind, self.rows, self.kd = gexec, tn, kind, rows, kd
        self.t = br.TYPES[tn]
        self.rt = br.real_of(self.t)
        self.cx = br.is_complex(self.t)
        self.nrhs, self.st1, self.ldn, aligned = LAYOUTS[layout] if isinstance(layout, str) else layout
        self.st0 = rows * self.st1
        if aligned:
            self.st0 = (self.st0 + 3) // 4 * 4 + 8
        self.lds = self.nrhs + pad_small                    # row stride of the small arrays
        self.sdt = np.dtype(br.storage_dtype(kind, self.t))
        nb = (kd + 1) * self.st0 + 16
        self.bases = Dev(gexec, np.full(nb * self.sdt.itemsize, FILL, np.uint8).view(self.sdt))
        t, rt, n, lds = self.t, self.rt, self.nrhs, self.lds
        self.an_t = rt if self.cx else t
        small = dict(residual_norm=np.full(n, CANARY, self.an_t), rnc=np.full((kd + 1, lds), CANARY, t),
                          an=np.full((3, lds), CANARY, self.an_t), scalars=np.full((kd + 1, lds), CANARY, t),
                          gsin=np.full((max(kd, 1), lds), CANARY, t), gcos=np.full((max(kd, 1), lds), CANARY, t),
                          h=np.full((kd + 2, lds), CANARY, t), buffer=np.full((kd + 2, lds), CANARY, t),
                          fin=np.full(n, 7, np.uint64), stop=np.zeros(n, np.uint8),
                          next=np.full((rows, self.ldn), CANARY, t),
                          residual=np.full((rows, self.ldn), CANARY, t))
        self.dev = {k: Dev(gexec, v) for k, v in small.items()}
        self.with_buffer = with_buffer

    def put(self, name, a):
        """a: rows x nrhs (or 1-d); written into the strided device array"""
        full = self.dev[name].get()
        if full.ndim == 2:
            full[:a.shape[0], :self.nrhs] = a
        else:
            full[:] = a
        self.dev[name] = Dev(self.gexec, full)
        return full

    def get(self, name, rows=None):
        full = self.dev[name].get()
        if full.ndim == 1:
            return full
        assert np.all(full[:, self.nrhs:] == full.dtype.type(CANARY)), name + ": padding overwritten"
        return np.ascontiguousarray(full[:rows, :self.nrhs])

    def basis_index(self):
        k, r, c = np.meshgrid(np.arange(self.kd + 1), np.arange(self.rows), np.arange(self.nrhs), indexing="ij")
        return k * self.st0 + r * self.st1 + c

    def get_bases(self):
        """(kd + 1) x rows x nrhs storage values; the bytes between them must still hold the fill"""
        flat = self.bases.get()
        idx = self.basis_index()
        mask = np.ones(flat.shape, bool)
        mask[idx.reshape(-1)] = False
        assert np.all(flat[mask].view(np.uint8) == FILL), "cb_gmres: wrote between the basis entries"
        return flat[idx]

    def put_bases(self, b):
        flat = self.bases.get()
        flat[self.basis_index()] = b
        self.bases = Dev(self.gexec, flat)

    def restart(self):
        d, st = self.dev, self.gexec.stream
        if self.cx:
            _call("gkoc_cb_gmres_restart_" + self.tn, st, self.rows, self.nrhs, self.kd, d["residual"], self.ldn,
                  d["residual_norm"], d["rnc"], self.lds, self.kind, self.bases, self.st0, self.st1, d["next"],
                  self.ldn, d["fin"])
        else:
            _call("gkoc_cb_gmres_restart_" + self.tn, st, self.rows, self.nrhs, self.kd, d["residual"], self.ldn,
                  d["residual_norm"], d["rnc"], self.lds, d["an"], self.lds, self.kind, self.bases, self.st0,
                  self.st1, d["scalars"], self.lds, d["next"], self.ldn, d["fin"])
        sync()

    def arnoldi(self, it, stream=None, **operands):
        """operands: device arrays that stand in for those of self.dev in this call; with a stream the step
        is only enqueued there"""
        d, st = {**self.dev, **operands}, self.gexec.stream if stream is None else stream
        buf = d["buffer"] if self.with_buffer else None
        head = (st, self.rows, self.nrhs, it, d["next"], self.ldn, d["gsin"], self.lds, d["gcos"], self.lds,
                d["residual_norm"], d["rnc"], self.lds, self.kind, self.bases, self.st0, self.st1)
        tail = (d["h"], self.lds, buf, self.lds, d["an"], self.lds, d["fin"], d["stop"])
        if self.cx:
            _call("gkoc_cb_gmres_arnoldi_" + self.tn, *head, *tail)
        else:
            _call("gkoc_cb_gmres_arnoldi_" + self.tn, *head, d["scalars"], self.lds, *tail)
        if stream is None:
            sync()

    def solve(self, hess, ld_h, y, out):
        d, st = self.dev, self.gexec.stream
        head = (st, self.rows, self.nrhs, d["rnc"], self.lds, self.kind, self.bases, self.st0, self.st1)
        tail = (hess, ld_h, y, self.lds, out, self.ldn, d["fin"])
        if self.cx:
            _call("gkoc_cb_gmres_solve_krylov_" + self.tn, *head, *tail)
        else:
            _call("gkoc_cb_gmres_solve_krylov_" + self.tn, *head, d["scalars"], self.lds, *tail)
        sync()

    def scalars(self):
        return None if self.cx else self.get("scalars")

    def ref_state(self, ar, rounds=3):
        return br.CbGmres(ar, self.t, self.kind, self.rows, self.nrhs, self.kd, rounds)


def _t_corr(st):
    """cb_correction in the value type: T(2) / T(max of the integer type)"""
    if st.kind < br.I64:
        return st.t(1)
    return st.t(2) / st.t(np.iinfo(br.storage_dtype(st.kind, st.t)).max)


# ------------------------------------------------------------------------------------ rejected pairs
@pytest.mark.parametrize("pair", REJECTED, ids=_ids)
def test_pairs_the_header_excludes_raise_before_a_launch(gexec, pair):
    from ginkgo_amd._lib import NotSupported
    tn, kind = pair
    st = State(gexec, tn, br.KEEP, 40, 3, "three")          # buffers wide enough for any storage type
    st.kind = kind
    before = {k: v.get() for k, v in st.dev.items()}
    b0 = st.bases.get()
    hess = Dev(gexec, np.full((4, 16), CANARY, st.t))
    for fn in (st.restart, lambda: st.arnoldi(0), lambda: st.solve(hess, 16, st.dev["h"], st.dev["next"])):
        with pytest.raises(NotSupported):
            fn()
    sync()
    for k, v in st.dev.items():
        assert same_bits(v.get(), before[k]), k + " written by a rejected call"
    assert same_bits(st.bases.get(), b0)


# -------------------------------------------------------------------------------------------- restart
def _residual(rng, t, rows, nrhs):
    """random columns with, where there is room, entries that land in the half-subnormal range after the
    normalisation, both zeros, and one entry of clearly largest magnitude"""
    r = _rand(rng, (rows, nrhs), t)
    if rows >= 16:
        nrm = np.sqrt(rows / 3.0)
        r[1] = 3e-5 * nrm
        r[2] = -3e-5 * nrm
        r[3] = 6.09e-5 * nrm
        r[4] = 6.2e-5 * nrm
        r[5] = 0.0
        r[6] = -0.0
        r[7] = 1e-9
        r[rows - 1] = -1.75 if not br.is_complex(t) else -1.75 + 0.5j
    return r


def _check_restart(gexec, tn, kind, rows, kd, layout):
    t = br.TYPES[tn]
    st = State(gexec, tn, kind, rows, kd, layout, pad_small=2 if layout == "three_padded" else 0)
    rng = np.random.default_rng(rows * 31 + kd)
    res = _residual(rng, t, rows, st.nrhs)
    res_full = st.put("residual", res)
    st.restart()
    assert same_bits(st.dev["residual"].get(), res_full)
    rn = st.get("residual_norm")
    hp, pl = st.ref_state(br.hp(t)), st.ref_state(br.plain(t))
    hp.restart(res), pl.restart(res)
    ok, ratio = br.rule_r(rn, hp.residual_norm, pl.residual_norm, t)
    _note("restart norm", tn, kind, ratio)
    assert ok, ratio
    rnc = st.get("rnc")
    assert np.array_equal(rnc[0], rn.astype(t)) and np.all(rnc[1:] == 0)
    assert np.all(st.get("fin") == 0)
    nxt = st.get("next")
    want_next = np.stack([br.div_by_real(res[:, c], rn[c]) for c in range(st.nrhs)], axis=1)
    assert same_bits(nxt, want_next.astype(t)), "next_krylov != residual / (the kernel's) norm"
    bases = st.get_bases()
    scal = st.scalars()
    if kind >= br.I64:
        an = st.get("an")
        wide = np.abs(res.astype(np.longdouble))
        ok, _ = br.rule_r(an[2], wide.max(axis=0), np.abs(res).max(axis=0), t)
        assert ok
        corr = _t_corr(st)
        assert same_bits(scal[0], ((an[2] / rn) * corr).astype(t)), "scalar of vector 0"
        assert np.all(scal[1:] == corr)
    for c in range(st.nrhs):
        want = br.store(kind, t, nxt[:, c], None if scal is None else scal[0, c])
        assert same_bits(bases[0, :, c], want), f"bases[0] != store(next), column {c}"
    assert np.all(bases[1:].view(np.uint8) == 0), "bases[1:] not zeroed"
    if kind == br.F16 and rows >= 16:
        assert np.all(bases[0, [1, 2, 5, 6, 7]].view(np.uint16) & 0x7fff == 0)      # flushed, with their signs
        assert np.all(bases[0, [2, 6]].view(np.uint16) == 0x8000) and np.all(bases[0, [1, 5]].view(np.uint16) == 0)
    if kind >= br.I64 and rows >= 16:
        top = np.iinfo(st.sdt).max // 2
        assert np.all(np.abs(bases[0, rows - 1].astype(np.float64)) >= top * 0.999)
    return st


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_restart(gexec, pair, layout):
    tn, kind = pair
    for rows, kd in ((1, 1), (3, 5), (4, 1), (5, 5), (1023, 5), (1024, 1), (1025, 30), (4099, 5)):
        _check_restart(gexec, tn, kind, rows, kd, layout)


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("layout", ["unit", "three_padded"])
def test_restart_many_rows(gexec, pair, layout):
    _check_restart(gexec, pair[0], pair[1], 70001, 1, layout)


# -------------------------------------------------------------------------------------------- arnoldi
def _decompress(st, bases, scal, k, c, wt):
    return br.load(st.kind, bases[k, :, c], wt, None if scal is None else scal[k, c])


def _sync_refs(st, refs):
    bases, scal = st.get_bases(), st.scalars()
    g = (st.get("gsin")[:st.kd], st.get("gcos")[:st.kd], st.get("rnc"), st.get("fin"))
    for r in refs:
        r.sync_from(bases, scal, *g)
    return bases, scal


def _free_plain(st, res, its, stop=None):
    """the plain restatement running on its own through the same emulated storage: its defects"""
    pl = st.ref_state(br.plain(st.t))
    nxt = pl.restart(res)
    hraw = np.zeros((its + 1, its, st.nrhs), np.clongdouble)
    for it in range(its):
        w = np.stack([_operator(pl.basis(it, c)) for c in range(st.nrhs)], axis=1).astype(st.t)
        nxt = pl.arnoldi(it, w)
        hraw[:it + 2, it] = pl.hess_raw[it]
    return pl, hraw


def _defects(st_like, its, nrhs, hraw):
    """(norm defect, orthogonality defect, Arnoldi relation defect), maxima over the cycle and the columns"""
    nd = od = ad = 0.0
    for c in range(nrhs):
        v = np.stack([br.decompressed(st_like, k, c) for k in range(its + 1)], axis=1)
        av = np.stack([_operator(v[:, k]) for k in range(its)], axis=1)
        ad = max(ad, float(np.max(np.abs(av - v @ hraw[:, :, c]))))
        for k in range(1, its + 1):
            nd = max(nd, br.norm_defect(st_like, k, c))
            od = max(od, br.orth_defect(st_like, k, c))
    return nd, od, ad


class _Snapshot:
    """a kernel state in the shape binding_refs' property functions expect"""

    def __init__(self, st, bases, scal):
        self.kind, self.t, self.bases = st.kind, st.t, bases
        self.scalars = np.ones(bases.shape[::2], np.longdouble) if scal is None else scal


def _run_arnoldi(gexec, tn, kind, rows, kd, layout, with_buffer):
    t = br.TYPES[tn]
    its = min(kd, rows - 1)
    st = State(gexec, tn, kind, rows, kd, layout, with_buffer, pad_small=2 if layout == "three_padded" else 0)
    rng = np.random.default_rng(rows + kd)
    res = _rand(rng, (rows, st.nrhs), t)
    st.put("residual", res)
    st.restart()
    st.put("gsin", np.zeros((max(kd, 1), st.nrhs), t)), st.put("gcos", np.zeros((max(kd, 1), st.nrhs), t))
    hp, pl = st.ref_state(br.hp(t)), st.ref_state(br.plain(t))
    eps = br.eps_of(t)
    hraw = np.zeros((its + 1, its, st.nrhs), np.clongdouble)
    last_rn = st.get("residual_norm").astype(np.float64)
    giv_defect = giv_plain = 0.0
    for it in range(its):
        bases, scal = _sync_refs(st, (hp, pl))
        w = np.stack([_operator(_decompress(st, bases, scal, it, c, t)) for c in range(st.nrhs)], axis=1).astype(t)
        st.put("next", w)
        st.put("h", np.full((kd + 2, st.nrhs), CANARY, t))
        st.arnoldi(it)
        n_hp, n_pl = hp.arnoldi(it, w), pl.arnoldi(it, w)
        nxt, h = st.get("next"), st.get("h")[:it + 2]
        bases, scal = st.get_bases(), st.scalars()
        rnc, rn, an = st.get("rnc"), st.get("residual_norm"), st.get("an")
        gs, gc = st.get("gsin"), st.get("gcos")
        assert np.all(st.get("fin") == it + 1)
        q = max(br.quantum(kind, t, None if scal is None else np.max(scal[:it + 2])), 0.0)
        for name, got, ref, plain_v, quant in (
                ("next", nxt, n_hp, n_pl, 0.0), ("hessenberg", h, hp.hess[it], pl.hess[it], q),
                ("rnc", rnc[:it + 2], hp.rnc[:it + 2], pl.rnc[:it + 2], q),
                ("residual_norm", rn, hp.residual_norm, pl.residual_norm, q),
                ("arnoldi_norm", an[1:2], hp.an[1:2], pl.an[1:2], 0.0),
                ("givens", np.stack([gs[it], gc[it]]), np.stack([hp.gsin[it], hp.gcos[it]]),
                 np.stack([pl.gsin[it], pl.gcos[it]]), q)):
            scale = float(np.max(np.abs(ref)))
            ok, ratio = br.rule_r(got, ref, plain_v, t, extra=2 * quant * scale)
            _note("arnoldi " + name, tn, kind, ratio)
            assert ok, (name, it, ratio)
        assert h[it + 1].tolist() == [0] * st.nrhs
        # what was stored is store(the kernel's own next_krylov) with the kernel's own scalar
        for c in range(st.nrhs):
            if kind >= br.I64:
                assert same_bits(scal[it + 1, c:c + 1], ((an[2, c:c + 1] / an[1, c:c + 1]) * _t_corr(st)).astype(t))
            want = br.store(kind, t, nxt[:, c], None if scal is None else scal[it + 1, c])
            assert same_bits(bases[it + 1, :, c], want), f"bases[{it + 1}] != store(next), column {c}"
        # exact-arithmetic identities of the rotation and the residual norm
        one = np.abs(gc[it].astype(np.clongdouble)) ** 2 + np.abs(gs[it].astype(np.clongdouble)) ** 2
        one_pl = np.abs(pl.gcos[it].astype(np.clongdouble)) ** 2 + np.abs(pl.gsin[it].astype(np.clongdouble)) ** 2
        giv_defect = max(giv_defect, float(np.max(np.abs(one - 1))))
        giv_plain = max(giv_plain, float(np.max(np.abs(one_pl - 1))))
        if st.cx:       # |z| through hypot: numpy's and the device's are each within an ulp of the true value
            assert np.all(np.abs(rn - np.abs(rnc[it + 1])) <= 2 * np.spacing(rn))
        else:
            assert same_bits(rn, np.abs(rnc[it + 1]))
        assert np.all(rn.astype(np.float64) <= last_rn * (1 + 4 * eps))
        last_rn = rn.astype(np.float64)
        for c in range(st.nrhs):
            hraw[:it + 2, it, c] = br.unrotate(h[:, c].astype(np.clongdouble), gc[:, c].astype(np.clongdouble),
                                               gs[:, c].astype(np.clongdouble), it)
    assert giv_defect <= 4 * giv_plain + 8 * eps
    if its:
        bases, scal = st.get_bases(), st.scalars()
        mine = _defects(_Snapshot(st, bases, scal), its, st.nrhs, hraw)
        free, hraw_pl = _free_plain(st, res, its)
        theirs = _defects(free, its, st.nrhs, hraw_pl)
        hmax = float(np.max(np.abs(hraw)))
        for name, a, b, scale in (("norm defect", mine[0], theirs[0], 1.0), ("orth defect", mine[1], theirs[1], 1.0),
                                  ("arnoldi relation", mine[2], theirs[2], hmax)):
            _note(name + " / plain's", tn, kind, a / max(b, eps * scale))
            assert a <= 4 * b + 8 * eps * scale, (name, a, b)
    return st


ARNOLDI = [("unit", 3, 5, True), ("unit", 5, 5, False), ("unit", 1023, 5, True), ("unit", 1025, 30, False),
           ("unit_aligned", 1025, 5, True), ("unit_aligned", 4, 1, True), ("unit", 4099, 5, False),
           ("stride2", 1025, 5, True), ("stride2", 5, 5, False), ("three", 1024, 5, True),
           ("three", 4099, 5, False), ("three_padded", 1023, 30, True), ("three_padded", 3, 5, False)]


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("layout,rows,kd,with_buffer", ARNOLDI)
def test_arnoldi(gexec, pair, layout, rows, kd, with_buffer):
    _run_arnoldi(gexec, pair[0], pair[1], rows, kd, layout, with_buffer)


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("layout", ["unit", "three"])
def test_arnoldi_many_rows(gexec, pair, layout):
    _run_arnoldi(gexec, pair[0], pair[1], 70001, 1 if layout == "three" else 5, layout, True)


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("layout,rows", [("unit", 1025), ("three", 1023), ("unit_aligned", 4099)])
def test_arnoldi_reorthogonalises(gexec, pair, layout, rows):
    """next_krylov = sum_k a_k basis_k + 1e-6 w (w a unit vector orthogonal to the basis): one Gram-Schmidt
    round leaves a vector that is far from orthogonal (tests/test_binding_refs_cpu.py shows a factor above
    100 over this bound), so the kernel must take the second round - decided on the device.  With three
    right-hand sides only the middle column is of that kind."""
    tn, kind = pair
    t = br.TYPES[tn]
    its = 5
    st = _run_arnoldi(gexec, tn, kind, rows, its + 1, layout, True)
    # the cycle above ran its + 1 steps; redo the last one with the nearly dependent vector
    bases, scal = st.get_bases(), st.scalars()
    rng = np.random.default_rng(rows)
    wide = np.clongdouble if st.cx else np.longdouble
    w = np.stack([_operator(_decompress(st, bases, scal, its, c, t)) for c in range(st.nrhs)], axis=1).astype(t)
    c = st.nrhs // 2
    v = np.stack([_decompress(st, bases, scal, k, c, wide) for k in range(its + 1)], axis=1)
    z = _rand(rng, (rows,), t).astype(wide)
    for _ in range(2):
        for k in range(its + 1):
            z = z - np.sum(z * np.conj(v[:, k])) / np.sum(np.abs(v[:, k]) ** 2) * v[:, k]
    z = z / np.sqrt(np.sum(np.abs(z) ** 2))
    w[:, c] = (v @ rng.uniform(0.5, 1.5, its + 1) + 1e-6 * z).astype(t)
    fin = st.get("fin")
    st.put("fin", fin - 1)
    pl = st.ref_state(br.plain(t))
    _sync_refs(st, (pl,))
    st.put("next", w)
    st.arnoldi(its)
    pl.arnoldi(its, w)
    assert pl.rounds_taken[c] >= 2
    mine = br.orth_defect(_Snapshot(st, st.get_bases(), st.scalars()), its + 1, c)
    theirs = br.orth_defect(pl, its + 1, c)
    _note("reorth defect / plain's", tn, kind, mine / max(theirs, br.eps_of(t)))
    assert mine <= 4 * theirs + 8 * br.eps_of(t), (mine, theirs)


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_arnoldi_leaves_a_stopped_column_alone(gexec, pair):
    tn, kind = pair
    t = br.TYPES[tn]
    rows, kd = 1025, 3
    st = State(gexec, tn, kind, rows, kd, "three")
    rng = np.random.default_rng(5)
    res = _rand(rng, (rows, 3), t)
    st.put("residual", res)
    st.restart()
    st.put("stop", np.array([0, br.STOPPED, 0], np.uint8))
    w = _rand(rng, (rows, 3), t)
    w[:, 1] = np.nan
    st.put("next", w)
    names = ("next", "h", "rnc", "gsin", "gcos", "fin", "residual_norm") + (() if st.cx else ("scalars",))
    before = {k: st.dev[k].get() for k in names}
    b0 = st.get_bases()
    st.arnoldi(0)
    for k in names:
        after = st.dev[k].get()
        if after.ndim == 1:
            assert same_bits(after[1:2], before[k][1:2]), k
        else:
            assert same_bits(after[:, 1], before[k][:, 1]), k + ": stopped column written"
    b1 = st.get_bases()
    assert same_bits(b1[:, :, 1], b0[:, :, 1])
    assert np.all(st.get("fin") == [1, 0, 1])
    hp, pl = st.ref_state(br.hp(t)), st.ref_state(br.plain(t))
    stop = np.array([0, br.STOPPED, 0], np.uint8)
    for r in (hp, pl):
        r.restart(res)
        r.sync_from(b0, st.scalars() if not st.cx else None, 0, 0, before["rnc"][:, :3], 0)
    with np.errstate(all="ignore"):
        n_hp, n_pl = hp.arnoldi(0, w, stop), pl.arnoldi(0, w, stop)
    for col in (0, 2):
        ok, ratio = br.rule_r(st.get("next")[:, col], n_hp[:, col], n_pl[:, col], t)
        assert ok, ratio


@pytest.mark.parametrize("pair", [("f64", br.KEEP), ("f32", br.KEEP), ("c128", br.KEEP)], ids=_ids)
def test_arnoldi_norm_of_a_zero_column_is_plus_zero(gexec, pair):
    """The middle one of three columns has next_krylov = 0 and residual_norm_collection(0) = 0: its Hessenberg
    entries are zero, the rotation is (cos, sin) = (0, 1) and the next residual norm is -conj(1) * 0, a
    negative zero for the real types.  residual_norm is its abs, as in the reference: +0.0.  The other two
    columns are ordinary and held against the references like test_arnoldi's."""
    tn, kind = pair
    t = br.TYPES[tn]
    rows, kd = 5, 1
    st = State(gexec, tn, kind, rows, kd, "three")
    rng = np.random.default_rng(11)
    st.put("residual", _rand(rng, (rows, 3), t))
    st.restart()
    st.put("gsin", np.zeros((kd, 3), t)), st.put("gcos", np.zeros((kd, 3), t))
    rnc = st.get("rnc")
    rnc[0, 1] = 0
    st.put("rnc", rnc)
    hp, pl = st.ref_state(br.hp(t)), st.ref_state(br.plain(t))
    bases, scal = _sync_refs(st, (hp, pl))
    w = np.stack([_operator(_decompress(st, bases, scal, 0, c, t)) for c in range(3)], axis=1).astype(t)
    w[:, 1] = 0
    st.put("next", w)
    st.arnoldi(0)
    with np.errstate(all="ignore"):         # the references divide the zero column by its norm as well
        n_hp, n_pl = hp.arnoldi(0, w), pl.arnoldi(0, w)
    rn, h, rnc = st.get("residual_norm"), st.get("h")[:2], st.get("rnc")
    assert np.all(h[:, 1] == 0) and rnc[1, 1] == 0
    assert rn[1] == 0 and not np.signbit(rn[1])
    gs, gc = st.get("gsin"), st.get("gcos")
    assert gc[0, 1] == 0 and gs[0, 1] == 1
    cols = [0, 2]
    for name, got, ref, plain_v in (
            ("next", st.get("next"), n_hp, n_pl), ("hessenberg", h, hp.hess[0], pl.hess[0]),
            ("rnc", rnc, hp.rnc, pl.rnc), ("residual_norm", rn[None], hp.residual_norm[None], pl.residual_norm[None]),
            ("givens", np.stack([gs[0], gc[0]]), np.stack([hp.gsin[0], hp.gcos[0]]),
             np.stack([pl.gsin[0], pl.gcos[0]]))):
        ok, ratio = br.rule_r(got[:, cols], ref[:, cols], plain_v[:, cols], t)
        assert ok, (name, ratio)
    if not st.cx:
        assert same_bits(rn[cols], np.abs(rnc[1, cols]))


# ------------------------------------------------------------------- a step's scratch is its own
def _walsh(k, rows):
    """row k of the Sylvester-Hadamard matrix of order 1024 on rows 1 .. 1024, zero elsewhere: entries +-1,
    different k orthogonal, squared norm 1024 - and the rows straddle the two row blocks of 1024"""
    r, par = np.arange(1024), np.zeros(1024, np.int64)
    for b in range(10):
        par ^= ((r & k) >> b) & 1
    v = np.zeros(rows)
    v[1:1025] = 1 - 2 * par
    return v


def _exact_steps(gexec, tn, seed, first):
    """Operands of the Arnoldi steps first .. first + 3 of a two-column problem in which every sum is exact
    (integers over 32, far below 2^24): basis vector k of column c is a Walsh vector over 32 (norm one), the
    next_krylov of step it the vectors 0 .. it with Gaussian-integer coefficients of parts in [-3, 3] plus a
    multiple of vector it + 1, which is what the step leaves: times 4 in column 0, times 1 in column 1 (the
    norm drops enough for a re-orthogonalisation round), times a unit that changes with the step.  Every step
    has its own next_krylov, Hessenberg column and residual_norm.  Returns (state, operands per step)."""
    t = br.TYPES[tn]
    rows, kd = 1025, 5
    st = State(gexec, tn, br.KEEP, rows, kd, (2, 2, 2, False))
    rng = np.random.default_rng(seed)
    walsh = np.stack([np.stack([_walsh(1 + 32 * seed + 8 * c + k, rows) for c in range(2)], axis=1)
                      for k in range(kd + 1)])
    st.put_bases((walsh / 32).astype(st.sdt))
    rot = np.zeros((kd, 2), t)
    st.put("gsin", rot)
    rot[:first] = 1                                       # the steps before `first`: identity rotations
    st.put("gcos", rot)
    st.put("rnc", rng.integers(1, 9, (kd + 1, 2)).astype(t))
    st.put("fin", np.full(2, first, np.uint64))
    ops = []
    for it in range(first, first + 4):
        a = rng.integers(-3, 4, (it + 1, 2)) + 1j * rng.integers(-3, 4, (it + 1, 2))
        lead = np.array([4, 1]) * (1, 1j, -1, -1j)[it % 4]
        w = np.einsum("kc,krc->rc", a, walsh[:it + 1]) + lead * walsh[it + 1]
        ops.append(dict(next=Dev(gexec, w.astype(t)), h=Dev(gexec, np.full((kd + 2, 2), CANARY, t)),
                        residual_norm=Dev(gexec, np.full(2, CANARY, st.rt))))
    return st, ops


def _step_outputs(st, ops):
    return ([v.get() for o in ops for v in o.values()] + [st.get_bases()] +
            [st.get(k) for k in ("gsin", "gcos", "rnc", "an", "fin")])


@pytest.mark.parametrize("pair", [("c128", br.KEEP), ("c64", br.KEEP)], ids=_ids)
def test_arnoldi_scratch_is_private_to_the_step(gexec, pair):
    """Steps 0 .. 3 of problem A on a second stream that a delay kernel holds, each followed at once by step
    it + 1 of an independent problem B on the executor's stream - B's scratch request is the larger one every
    time, and all of A's steps are still waiting when B's run.  A's outputs must be, bit for bit, those of the
    same four steps run alone: the partials, coefficients and flags of a step belong to that step."""
    import ctypes as C
    import torch
    tn = pair[0]
    alone, ops = _exact_steps(gexec, tn, 0, 0)
    for it in range(4):
        alone.arnoldi(it, **ops[it])
    want = _step_outputs(alone, ops)
    assert np.all(want[-1] == 4)
    held, ops_a = _exact_steps(gexec, tn, 0, 0)
    other, ops_b = _exact_steps(gexec, tn, 1, 1)
    side = torch.cuda.Stream()
    sst = C.c_void_p(side.cuda_stream)
    sync()
    _call("gkoc_debug_delay", sst, C.c_int64(3000), 1, 64, 0)
    for it in range(4):
        held.arnoldi(it, stream=sst, **ops_a[it])
        other.arnoldi(it + 1, stream=gexec.stream, **ops_b[it])
    sync()
    got = _step_outputs(held, ops_a)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), f"output {i} of the held steps differs from the run alone"
    assert np.all(np.isfinite(np.concatenate([v.get().reshape(-1) for o in ops_b for v in o.values()])))


# --------------------------------------------------------------------------------------- solve_krylov
@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("layout,rows,kd", [("unit", 1025, 30), ("unit", 5, 5), ("unit_aligned", 4099, 5),
                                            ("stride2", 1023, 5), ("three", 1025, 30), ("three_padded", 70001, 5),
                                            ("unit", 1, 1)])
def test_solve_krylov(gexec, pair, layout, rows, kd):
    """y against the long-double back substitution (H upper triangular, |diagonal| in [0.5, 2]); entries of
    y past final_iter_nums untouched; before_preconditioner = sum_k decompress(bases_k) y_k with the kernel's
    own y; per-column final_iter_nums, one of them zero (that column of the output is zero)"""
    tn, kind = pair
    t = br.TYPES[tn]
    st = State(gexec, tn, kind, rows, kd, layout)
    n = st.nrhs
    rng = np.random.default_rng(rows + kd)
    fin = np.array([kd, min(2, kd), 0][:n] if n > 1 else [kd], np.uint64)
    hess = np.zeros((kd, kd * n), t)
    for c in range(n):
        hm = np.triu(_rand(rng, (kd, kd), t))
        d = rng.uniform(0.5, 2, kd) * rng.choice([-1, 1], kd)
        hm[np.arange(kd), np.arange(kd)] = d
        hess[:, c::n] = hm
    rnc = _rand(rng, (kd + 1, n), t)
    st.put("rnc", rnc), st.put("fin", fin)
    scal = None
    if not st.cx:
        scal = (rng.uniform(0.5, 1.5, (kd + 1, n)) * br.correction(kind)).astype(t)
        st.put("scalars", scal)
    vecs = _rand(rng, (kd + 1, rows, n), t) / np.sqrt(rows)
    bases = np.zeros((kd + 1, rows, n), st.sdt)
    for k in range(kd + 1):
        for c in range(n):
            bases[k, :, c] = br.store(kind, t, vecs[k, :, c] * (0.9 / np.max(np.abs(vecs[k, :, c]))) *
                                      (scal[k, c] / br.correction(kind) if kind >= br.I64 else 1.0),
                                      None if scal is None else scal[k, c])
    st.put_bases(bases)
    dh = Dev(gexec, hess)
    dy = Dev(gexec, np.full((kd, st.lds), CANARY, t))
    dout = Dev(gexec, np.full((rows, st.ldn), CANARY, t))
    st.solve(dh, kd * n, dy, dout)
    y, out = dy.get(), dout.get()
    assert np.all(out[:, n:] == t(CANARY))
    assert same_bits(st.get_bases(), bases) and same_bits(dh.get(), hess)
    hp, pl = br.hp(t), br.plain(t)
    for c in range(n):
        mm = int(fin[c])
        assert np.all(y[mm:, c] == t(CANARY)), "y past final_iter_nums written"
        hm = hess[:mm, c::n][:, :mm]
        ok, ratio = br.rule_r(y[:mm, c], br.solve_upper(hp, hm, rnc[:mm, c]), br.solve_upper(pl, hm, rnc[:mm, c]), t)
        _note("solve_krylov y", tn, kind, ratio)
        assert ok, ratio
        ref, plain_v = np.zeros(rows, hp.wt), np.zeros(rows, pl.wt)
        for k in range(mm):
            s = None if scal is None else scal[k, c]
            ref = ref + br.load(kind, bases[k, :, c], hp.wt, s) * hp.wt(y[k, c])
            plain_v = (plain_v + (br.load(kind, bases[k, :, c], pl.wt, s) * y[k, c]).astype(t)).astype(t)
        if mm == 0:
            assert np.all(out[:, c] == 0)
        ok, ratio = br.rule_r(out[:, c], ref, plain_v, t)
        _note("solve_krylov Vy", tn, kind, ratio)
        assert ok, ratio


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_solve_krylov_without_rows(gexec, pair):
    """rows = 0 (a rank without rows): y is still the back substitution, nothing else is written, status 0"""
    tn, kind = pair
    t = br.TYPES[tn]
    kd = 3
    st = State(gexec, tn, kind, 0, kd, "three")
    rng = np.random.default_rng(3)
    hess = np.zeros((kd, kd * 3), t)
    for c in range(3):
        hm = np.triu(_rand(rng, (kd, kd), t))
        hm[np.arange(kd), np.arange(kd)] = rng.uniform(0.5, 2, kd)
        hess[:, c::3] = hm
    rnc = _rand(rng, (kd + 1, 3), t)
    fin = np.array([3, 1, 0], np.uint64)
    st.put("rnc", rnc), st.put("fin", fin)
    dh, dy = Dev(gexec, hess), Dev(gexec, np.full((kd, 3), CANARY, t))
    dout = Dev(gexec, np.full((1, 3), CANARY, t))
    st.solve(dh, kd * 3, dy, dout)
    y = dy.get()
    assert np.all(dout.get() == t(CANARY))
    for c in range(3):
        mm = int(fin[c])
        hm = hess[:mm, c::3][:, :mm]
        ok, ratio = br.rule_r(y[:mm, c], br.solve_upper(br.hp(t), hm, rnc[:mm, c]),
                              br.solve_upper(br.plain(t), hm, rnc[:mm, c]), t)
        assert ok, ratio
        assert np.all(y[mm:, c] == t(CANARY))


# ------------------------------------------------------------------------------------------ end to end
def _ld_matvec(a):
    data, ind, ptr = a.data.astype(np.longdouble), a.indices, a.indptr[:-1]
    return lambda x: np.add.reduceat(data * x[ind], ptr)


def _cb_gmres_on_device(gexec, tn, kind, a_sp, b, kd, target, limit):
    """CB-GMRES(kd) (core/solver/cb_gmres.cpp, identity preconditioner) over common_gmres::initialize, the
    three cb_gmres entry points and Csr.apply.  A cycle ends when the recurrence's residual norm reaches the
    target; the loop ends when the true residual of x, computed in numpy, confirms it.

    The iterate x and the residual b - A x at the start of a cycle are held in double (complex<double>); for
    the float value types that makes every cycle a step of iterative refinement: the residual is scaled to
    norm one, rounded to the value type and handed to restart, all three kernels and the products inside the
    cycle run in the value type, and the correction they return is scaled back and added to x in double.  For
    the double value types this is the plain loop (scale one, nothing rounded).  Returns (x, iterations,
    relative true residual)"""
    import torch
    import ginkgo_amd as g
    t = br.TYPES[tn]
    cx = br.is_complex(t)
    n = a_sp.shape[0]
    tt = {"f64": torch.float64, "f32": torch.float32, "c128": torch.complex128, "c64": torch.complex64}[tn]
    tw = torch.complex128 if cx else torch.float64
    rt = br.real_of(t)
    narrow = rt == np.float32
    a = g.Csr.from_scipy(gexec, a_sp.astype(rt))
    a_w = g.Csr.from_scipy(gexec, a_sp.astype(np.float64)) if narrow else a
    dev = gexec.device

    def spmv(mat, src, dst):
        if cx:      # a real matrix on (re, im) pairs: two real right-hand sides
            mat.apply(g.Dense(gexec, torch.view_as_real(src[:, 0])), g.Dense(gexec, torch.view_as_real(dst[:, 0])))
        else:
            mat.apply(g.Dense(gexec, src), g.Dense(gexec, dst))

    def z(*shape, dtype=tt):
        return torch.zeros(shape, dtype=dtype, device=dev)
    rtt = torch.float32 if narrow else torch.float64
    bw = z(n, 1, dtype=tw)
    bw.copy_(torch.from_numpy(b.reshape(-1, 1)))
    x, rw, tmpw = z(n, 1, dtype=tw), z(n, 1, dtype=tw), z(n, 1, dtype=tw)
    r, nxt, tmp, dx = z(n, 1), z(n, 1), z(n, 1), z(n, 1)
    gsin, gcos, rnc, hess = z(kd, 1), z(kd, 1), z(kd + 1, 1), z(kd + 1, kd)
    y, h_it, buf = z(kd, 1), z(kd + 2, 1), z(kd + 2, 1)
    rn = z(1, dtype=rtt)
    an = z(3, 1, dtype=rtt)
    scal = z(kd + 1, 1)
    fin = torch.zeros(1, dtype=torch.int64, device=dev)
    stop = torch.zeros(1, dtype=torch.uint8, device=dev)
    sdt = np.dtype(br.storage_dtype(kind, t))
    bases = torch.zeros((kd + 1) * n * sdt.itemsize + 64, dtype=torch.uint8, device=dev)
    s = gexec.stream
    bn = float(np.linalg.norm(b))
    iters, res = 0, 1.0
    r.copy_(bw)
    _call("gkoc_common_gmres_initialize_" + tn, s, n, 1, r.clone(), 1, r, 1, gsin, 1, gcos, 1, kd, stop)
    while iters < limit:
        spmv(a_w, x, tmpw)
        torch.sub(bw, tmpw, out=rw)
        scale = float(torch.linalg.vector_norm(rw).item()) if narrow else 1.0
        r.copy_(rw / scale)
        if cx:
            _call("gkoc_cb_gmres_restart_" + tn, s, n, 1, kd, r, 1, rn, rnc, 1, kind, bases, n, 1, nxt, 1, fin)
        else:
            _call("gkoc_cb_gmres_restart_" + tn, s, n, 1, kd, r, 1, rn, rnc, 1, an, 1, kind, bases, n, 1, scal, 1,
                  nxt, 1, fin)
        hess.zero_()
        for it in range(kd):
            spmv(a, nxt, tmp)
            nxt.copy_(tmp)
            head = (s, n, 1, it, nxt, 1, gsin, 1, gcos, 1, rn, rnc, 1, kind, bases, n, 1)
            tail = (h_it, 1, buf, 1, an, 1, fin, stop)
            if cx:
                _call("gkoc_cb_gmres_arnoldi_" + tn, *head, *tail)
            else:
                _call("gkoc_cb_gmres_arnoldi_" + tn, *head, scal, 1, *tail)
            hess[:it + 2, it] = h_it[:it + 2, 0]
            iters += 1
            if float(rn.item()) * scale / bn <= target or iters >= limit:
                break
        head = (s, n, 1, rnc, 1, kind, bases, n, 1)
        tail = (hess, kd, y, 1, dx, 1, fin)
        if cx:
            _call("gkoc_cb_gmres_solve_krylov_" + tn, *head, *tail)
        else:
            _call("gkoc_cb_gmres_solve_krylov_" + tn, *head, scal, 1, *tail)
        x += dx.to(tw) * scale
        torch.cuda.synchronize()
        xh = x.cpu().numpy()[:, 0]
        res = float(np.linalg.norm(b - a_sp @ xh) / bn)
        if res <= target:
            break
    return xh, iters, res


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("matrix", ["stencil7", "convdiff"])
def test_cb_gmres_end_to_end(gexec, pair, matrix):
    """CB-GMRES(30) on the 12^3 7-point stencil and its convection-diffusion variant.  The stopping target is
    an input: relative true residual 1e-9 for double with KEEP / F32 / I64 / I32 storage, for every other pair
    ten times the smallest true residual the long-double-arithmetic reference loop with that emulated storage
    reaches within three cycles.  The kernel loop must confirm the target in the reference loop's iteration
    count + 20 % (at least + 5).

    For the float value types that target (2e-14 ... 3e-9) is below what a solution vector held in float can
    reach (about 1e-7), so the driver keeps x and the cycle's starting residual in double and uses each
    CB-GMRES cycle as a step of iterative refinement (_cb_gmres_on_device); the kernels and the products
    inside a cycle run in the value type.  On an MI355X every pair then needs the reference's iteration count
    to within one iteration (58 ... 87), with true residuals of 1.6e-14 ... 3.2e-09 under their targets."""
    tn, kind = pair
    t = br.TYPES[tn]
    a_sp = br.model_matrices(12)[matrix]
    n = a_sp.shape[0]
    rng = np.random.default_rng(31)
    b = rng.uniform(-1, 1, n)
    bi = rng.uniform(-1, 1, n)
    if br.is_complex(t):
        b = b + 1j * bi
    mv = _ld_matvec(a_sp)
    if tn == "f64" and kind in (br.KEEP, br.F32, br.I64, br.I32):
        target, best = 1e-9, None
    else:
        _, _, best = br.cb_gmres_solve(br.hp(t), t, kind, mv, b, 30, 0.0, 3)
        target = 10 * best
    _, ref_iters, ref_res = br.cb_gmres_solve(br.hp(t), t, kind, mv, b, 30, target, 40)
    assert ref_res <= target
    limit = max(int(np.ceil(1.2 * ref_iters)), ref_iters + 5)
    x, iters, res = _cb_gmres_on_device(gexec, tn, kind, a_sp, b, 30, target, limit)
    print(f"CB-GMRES(30) {matrix} {tn}/{br.KIND_NAMES[kind]}: target {target:.3e} (reference best in three "
          f"cycles {best}), reference {ref_iters} iterations, limit {limit}; kernels {iters} iterations, "
          f"true residual {res:.3e}")
    assert res <= target, (res, target)
    assert iters <= limit


def test_zz_print_ratios():
    """largest |kernel - ref| / (eps max|ref|) per output, value type and storage kind seen in this run (for
    the property rows: the kernel's defect over the plain restatement's)"""
    for key, ratio in sorted(RATIOS.items()):
        print("cb_gmres ratio %-28s %-5s %-5s %10.2f" % (key + (ratio,)))
