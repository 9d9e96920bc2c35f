"""tests/mixed_refs.py against formulations that share no code with it (no GPU):

* real triples: the plain restatement equals oracle.csr_spmv_mixed / oracle.ell_spmv_mixed (pinned by the live
  reference, tests/test_mixed_cpu.py) bit for bit on every case family of tests/test_mixed_triples_gpu.py, in both
  index types, every kind of call (plain, advanced, beta == 0 over NaN, alpha == 0, integers), nrhs 1 and 3;
* complex triples: on well-scaled input the restatement agrees with a dense numpy product in AT (numpy's own
  complex arithmetic) within the bound, and the long-double value with a dense long-double product to a few
  long-double roundings;
* the bound (m + 8) eps(AT) S + eps(OT) |ref|: the restatement stays inside it on every case family and on rows
  of 0 .. 2500 entries with values spread over 1e-2 .. 1e2, and a row that lost its product of median magnitude
  falls outside it (figures printed, pytest -s);
* the cancellation row gives exactly 1 in AT and 0 when added in the narrow type;
* row_gather: `astype`, and the advanced form against the expression written out in numpy."""
import numpy as np
import pytest

import binding_refs as br
import mixed_refs as mr

FMTS = ("csr", "ell")
EXTRA = ("n_rows_0", "n_cols_0_empty_matrix")


def _families(fmt):
    return list(mr.CSR_FAMILIES if fmt == "csr" else mr.ELL_FAMILIES) + list(EXTRA)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8),
                                                                        b.reshape(-1).view(np.uint8))


def test_the_sixteen_triples():
    assert len(mr.TRIPLES) == 16 and len(mr.PLAIN) == 11 and len(mr.PLAIN_REAL) == 5 and len(mr.PLAIN_CPLX) == 6
    assert mr.widest(np.float32, np.float32, np.float64) is np.float64
    assert mr.widest(np.complex64, np.complex64, np.complex64) is np.complex64
    assert mr.widest(np.complex64, np.complex128) is np.complex128
    with pytest.raises(AssertionError):
        mr.widest(np.float64, np.complex64)
    for t in mr.PLAIN:                                   # a non-uniform triple always computes in the wide type
        assert mr.widest(*[mr.dt(x) for x in t]) in (np.float64, np.complex128)


@pytest.mark.parametrize("triple", mr.PLAIN_REAL + [("f32", "f64", "f64")], ids=mr.tid)
@pytest.mark.parametrize("fmt", FMTS)
def test_real_triples_equal_the_oracle_bit_for_bit(oracle, fmt, triple):
    checked = 0
    for name in _families(fmt):
        for nrhs in (1, 3):
            for kind in mr.kinds_of(name):
                x = mr.spmv_inputs(fmt, name, triple, nrhs, kind)
                p = x.reference()
                adv = dict(alpha=x.alpha, beta=x.beta, c=x.c) if x.alpha is not None else {}
                for idx in (np.int32, np.int64):
                    if fmt == "csr":
                        want = oracle.csr_spmv_mixed(x.ptrs.astype(idx), x.cols.astype(idx), x.vals, x.b,
                                                     mr.dt(triple[2]), **adv)
                    else:
                        want = oracle.ell_spmv_mixed(x.n_rows, x.k, x.stride, x.cols.astype(idx), x.vals, x.b,
                                                     mr.dt(triple[2]), **adv)
                    assert _same_bits(p.plain, want.reshape(p.plain.shape)), (name, nrhs, kind, idx)
                if kind == "integers":
                    assert np.array_equal(p.plain.astype(np.longdouble), p.ref), (name, nrhs)
                if kind == "beta_zero_over_nan_c":
                    assert np.all(np.isfinite(p.plain)), (name, nrhs)
                checked += p.plain.size
    assert checked > 5000


def _dense(x, wt):
    a = np.zeros((x.n_rows, x.n_cols), wt)
    if x.fmt == "csr":
        for r in range(x.n_rows):
            for k in range(int(x.ptrs[r]), int(x.ptrs[r + 1])):
                a[r, int(x.cols[k])] += wt(x.vals[k])
    else:
        for i in range(x.k):
            for r in range(x.n_rows):
                col = int(x.cols[r + i * x.stride])
                if col != -1:
                    a[r, col] += wt(x.vals[r + i * x.stride])
    return a


def _well_scaled(x, rng):
    """the same structure with values of modulus about one"""
    keep = ~np.isnan(x.vals.real)
    x.vals = x.vals.copy()
    x.vals[keep] = mr.values(rng, int(keep.sum()), x.vals.dtype)
    return x


@pytest.mark.parametrize("triple", [t for t in mr.TRIPLES if t[0] in mr.CPLX], ids=mr.tid)
@pytest.mark.parametrize("fmt", FMTS)
def test_complex_triples_against_numpy_and_long_double(fmt, triple):
    at, ot = mr.widest(*[mr.dt(t) for t in triple]), mr.dt(triple[2])
    rng = np.random.default_rng(5)
    names = [n for n in _families(fmt) if n not in mr.ONES_B and "2500" not in n]
    for name in names:
        for kind in ("plain", "advanced", "beta_zero_over_nan_c"):
            x = _well_scaled(mr.spmv_inputs(fmt, name, triple, 3, kind), rng)
            p = x.reference()
            for wt, got, tol in ((at, p.plain, mr.bound(p, at, ot)),
                                 (np.clongdouble, p.ref, (p.m + 8) * np.finfo(np.longdouble).eps * p.S)):
                want = _dense(x, wt) @ x.b.astype(wt)
                if x.alpha is not None:
                    want = wt(x.alpha) * want
                    if x.beta != 0:
                        want = want + wt(x.beta) * x.c.astype(wt)
                err = np.abs(got.astype(np.clongdouble) - want.astype(np.clongdouble))
                assert np.all(err <= tol), (name, kind, wt, float(np.max(err - tol)))
            err = np.abs(p.plain.astype(np.clongdouble) - p.ref)
            assert np.all(err <= mr.bound(p, at, ot)), (name, kind)


def _without_median_product(x):
    """the Csr inputs without, in every non-empty row, the entry whose |alpha v b| is the row's median (column 0
    of b); returns the new inputs and the rows that lost one"""
    keep = np.ones(len(x.vals), bool)
    rows = []
    for r in range(x.n_rows):
        lo, hi = int(x.ptrs[r]), int(x.ptrs[r + 1])
        if hi > lo:
            mag = np.abs(x.vals[lo:hi].astype(np.complex128)) * np.abs(x.b[x.cols[lo:hi], 0].astype(np.complex128))
            keep[lo + int(np.argsort(mag)[(hi - lo) // 2])] = False
            rows.append(r)
    y = mr.Inputs(**x.__dict__)
    lens = np.diff(x.ptrs)
    lens[rows] -= 1
    y.ptrs = np.concatenate([[0], np.cumsum(lens)])
    y.cols, y.vals = x.cols[keep], x.vals[keep]
    return y, np.array(rows)


@pytest.mark.parametrize("triple", mr.PLAIN_CPLX, ids=mr.tid)
def test_the_bound_holds_the_restatement_and_rejects_a_lost_product(triple):
    at, ot = np.complex128, mr.dt(triple[2])
    used, missed = 0.0, np.inf
    mr.CSR_FAMILIES["rows_of_0_to_2500_entries"] = [0, 1, 2, 3, 7, 64, 65, 1000, 1024, 1025, 2500]
    try:
        cases = [("csr", n) for n in mr.CSR_FAMILIES if n not in mr.ONES_B] + \
                [("ell", n) for n in mr.ELL_FAMILIES if n not in mr.ONES_B]
        for fmt, name in cases:
            for kind in ("plain", "advanced"):
                x = mr.spmv_inputs(fmt, name, triple, 1, kind)
                p = x.reference()
                tol = mr.bound(p, at, ot)
                err = np.abs(p.plain.astype(np.clongdouble) - p.ref)
                assert np.all(err <= tol), (fmt, name, kind)
                some = tol > 0
                used = max(used, float(np.max(err[some] / tol[some]))) if some.any() else used
                if fmt == "csr":
                    y, rows = _without_median_product(x)
                    q = y.reference()
                    err = np.abs(q.plain.astype(np.clongdouble) - p.ref)[rows]
                    assert np.all(err > tol[rows]), (name, kind, rows[np.argmin(err / tol[rows])])
                    missed = min(missed, float(np.min(err / tol[rows])))
    finally:
        del mr.CSR_FAMILIES["rows_of_0_to_2500_entries"]
    print("bound | %s | restatement uses at most %.3f of it | a lost median product exceeds it by %.1f x or more"
          % (mr.tid(triple), used, missed))


@pytest.mark.parametrize("triple", mr.PLAIN + [("f32", "f64", "f64")], ids=mr.tid)
@pytest.mark.parametrize("fmt", FMTS)
def test_cancellation_row(fmt, triple):
    narrow = np.complex64 if triple[0] in mr.CPLX else np.float32
    want = mr.cancellation_want(mr.dt(triple[2]))
    for kind in ("plain", "advanced"):
        x = mr.spmv_inputs(fmt, "cancellation_row", triple, 3, kind)
        p = x.reference()
        assert np.all(p.plain == want) and p.plain.dtype == mr.dt(triple[2]) and np.all(p.ref == want)
        assert np.all(x.reference(at=narrow).plain == 0), "2^30 + 1 rounds to 2^30 in float"
        x = mr.spmv_inputs(fmt, "wide_matrix_values_survive", triple, 3, kind)
        assert np.all(x.reference().plain == mr.survive_want(triple[0], triple[2]))


@pytest.mark.parametrize("vt,ot", [("f64", "f32"), ("f32", "f64"), ("c128", "c64"), ("c64", "c128")])
def test_row_gather_restatement(vt, ot):
    tv, to = mr.dt(vt), mr.dt(ot)
    at = mr.widest(tv, to)
    rng = np.random.default_rng(3)
    orig = np.concatenate([mr.special_sources(tv).reshape(-1, 2), mr.values(rng, (40, 2), tv)])
    rows = np.array([len(orig) - 1, 0, 3, 3, 3, 8, 1, 2, 4, 5, 6, 7])
    g = mr.row_gather(orig, rows, to)
    with np.errstate(over="ignore"):
        assert _same_bits(g.plain, orig[rows].astype(to))
    if vt == "f64":                                       # what the conversion must do with the special values
        narrowed = mr.row_gather(mr.special_sources(tv).reshape(-1, 1), np.arange(len(mr.SPECIAL)), to).plain[:, 0]
        got = dict(zip(mr.SPECIAL[1:], narrowed[1:]))
        assert mr.SPECIAL[0] == 0 and np.signbit(mr.SPECIAL[0]) and narrowed[0] == 0 and np.signbit(narrowed[0])
        assert got[1e300] == np.inf and got[-1e300] == -np.inf and got[3.5e38] == np.inf
        assert got[1e-40] == np.float32(1e-40) != 0 and got[1e-310] == 0
        assert got[1 + 2.0 ** -24] == 1 and got[1 + 3 * 2.0 ** -24] == np.float32(1 + 2.0 ** -22)    # ties to even
        assert got[2.0 ** -150] == 0 and got[1.5 * 2.0 ** -149] == np.float32(2.0 ** -148)
    orig = mr.values(rng, (50, 3), tv, spread=True)
    rows = rng.integers(0, 50, 77)
    out = mr.values(rng, (77, 3), to)
    alpha, beta = mr.scalars(tv, tv)
    g = mr.row_gather(orig, rows, to, alpha, beta, out)
    if not br.is_complex(tv):
        want = ((alpha * orig[rows]).astype(at) + at(beta) * out.astype(at)).astype(to)
        assert _same_bits(g.plain, want)
        assert np.all(np.abs(g.plain.astype(np.longdouble) - g.ref) <= mr.gather_bound(g, at, to))
    else:
        want = (alpha * orig[rows]).astype(tv).astype(at) + at(beta) * out.astype(at)
        tol = mr.gather_bound(g, at, to)
        # numpy's product in the source type and the textbook one each round within 3 eps(VT) of their term
        own = 6 * br.eps_of(tv) * np.abs(np.longdouble(np.abs(alpha)) * np.abs(orig[rows]).astype(np.longdouble))
        assert np.all(np.abs(g.plain.astype(np.clongdouble) - want.astype(np.clongdouble)) <= tol + own)
        assert np.all(np.abs(g.plain.astype(np.clongdouble) - g.ref) <= tol)
