"""Csr kernels that only the C++ binding calls, through the C ABI against tests/csr_struct_refs.py:
csr::spgemm_reuse / advanced_spgemm_reuse / spgeam_numeric (csrc/misc.hip), the index-set sub-matrix pair
(csrc/conversions.hip) and build_lookup_offsets / build_lookup (csrc/csr_lookup.hip).

The value kernels promise the reference's order with every operation rounded on its own, so they are first
compared bit for bit with the plain restatement and then under rule R with the long-double reference; the
index-set results are copies and the lookup tables integers, both compared exactly.  Every call's inputs are
read back and compared bit for bit, every output is followed by a canary.  The last test prints the largest
observed |kernel - ref| / (eps max|ref|) per entry point (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import binding_refs as br
import csr_struct_refs as cr
from binding_gpu import CANARY, Dev, DevCsr, call as _call, grid_cap_rows as _grid_cap_rows, out_buf as _out, \
    same_bits, sync, tail_ok as _tail_ok

pytestmark = pytest.mark.gpu

TN = ["f64", "f32", "c128", "c64"]
IT = {"i32": np.int32, "i64": np.int64}
STATS = {}
TRIPLET_BITS = {}


def _note(name, tn, ratio):
    STATS[(name, tn)] = max(STATS.get((name, tn), 0.0), float(ratio))


def _matrix(rng, rows, cols, density, t, empty_rows=()):
    p, c = cr.random_pattern(rng, rows, cols, density, empty_rows)
    return p, c, cr.random_values(rng, len(c), t)


# ------------------------------------------------------------------------------ SpGEMM reuse
def _spgemm_case(name, t):
    """A, B, D and the patterns of C: exact product, a strict superset, a strict subset"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "1x1":
        A, B, D = _matrix(rng, 1, 1, 1.1, t), _matrix(rng, 1, 1, 1.1, t), _matrix(rng, 1, 1, 1.1, t)
    elif name == "small":
        A, B, D = _matrix(rng, 17, 9, 0.3, t, (4,)), _matrix(rng, 9, 23, 0.3, t, (2,)), _matrix(rng, 17, 23, 0.2, t)
    elif name == "random":                       # empty rows in A, in B and (rows 0, 150) in C
        A, B = _matrix(rng, 300, 200, 0.05, t, (0, 150)), _matrix(rng, 200, 250, 0.05, t, (3, 100))
        D = _matrix(rng, 300, 250, 0.03, t, (0, 150, 7))
    else:                                        # the 7-point stencil squared
        p, c, v = cr.stencil7(6)
        A = (p, c, (v * rng.uniform(0.5, 1.5, len(v))).astype(t))
        B = (p, c, (v * rng.uniform(0.5, 1.5, len(v))).astype(t))
        D = _matrix(rng, 216, 216, 0.03, t)
    exact = cr.product_pattern(A[:2], B[:2])
    n_cols = int(max(B[1].max(initial=0), D[1].max(initial=0))) + 1
    extra = cr.random_pattern(rng, len(A[0]) - 1, n_cols, 0.04)
    sup = cr.product_pattern(A[:2], B[:2], (D[0], D[1]))
    sup = cr.product_pattern((np.arange(len(sup[0])), np.arange(len(sup[0]) - 1)), sup, extra)   # I sup + extra
    pats = {"exact": exact, "superset": sup, "subset": cr.every_other(exact)}
    if name == "1x1":
        del pats["subset"]                       # (a single entry has no strict subset but the empty one)
        pats["empty"] = (np.zeros(2, np.int64), np.zeros(0, np.int64))
    return A, B, D, pats


_REF_CACHE = {}


def _spgemm_refs(name, tn, pat_name, adv):
    key = (name, tn, pat_name, adv)
    if key not in _REF_CACHE:
        t = br.TYPES[tn]
        A, B, D, pats = _spgemm_case(name, t)
        alpha, beta = _scalars(t) if adv else (None, None)
        _REF_CACHE[key] = [cr.spgemm_reuse(ar, A, B, pats[pat_name], alpha, beta, D if adv else None)
                           for ar in (br.plain(t), br.hp(t))]
    return _REF_CACHE[key]


def _scalars(t):
    return (t(0.7 - 0.2j), t(-1.3 + 0.4j)) if br.is_complex(t) else (t(0.7), t(-1.3))


def _run_spgemm(gexec, tn, in_, A, B, pat, alpha=None, beta=None, D=None):
    t, it = br.TYPES[tn], IT[in_]
    da, db, dc = DevCsr(gexec, it, *A), DevCsr(gexec, it, *B), DevCsr(gexec, it, *pat)
    dd = DevCsr(gexec, it, *D) if D is not None else None
    nnz = len(pat[1])
    out = _out(gexec, nnz, t)                     # NaN everywhere: must be overwritten, never accumulated into
    sc = [Dev(gexec, np.array([v], t)) if v is not None else None for v in (alpha, beta)]
    _call("gkoc_csr_spgemm_reuse_" + tn + "_" + in_, gexec.stream, len(A[0]) - 1, *da.dev, *db.dev, sc[0], sc[1],
          *(dd.dev if dd else [None] * 3), *dc.dev, out)
    sync()
    got = out.get()
    assert _tail_ok(got, nnz)
    assert da.unchanged() and db.unchanged() and dc.unchanged() and (dd is None or dd.unchanged())
    return got[:nnz]


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("name", ["1x1", "small", "random", "stencil"])
def test_spgemm_reuse(gexec, name, tn, in_):
    t = br.TYPES[tn]
    A, B, D, pats = _spgemm_case(name, t)
    alpha, beta = _scalars(t)
    for pat_name, pat in pats.items():
        for adv in (False, True):
            got = _run_spgemm(gexec, tn, in_, A, B, pat, *((alpha, beta, D) if adv else ()))
            plain, ref = _spgemm_refs(name, tn, pat_name, adv)
            assert np.all(np.isfinite(got.view(br.real_of(t))))
            assert same_bits(got, plain), (pat_name, adv, np.max(np.abs(got - plain), initial=0))
            ok, ratio = br.rule_r(got, ref, plain, t)
            assert ok, (pat_name, adv, ratio)
            _note("spgemm_reuse" + (" advanced" if adv else ""), tn, ratio)
    # a superset's extra entries come out as zero in the plain form
    exact, sup = pats["exact"], pats["superset"]
    got = _run_spgemm(gexec, tn, in_, A, B, sup)
    for r in range(len(A[0]) - 1):
        have = set(exact[1][exact[0][r]:exact[0][r + 1]].tolist())
        for k in range(sup[0][r], sup[0][r + 1]):
            if int(sup[1][k]) not in have:
                assert got[k] == 0 and not np.signbit(got[k].real)


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
def test_spgemm_reuse_special_scalars(gexec, tn, in_):
    """The contract as the kernel is written: alpha and beta are multiplied in whatever their value, so
    alpha = 0 gives 0 + beta d on finite input, and beta = 0 does NOT mask D - 0 * NaN = NaN reaches every
    entry of C that D's pattern touches (the reference's advanced_spgemm_reuse multiplies the same way) and
    no other."""
    t = br.TYPES[tn]
    A, B, D, pats = _spgemm_case("small", t)
    pat = pats["superset"]
    _, beta = _scalars(t)
    got = _run_spgemm(gexec, tn, in_, A, B, pat, t(0), beta, D)
    assert same_bits(got, cr.spgemm_reuse(br.plain(t), A, B, pat, t(0), beta, D))
    only_d = cr.spgemm_reuse(br.plain(t), (A[0], A[1], np.zeros_like(A[2])), B, pat, t(1), beta, D)
    assert np.array_equal(got, only_d)                                   # (up to the sign of a zero)
    alpha, _ = _scalars(t)
    dn = (D[0], D[1], np.full(len(D[1]), np.nan, t))
    got = _run_spgemm(gexec, tn, in_, A, B, pat, alpha, t(0), dn)
    want = cr.spgemm_reuse(br.plain(t), A, B, pat, alpha, t(0), dn)
    assert np.array_equal(got, want, equal_nan=True)
    touched = np.zeros(len(pat[1]), bool)
    for r in range(len(A[0]) - 1):
        pos = cr._find(pat[1][pat[0][r]:pat[0][r + 1]], D[1][D[0][r]:D[0][r + 1]])
        touched[pat[0][r] + pos[pos >= 0]] = True
    assert touched.any() and not touched.all() and np.array_equal(np.isnan(got), touched)


def test_spgemm_reuse_argument_checks(gexec):
    from ginkgo_amd._lib import GkoError
    t = np.float64
    A, B, D, pats = _spgemm_case("small", t)
    pat = pats["exact"]
    da, db, dc, dd = (DevCsr(gexec, np.int32, *m) for m in (A, B, pat, D))
    one = Dev(gexec, np.ones(1, t))
    out = _out(gexec, len(pat[1]), t, fill=CANARY)
    n = len(A[0]) - 1
    for alpha, beta, d in ((one, None, dd.dev), (None, one, dd.dev), (one, one, [None] * 3)):
        with pytest.raises(GkoError, match="-1|go together"):
            _call("gkoc_csr_spgemm_reuse_f64_i32", gexec.stream, n, *da.dev, *db.dev, alpha, beta, *d, *dc.dev, out)
    _call("gkoc_csr_spgemm_reuse_f64_i32", gexec.stream, 0, *da.dev, *db.dev, None, None, None, None, None,
          *dc.dev, out)
    _call("gkoc_csr_spgeam_numeric_f64_i32", gexec.stream, 0, one, *da.dev, one, *da.dev, dc.dev[0], out)
    sync()
    assert np.all(out.get() == CANARY)


def _triplet_product(gexec, tn, in_, A, B, alpha, beta, D):
    """C = A B or alpha A B + beta D through gkoc_csr_spgemm_count / expand, sort_row_major, sum_duplicates and
    convert_idxs_to_ptrs (the path tests/test_conversions_gpu.py tests); (ptrs, cols, vals)"""
    from ginkgo_amd._lib import lib
    t, it = br.TYPES[tn], IT[in_]
    s = tn + "_" + in_
    n = len(A[0]) - 1
    da, db = DevCsr(gexec, it, *A), DevCsr(gexec, it, *B)
    dd = DevCsr(gexec, it, *D).dev if D is not None else [None] * 3
    off = Dev(gexec, np.zeros(n + 1, np.int64))
    total = C.c_int64(0)
    _call("gkoc_csr_spgemm_count_" + in_, gexec.stream, n, da.dev[0], da.dev[1], db.dev[0], dd[0], off,
          C.byref(total))
    tot = total.value
    tr, tc, tv = (Dev(gexec, np.zeros(max(tot, 1), x)) for x in (it, it, t))
    sc = [Dev(gexec, np.array([v], t)) if v is not None else None for v in (alpha, beta)]
    _call("gkoc_csr_spgemm_expand_" + s, gexec.stream, n, sc[0], *da.dev, *db.dev, sc[1], *dd, off, tr, tc, tv)
    f = lib().gkoc_sort_row_major_workspace_bytes
    f.restype = C.c_size_t
    nb = max(f(C.c_int64(tot), C.c_size_t(np.dtype(t).itemsize), C.c_size_t(np.dtype(it).itemsize)), 1)
    work = Dev(gexec, np.zeros(nb, np.uint8))
    _call("gkoc_sort_row_major_" + s, gexec.stream, tot, tr, tc, tv, work, C.c_size_t(nb))
    f = lib().gkoc_compact_workspace_bytes
    f.restype = C.c_size_t
    nb = max(f(C.c_int64(tot)), 1)
    w2 = Dev(gexec, np.zeros(nb, np.uint8))
    kept = C.c_int64(0)
    _call("gkoc_sum_duplicates_count_" + in_, gexec.stream, tot, tr, tc, w2, C.c_size_t(nb), C.byref(kept))
    k = kept.value
    orow, ocol, oval = (Dev(gexec, np.zeros(max(k, 1), x)) for x in (it, it, t))
    _call("gkoc_sum_duplicates_fill_" + s, gexec.stream, tot, tr, tc, tv, w2, orow, ocol, oval)
    ptrs = Dev(gexec, np.zeros(n + 1, it))
    _call("gkoc_convert_idxs_to_ptrs_" + in_, gexec.stream, k, orow, n, ptrs)
    sync()
    return ptrs.get().astype(np.int64), ocol.get()[:k].astype(np.int64), oval.get()[:k]


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("name", ["small", "random", "stencil"])
def test_spgemm_reuse_against_the_triplet_path(gexec, name, tn, in_):
    """The triplet path gives pattern and values of the product; the reuse kernel on that pattern agrees with
    it under rule R.  Bit for bit they agree in the plain form (the same order: 0 + products); in the advanced
    form the triplet path adds beta d FIRST (0 + beta d + products), the reuse kernel LAST, so entries that get
    D and at least two products may differ in the last bits - recorded per case, printed by the last test."""
    t = br.TYPES[tn]
    A, B, D, _ = _spgemm_case(name, t)
    alpha, beta = _scalars(t)
    for adv in (False, True):
        args = (alpha, beta, D) if adv else (None, None, None)
        ptrs, cols, vals = _triplet_product(gexec, tn, in_, A, B, *args)
        pat = cr.product_pattern(A[:2], B[:2], (D[0], D[1]) if adv else None)
        assert np.array_equal(ptrs, pat[0]) and np.array_equal(cols, pat[1])
        got = _run_spgemm(gexec, tn, in_, A, B, pat, *(args if adv else ()))
        ref = cr.spgemm_reuse(br.hp(t), A, B, pat, *args)
        plain = cr.spgemm_reuse(br.plain(t), A, B, pat, *args)
        for v in (got, vals):
            ok, ratio = br.rule_r(v, ref, plain, t)
            assert ok, ratio
        same = same_bits(got, vals)
        TRIPLET_BITS[(name, "advanced" if adv else "plain", tn, in_)] = \
            "same bits" if same else "%d of %d entries differ" % (np.count_nonzero(got != vals), len(vals))
        if not adv:
            assert same


# ------------------------------------------------------------------------------ SpGEAM numeric
def _run_spgeam(gexec, tn, in_, alpha, A, beta, B, c_ptrs, nnz):
    t, it = br.TYPES[tn], IT[in_]
    da, db = DevCsr(gexec, it, *A), DevCsr(gexec, it, *B)
    dp = Dev(gexec, np.asarray(c_ptrs).astype(it))
    out = _out(gexec, nnz, t)
    sc = [Dev(gexec, np.array([v], t)) for v in (alpha, beta)]
    _call("gkoc_csr_spgeam_numeric_" + tn + "_" + in_, gexec.stream, len(c_ptrs) - 1, sc[0], *da.dev, sc[1],
          *db.dev, dp, out)
    sync()
    got = out.get()
    assert _tail_ok(got, nnz) and da.unchanged() and db.unchanged()
    assert same_bits(dp.get(), np.asarray(c_ptrs).astype(it))
    return got[:nnz]


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("rows,cols,dens", [(1, 1, 1.1), (17, 23, 0.3), (300, 250, 0.05), (216, 216, 0)])
def test_spgeam_numeric(gexec, tn, in_, rows, cols, dens):
    t = br.TYPES[tn]
    rng = np.random.default_rng(rows + cols)
    if dens:
        empty = ((0, rows // 2), (0, 5)) if rows > 5 else ((), ())
        A, B = _matrix(rng, rows, cols, dens, t, empty[0]), _matrix(rng, rows, cols, dens, t, empty[1])
    else:                                    # the stencil plus a random matrix that overlaps it partly
        p, c, v = cr.stencil7(6)
        A, B = (p, c, (v * rng.uniform(0.5, 1.5, len(v))).astype(t)), _matrix(rng, rows, cols, 0.03, t)
    eye = (np.arange(rows + 1), np.arange(rows))
    pat = cr.product_pattern(eye, A[:2], B[:2])                      # the union
    nnz = len(pat[1])
    for alpha, beta in (_scalars(t), (t(0), t(1)), (t(1), t(0))):
        got = _run_spgeam(gexec, tn, in_, alpha, A, beta, B, pat[0], nnz)
        plain = cr.spgeam_numeric(br.plain(t), alpha, A, beta, B, pat[0])
        assert np.all(np.isfinite(got.view(br.real_of(t))))
        assert same_bits(got, plain), np.max(np.abs(got - plain), initial=0)
        ok, ratio = br.rule_r(got, cr.spgeam_numeric(br.hp(t), alpha, A, beta, B, pat[0]), plain, t)
        assert ok, ratio
        _note("spgeam_numeric", tn, ratio)
    # C = A + A on A's own pattern, and B's values against the dense sum on the union
    got = _run_spgeam(gexec, tn, in_, t(1), A, t(1), A, A[0], len(A[1]))
    assert np.array_equal(got, A[2] + A[2])


# --------------------------------------------------------------------- rows beyond the grid cap
@pytest.mark.parametrize("tn,in_", [("f64", "i32"), ("f32", "i64")])
def test_spgemm_reuse_rows_beyond_the_grid_cap(gexec, tn, in_):
    """one row more than a block past 256 * 4 * max_stream_blocks threads: diagonal A, B, C with small integer
    values, every row of C compared - the last one too"""
    t = br.TYPES[tn]
    n = _grid_cap_rows() + 257
    ptrs, cols = np.arange(n + 1), np.arange(n)
    a, b, d = ((np.arange(n) + s) % m + 1 for s, m in ((0, 7), (3, 5), (1, 3)))
    A, B, D, pat = (ptrs, cols, a.astype(t)), (ptrs, cols, b.astype(t)), (ptrs, cols, d.astype(t)), (ptrs, cols)
    got = _run_spgemm(gexec, tn, in_, A, B, pat)
    assert np.array_equal(got, (a * b).astype(t)), np.flatnonzero(got != (a * b).astype(t))[:4]
    got = _run_spgemm(gexec, tn, in_, A, B, pat, t(2), t(-3), D)
    assert np.array_equal(got, (2 * a * b - 3 * d).astype(t))


@pytest.mark.parametrize("tn,in_", [("f64", "i32"), ("f32", "i64")])
def test_spgeam_numeric_rows_beyond_the_grid_cap(gexec, tn, in_):
    t = br.TYPES[tn]
    n = _grid_cap_rows() + 257
    ptrs, cols = np.arange(n + 1), np.arange(n)
    a, b = (np.arange(n) % 7 + 1), (np.arange(n) + 3) % 5 + 1
    got = _run_spgeam(gexec, tn, in_, t(2), (ptrs, cols, a.astype(t)), t(-3), (ptrs, cols, b.astype(t)), ptrs, n)
    assert np.array_equal(got, (2 * a - 3 * b).astype(t)), np.flatnonzero(got != (2 * a - 3 * b).astype(t))[:4]


# ---------------------------------------------------------------------------------- index sets
INDEX_SETS = {
    "all": ([(0, 40)], [(0, 50)]),
    "one of each": ([(7, 8)], [(11, 12)]),
    "several": ([(0, 1), (3, 9), (9, 15), (39, 40)], [(0, 1), (4, 10), (10, 11), (30, 41), (49, 50)]),
    "inner": ([(5, 20), (25, 30)], [(2, 3), (20, 45)]),
}


def _run_index_set(gexec, tn, in_, rs, cs, A, size=None):
    """count, the caller's scan, fill; (counts, out_cols, out_vals)"""
    t, it = br.TYPES[tn], IT[in_]
    s = tn + "_" + in_
    da = DevCsr(gexec, it, *A)
    n = rs.num_elems
    sets = [Dev(gexec, x.astype(it)) for x in (rs.begin, rs.superset, cs.begin, cs.end, cs.superset)]
    size = cs.size if size is None else size
    counts = _out(gexec, n + 1, it, fill=0, tail=2)                  # entry n: room for the scan's total
    _call("gkoc_csr_count_in_index_set_" + s, gexec.stream, n, rs.num_subsets, sets[0], sets[1], cs.num_subsets,
          sets[2], sets[3], size, da.dev[0], da.dev[1], counts)
    sync()
    got_counts = counts.get()
    assert _tail_ok(got_counts, n + 1) and got_counts[n] == 0
    _call("gkoc_prefix_sum_nonnegative_" + in_, gexec.stream, counts, n + 1)
    sync()
    out_ptrs = counts.get()[:n + 1]
    nnz = int(out_ptrs[n])
    oc, ov = _out(gexec, nnz, it, fill=-5), _out(gexec, nnz, t)
    _call("gkoc_csr_submatrix_from_index_set_" + s, gexec.stream, n, rs.num_subsets, sets[0], sets[1],
          cs.num_subsets, sets[2], sets[3], sets[4], size, *da.dev, counts, oc, ov)
    sync()
    goc, gov = oc.get(), ov.get()
    assert _tail_ok(goc, nnz) and _tail_ok(gov, nnz) and da.unchanged()
    for d, h in zip(sets, (rs.begin, rs.superset, cs.begin, cs.end, cs.superset)):
        assert same_bits(d.get(), h.astype(it))
    assert same_bits(counts.get()[:n + 1], out_ptrs)
    return got_counts[:n], out_ptrs, goc[:nnz], gov[:nnz]


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("tn", TN)
@pytest.mark.parametrize("sets", list(INDEX_SETS))
def test_index_set_submatrix(gexec, tn, in_, sets):
    t, it = br.TYPES[tn], IT[in_]
    rows, cols = 40, 50
    A = _matrix(np.random.default_rng(17), rows, cols, 0.25, t, (3, 12, 39))
    rr, cc = INDEX_SETS[sets]
    rs, cs = cr.IndexSet(rr, rows), cr.IndexSet(cc, cols)
    counts, ptrs, oc, ov = _run_index_set(gexec, tn, in_, rs, cs, A)
    want = cr.index_set_count(rs, cs, A[:2])
    assert np.array_equal(counts, want) and np.array_equal(ptrs, np.concatenate([[0], np.cumsum(want)]))
    wc, wv = cr.index_set_fill(rs, cs, A)
    assert np.array_equal(oc, wc) and same_bits(ov, wv)
    if sets == "all":                                    # reproduces the rows
        assert np.array_equal(counts, np.diff(A[0])) and np.array_equal(oc, A[1]) and same_bits(ov, A[2])
    # an index space that ends inside the column set: columns >= col_set_size are dropped
    counts, ptrs, oc, ov = _run_index_set(gexec, tn, in_, rs, cs, A, size=33)
    cs.size = 33
    want = cr.index_set_count(rs, cs, A[:2])
    wc, wv = cr.index_set_fill(rs, cs, A)
    assert np.array_equal(counts, want) and np.array_equal(oc, wc) and same_bits(ov, wv)
    assert len(wc) == 0 or A[1][np.isin(A[2], wv)].max() < 33


@pytest.mark.parametrize("in_", list(IT))
def test_index_set_edges(gexec, in_):
    tn, t, it = "f64", np.float64, IT[in_]
    rng = np.random.default_rng(23)
    rows, cols = 40, 50
    p, c = cr.random_pattern(rng, rows, cols, 0.25, (3,))
    keep = (c < 20) | (c >= 26)                                     # nothing stored in columns [20, 26)
    p = np.concatenate([[0], np.cumsum([np.count_nonzero(keep[p[r]:p[r + 1]]) for r in range(rows)])])
    A = (p, c[keep], cr.random_values(rng, int(keep.sum()), t))
    rs = cr.IndexSet([(0, 10), (30, 40)], rows)
    counts, ptrs, oc, ov = _run_index_set(gexec, tn, in_, rs, cr.IndexSet([(20, 23), (23, 26)], cols), A)
    assert np.all(counts == 0) and np.all(ptrs == 0) and len(oc) == 0
    # no result rows: nothing is launched, nothing is touched
    out = _out(gexec, 4, it, fill=CANARY)
    da = DevCsr(gexec, it, *A)
    _call("gkoc_csr_count_in_index_set_f64_" + in_, gexec.stream, 0, 0, None, None, 0, None, None, cols,
          da.dev[0], da.dev[1], out)
    _call("gkoc_csr_submatrix_from_index_set_f64_" + in_, gexec.stream, 0, 0, None, None, 0, None, None, None,
          cols, *da.dev, out, out, None)
    sync()
    assert np.all(out.get() == it(CANARY))


def test_index_set_rows_beyond_the_grid_cap(gexec):
    """the CV_LAUNCH style (capped grid, GKOC_FOR_EACH): one result row per matrix row, diagonal matrix"""
    n = _grid_cap_rows() + 257
    it = np.int32
    da = DevCsr(gexec, it, np.arange(n + 1), np.arange(n))
    sets = [Dev(gexec, np.array(x, it)) for x in ([0], [0, n], [0, n - 1], [n - 2, n], [0, n - 2])]
    counts = _out(gexec, n, it, fill=-5)
    _call("gkoc_csr_count_in_index_set_f64_i32", gexec.stream, n, 1, sets[0], sets[1], 2, sets[2], sets[3], n,
          da.dev[0], da.dev[1], counts)
    sync()
    got = counts.get()
    want = np.ones(n, it)
    want[n - 2] = 0                                                  # the one column no subset holds
    assert _tail_ok(got, n) and np.array_equal(got[:n], want), np.flatnonzero(got[:n] != want)[:4]


# -------------------------------------------------------------------------------------- lookup
def _lookup_rows(it):
    top = 2 ** 31 - 2
    rows = [[], [5], list(range(10, 30)), [top - 3, top - 2, top - 1, top],               # empty, single, full
            [100, 131], list(range(100, 132, 2)), [c for c in range(100, 132) if c != 117],   # range 32
            [0, 32], [c for c in range(0, 33) if c % 3 != 1],                             # range 33
            [1, 64], list(range(1, 65, 3)), [c for c in range(1, 65) if c != 2],          # range 64
            [1, 65], list(range(1, 66, 2)), [c for c in range(1, 66) if c != 64],         # range 65
            [0, 10, 63], [0, 10, 64], [0, 10, 95], [0, 10, 96],     # 3 entries: 6 hash slots; 4, 6, 6, 8 bitmap words
            [7, 500, 100000, 2000000],                              # wide and sparse: hash
            [3, 163, 323, 483],                                     # 8 slots, p = 5: all four hash to slot 7
            [3, 11, 19, 27],                                        # the same collisions where only hash is allowed
            [top - 300, top - 150, top - 2]]                        # col * p wraps in uint32
    if it == np.int64:
        rows += [[2 ** 32 + 1, 2 ** 32 + 70, 2 ** 33 + 5], [2 ** 40 + 3, 2 ** 40 + 163, 2 ** 40 + 323, 2 ** 40 + 483]]
    rng = np.random.default_rng(31)
    for _ in range(3000):
        n = int(rng.integers(0, 40))
        width = int(rng.choice([40, 200, 5000]))
        base = int(rng.integers(0, 100000))
        rows.append(sorted(set((base + rng.integers(0, width, n)).tolist())))
    return rows


def _probe_columns(row, special):
    """columns to ask the decoder about: every one of [min - 1, max + 1] for the hand-made rows with a range
    below 200000 and random rows with one below 256, else the neighbours of every stored column"""
    if not row:
        return [0, 5]
    lo, hi = row[0] - 1, row[-1] + 1
    if hi - lo < (200000 if special else 256):
        return range(max(lo, 0), hi + 1)
    return sorted({max(c + d, 0) for c in row for d in (-1, 0, 1)} | {lo + 600, max(hi - 600, 0)})


@pytest.mark.parametrize("in_", list(IT))
@pytest.mark.parametrize("allowed", range(8))
def test_build_lookup(gexec, in_, allowed):
    it = IT[in_]
    bits = np.dtype(it).itemsize * 8
    rows = _lookup_rows(it)
    n = len(rows)
    n_special = n - 3000
    ptrs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = np.array([c for r in rows for c in r], np.int64)
    da = DevCsr(gexec, it, ptrs, cols)
    offs = _out(gexec, n + 1, it, fill=-5, tail=1)
    _call("gkoc_csr_build_lookup_offsets_" + in_, gexec.stream, n, *da.dev, allowed, offs)
    sync()
    got_offs = offs.get()
    want_offs = cr.lookup_offsets(ptrs, cols, allowed, it)
    assert _tail_ok(got_offs, n + 1) and same_bits(got_offs[:n + 1], want_offs)
    total = int(want_offs[n])
    desc = _out(gexec, n, np.int64, fill=-5, tail=1)
    storage = Dev(gexec, np.full(total + 16, -777, np.int32))
    _call("gkoc_csr_build_lookup_" + in_, gexec.stream, n, *da.dev, allowed, offs, desc, storage)
    sync()
    got_desc, got_st = desc.get(), storage.get()
    assert da.unchanged() and same_bits(offs.get(), got_offs)
    want_desc, want_st, written = cr.lookup_build(ptrs, cols, allowed, want_offs, it)
    assert np.array_equal(np.diff(want_offs.astype(np.int64)), written)
    assert _tail_ok(got_desc, n) and same_bits(got_desc[:n], want_desc)
    assert same_bits(got_st[:total], want_st) and np.all(got_st[total:] == -777)
    # the rows meant to hit a branch do hit it
    if allowed == 7:
        kinds = [int(d) & 7 for d in want_desc[:n_special]]
        assert kinds[:4] == [1, 1, 1, 1] and kinds[4:7] == [2, 2, 2] and kinds[12] == 4 and kinds[13:15] == [2, 2]
        assert kinds[15:19] == [2, 2, 2, 4] and kinds[19:21] == [4, 4] and kinds[22] == 4
    if allowed & 4:
        r = 20 if allowed & 2 else 21                # the colliding row that is a hash table here
        st = want_st[want_offs[r]:want_offs[r + 1]]
        assert (int(want_desc[r]) >> 32) == 5 and list(st[[7, 0, 1, 2]]) == [0, 1, 2, 3]   # wrapped past the end
    # independently: a consumer of the device's tables finds every stored entry and no other column
    for r, row in enumerate(rows):
        st = got_st[got_offs[r]:got_offs[r + 1]]
        if (int(got_desc[r]) & 7) == 0:
            assert len(st) == 0
            continue
        stored = {c: k for k, c in enumerate(row)}
        for c in _probe_columns(row, r < n_special):
            assert cr.lookup_position(got_desc[r], st, row, c, bits) == stored.get(c, -1), (r, c)


@pytest.mark.parametrize("in_", list(IT))
def test_build_lookup_without_rows(gexec, in_):
    it = IT[in_]
    offs = _out(gexec, 1, it, fill=-5, tail=2)
    _call("gkoc_csr_build_lookup_offsets_" + in_, gexec.stream, 0, None, None, 7, offs)
    _call("gkoc_csr_build_lookup_" + in_, gexec.stream, 0, None, None, 7, offs, None, None)
    sync()
    got = offs.get()
    assert got[0] == 0 and _tail_ok(got, 1)


def test_print_tables():
    print("\nlargest observed |kernel - ref| / (eps max|ref|)")
    print("| entry point | " + " | ".join(TN) + " |")
    for name in sorted({k[0] for k in STATS}):
        print("| " + name + " | " + " | ".join("%.2f" % STATS.get((name, tn), float("nan")) for tn in TN) + " |")
    print("\nreuse kernel against the triplet path, bit for bit")
    for key in sorted(TRIPLET_BITS):
        print("| " + " | ".join(key) + " | " + TRIPLET_BITS[key] + " |")
