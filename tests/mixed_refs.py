"""numpy restatements of the mixed-precision products of ginkgo_amd/csrc/mixed_precision.hip: csr / ell spmv
and advanced_spmv for any of the 16 (matrix, input, output) value-type triples, and dense::row_gather /
advanced_row_gather between two precisions.  Same conventions as tests/binding_refs.py (`Arith`, `hp`, `plain`)
and the textbook complex product of tests/csr_struct_refs.py (`mul`, `add`); nothing here touches a GPU.
tests/test_mixed_refs_cpu.py checks these functions against the oracle (real triples, bit for bit), numpy's own
complex arithmetic and the long-double value.

The operation as include/gko_cdna4.h states it.  AT = arithmetic_type = the widest of the three types.  Every
operand is widened to AT as it is loaded; alpha has the matrix' type, beta the output's.  A row starts from
    Csr: c * beta      Ell: beta * c      both: an exact zero when beta == 0 (c is not read), or without scalars,
then adds (alpha * v_k) * b_k for its stored entries in k order (Ell: the column slices in order, padding -1
skipped), every product the textbook one (ac - bd, ad + bc) with each real operation rounded on its own, every
addition rounded; the result is narrowed to the output type once, on the store.

`csr_spmv` / `ell_spmv` return a `Product`:
    ref    the value in np.longdouble / np.clongdouble (same formula, nothing rounded to AT)
    plain  the restatement above in AT, narrowed to the output type
    S      |beta||c| + sum_k |alpha||v_k||b_k| per output entry, long double
    m      stored entries of the row, per output entry
`bound(p, at, ot)` = (m + 8) eps(AT) S + eps(OT) |ref| is what a kernel may miss `ref` by: m additions cost at most
eps(AT) / 2 each of a partial sum bounded by S, the two textbook products under 3 eps(AT) each of their term
(three roundings of eps / 2 per part, sqrt(2) for the modulus), beta c and the last addition make up the rest of
the 8, and the final term is the one narrowing (eps(OT) / 2 per part).

`row_gather` returns a `Gather(ref, plain, S)`: plain form `astype`; advanced form
OT(AT(alpha * orig) + AT(beta) * AT(out)) with alpha * orig formed in the SOURCE type (alpha and beta both have
it), S = |alpha||orig| + |beta||out|.  `ref` is the long-double value of alpha orig + beta out, except that a
NARROW source keeps its product as the source type forms it: rounding that product to the narrow type is part of
the operation (it moves the result by eps(narrow), far more than any bound in eps(AT)), so the reference takes
the textbook product in the source type as its first term and adds the rest in long double."""
import collections

import numpy as np

import binding_refs as br
import csr_struct_refs as cr

CODE = {"f64": 0, "f32": 1, "c128": 2, "c64": 3}           # GKOC_VT_*
REAL, CPLX = ("f64", "f32"), ("c128", "c64")
TRIPLES = [(m, i, o) for fam in (REAL, CPLX) for m in fam for i in fam for o in fam]
UNIFORM = [t for t in TRIPLES if t[0] == t[1] == t[2]]
TUNED = UNIFORM + [("f32", "f64", "f64")]                   # routed to csr_spmv.hip / formats.hip / complex_blas.hip
PLAIN = [t for t in TRIPLES if t not in TUNED]              # the two plain kernels of mixed_precision.hip
PLAIN_REAL = [t for t in PLAIN if t[0] in REAL]
PLAIN_CPLX = [t for t in PLAIN if t[0] in CPLX]

Product = collections.namedtuple("Product", "ref plain S m")
Gather = collections.namedtuple("Gather", "ref plain S")


def dt(name):
    return br.TYPES[name]


def tid(triple):
    return "-".join(triple)


def widest(*types):
    """arithmetic_type: the wide type of the family if any operand has it"""
    types = [np.dtype(t).type for t in types]
    cx = br.is_complex(types[0])
    assert all(br.is_complex(t) == cx for t in types), "real and complex value types in one product"
    wide = np.complex128 if cx else np.float64
    return wide if wide in types else (np.complex64 if cx else np.float32)


def _narrow(x, ot):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(ot)


def _sum_rows(ar, start, prod, erow, erank):
    """start (n_rows x nrhs) plus the products (entries x nrhs) of each row in rank order, each addition rounded"""
    out = start.copy()
    if len(erank) == 0:
        return out
    order = np.argsort(erank, kind="stable")
    ranks = erank[order]
    cuts = np.searchsorted(ranks, np.arange(int(ranks[-1]) + 2))
    for r in range(len(cuts) - 1):
        e = order[cuts[r]:cuts[r + 1]]                       # at most one entry per row
        out[erow[e]] = cr.add(ar, out[erow[e]], prod[e])
    return out


def _product(ar, order, erow, erank, ecol, vals, b, n_rows, alpha, beta, c):
    """one arithmetic: the rows' sums in ar.wt, not narrowed.  order: 'c*beta' (Csr) or 'beta*c' (Ell)"""
    b = ar.a(b)
    nrhs = b.shape[1]
    v = ar.a(vals)
    if alpha is not None:
        v = cr.mul(ar, ar.wt(alpha), v)
    prod = cr.mul(ar, v[:, None], b[ecol].reshape(len(ecol), nrhs))
    start = np.zeros((n_rows, nrhs), ar.wt)
    if alpha is not None and ar.wt(beta) != 0:
        cc, bb = ar.a(c).reshape(n_rows, nrhs), ar.wt(beta)
        start = cr.mul(ar, cc, bb) if order == "c*beta" else cr.mul(ar, bb, cc)
    return _sum_rows(ar, start, prod, erow, erank)


def _spmv(order, erow, erank, ecol, vals, b, n_rows, ot, alpha, beta, c, at):
    b = np.asarray(b)
    assert b.ndim == 2 and (alpha is None) == (beta is None)
    ot = np.dtype(ot).type
    at = widest(vals.dtype, b.dtype, ot) if at is None else at
    if alpha is not None:
        alpha, beta = vals.dtype.type(alpha), ot(beta)       # their own types, then widened like everything else
        c = np.asarray(c, ot)
    args = (order, erow, erank, ecol, vals, b, n_rows, alpha, beta, c)
    ref = _product(br.hp(at), *args)
    plain = _narrow(_product(br.plain(at), *args), ot)
    ld = np.longdouble
    terms = np.abs(vals).astype(ld)[:, None] * np.abs(b[ecol].reshape(len(ecol), b.shape[1])).astype(ld)
    S = np.zeros((n_rows, b.shape[1]), ld)
    if alpha is not None:
        terms = terms * ld(np.abs(alpha))
        if beta != 0:
            S = ld(np.abs(beta)) * np.abs(c.reshape(n_rows, b.shape[1])).astype(ld)
    np.add.at(S, erow, terms)
    m = np.bincount(erow, minlength=n_rows).astype(np.int64)[:, None] * np.ones((1, b.shape[1]), np.int64)
    return Product(ref, plain, S, m)


def csr_spmv(row_ptrs, col_idxs, vals, b, ot, alpha=None, beta=None, c=None, at=None):
    """c = A b, or alpha A b + beta c; vals, b (n_cols x nrhs) and ot are any of the 16 triples.  `at` overrides
    the arithmetic type (the CPU test adds the cancellation row in the narrow type with it)"""
    ptrs = np.asarray(row_ptrs, np.int64)
    n_rows = len(ptrs) - 1
    lens = np.diff(ptrs)
    erow = np.repeat(np.arange(n_rows), lens)
    erank = np.arange(int(ptrs[-1]) - int(ptrs[0])) - (ptrs[:-1] - ptrs[0])[erow]
    ecol = np.asarray(col_idxs, np.int64)
    return _spmv("c*beta", erow, erank, ecol, np.asarray(vals), b, n_rows, ot, alpha, beta, c, at)


def ell_spmv(n_rows, k, stride, col_idxs, vals, b, ot, alpha=None, beta=None, c=None, at=None):
    """the same for Ell: entry (row, i) at row + i * stride, column -1 = padding (its value is never used)"""
    cols = np.asarray(col_idxs, np.int64)[:k * stride].reshape(k, stride)[:, :n_rows]
    v = np.asarray(vals)[:k * stride].reshape(k, stride)[:, :n_rows]
    stored = cols != -1
    rank = np.cumsum(stored, axis=0) - 1                                     # entries of the row before this one
    i, row = np.nonzero(stored)                                              # slice-major: k order inside a row
    return _spmv("beta*c", row, rank[i, row], cols[i, row], v[i, row], b, n_rows, ot, alpha, beta, c, at)


def bound(p, at, ot):
    """(m + 8) eps(AT) S + eps(OT) |ref| per output entry, long double"""
    return (p.m + 8) * np.longdouble(br.eps_of(at)) * p.S + np.longdouble(br.eps_of(ot)) * np.abs(p.ref)


def row_gather(orig, rows, ot, alpha=None, beta=None, out=None):
    """out(i, :) = orig(rows[i], :) converted, or OT(AT(alpha * orig) + AT(beta) * AT(out)), AT the wider type"""
    orig = np.asarray(orig)
    vt, ot = orig.dtype.type, np.dtype(ot).type
    at = widest(vt, ot)
    src = orig[np.asarray(rows, np.int64)]
    h = br.hp(at)
    if alpha is None:
        return Gather(h.a(src), _narrow(src, ot), None)
    alpha, beta = vt(alpha), vt(beta)
    pv, pa = br.plain(vt), br.plain(at)
    scaled = cr.mul(pv, alpha, src)                                          # in the source type
    kept = cr.mul(pa, pa.wt(beta), pa.a(out))
    plain = _narrow(cr.add(pa, pa.a(scaled), kept), ot)
    first = cr.mul(h, h.wt(alpha), h.a(src)) if vt is at else h.a(scaled)    # (see the module docstring)
    ref = first + cr.mul(h, h.wt(beta), h.a(out))
    ld = np.longdouble
    S = ld(np.abs(alpha)) * np.abs(src).astype(ld) + ld(np.abs(beta)) * np.abs(np.asarray(out)).astype(ld)
    return Gather(ref, plain, S)


def gather_bound(g, at, ot):
    """8 eps(AT) (|alpha||orig| + |beta||out|) + eps(OT) |ref|: two textbook products under 3 eps(AT) each of
    their term, one addition, and the one narrowing"""
    return 8 * np.longdouble(br.eps_of(at)) * g.S + np.longdouble(br.eps_of(ot)) * np.abs(g.ref)


# ------------------------------------------------------------------------------------------ inputs
def values(rng, shape, t, spread=False):
    """uniform in (-1, 1), both parts of a complex type; spread: times 10^k, k = -2 .. 2 per entry"""
    t = np.dtype(t).type
    v = rng.uniform(-1, 1, shape)
    if br.is_complex(t):
        v = v + 1j * rng.uniform(-1, 1, shape)
    if spread:
        v = v * 10.0 ** rng.integers(-2, 3, shape)
    return np.asarray(v).astype(t)


def integers(rng, shape, t):
    """(Gaussian) integers in [-3, 3]: every product and sum of the cases below is exact in float and double"""
    t = np.dtype(t).type
    v = rng.integers(-3, 4, shape).astype(np.float64)
    if br.is_complex(t):
        v = v + 1j * rng.integers(-3, 4, shape)
    return np.asarray(v).astype(t)


def _spread(total, rows):
    """`rows` row lengths that add up to `total`, as even as possible"""
    return [total // rows + (1 if r < total % rows else 0) for r in range(rows)]


def _short(seed, rows):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 7, rows)]


# Csr: the plain kernel gives one wave 64 rows (a "segment") and walks the segment's entries in LDS chunks of
# mixed_chunk = 1024 products.  name -> row lengths
CSR_FAMILIES = collections.OrderedDict([
    ("rows_1", [5]),
    ("rows_63", _short(63, 63)),
    ("rows_64", _short(64, 64)),
    ("rows_65_last_segment_of_one_row", _short(65, 64) + [4]),
    ("rows_129", _short(129, 128) + [3]),
    ("segment_of_1023_entries", _spread(1023, 64) + [2, 0, 3]),
    ("segment_of_1024_entries", _spread(1024, 64) + [2, 0, 3]),
    ("segment_of_1025_entries", _spread(1025, 64) + [2, 0, 3]),
    ("segment_of_2048_entries", _spread(2048, 64) + [2, 0, 3]),
    ("segment_of_2049_entries", _spread(2049, 64) + [2, 0, 3]),
    ("row_ends_on_the_chunk_boundary", [1000, 24, 30, 0, 5]),
    ("row_straddles_the_chunk_boundary", [1000, 50, 30, 0, 5]),
    ("row_of_2500_spans_three_chunks", [10, 2500, 7, 0, 40]),
    ("empty_segment_between_two", [3] * 64 + [0] * 64 + [2] * 64),
    ("empty_first_and_last_rows_of_a_segment", [0] + [3] * 62 + [0, 0] + [2] * 62 + [0]),
    ("cancellation_row", None),
    ("wide_matrix_values_survive", None),
])
# Ell: one lane per row, 256 rows per block.  name -> (n_rows, k, stride - n_rows, padding)
ELL_FAMILIES = collections.OrderedDict([
    ("rows_1", (1, 3, 0, "none")),
    ("rows_255", (255, 4, 0, "tail")),
    ("rows_256", (256, 4, 0, "tail")),
    ("rows_257", (257, 4, 0, "tail")),
    ("k_0", (70, 0, 0, "none")),
    ("stride_larger_than_rows", (70, 3, 9, "tail")),
    ("padding_in_the_middle_of_a_row", (130, 5, 3, "middle")),
    ("padding_in_a_whole_column_slice", (130, 5, 0, "slice")),
    ("cancellation_row", None),
    ("wide_matrix_values_survive", None),
])
CANCEL = [2.0 ** 30, 1.0, -2.0 ** 30]
SURVIVE = [2.0 ** 30 + 1, -2.0 ** 30]        # a wide matrix type holds 2^30 + 1, a narrow one stores 2^30
ONES_B = {"cancellation_row": CANCEL, "wide_matrix_values_survive": SURVIVE}


def _cancel_values(t, name="cancellation_row"):
    v = np.array(ONES_B[name])
    return (v + 1j * v).astype(t) if br.is_complex(t) else v.astype(t)


def cancellation_want(t):
    """[2^30, 1, -2^30] . [1, 1, 1] (complex: the same in both parts of the values, b = 1): exactly 1 when added
    in a wide type, 0 when 2^30 + 1 is rounded to float"""
    return np.dtype(t).type(1 + 1j) if br.is_complex(t) else np.dtype(t).type(1)


def survive_want(mt, ot):
    """[2^30 + 1, -2^30] . [1, 1] with the values stored in mt: 1 if mt is a wide type (the values must reach the
    arithmetic as stored), 0 if the matrix itself is narrow"""
    mt, ot = (np.dtype(dt(t) if isinstance(t, str) else t).type for t in (mt, ot))
    return cancellation_want(ot) if mt in (np.float64, np.complex128) else ot(0)


def csr_case(name, mt, seed=0, exact=False):
    """(n_cols, row_ptrs, col_idxs, vals) int64 / value type mt; sorted, duplicate-free rows"""
    mt = dt(mt) if isinstance(mt, str) else mt
    if name in ONES_B:
        v = _cancel_values(mt, name)
        return 5, np.array([0, len(v)]), np.array([0, 2, 4][:len(v)]), v
    lens = CSR_FAMILIES[name]
    rng = np.random.default_rng([seed, len(lens), sum(lens)])
    n_cols = max(max(lens) + 7, 97)
    cols = [np.sort(rng.choice(n_cols, n, replace=False)) for n in lens]
    ptrs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate(cols + [np.zeros(0, np.int64)]).astype(np.int64)
    vals = integers(rng, len(cols), mt) if exact else values(rng, len(cols), mt, spread=True)
    return n_cols, ptrs, cols, vals


def ell_case(name, mt, seed=0, exact=False):
    """(n_rows, n_cols, k, stride, col_idxs, vals); the values of padding are NaN: they must never be used"""
    mt = dt(mt) if isinstance(mt, str) else mt
    if name in ONES_B:
        v = _cancel_values(mt, name)
        return 1, 5, len(v), 1, np.array([0, 2, 4][:len(v)]), v
    n_rows, k, extra, padding = ELL_FAMILIES[name]
    rng = np.random.default_rng([seed, n_rows, k, extra])
    n_cols, stride = 97, n_rows + extra
    cols = np.full((k, stride), -1, np.int64)
    vals = np.full((k, stride), np.nan, mt)
    for r in range(n_rows):
        keep = np.ones(k, bool)
        if padding == "tail":
            keep = np.arange(k) < (k - r % (k + 1))              # rows of k, k - 1, ... 0 entries
        elif padding == "middle":
            keep[1 + r % (k - 2)] = False
        elif padding == "slice":
            keep[2] = False
            keep[4] = r % 3 != 0
        cols[keep, r] = np.sort(rng.choice(n_cols, int(keep.sum()), replace=False))
    stored = cols != -1
    n = int(stored.sum())
    vals[stored] = integers(rng, n, mt) if exact else values(rng, n, mt, spread=True)
    return n_rows, n_cols, k, stride, cols.reshape(-1), vals.reshape(-1)


KINDS = ("plain", "advanced", "beta_zero_over_nan_c", "alpha_zero", "integers")


class Inputs:
    """one call: fmt, name, triple, nrhs, kind, n_rows, n_cols, vals, cols, b, c, alpha, beta and ptrs (Csr)
    or k, stride (Ell); alpha is None for the plain form"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def reference(self, at=None):
        a = (self.b, dt(self.triple[2]), self.alpha, self.beta, self.c, at)
        if self.fmt == "csr":
            return csr_spmv(self.ptrs, self.cols, self.vals, *a)
        return ell_spmv(self.n_rows, self.k, self.stride, self.cols, self.vals, *a)


def spmv_inputs(fmt, name, triple, nrhs, kind):
    """the inputs of case family `name` for one triple; index arrays are int64, the caller narrows them.
    name: a key of CSR_FAMILIES / ELL_FAMILIES, "n_rows_0" or "n_cols_0_empty_matrix" """
    mt, it, ot = triple
    exact = kind == "integers"
    rng = np.random.default_rng([CODE[mt], CODE[it], CODE[ot], nrhs, KINDS.index(kind)])
    d = dict(fmt=fmt, name=name, triple=triple, nrhs=nrhs, kind=kind)
    if name in ("n_rows_0", "n_cols_0_empty_matrix"):
        n_rows = 0 if name == "n_rows_0" else 5
        n_cols = 9 if name == "n_rows_0" else 0
        d.update(n_rows=n_rows, n_cols=n_cols, vals=np.zeros(0, dt(mt)), cols=np.zeros(0, np.int64),
                 ptrs=np.zeros(n_rows + 1, np.int64), k=0, stride=n_rows)
    elif fmt == "csr":
        n_cols, ptrs, cols, vals = csr_case(name, mt, exact=exact)
        d.update(n_rows=len(ptrs) - 1, n_cols=n_cols, ptrs=ptrs, cols=cols, vals=vals)
    else:
        n_rows, n_cols, k, stride, cols, vals = ell_case(name, mt, exact=exact)
        d.update(n_rows=n_rows, n_cols=n_cols, k=k, stride=stride, cols=cols, vals=vals)
    cancel = name in ONES_B
    b, c = operands(rng, d["n_rows"], d["n_cols"], nrhs, it, ot, exact=exact, ones=cancel)
    alpha = beta = None
    if kind != "plain":
        alpha, beta = scalars(mt, ot, exact)
        if cancel:
            alpha, beta = dt(mt)(1), dt(ot)(0)
        if kind == "beta_zero_over_nan_c":
            beta = dt(ot)(0)
            c[:] = np.nan
        if kind == "alpha_zero":
            alpha = dt(mt)(0)
    d.update(b=b, c=c, alpha=alpha, beta=beta)
    return Inputs(**d)


def kinds_of(name):
    return ("plain", "advanced") if name in ONES_B else KINDS


def operands(rng, n_rows, n_cols, nrhs, it, ot, exact=False, ones=False):
    """b (n_cols x nrhs) and c (n_rows x nrhs)"""
    it, ot = (dt(t) if isinstance(t, str) else t for t in (it, ot))
    if ones:
        return np.ones((n_cols, nrhs), it), values(rng, (n_rows, nrhs), ot)
    make = integers if exact else values
    return make(rng, (n_cols, nrhs), it), make(rng, (n_rows, nrhs), ot)


def scalars(mt, ot, exact=False):
    """alpha in the matrix' type, beta in the output's"""
    mt, ot = (dt(t) if isinstance(t, str) else t for t in (mt, ot))
    a, b = (2 - 1j, -1 + 3j) if exact else (-1.7 + 0.6j, 0.3 - 1.1j)
    return (mt(a) if br.is_complex(mt) else mt(a.real)), (ot(b) if br.is_complex(ot) else ot(b.real))


SPECIAL = [-0.0, 0.0, np.nan, 1e300, -1e300, 3.5e38, 1e-40, -1e-45, 1e-310, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24,
           1 + 2.0 ** -23, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149, np.inf, -np.inf, 16777217.0]


def special_sources(t):
    """-0.0, NaN, values that overflow when narrowed, the float subnormal range, ties; complex: in both parts"""
    s = np.array(SPECIAL)
    if br.is_complex(t):
        z = np.empty(len(s), np.complex128)
        z.real, z.imag = s, np.roll(s, 5)
        s = z
    with np.errstate(over="ignore"):
        return s.astype(t)
