"""numpy restatements of the value-carrying kernels that only the C++ binding calls and that
tests/test_cdense_gpu.py, test_format_helpers_gpu.py and test_array_components_gpu.py reach through the C ABI:
the complex Dense BLAS-1 and conversions, the complex Csr scaling, the complex Coo product, scalar and
block-transpose Jacobi on complex values (ginkgo_amd/csrc/complex_blas.hip, jacobi.hip), ell::copy and the Ell /
Sellp diagonals (coo.hip, conversions.hip), the real Dense helpers and the array components.

Same conventions as tests/binding_refs.py and tests/csr_struct_refs.py, whose machinery this file uses: value
operations take an `Arith`; `hp(T)` = long double is the expected value, `plain(T)` = the value type with every
real operation rounded on its own (complex products as (ac - bd, ad + bc)) is what the kernels promise to match
bit for bit and what sizes rule R.  Copies, gathers and integer kernels have one restatement; their independent
formulations live in tests/test_value_kernel_refs_cpu.py.  Nothing here touches a GPU.

The quotient.  complex_blas.hip divides by Smith's scaled quotient, the operator/ of csrc/complex_type.hpp
(`smith`).  `unscaled_quotient` is the conjugate form a (conj b) / |b|^2 that the file
used before: kept here only so that the CPU test can show that the sweep of `quotient_sweep` rejects it.

Layouts.  Ell: entry k of row r at r + k * stride, padding value 0 / column -1.  Sellp: slice sl holds the rows
sl * slice_size ..., entry i of local row lr at lr + i * slice_size for i in [slice_sets[sl], slice_sets[sl + 1]).
Jacobi blocks: block b starts at group_offset * (b >> group_power) + block_offset * (b & (2^group_power - 1)),
its entry (i, j) is `stride` = block_offset << group_power entries per column apart: start + i + j * stride."""
import numpy as np

import binding_refs as br
import csr_struct_refs as cr


def _is_hp(ar):
    return ar.wt in (np.longdouble, np.clongdouble)


def _pair(ar, re, im):
    out = np.empty(np.broadcast(re, im).shape, ar.wt)
    out.real, out.imag = re, im
    return out


# -------------------------------------------------------------------------------- the quotient
def smith(ar, a, b):
    """a / b for complex a, b.  hp: the long-double quotient.  plain: Smith's scaled quotient as
    csrc/complex_type.hpp writes it, every real operation rounded in the value type"""
    a, b = np.asarray(a, ar.wt), np.asarray(b, ar.wt)
    if _is_hp(ar):
        return np.asarray(a / b, ar.wt)
    are, aim, bre, bim = a.real, a.imag, b.real, b.imag
    big = np.abs(bre) >= np.abs(bim)
    with np.errstate(all="ignore"):
        r = bim / bre
        den = bre + bim * r
        re1, im1 = (are + aim * r) / den, (aim - are * r) / den
        r = bre / bim
        den = bre * r + bim
        re2, im2 = (are * r + aim) / den, (aim * r - are) / den
    return _pair(ar, np.where(big, re1, re2), np.where(big, im1, im2))


def unscaled_quotient(ar, a, b):
    """the conjugate form in the value type: (a conj b) / (b.re^2 + b.im^2)"""
    a, b = np.asarray(a, ar.wt), np.asarray(b, ar.wt)
    with np.errstate(all="ignore"):
        d = b.real * b.real + b.imag * b.imag
        return _pair(ar, (a.real * b.real + a.imag * b.imag) / d, (a.imag * b.real - a.real * b.imag) / d)


SWEEP_EXPONENTS = {"c64": [-120, -80, -70, -40, 0, 40, 62, 70, 100],
                   "c128": [-1000, -600, -530, -300, 0, 300, 505, 540, 900]}


def quotient_sweep(tn):
    """divisors whose moduli sweep the range of the type, both branches of Smith's quotient (|re| >= |im| and
    the opposite) and both signs at every exponent, and numerators of modulus about 1 for each of them.
    c64: 2^-120 .. 2^100 as the issue lists them; c128: the corresponding points - |b|^2 is subnormal at
    2^-530, underflows to 0 at 2^-600, is about to overflow at 2^505 and overflows at 2^540 - and the ends
    2^-1000, 2^900."""
    t = br.TYPES[tn]
    shapes = np.array([0.75 + 0.5j, -0.3125 + 0.9375j, 0.625 - 0.59375j, -1.0 - 0.0625j, 1.0, 1.0j])
    nums = np.array([0.8125 - 0.5625j, -0.4375 + 0.90625j, 1.0, -0.6875 - 0.71875j, 0.59375 + 0.78125j, -1.0j])
    b = np.concatenate([np.ldexp(shapes.real, e) + 1j * np.ldexp(shapes.imag, e) for e in SWEEP_EXPONENTS[tn]])
    a = np.tile(nums, len(SWEEP_EXPONENTS[tn]))
    return a.astype(t), b.astype(t)


def entrywise_check(got, ref, pl, t):
    """rule R entry by entry - every entry has its own scale - wherever the reference is a normal number of
    the type (not within a factor 2 of its ends): got must be finite there.  Returns (ok, index of the first
    failure or -1, largest |got - ref| / (eps |ref|))"""
    fi = np.finfo(br.real_of(t))
    ref, got, pl = (np.asarray(z).reshape(-1) for z in (ref, got, pl))
    mod = np.abs(ref)
    normal = (mod >= np.longdouble(fi.tiny) * 2) & (mod <= np.longdouble(fi.max) / 2)
    worst, bad = 0.0, -1
    for i in np.flatnonzero(normal):
        ok = bool(np.isfinite(got[i].real) and np.isfinite(got[i].imag))
        if ok:
            ok, ratio = br.rule_r(got[i:i + 1], ref[i:i + 1], pl[i:i + 1], t)
            worst = max(worst, ratio)
        if not ok and bad < 0:
            bad = int(i)
    return bad < 0, bad, worst


def quotient_check(got, a, b, t):
    """the acceptance of "The quotient" for got = a / b: finite wherever the long-double quotient is a normal
    number of the type, and within rule R, sized by plain Smith, of it"""
    return entrywise_check(got, smith(br.hp(t), a, b), smith(br.plain(t), a, b), t)


# --------------------------------------------------------------------------- Dense BLAS-1 (complex)
SCALE, INV_SCALE, ADD_SCALED, SUB_SCALED = range(4)


def _times(ar, v, a, real_scalar):
    """v * a: textbook product for a complex scalar, (re a, im a) for a real one"""
    if real_scalar:
        v = np.asarray(v, ar.wt)
        return _pair(ar, v.real * a, v.imag * a)
    return cr.mul(ar, v, a)


def axpy(ar, op, alpha, x, y, real_scalar):
    """dense::scale / inv_scale / add_scaled / sub_scaled on complex y (rows x cols); alpha holds 1 or cols
    scalars (complex, or reals when real_scalar); x is unused by the two scalings"""
    y = ar.a(y)
    a = np.asarray(alpha, ar.rt if real_scalar else ar.wt).reshape(1, -1)
    a = np.broadcast_to(a, (1, y.shape[1])) if a.shape[1] == 1 else a
    a = np.broadcast_to(a, y.shape)
    if op == SCALE:
        return _times(ar, y, a, real_scalar)
    if op == INV_SCALE:
        if real_scalar:
            with np.errstate(all="ignore"):
                return _pair(ar, y.real / a, y.imag / a)
        return smith(ar, y, a)
    ax = _times(ar, ar.a(x), a, real_scalar)
    return cr.add(ar, y, ax) if op == ADD_SCALED else np.asarray(y - ax, ar.wt)


def squared_norm2(ar, x):
    """per column sum_i (re^2 + im^2): reals"""
    x = ar.a(x)
    terms = np.asarray(x.real * x.real + x.imag * x.imag, ar.rt)
    ones = np.ones(terms.shape[0], ar.rt)
    return np.array([np.real(ar.dot(terms[:, j], ones)) for j in range(terms.shape[1])], ar.rt)


def squared_norm2_depth(rows):
    """additions on the longest path of cx_reduce (complex_blas.hip): nb = min(ceil(rows / 2048), 256) blocks of
    256 threads, every thread adds its ceil(rows / (256 nb)) terms in turn, the block adds 256 values in a tree
    (8 levels); the second stage does the same with the nb partial sums"""
    nb = min(-(-rows // 2048), 256)
    return -(-rows // (256 * nb)) + 8 + -(-nb // 256) + 8


def absolute(ar, x):
    """|x| = hypot(re, im)"""
    x = ar.a(x)
    return np.asarray(np.hypot(x.real, x.imag), ar.rt)


def is_nonzero(x):
    """a value is zero if both parts are (-0.0 is zero, NaN is not)"""
    x = np.asarray(x)
    return (x.real != 0) | (x.imag != 0)


def count_nonzeros_per_row(x):
    return np.count_nonzero(is_nonzero(x), axis=1).astype(np.int64)


def dense_to_csr(x):
    """(row_ptrs, cols, values) of the non-zero entries in row-major order, values as stored"""
    x = np.asarray(x)
    nz = is_nonzero(x)
    ptrs = np.concatenate([[0], np.cumsum(np.count_nonzero(nz, axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(nz)
    return ptrs, cols.astype(np.int64), x[rows, cols]


def row_gather(rows, orig):
    out = np.empty((len(rows), orig.shape[1]), orig.dtype)
    for i, r in enumerate(rows):
        out[i] = orig[int(r)]
    return out


def fill_in_matrix_data(rows, cols, vals, out0):
    """out(row, col) = value for triplets with distinct positions; everything else keeps what out held"""
    out = np.array(out0, copy=True)
    for r, c, v in zip(rows, cols, vals):
        out[int(r), int(c)] = v
    return out


def add_scaled_identity_real(ar, alpha, beta, m):
    """m = beta m + alpha I with real scalars on a complex matrix: (re beta, im beta), then re + alpha on the
    first min(rows, cols) diagonal positions"""
    m = ar.a(m)
    out = _pair(ar, m.real * ar.rt(beta), m.imag * ar.rt(beta))
    k = min(m.shape)
    idx = np.arange(k)
    out.real[idx, idx] = out.real[idx, idx] + ar.rt(alpha)
    return out


# ------------------------------------------------------------------------------- Csr / Coo (complex)
def csr_scale_by_diagonal(ar, ptrs, cols, diag, mode, vals):
    """mode 0: vals[k] *= diag[row]; 1: vals[k] *= (1 / diag[row]) - a reciprocal, then a product; 2: vals[k]
    *= diag[col[k]]"""
    ptrs = np.asarray(ptrs, np.int64)
    row_of = np.repeat(np.arange(len(ptrs) - 1), np.diff(ptrs))
    d = ar.a(diag)
    if mode == 1:
        d = smith(ar, np.ones(d.shape, ar.wt), d)
    s = d[np.asarray(cols, np.int64)] if mode == 2 else d[row_of]
    return cr.mul(ar, ar.a(vals), s)


def coo_spmv2(rows, cols, vals, b, c0, alpha=None):
    """c0 + [alpha] A b in long double, and per output entry the number m of entries that land on it and
    S = |c0| + sum_k |alpha| |v_k| |b_k|: any order of m rounded additions of rounded products stays within
    (m + 4) eps S of the exact value (two products of at most eps |x||y| per part each, m additions of eps / 2
    of a partial sum that S bounds, sqrt(2) from the parts to the modulus)"""
    wide = np.clongdouble
    c = np.array(c0, wide)
    S = np.abs(c).astype(np.longdouble)
    m = np.zeros(c.shape, np.int64)
    b = np.asarray(b, wide)
    al = wide(1) if alpha is None else wide(alpha)
    for r, col, v in zip(rows, cols, np.asarray(vals, wide)):
        t = al * (v * b[int(col)])
        c[int(r)] += t
        S[int(r)] += np.abs(al) * np.abs(v) * np.abs(b[int(col)])
        m[int(r)] += 1
    return c, m, S


def coo_spmv2_fast(rows, cols, vals, b, c0, alpha=None):
    """the same with np.add.at (the 20 000-entry cases)"""
    wide = np.clongdouble
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    al = wide(1) if alpha is None else wide(alpha)
    t = al * (np.asarray(vals, wide)[:, None] * np.asarray(b, wide)[cols])
    c = np.array(c0, wide)
    np.add.at(c, rows, t)
    S = np.abs(np.asarray(c0, wide)).astype(np.longdouble)
    np.add.at(S, rows, np.abs(t).astype(np.longdouble))
    m = np.zeros(c.shape, np.int64)
    np.add.at(m, rows, 1)
    return c, m, S


# ------------------------------------------------------------------------------------ Ell / Sellp
def ell_copy(n_rows, k, src_stride, src_cols, src_vals, dst_stride, dst_cols0, dst_vals0):
    """the n_rows x k stored slots move to the other stride; slots of the padding rows n_rows .. dst_stride keep
    what the target held"""
    dc, dv = np.array(dst_cols0, copy=True), np.array(dst_vals0, copy=True)
    for i in range(k):
        dc[i * dst_stride:i * dst_stride + n_rows] = src_cols[i * src_stride:i * src_stride + n_rows]
        dv[i * dst_stride:i * dst_stride + n_rows] = src_vals[i * src_stride:i * src_stride + n_rows]
    return dc, dv


def ell_extract_diagonal(n, ell_k, stride, cols, vals, diag0):
    """diag[r] = the value of the FIRST slot of row r whose column is r, whatever the value (padding is told by
    its column -1, never by its value 0); rows without one keep what diag held"""
    diag = np.array(diag0, copy=True)
    r = np.arange(n)
    for k in reversed(range(ell_k)):                   # the first matching slot is written last
        hit = np.asarray(cols[k * stride:k * stride + n]).astype(np.int64) == r
        diag[hit] = vals[k * stride:k * stride + n][hit]
    return diag


def sellp_extract_diagonal(n, slice_size, slice_sets, cols, vals, diag0):
    diag = np.array(diag0, copy=True)
    for sl in range(len(slice_sets) - 1):
        r = np.arange(sl * slice_size, min((sl + 1) * slice_size, n))
        for i in reversed(range(int(slice_sets[sl]), int(slice_sets[sl + 1]))):
            at = i * slice_size + (r - sl * slice_size)
            hit = np.asarray(cols[at]).astype(np.int64) == r
            diag[r[hit]] = vals[at[hit]]
    return diag


def ell_from_rows(rows_of_entries, stride, ell_k, t, it):
    """Ell arrays (cols, vals) from per-row lists of (col, value); padding value 0, column -1"""
    cols = np.full(stride * ell_k, -1, it)
    vals = np.zeros(stride * ell_k, t)
    for r, ents in enumerate(rows_of_entries):
        for k, (c, v) in enumerate(ents):
            cols[r + k * stride], vals[r + k * stride] = c, v
    return cols, vals


def sellp_from_rows(rows_of_entries, slice_size, t, it):
    """Sellp arrays (slice_sets, cols, vals): every slice as wide as its longest row"""
    n = len(rows_of_entries)
    n_slices = -(-n // slice_size)
    widths = [max([len(e) for e in rows_of_entries[s * slice_size:(s + 1) * slice_size]] + [0])
              for s in range(n_slices)]
    sets = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint64)
    total = int(sets[-1]) * slice_size
    cols, vals = np.full(total, -1, it), np.zeros(total, t)
    for r, ents in enumerate(rows_of_entries):
        sl, lr = divmod(r, slice_size)
        for k, (c, v) in enumerate(ents):
            pos = lr + (int(sets[sl]) + k) * slice_size
            cols[pos], vals[pos] = c, v
    return sets, cols, vals


def ell_from_table(C, V, stride, it):
    """Ell arrays from an n x k table of columns (-1 = padding) and values"""
    n, k = C.shape
    cols, vals = np.full(stride * k, -1, it), np.zeros(stride * k, V.dtype)
    for j in range(k):
        cols[j * stride:j * stride + n] = C[:, j]
        vals[j * stride:j * stride + n] = np.where(C[:, j] >= 0, V[:, j], 0)
    return cols, vals


def sellp_from_table(C, V, slice_size, it):
    """Sellp arrays (slice_sets, cols, vals) from the same table; a row's entries are its leading slots, every
    slice is as wide as its longest row"""
    n, k = C.shape
    n_slices = -(-n // slice_size)
    length = np.count_nonzero(C >= 0, axis=1)
    padded_len = np.zeros(n_slices * slice_size, np.int64)
    padded_len[:n] = length
    widths = padded_len.reshape(n_slices, slice_size).max(axis=1) if n_slices else np.zeros(0, np.int64)
    sets = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint64)
    total = int(sets[-1]) * slice_size
    cols, vals = np.full(total, -1, it), np.zeros(total, V.dtype)
    r = np.arange(n)
    sl, lr = r // slice_size, r % slice_size
    for j in range(k):
        has = j < length
        pos = lr[has] + (sets[sl[has]].astype(np.int64) + j) * slice_size
        cols[pos], vals[pos] = C[has, j], V[has, j]
    return sets, cols, vals


# ------------------------------------------------------------------------------------------ Jacobi
def invert_diagonal(ar, d):
    """1 / d with Smith's quotient; an entry that is zero (both parts, either sign) inverts as one"""
    d = ar.a(d).copy()
    d[~is_nonzero(d)] = 1
    return smith(ar, np.ones(d.shape, ar.wt), d)


def scalar_apply(ar, diag, b, alpha=None, beta=None, x0=None):
    """x = b diag[row], or beta x + (alpha b) diag[row]"""
    d = ar.a(diag).reshape(-1, 1)
    if alpha is None:
        return cr.mul(ar, ar.a(b), d)
    return cr.add(ar, cr.mul(ar, ar.wt(beta), ar.a(x0)), cr.mul(ar, cr.mul(ar, ar.wt(alpha), ar.a(b)), d))


def block_start(scheme, b):
    bo, go, gp = int(scheme.block_offset), int(scheme.group_offset), int(scheme.group_power)
    return go * (b >> gp) + bo * (b & ((1 << gp) - 1))


def block_storage_size(scheme, num_blocks):
    """entries of the block storage: whole groups (compute_storage_space)"""
    gp = int(scheme.group_power)
    return int(scheme.group_offset) * (-(-num_blocks // (1 << gp)))


def jacobi_transpose(scheme, block_ptrs, blocks, conj, out0):
    """every block transposed (conjugated with conj) into the same place of out; storage between the blocks
    keeps what out held"""
    out = np.array(out0, copy=True)
    stride = int(scheme.block_offset) << int(scheme.group_power)
    for b in range(len(block_ptrs) - 1):
        bs = int(block_ptrs[b + 1] - block_ptrs[b])
        base = block_start(scheme, b)
        i, j = np.meshgrid(np.arange(bs), np.arange(bs), indexing="ij")
        v = blocks[base + j + i * stride]                  # in(j, i)
        out[base + i + j * stride] = conj_array(v) if conj else v
    return out


def jacobi_blocks_dense(scheme, block_ptrs, blocks):
    """the blocks as a list of dense matrices (the independent view of the CPU test)"""
    stride = int(scheme.block_offset) << int(scheme.group_power)
    res = []
    for b in range(len(block_ptrs) - 1):
        bs = int(block_ptrs[b + 1] - block_ptrs[b])
        base = block_start(scheme, b)
        res.append(np.array([[blocks[base + i + j * stride] for j in range(bs)] for i in range(bs)],
                            blocks.dtype).reshape(bs, bs))
    return res


def initialize_precisions(source, n):
    source = np.asarray(source, np.uint8)
    return source[np.arange(n) % len(source)] if n else np.zeros(0, np.uint8)


# -------------------------------------------------------------------------------- array components
def conj_array(x):
    """the sign bit of the imaginary part flipped, the real part untouched - also for 0 and NaN"""
    x = np.ascontiguousarray(x)
    rt = br.real_of(x.dtype)
    parts = x.view(rt).copy().reshape(-1, 2)
    bits = parts.view(np.uint32 if rt == np.float32 else np.uint64)
    bits[:, 1] ^= bits.dtype.type(1) << bits.dtype.type(bits.dtype.itemsize * 8 - 1)
    return parts.reshape(-1).view(x.dtype).reshape(x.shape)


def random_bits(rng, n, t):
    """n values of type t from random bit patterns: NaNs with payloads, infinities, subnormals, -0.0"""
    t = np.dtype(t)
    raw = rng.integers(0, 256, n * t.itemsize, dtype=np.uint8).view(t).copy()
    if n > 4 and t.kind in "fc":
        raw[1], raw[2] = -0.0, np.inf
        raw[3] = np.nan
    return raw


def edge_reals(rt):
    """values of the real type rt at the edges a conversion or a modulus can trip on"""
    fi = np.finfo(rt)
    return np.array([0.0, -0.0, 1.0, -1.5, fi.tiny, -fi.tiny, fi.smallest_subnormal, fi.tiny / 8, fi.max, -fi.max,
                     fi.max / 2, np.sqrt(fi.max) * 1.5, np.sqrt(fi.tiny) / 3, fi.eps, 1 + fi.eps, np.inf, -np.inf,
                     np.nan], rt)
