"""numpy restatements of the kernels around Csr that only the C++ binding calls: csr::spgemm_reuse /
advanced_spgemm_reuse / spgeam_numeric, the index-set sub-matrix pair, build_lookup_offsets / build_lookup,
row_wise_absolute_sum and the diagonal scan, matrix::Diagonal and the SparsityCsr pair.  Same conventions as
tests/binding_refs.py: value operations take an `Arith` (`hp(T)` = long double, the expected value;
`plain(T)` = the value type with every operation rounded on its own, the restatement the kernels promise to
match bit for bit and that sizes rule R).  A Csr matrix is a tuple (row_ptrs, col_idxs, values) of numpy
arrays, a pattern the first two.  Nothing here touches a GPU; tests/test_csr_struct_refs_cpu.py checks these
functions against independent formulations.

SpGEMM reuse (ginkgo_amd/csrc/misc.hip): a row of C starts from 0; the products a_ik b_kj are added in the
storage order of A's row, then of B's row ((alpha a) b in the advanced form), then beta d in the storage
order of D's row.  A column that C's pattern does not hold is dropped.  SpGEAM numeric merges the sorted rows
of A and B: alpha a + beta b with a zero operand where one of them has no entry; slots of C's row beyond the
merged row are left alone.

Index sets (ginkgo_amd/csrc/conversions.hip, csr_index_set_kernel, and include/gko_cdna4.h).  A
gko::index_set is a sorted list of disjoint half-open ranges ("subsets") of [0, size).  The entry points take
    n_result_rows  the number of rows of the row index set (sum of its subset lengths)
    n_row_subsets, row_begin[j], row_superset[j]
                   subset j holds the matrix rows row_begin[j] ..., its first result row is row_superset[j]
                   (exclusive sums of the subset lengths: index_set::get_superset_indices(), n + 1 entries)
    n_col_subsets, col_begin[b], col_end[b], col_superset[b]
                   an entry with column c in [col_begin[b], col_end[b]) is kept and gets the column
                   col_superset[b] + (c - col_begin[b]); the count does not take col_superset
    col_set_size   index_set::get_size(), the bound of the index space ("the columns of the column index
                   set"): an entry with column >= col_set_size is dropped before any subset is searched
    in_rp / in_ci / in_v   the source matrix;  counts: n_result_rows entries
    out_rp         exclusive sums of counts (the caller scans);  out_ci / out_v: the kept entries in the
                   source row's storage order, values copied.

Lookup tables (ginkgo_amd/csrc/csr_lookup.hip:1-17): per row a 64-bit descriptor and int32 storage,
    full   (1): the row holds every column of [min_col, min_col + len); descriptor 1, no storage
    bitmap (2): blocks = ceil(range / 32); descriptor blocks << 32 | 2; storage = blocks ranks (entries in
                front of each block) then blocks 32-bit masks
    hash   (4): slots = max(2 len, 1); p = 1 | floor(slots * 0.61803398875); descriptor p << 32 | 4;
                storage = slots entries, -1 or the entry number, filled by linear probing from
                (col * p) mod 2^bits(index type) mod slots in row order
    none   (0): no storage.
`allowed` is the bit set of kinds the caller accepts.  A row is full if that is allowed and len == range;
else bitmap if allowed and 2 blocks <= slots; else hash if allowed; else none with no storage.

Diagonal (misc.hip:28-87): apply_to_dense c(r, j) = b(r, j) * diag[r], with `inverse` b(r, j) * (T(1) /
diag[r]) - a reciprocal and a product, not a quotient; right_apply_to_dense c(r, j) = b(r, j) * diag[j];
apply_to_csr / right_apply_to_csr the same on the values of a Csr in place (row ptrs, or the column of every
entry); convert_to_csr: row_ptrs = 0 .. n, cols = 0 .. n - 1, values = diag; fill_in_matrix_data:
diag[r] = value of every triplet with row == col (unique per position here).  The complex reciprocal is
Smith's quotient of complex_type.hpp.  SparsityCsr (misc.hip:89-119): counts[r] = number of entries of row r
with column r, counts[n_rows] = 0; remove: adj_ptrs[r] = row_ptrs[r] - prefix[r] and the row without its
diagonal entries, order kept."""
import numpy as np

import binding_refs as br

FULL, BITMAP, HASH = 1, 2, 4
BLOCK = 32


# ------------------------------------------------------------------------------ value arithmetic
def _is_hp(ar):
    return ar.wt in (np.longdouble, np.clongdouble)


def mul(ar, x, y):
    """x * y element-wise in ar; complex value types: the textbook product, each real operation rounded"""
    x, y = np.asarray(x, ar.wt), np.asarray(y, ar.wt)
    if np.iscomplexobj(x) and not _is_hp(ar):
        out = np.empty(np.broadcast(x, y).shape, ar.wt)
        out.real = x.real * y.real - x.imag * y.imag
        out.imag = x.real * y.imag + x.imag * y.real
        return out
    return np.asarray(x * y, ar.wt)


def add(ar, x, y):
    return np.asarray(np.asarray(x, ar.wt) + np.asarray(y, ar.wt), ar.wt)


def reciprocal(ar, d):
    """T(1) / d; complex value types: Smith's quotient with the numerator (1, 0)"""
    d = np.asarray(d, ar.wt)
    if not np.iscomplexobj(d) or _is_hp(ar):
        return np.asarray(ar.wt(1) / d, ar.wt)
    rt = ar.rt
    are, aim = rt(1), rt(0)
    bre, bim = d.real, d.imag
    out = np.empty(d.shape, ar.wt)
    big = np.abs(bre) >= np.abs(bim)
    with np.errstate(all="ignore"):
        r = bim / bre
        den = bre + bim * r
        re1, im1 = (are + aim * r) / den, (aim - are * r) / den
        r = bre / bim
        den = bre * r + bim
        re2, im2 = (are * r + aim) / den, (aim * r - are) / den
    out.real, out.imag = np.where(big, re1, re2), np.where(big, im1, im2)
    return out


# ------------------------------------------------------------------------------ SpGEMM / SpGEAM
def _find(c_cols_row, cols):
    """position of each of `cols` in the sorted, duplicate-free row c_cols_row, -1 where absent"""
    cols = np.asarray(cols, np.int64)
    row = np.asarray(c_cols_row, np.int64)
    if row.size == 0:
        return np.full(cols.shape, -1, np.int64)
    pos = np.searchsorted(row, cols)
    ok = (pos < row.size) & (row[np.minimum(pos, row.size - 1)] == cols)
    return np.where(ok, pos, -1)


def spgemm_reuse(ar, A, B, C_pattern, alpha=None, beta=None, D=None):
    """values of C = A B (alpha is None) or alpha A B + beta D on the pattern C_pattern = (c_ptrs, c_cols)"""
    ap, ac, av = A
    bp, bc, bv = B
    cp, cc = C_pattern
    av, bv = ar.a(av), ar.a(bv)
    adv = alpha is not None
    out = np.zeros(len(cc), ar.wt)
    if adv:
        dp, dc, dv = D
        sa = mul(ar, ar.wt(alpha), av)                    # (alpha a), then * b
        bd = mul(ar, ar.wt(beta), ar.a(dv))
    else:
        sa = av
    for row in range(len(cp) - 1):
        cb, ce = int(cp[row]), int(cp[row + 1])
        crow = cc[cb:ce]
        for an in range(int(ap[row]), int(ap[row + 1])):
            k = int(ac[an])
            b0, b1 = int(bp[k]), int(bp[k + 1])
            pos = _find(crow, bc[b0:b1])                  # a row of B holds every column once
            keep = pos >= 0
            at = cb + pos[keep]
            out[at] = add(ar, out[at], mul(ar, sa[an], bv[b0:b1][keep]))
        if adv:
            d0, d1 = int(dp[row]), int(dp[row + 1])
            pos = _find(crow, dc[d0:d1])
            keep = pos >= 0
            at = cb + pos[keep]
            out[at] = add(ar, out[at], bd[d0:d1][keep])
    return out


def spgeam_numeric(ar, alpha, A, beta, B, c_ptrs, c0=None):
    """values of alpha A + beta B, rows merged by column; c0: what the value array held before (slots of a
    row of C beyond the merged row keep it)"""
    ap, ac, av = A
    bp, bc, bv = B
    av, bv = ar.a(av), ar.a(bv)
    out = np.zeros(int(c_ptrs[-1]), ar.wt) if c0 is None else ar.a(c0).copy()
    va, vb = ar.wt(alpha), ar.wt(beta)
    for row in range(len(c_ptrs) - 1):
        a0, a1, b0, b1 = int(ap[row]), int(ap[row + 1]), int(bp[row]), int(bp[row + 1])
        union = np.union1d(ac[a0:a1], bc[b0:b1])
        n = min(union.size, int(c_ptrs[row + 1]) - int(c_ptrs[row]))
        union = union[:n]
        x, y = np.zeros(n, ar.wt), np.zeros(n, ar.wt)
        pa, pb = _find(union, ac[a0:a1]), _find(union, bc[b0:b1])
        x[pa[pa >= 0]] = av[a0:a1][pa >= 0]
        y[pb[pb >= 0]] = bv[b0:b1][pb >= 0]
        o = int(c_ptrs[row])
        out[o:o + n] = add(ar, mul(ar, va, x), mul(ar, vb, y))
    return out


def product_pattern(A_pattern, B_pattern, D_pattern=None):
    """the pattern of A B (+ D): union of the contributing columns per row, ascending"""
    ap, ac = A_pattern
    bp, bc = B_pattern
    ptrs, cols = [0], []
    for row in range(len(ap) - 1):
        s = set()
        for an in range(int(ap[row]), int(ap[row + 1])):
            k = int(ac[an])
            s.update(int(c) for c in bc[int(bp[k]):int(bp[k + 1])])
        if D_pattern is not None:
            s.update(int(c) for c in D_pattern[1][int(D_pattern[0][row]):int(D_pattern[0][row + 1])])
        cols.extend(sorted(s))
        ptrs.append(len(cols))
    return np.array(ptrs, np.int64), np.array(cols, np.int64)


def every_other(pattern):
    """a strict subset of a pattern: every second entry of each row"""
    ptrs, cols = pattern
    rows = [cols[int(ptrs[r]):int(ptrs[r + 1])][::2] for r in range(len(ptrs) - 1)]
    return (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
            np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64))


# ------------------------------------------------------------------------------------ index sets
class IndexSet:
    """gko::index_set from sorted, disjoint half-open ranges of [0, size)"""

    def __init__(self, ranges, size):
        self.begin = np.array([b for b, _ in ranges], np.int64)
        self.end = np.array([e for _, e in ranges], np.int64)
        assert np.all(self.begin < self.end) and np.all(self.end[:-1] <= self.begin[1:])
        assert len(ranges) == 0 or (self.begin[0] >= 0 and self.end[-1] <= size)
        self.superset = np.concatenate([[0], np.cumsum(self.end - self.begin)]).astype(np.int64)
        self.num_elems, self.size, self.num_subsets = int(self.superset[-1]), int(size), len(ranges)

    def rows(self):
        """the elements in result order"""
        return [i for b, e in zip(self.begin, self.end) for i in range(int(b), int(e))]

    def local(self, c):
        """index of c inside the set, None if it is not an element"""
        if c >= self.size:
            return None
        for j in range(self.num_subsets):
            if self.begin[j] <= c < self.end[j]:
                return int(self.superset[j] + c - self.begin[j])
        return None


def index_set_count(row_set, col_set, A_pattern):
    ptrs, cols = A_pattern
    return np.array([sum(col_set.local(int(c)) is not None for c in cols[int(ptrs[r]):int(ptrs[r + 1])])
                     for r in row_set.rows()], np.int64)


def index_set_fill(row_set, col_set, A):
    """(cols, vals) of the sub-matrix, rows back to back in the source rows' storage order"""
    ptrs, cols, vals = A
    oc, ov = [], []
    for r in row_set.rows():
        for k in range(int(ptrs[r]), int(ptrs[r + 1])):
            loc = col_set.local(int(cols[k]))
            if loc is not None:
                oc.append(loc)
                ov.append(vals[k])
    return np.array(oc, np.int64), np.array(ov, np.asarray(vals).dtype)


# ---------------------------------------------------------------------------------------- lookup
def _row_shape(ptrs, cols, row):
    begin = int(ptrs[row])
    n = int(ptrs[row + 1]) - begin
    min_col = int(cols[begin]) if n else 0
    rng = int(cols[begin + n - 1]) - min_col + 1 if n else 0
    return begin, n, min_col, rng


def _row_kind(n, rng, allowed):
    """(kind, storage) of a row of n entries spanning rng columns"""
    if (allowed & FULL) and n == rng:
        return FULL, 0
    slots = max(2 * n, 1)
    words = 2 * ((rng + BLOCK - 1) // BLOCK)
    if (allowed & BITMAP) and words <= slots:
        return BITMAP, words
    if allowed & HASH:
        return HASH, slots
    return 0, 0


def lookup_offsets(ptrs, cols, allowed, it):
    sizes = [_row_kind(*_row_shape(ptrs, cols, r)[1::2], allowed)[1] for r in range(len(ptrs) - 1)]
    return np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(it)


def lookup_build(ptrs, cols, allowed, offsets, it):
    """(row_desc int64[n], storage int32[offsets[n]], written[n]): written = the number of storage words the
    construction of each row stored"""
    n_rows = len(ptrs) - 1
    bits = np.dtype(it).itemsize * 8
    desc = np.zeros(n_rows, np.int64)
    storage = np.full(int(offsets[n_rows]), -12345, np.int32)
    written = np.zeros(n_rows, np.int64)
    for row in range(n_rows):
        begin, n, min_col, rng = _row_shape(ptrs, cols, row)
        kind, _ = _row_kind(n, rng, allowed)
        o = int(offsets[row])
        c = [int(v) for v in cols[begin:begin + n]]
        desc[row] = kind
        if kind == BITMAP:
            blocks = (rng + BLOCK - 1) // BLOCK
            desc[row] = (blocks << 32) | BITMAP
            masks = [0] * blocks
            for v in c:
                masks[(v - min_col) // BLOCK] |= 1 << ((v - min_col) % BLOCK)
            seen = 0
            for b in range(blocks):
                storage[o + b] = seen
                storage[o + blocks + b] = np.uint32(masks[b]).astype(np.int32)
                seen += bin(masks[b]).count("1")
            written[row] = 2 * blocks
        elif kind == HASH:
            slots = max(2 * n, 1)
            p = 1 | int(slots * 0.61803398875)
            desc[row] = (p << 32) | HASH
            table = [-1] * slots
            for k, v in enumerate(c):
                h = ((v * p) % (1 << bits)) % slots
                while table[h] != -1:
                    h = h + 1 if h + 1 < slots else 0
                table[h] = k
            storage[o:o + slots] = table
            written[row] = slots
    return desc, storage, written


def lookup_position(desc, storage_slice, row_cols, col, bits=32):
    """the position of `col` in the row as a consumer of the table finds it, -1 if it is absent.
    desc: the row's descriptor, storage_slice: its piece of the storage, row_cols: the row's columns"""
    desc, col = int(desc), int(col)
    kind, n = desc & 0xffffffff, len(row_cols)
    if kind == 0:                                   # no table: the consumer searches the row
        hit = [k for k in range(n) if int(row_cols[k]) == col]
        return hit[0] if hit else -1
    if n == 0:
        return -1
    rel = col - int(row_cols[0])
    if kind == FULL:
        return rel if 0 <= rel < n else -1
    if kind == BITMAP:
        blocks = desc >> 32
        block, bit = rel // BLOCK, rel % BLOCK
        if rel < 0 or block >= blocks:
            return -1
        mask = int(np.int32(storage_slice[blocks + block]).astype(np.uint32))
        if not (mask >> bit) & 1:
            return -1
        return int(storage_slice[block]) + bin(mask & ((1 << bit) - 1)).count("1")
    assert kind == HASH
    p, slots = desc >> 32, len(storage_slice)
    h = (((col % (1 << bits)) * p) % (1 << bits)) % slots
    for _ in range(slots):
        k = int(storage_slice[h])
        if k == -1:
            return -1
        if int(row_cols[k]) == col:
            return k
        h = h + 1 if h + 1 < slots else 0
    raise AssertionError("hash table without a free slot")


# ------------------------------------------------------------------------- row sums and diagonal
def row_abs_sum(ar, ptrs, vals):
    """sum_k |a_k| per row, left to right (complex: the modulus)"""
    mag = np.abs(ar.a(vals)).astype(ar.rt)
    out = np.zeros(len(ptrs) - 1, ar.rt)
    for r in range(len(ptrs) - 1):
        seg = mag[int(ptrs[r]):int(ptrs[r + 1])]
        if seg.size:
            out[r] = np.cumsum(seg, dtype=ar.rt)[-1] if not _is_hp(ar) else np.sum(seg)
    return out


def extract_diagonal(ptrs, cols, vals, out0):
    """out[r] = the first entry of row r with column r; rows without one keep out0[r]"""
    out = np.array(out0).copy()
    for r in range(len(ptrs) - 1):
        for k in range(int(ptrs[r]), int(ptrs[r + 1])):
            if int(cols[k]) == r:
                out[r] = vals[k]
                break
    return out


# ------------------------------------------------------------------------------------- Diagonal
def diag_apply_dense(ar, diag, b, inverse=False):
    d = ar.a(diag)
    return mul(ar, ar.a(b), (reciprocal(ar, d) if inverse else d)[:, None])


def diag_right_apply_dense(ar, diag, b):
    return mul(ar, ar.a(b), ar.a(diag)[None, :])


def diag_apply_csr(ar, diag, ptrs, vals, inverse=False):
    d = ar.a(diag)
    scal = reciprocal(ar, d) if inverse else d
    rows = np.repeat(np.arange(len(ptrs) - 1), np.diff(np.asarray(ptrs, np.int64)))
    return mul(ar, ar.a(vals), scal[rows])


def diag_right_apply_csr(ar, diag, cols, vals):
    return mul(ar, ar.a(vals), ar.a(diag)[np.asarray(cols, np.int64)])


def diag_to_csr(diag, it):
    n = len(diag)
    return np.arange(n + 1, dtype=it), np.arange(n, dtype=it), np.array(diag).copy()


def diag_fill(rows, cols, vals, diag0):
    out = np.array(diag0).copy()
    for r, c, v in zip(rows, cols, vals):
        if r == c:
            out[int(r)] = v
    return out


# ---------------------------------------------------------------------------------- SparsityCsr
def count_diagonal(ptrs, cols):
    n = len(ptrs) - 1
    return np.array([sum(int(c) == r for c in cols[int(ptrs[r]):int(ptrs[r + 1])]) for r in range(n)] + [0],
                    np.int64)


def remove_diagonal(ptrs, cols, prefix):
    n = len(ptrs) - 1
    adj_ptrs = np.asarray(ptrs, np.int64) - np.asarray(prefix, np.int64)
    idxs = [int(c) for r in range(n) for c in cols[int(ptrs[r]):int(ptrs[r + 1])] if int(c) != r]
    return adj_ptrs, np.array(idxs, np.int64)


# ---------------------------------------------------------------------------------- test matrices
def random_pattern(rng, rows, cols, density, empty_rows=()):
    """sorted, duplicate-free random rows; (ptrs, cols) int64"""
    ptrs, idx = [0], []
    for r in range(rows):
        if r not in empty_rows:
            idx.extend(np.flatnonzero(rng.random(cols) < density).tolist())
        ptrs.append(len(idx))
    return np.array(ptrs, np.int64), np.array(idx, np.int64)


def random_values(rng, n, t):
    v = rng.uniform(-1, 1, n)
    return (v + 1j * rng.uniform(-1, 1, n)).astype(t) if br.is_complex(t) else v.astype(t)


def to_dense(M, shape, wt):
    ptrs, cols, vals = M
    out = np.zeros(shape, wt)
    for r in range(shape[0]):
        for k in range(int(ptrs[r]), int(ptrs[r + 1])):
            out[r, int(cols[k])] += wt(vals[k])
    return out


def stencil7(grid):
    """7-point stencil on grid^3 points, sorted rows; (ptrs, cols, float64 values)"""
    n = grid ** 3
    ptrs, cols, vals = [0], [], []
    for i in range(n):
        x, y, z = i % grid, (i // grid) % grid, i // (grid * grid)
        ent = [(i, 6.0)]
        for ok, j in ((x > 0, i - 1), (x < grid - 1, i + 1), (y > 0, i - grid), (y < grid - 1, i + grid),
                      (z > 0, i - grid * grid), (z < grid - 1, i + grid * grid)):
            if ok:
                ent.append((j, -1.0))
        ent.sort()
        cols.extend(c for c, _ in ent)
        vals.extend(v for _, v in ent)
        ptrs.append(len(cols))
    return np.array(ptrs, np.int64), np.array(cols, np.int64), np.array(vals, np.float64)
