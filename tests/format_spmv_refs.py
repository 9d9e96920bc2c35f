"""numpy restatements of the ELL and SELL-P products (ginkgo_amd/csrc/formats.hip for float / double,
complex_formats.hip for the complex types) and of the set-up kernels that build the two formats:
compute_max_row_nnz, sellp compute_slice_sets, convert_ptrs_to_sizes, convert_idxs_to_ptrs,
csr convert_to_ell / convert_to_sellp.  Same conventions as tests/binding_refs.py: `hp(T)` is the long-double
expected value, `plain(T)` the restatement in the value type with every operation rounded on its own - the
bits the real kernels promise, and what sizes rule R for the complex ones.  Nothing here touches a GPU;
tests/test_format_spmv_refs_cpu.py checks these functions against independent formulations.

Layouts (include/gko_cdna4.h, "ELL SpMV" / "SELL-P SpMV"):
    ELL      slot j of row r at r + j * stride, k slots per row, stride >= n_rows
    SELL-P   slot j of row r of slice s = r // slice_size at (slice_sets[s] + j) * slice_size + r % slice_size,
             slice_lengths[s] slots per row of the slice (the longest row rounded up to stride_factor),
             slice_sets the exclusive sums of slice_lengths (n_slices + 1 entries, uint64)
A slot counts by its column alone: column -1 is padding, wherever it sits and whatever value it carries.

Order of the operations.  Real types: s = beta * c if beta != 0 else 0; then s += (alpha * v) * x slot by
slot (v * x in the plain form).  Complex types: sum += v * x slot by slot with the textbook product, then
alpha * sum, then + beta * c unless beta == 0.  beta == 0 never reads c.

The builders take a matrix as a list of rows, each a list of (column, value) slots."""
import numpy as np

import binding_refs as br
from csr_struct_refs import add, mul

PAD = -1


# ------------------------------------------------------------------------------------------ builders
def ell_build(rows, k, stride, vt, it):
    """(cols, vals) of k * stride entries; slots a row does not give, and rows n_rows .. stride, are (-1, +0)"""
    n = len(rows)
    assert stride >= n and all(len(r) <= k for r in rows)
    cols, vals = np.full(k * stride, PAD, it), np.zeros(k * stride, vt)
    for r, slots in enumerate(rows):
        for j, (c, v) in enumerate(slots):
            cols[r + j * stride], vals[r + j * stride] = c, v
    return cols, vals


def _ceil_to(v, f):
    return (v + f - 1) // f * f


def sellp_build(rows, slice_size, stride_factor, vt, it):
    """(slice_sets, slice_lengths, cols, vals); a slice is as long as its longest row (padding slots inside a
    row count), rounded up to stride_factor"""
    n = len(rows)
    ns = (n + slice_size - 1) // slice_size
    lens = np.zeros(ns, np.uint64)
    for s in range(ns):
        lens[s] = max(_ceil_to(len(r), stride_factor) for r in rows[s * slice_size:(s + 1) * slice_size])
    sets = np.zeros(ns + 1, np.uint64)
    sets[1:] = np.cumsum(lens)
    total = int(sets[-1]) * slice_size
    cols, vals = np.full(total, PAD, it), np.zeros(total, vt)
    for r, slots in enumerate(rows):
        s, l = divmod(r, slice_size)
        for j, (c, v) in enumerate(slots):
            at = (int(sets[s]) + j) * slice_size + l
            cols[at], vals[at] = c, v
    return sets, lens, cols, vals


def ell_slots(n_rows, k, stride, cols, vals):
    """the stored slots as n_rows x k arrays (columns, values)"""
    return (np.asarray(cols).reshape(k, stride)[:, :n_rows].T.copy(),
            np.asarray(vals).reshape(k, stride)[:, :n_rows].T.copy())


def sellp_slots(n_rows, slice_size, sets, lens, cols, vals):
    """the stored slots as n_rows x max(slice_lengths) arrays; slots past a slice's length are (-1, 0)"""
    width = int(lens.max()) if len(lens) else 0
    cm, vm = np.full((n_rows, width), PAD, np.asarray(cols).dtype), np.zeros((n_rows, width), np.asarray(vals).dtype)
    for s in range(len(lens)):
        r0, r1 = s * slice_size, min((s + 1) * slice_size, n_rows)
        ln, at = int(lens[s]), int(sets[s]) * slice_size
        cm[r0:r1, :ln] = cols[at:at + ln * slice_size].reshape(ln, slice_size)[:, :r1 - r0].T
        vm[r0:r1, :ln] = vals[at:at + ln * slice_size].reshape(ln, slice_size)[:, :r1 - r0].T
    return cm, vm


def dense_of(rows, n_cols, wt):
    """the matrix the slots describe (equal columns add up)"""
    out = np.zeros((len(rows), n_cols), wt)
    for r, slots in enumerate(rows):
        for c, v in slots:
            if c >= 0:
                out[r, c] += wt(v)
    return out


def rows_of_dense(d):
    """the non-zero entries of every row of a dense matrix, columns ascending"""
    return [[(int(c), d[r, c]) for c in np.flatnonzero(d[r])] for r in range(d.shape[0])]


# ------------------------------------------------------------------------------------------ products
def _slot_product(ar, t, cm, vm, b, alpha, beta, c):
    cx = br.is_complex(t)
    tt = np.dtype(t).type
    b, vm = ar.a(b), ar.a(vm)
    n, nrhs = cm.shape[0], b.shape[1]
    adv = alpha is not None
    if adv:
        alpha, beta = ar.wt(tt(alpha)), ar.wt(tt(beta))        # rounded to the value type first
    with np.errstate(all="ignore"):
        s = np.zeros((n, nrhs), ar.wt)
        if adv and not cx:
            if beta != 0:
                s = mul(ar, beta, ar.a(c))
            vm = mul(ar, alpha, vm)
        for j in range(cm.shape[1]):
            live = cm[:, j] >= 0
            x = b[np.where(live, cm[:, j], 0)] if b.shape[0] else np.zeros((n, nrhs), ar.wt)
            s = np.where(live[:, None], add(ar, s, mul(ar, vm[:, j:j + 1], x)), s)
        if adv and cx:
            ax = mul(ar, alpha, s)
            s = ax if beta == 0 else add(ar, ax, mul(ar, beta, ar.a(c)))
    return np.asarray(s, ar.wt)


def ell_product(t, n_rows, k, stride, cols, vals, b, alpha=None, beta=None, c=None):
    """(long-double expected value, plain restatement in t) of c = A b or alpha A b + beta c; b, c tight 2-d"""
    cm, vm = ell_slots(n_rows, k, stride, cols, vals)
    return tuple(_slot_product(ar, t, cm, vm, b, alpha, beta, c) for ar in (br.hp(t), br.plain(t)))


def sellp_product(t, n_rows, slice_size, sets, lens, cols, vals, b, alpha=None, beta=None, c=None):
    cm, vm = sellp_slots(n_rows, slice_size, sets, lens, cols, vals)
    return tuple(_slot_product(ar, t, cm, vm, b, alpha, beta, c) for ar in (br.hp(t), br.plain(t)))


# ------------------------------------------------------------------------------------------ set-up
def compute_max_row_nnz(row_ptrs):
    best = 0
    for r in range(len(row_ptrs) - 1):
        best = max(best, int(row_ptrs[r + 1]) - int(row_ptrs[r]))
    return best


def sellp_compute_slice_sets(row_ptrs, slice_size, stride_factor):
    """(slice_sets, slice_lengths), uint64; no rows: slice_sets = [0]"""
    n = len(row_ptrs) - 1
    ns = (n + slice_size - 1) // slice_size
    sets, lens = np.zeros(ns + 1, np.uint64), np.zeros(ns, np.uint64)
    for s in range(ns):
        longest = 0
        for r in range(s * slice_size, min((s + 1) * slice_size, n)):
            longest = max(longest, _ceil_to(int(row_ptrs[r + 1]) - int(row_ptrs[r]), stride_factor))
        lens[s] = longest
        sets[s + 1] = int(sets[s]) + longest
    return sets, lens


def convert_ptrs_to_sizes(ptrs):
    return np.array([int(ptrs[i + 1]) - int(ptrs[i]) for i in range(len(ptrs) - 1)], np.uint64)


def convert_idxs_to_ptrs(idxs, n, pt):
    """ptrs[r] = number of (ascending) idxs below r, r = 0 .. n"""
    counts = np.zeros(n + 2, np.int64)
    for i in np.asarray(idxs, np.int64):
        counts[i + 1] += 1
    return np.cumsum(counts)[:n + 1].astype(pt)


def csr_convert_to_ell(row_ptrs, cols, vals, k, stride, out_cols, out_vals):
    """the ELL arrays after the conversion wrote into (out_cols, out_vals): every slot of rows 0 .. n_rows is
    defined (an entry or (-1, +0)); rows n_rows .. stride keep what they held"""
    oc, ov = np.array(out_cols), np.array(out_vals)
    for r in range(len(row_ptrs) - 1):
        a, ln = int(row_ptrs[r]), int(row_ptrs[r + 1]) - int(row_ptrs[r])
        assert ln <= k
        for j in range(k):
            oc[r + j * stride], ov[r + j * stride] = (cols[a + j], vals[a + j]) if j < ln else (PAD, 0)
    return oc, ov


def csr_convert_to_sellp(row_ptrs, cols, vals, slice_size, sets, out_cols, out_vals):
    """the same for SELL-P: every slot of every existing row is defined.  The rows a partial last slice has
    room for beyond n_rows keep what they held, as in the reference (csr_kernels.cpp:529-569) - no product
    reads them"""
    oc, ov = np.array(out_cols), np.array(out_vals)
    for r in range(len(row_ptrs) - 1):
        s, l = divmod(r, slice_size)
        a, ln = int(row_ptrs[r]), int(row_ptrs[r + 1]) - int(row_ptrs[r])
        for j in range(int(sets[s + 1]) - int(sets[s])):
            at = (int(sets[s]) + j) * slice_size + l
            oc[at], ov[at] = (cols[a + j], vals[a + j]) if j < ln else (PAD, 0)
    return oc, ov


# ------------------------------------------------------------------------------------------ case families
ROWS = (1, 17, 33, 63, 64, 65, 128, 129, 255, 256, 257, 512, 513)
COLS = (1, 37, 300)
ELL_K = (0, 1, 7, 8, 9, 16, 17, 25)
SLICES = ((64, 1), (32, 2), (2, 2), (1, 1), (100, 3), (128, 1))
SELLP_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 25)
# (nrhs, ldb, ldc, b offset, c offset) -> the branch the launchers of formats.hip must take
LAYOUTS = (((1, 1, 1, 0, 0), "one unit"), ((1, 3, 2, 0, 0), "one strided"),
           ((2, 2, 4, 0, 0), "row 2"), ((2, 3, 3, 0, 0), "row 2"),
           ((3, 4, 4, 0, 0), "frag 4"), ((4, 4, 6, 0, 0), "frag 4"),
           ((3, 3, 5, 0, 0), "row 4"), ((4, 5, 4, 0, 0), "row 4"),
           ((4, 6, 6, 1, 0), "row 4"), ((4, 6, 6, 0, 1), "row 4"),
           ((5, 6, 6, 0, 0), "frag 8"), ((7, 8, 8, 0, 0), "frag 8"), ((8, 8, 10, 0, 0), "frag 8"),
           ((8, 9, 9, 0, 0), "row 8"), ((11, 11, 13, 0, 0), "row 8"),
           ((9, 10, 10, 0, 0), "frag 8"), ((11, 12, 12, 0, 0), "frag 8"), ((16, 16, 16, 0, 0), "frag 8"))
COMPLEX_LAYOUTS = ((1, 1, 1, 0, 0), (3, 4, 5, 0, 0), (8, 8, 8, 0, 0))
REAL_SCALARS = (None, (0.7, -1.3), (1.0, 1.0), (2.0, 0.0))
COMPLEX_SCALARS = (None, (0.5 - 2j, -1 + 0.5j), (0.5 - 2j, 0.0))


def branch_of(n_cols, nrhs, ldb, ldc, b_ptr, c_ptr, itemsize):
    """the launcher's own conditions (formats.hip: launch_fmt, which launch_ell and launch_sellp both end in, and
    frag_layout)"""
    frag = n_cols > 0 and nrhs >= 3 and ldb % 2 == 0 and ldc % 2 == 0 and \
        b_ptr % (2 * itemsize) == 0 and c_ptr % (2 * itemsize) == 0
    if nrhs == 1:
        return "one unit" if ldb == 1 else "one strided"
    if frag:
        return "frag 4" if nrhs <= 4 else "frag 8"
    return "row 2" if nrhs == 2 else ("row 4" if nrhs <= 4 else "row 8")


def values(rng, shape, t):
    v = rng.uniform(-1, 1, shape)
    if br.is_complex(t):
        v = v + 1j * rng.uniform(-1, 1, shape)
    return v.astype(t)


def entries(rng, t, n_cols, count, low=0):
    return list(zip(rng.integers(low, n_cols, count).tolist(), values(rng, count, t)))


def ell_rows(rng, t, n_rows, n_cols, k, family):
    """`cycle`: row r holds r mod (k + 1) entries (neighbouring lanes differ), the rest is padding behind them;
    `padfront`: the same with one padding slot that carries a value in front of the entries;
    `compact`: sorted distinct columns, non-zero values, no padding inside (survives a trip through dense)"""
    rows = []
    for r in range(n_rows):
        ln = r % (k + 1)
        if family == "compact":
            cs = np.sort(rng.choice(n_cols, min(ln, n_cols), replace=False))
            rows.append([(int(c), v + np.dtype(t).type(2)) for c, v in zip(cs, values(rng, len(cs), t))])
        elif family == "padfront" and ln >= 1:
            rows.append([(PAD, np.dtype(t).type(3.5))] + entries(rng, t, n_cols, ln - 1))
        else:
            rows.append(entries(rng, t, n_cols, ln))
    return rows


def sellp_rows(rng, t, n_rows, n_cols, slice_size, family):
    """`cycle`: row lengths cycle through SELLP_LENGTHS, so the slices inside one wave differ in length;
    `empties`: the same with whole slices emptied - the last one (two slices and more), the first (four and
    more) and one in the middle (five and more)"""
    ns = (n_rows + slice_size - 1) // slice_size
    empty = set()
    if family == "empties":
        empty |= {ns - 1} if ns >= 2 else set()
        empty |= {0} if ns >= 4 else set()
        empty |= {ns // 2} if ns >= 5 else set()
    return [[] if r // slice_size in empty else entries(rng, t, n_cols, SELLP_LENGTHS[r % len(SELLP_LENGTHS)])
            for r in range(n_rows)]


def trailing_empty_slice_in_shared_wave(slice_size, lens):
    """the shape of the fragment kernel's former out-of-bounds load: the last slice is empty (so its first
    slot lies at the end of the arrays) and a non-empty slice shares its 64-row wave"""
    if len(lens) < 2 or int(lens[-1]) != 0:
        return False
    first_row = (len(lens) - 1) * slice_size
    return any(int(v) > 0 for v in lens[first_row // 64 * 64 // slice_size:-1])


def ell_cases():
    """(layout index, n_rows, n_cols, k, stride, family, scalar index): every layout meets every row count,
    every k and every scalar pair"""
    out, i = [], 0
    for li in range(len(LAYOUTS)):
        for ri, n in enumerate(ROWS):
            k = ELL_K[i % len(ELL_K)]
            out.append((li, n, COLS[i % 3], k, n + 5 * (i % 2), ("cycle", "padfront")[(i // 2) % 2], (i // 3) % 4))
            i += 1
    return out


def sellp_cases():
    """(layout index, n_rows, n_cols, slice index, family, scalar index): every layout and every slice
    size meets every row count"""
    out, i = [], 0
    for li in range(len(LAYOUTS)):
        for si in range(len(SLICES)):
            for j in range(3):
                n = ROWS[(li + 3 * si + j) % len(ROWS)]
                out.append((li, n, COLS[i % 3], si, ("cycle", "empties")[i % 2], (i // 2) % 4))
                i += 1
    return out


def random_csr(rng, t, it, lengths, n_cols):
    lengths = np.asarray(lengths, np.int64)
    ptrs = np.zeros(len(lengths) + 1, it)
    ptrs[1:] = np.cumsum(lengths)
    nnz = int(ptrs[-1])
    return ptrs, rng.integers(0, n_cols, nnz).astype(it), values(rng, nnz, t)
