"""numpy restatement of the block-Jacobi contract of ginkgo_amd/csrc/jacobi.hip (include/gko_cdna4.h, "block-Jacobi"):
block detection, the storage scheme with the launchers' layout predicates, the Gauss-Jordan inversion, the products in
full and reduced storage, and the three fused kernels.  Independent of oracle/.

Same conventions as tests/binding_refs.py, whose `Arith` this file uses: `hp(T)` = long double is the expected value
where a tolerance applies, `plain(T)` = the value type with every real operation rounded on its own is what the kernels
promise to match bit for bit and what sizes rule R.  Complex arithmetic follows csrc/complex_type.hpp operation for
operation: the textbook product (csr_struct_refs.mul), Smith's quotient (value_kernel_refs.smith), == on both parts
(gmres_refs.is_zero).  The modulus of the pivot search is NOT copied from the kernel: it is hypot(re, im)
(gmres_refs.abs_v).  The layout helpers and the block transpose are those of tests/value_kernel_refs.py.

The inputs of tests/test_jacobi_kernels_gpu.py are built here as well (`generate_case`, `apply_case`, `fused_case`), so
that tests/test_jacobi_refs_cpu.py can assert on the same arrays what the GPU file relies on: the pivot margin of every
complex block and the exactly zero pivot of the singular ones.  Nothing here touches a GPU."""
import numpy as np

import binding_refs as br
import csr_struct_refs as cr
import gmres_refs as gr
import krylov_step_refs as ks
import value_kernel_refs as vr

PRECISIONS = (0x01, 0x02, 0x10, 0x11, 0x20)
PIVOT_MARGIN = 2.0 ** -10
_TN_ID = {"f64": 1, "f32": 2, "c128": 3, "c64": 4}


# ------------------------------------------------------------------------ storage scheme, layout predicates
class Scheme:
    """gkoc_jacobi_scheme; `stride` = entries between two columns of a block"""

    def __init__(self, block_offset, group_offset, group_power):
        self.block_offset, self.group_offset, self.group_power = int(block_offset), int(group_offset), int(group_power)

    @property
    def stride(self):
        return self.block_offset << self.group_power

    @property
    def group_size(self):
        return 1 << self.group_power

    def as_tuple(self):
        return self.block_offset, self.group_offset, self.group_power


def storage_scheme(max_block_size):
    """Jacobi::compute_storage_scheme with max_block_stride = 64: a group holds 64 / p2 blocks, p2 = the power of two
    at or above max_block_size"""
    p2 = 1
    while p2 < max_block_size:
        p2 *= 2
    group_size = 64 // p2
    return Scheme(max_block_size, max_block_size * group_size * max_block_size, group_size.bit_length() - 1)


def num_groups(scheme, num_blocks):
    return -(-num_blocks // scheme.group_size)


def storage_size(scheme, num_blocks):
    return vr.block_storage_size(scheme, num_blocks)


def subwarp_of(scheme):
    sub = 1
    while sub < scheme.block_offset:
        sub *= 2
    return sub


def wide_group_layout(scheme):
    """the layout of the tuned kernels: block_offset a power of two up to 16, a group is one 64-wide panel"""
    bo = scheme.block_offset
    return 1 <= bo <= 16 and (bo & (bo - 1)) == 0 and (bo << scheme.group_power) == 64


def wave_group_layout(scheme):
    return 1 <= scheme.block_offset <= 32 and (subwarp_of(scheme) << scheme.group_power) == 64


def groups_per_wave(block_offset, value_size):
    return 1 if block_offset * value_size >= 128 else 2


def lanes_groups_per_wave(scheme, value_size):
    """GPW of launch_apply_lanes_any"""
    sub = subwarp_of(scheme)
    if sub <= 8:
        return 4 if value_size <= 8 else 2
    if sub == 16:
        return 2 if value_size <= 8 else 1
    return 1


def fixed_workgroups(scheme, num_blocks, value_size, gpw=None):
    gpw = groups_per_wave(scheme.block_offset, value_size) if gpw is None else gpw
    return -(-num_groups(scheme, num_blocks) // (4 * gpw))


def xcd_map_applies(workgroups, tune):
    return tune != 0 and workgroups >= 2048


def apply_branch(scheme, value_size, nrhs, ldb, ldx, b_addr, x_addr, mfma_mode=2):
    """the kernel launch_apply picks: (name, pairs_ok) with name in fixed, multi4, multi8, mfma, general"""
    wide = wide_group_layout(scheme)
    if nrhs == 1 and ldb == 1 and ldx == 1 and wide:
        return "fixed", None
    mfma_from = {1: 2, 3: 4}.get(mfma_mode, 9)
    mfma = value_size == 8 and mfma_mode != 0 and nrhs >= mfma_from and scheme.block_offset == 8 and \
        scheme.group_power == 3
    if nrhs >= 2 and wide and not mfma:
        pairs = b_addr % (2 * value_size) == 0 and ldb % 2 == 0 and x_addr % (2 * value_size) == 0 and ldx % 2 == 0
        return ("multi4" if nrhs <= 4 else "multi8"), bool(pairs)
    return ("mfma" if mfma else "general"), None


def adaptive_branch(scheme, nrhs, ldb, ldx):
    return "fixed" if wide_group_layout(scheme) and nrhs == 1 and ldb == 1 and ldx == 1 else "general"


def any_branch(scheme, lanes_tune=0):
    return "lanes" if lanes_tune != 1 and wave_group_layout(scheme) else "rows"


def fused_workspace_bytes(n_rows, value_size):
    return ((n_rows + 63) // 64 + 4096 + 1024) * value_size


def step2_apply_fits(scheme, num_blocks, n_rows, value_size):
    if not wide_group_layout(scheme) or num_blocks <= 0 or n_rows <= 0:
        return False
    total = fused_workspace_bytes(n_rows, value_size) // value_size
    return fixed_workgroups(scheme, num_blocks, value_size) <= (total - 2 * 1024) // 2


# ------------------------------------------------------------------------------------------ find_blocks
PATTERNS = ("same", "alternate", "natural", "chain")


def pattern(kind, n, max_bs=4):
    """CSR patterns (row_ptrs, cols): `same`: every row has the columns {0, 1}, n > max_block_size rows give full
    blocks; `alternate`: no two neighbours alike; `natural`: runs of 3 max_bs + 1 equal rows, natural blocks larger
    than max_block_size; `chain`: every row its own diagonal, with max_block_size 1 a chain of n single-row blocks"""
    if n == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int64)
    if kind == "same":
        cols = np.tile([0, min(1, n - 1)], n)
        return np.arange(n + 1, dtype=np.int64) * 2, cols.astype(np.int64)
    if kind == "chain":
        return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64)
    if kind == "alternate":
        return np.arange(n + 1, dtype=np.int64), (np.arange(n) % 2).astype(np.int64)
    cols = np.arange(n) // (3 * max_bs + 1)
    return np.arange(n + 1, dtype=np.int64), cols.astype(np.int64)


def find_blocks(row_ptrs, cols, max_block_size):
    """natural blocks (runs of rows with the column pattern of the row above, cut at max_block_size), then greedy
    agglomeration: a block takes whole natural blocks while it stays within max_block_size -> block pointers"""
    rp, cols = np.asarray(row_ptrs, np.int64), np.asarray(cols, np.int64)
    n = rp.shape[0] - 1
    if n == 0:
        return np.zeros(1, np.int64)
    same = np.zeros(n, bool)
    length = np.diff(rp)
    if np.all(length == length[0]):                  # rows of one length: all neighbours compared at once
        c2 = cols[:n * length[0]].reshape(n, length[0])
        same[1:] = np.all(c2[1:] == c2[:-1], axis=1)
    else:
        for i in np.flatnonzero(length[1:] == length[:-1]) + 1:
            same[i] = np.array_equal(cols[rp[i - 1]:rp[i]], cols[rp[i]:rp[i + 1]])
    natural = [0]
    for i in range(1, n):
        if not same[i] or i - natural[-1] >= max_block_size:
            natural.append(i)
    natural.append(n)
    ptrs = [0]
    k = 0
    while ptrs[-1] < n:
        s = ptrs[-1]
        while k + 1 < len(natural) and natural[k + 1] <= s + max_block_size:
            k += 1
        ptrs.append(natural[k])
    return np.array(ptrs, np.int64)


# -------------------------------------------------------------------------------------------- inversion
def extract_block(wt, row_ptrs, cols, vals, start, bs):
    """the dense diagonal block: entries outside it dropped, missing ones zero, any column order"""
    B = np.zeros((bs, bs), wt)
    for r in range(bs):
        for k in range(int(row_ptrs[start + r]), int(row_ptrs[start + r + 1])):
            c = int(cols[k]) - start
            if 0 <= c < bs:
                B[r, c] = vals[k]
    return B


def _same_parts(a, b):
    """|re| and |im| of a and b have identical bits"""
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a.real).tobytes() == np.abs(b.real).tobytes() and np.abs(a.imag).tobytes() == np.abs(b.imag).tobytes()


def gauss_jordan(ar, block, pivots=None):
    """gauss_jordan_lds operation for operation.  Step k: the pivot is the first row of [k, bs) with the largest
    magnitude (or pivots[k]); rows k and pivot swap; a pivot d that is exactly zero ends the inversion with the
    block as it stands; else column k is divided by -d, B(k, k) = 0, every row r adds B(r, k) times row k, row k
    is divided by d and B(k, k) = 1 / d.
    Returns dict(B, perm, dead (the step of the zero pivot or None), pivots, margins): margins[k] = (largest,
    runner-up, tie) of the candidates' magnitudes, tie = the runner-up has the largest one's |re|, |im| bits"""
    B = ar.a(block).copy()
    bs = B.shape[0]
    perm = list(range(bs))
    used, margins, dead = [], [], None
    cx = np.iscomplexobj(B)
    with np.errstate(all="ignore"):
        for k in range(bs):
            mag = gr.abs_v(ar, B[k:, k])
            order = np.argsort(-mag, kind="stable")
            first = k + int(np.argmax(mag))
            runner = (mag[order[1]], _same_parts(B[k + order[0], k], B[k + order[1], k])) if bs - k > 1 else (None, False)
            margins.append((mag[order[0]], runner[0], runner[1]))
            cp = first if pivots is None else int(pivots[k])
            used.append(cp)
            if cp != k:
                B[[k, cp]] = B[[cp, k]]
                perm[k], perm[cp] = perm[cp], perm[k]
            d = B[k, k]
            if gr.is_zero(d):
                dead = k
                break
            B[:, k] = vr.smith(ar, B[:, k], -d) if cx else B[:, k] / -d
            B[k, k] = 0
            row_k = B[k].copy()
            B = cr.add(ar, B, cr.mul(ar, B[:, k:k + 1], row_k[None, :]))
            B[k] = vr.smith(ar, B[k], d) if cx else B[k] / d
            B[k, k] = cr.reciprocal(ar, np.asarray(d, ar.wt))
    return dict(B=B, perm=perm, dead=dead, pivots=used, margins=margins)


def generate(ar, row_ptrs, cols, vals, scheme, block_ptrs, out0, pivots=None):
    """the inverse blocks, column-permuted, in the interleaved scheme: entry (r, j) of the transformed block goes
    to column perm[j].  Storage outside the blocks' bs x bs entries keeps what out0 held.
    Returns (storage, runs): runs[b] = the gauss_jordan result of block b"""
    out = np.array(out0, dtype=ar.wt, copy=True)
    runs = []
    for b in range(len(block_ptrs) - 1):
        start, bs = int(block_ptrs[b]), int(block_ptrs[b + 1] - block_ptrs[b])
        run = gauss_jordan(ar, extract_block(ar.wt, row_ptrs, cols, vals, start, bs),
                           None if pivots is None else pivots[b])
        base = vr.block_start(scheme, b)
        for j in range(bs):
            out[base + np.arange(bs) + run["perm"][j] * scheme.stride] = run["B"][:, j]
        runs.append(run)
    return out, runs


def block_entries(scheme, block_ptrs):
    """per distinct block size: (ids of the blocks, their first rows, idx) with idx[b, i, j] = the storage index
    of entry (i, j) of block ids[b]"""
    ptrs = np.asarray(block_ptrs, np.int64)
    sizes = np.diff(ptrs)
    ids_all = np.arange(sizes.shape[0], dtype=np.int64)
    base = scheme.group_offset * (ids_all >> scheme.group_power) + scheme.block_offset * (ids_all & (scheme.group_size - 1))
    res = []
    for bs in np.unique(sizes):
        if bs == 0:
            continue
        ids = ids_all[sizes == bs]
        i = np.arange(bs, dtype=np.int64)
        idx = base[ids][:, None, None] + i[None, :, None] + i[None, None, :] * scheme.stride
        res.append((ids, ptrs[ids], idx))
    return res


def entry_mask(scheme, block_ptrs, size):
    """True where the storage holds an entry of a block"""
    m = np.zeros(size, bool)
    for _, _, idx in block_entries(scheme, block_ptrs):
        m[idx.reshape(-1)] = True
    return m


# --------------------------------------------------------------------------------------- reduced storage
def storage_kind(rt, p):
    """precision_reduction byte -> storage kind of a part of type rt: double parts have the five reduced types,
    float parts fall on half ((0,1), (0,2), (1,1)) and the upper 16 bits ((1,0), (2,0)); 0 = the part itself"""
    p = int(p)
    if np.dtype(rt) == np.float64:
        return p if p in PRECISIONS else 0
    return 0x02 if p in (0x01, 0x02, 0x11) else 0x11 if p in (0x10, 0x20) else 0


def _narrow(kind, v):
    """parts (double or float) -> the stored words of `kind` (the comment above stored<> in jacobi.hip): 0x01 float,
    0x02 half through float (round to nearest even, below the normal half range signed zero), 0x10 / 0x20 the upper
    32 / 16 bits of the double, 0x11 the upper 16 bits of the float"""
    v = np.ascontiguousarray(v)
    with np.errstate(all="ignore"):
        if kind == 0x01:
            return v.astype(np.float32)
        if kind == 0x02:
            return br.f32_to_half(v.astype(np.float32)).view(np.uint16)
        if kind == 0x10:
            return (v.astype(np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)
        if kind == 0x20:
            return (v.astype(np.float64).view(np.uint64) >> np.uint64(48)).astype(np.uint16)
        if kind == 0x11:
            return (v.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    raise ValueError(kind)


def _widen(kind, w):
    """stored words -> double (subnormal halves read as signed zero)"""
    if kind == 0x01:
        return w.astype(np.float64)
    if kind == 0x02:
        return br.half_to_f32(w.view(np.float16)).astype(np.float64)
    if kind == 0x10:
        return (w.astype(np.uint64) << np.uint64(32)).view(np.float64)
    if kind == 0x20:
        return (w.astype(np.uint64) << np.uint64(48)).view(np.float64)
    if kind == 0x11:
        return (w.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    raise ValueError(kind)


_WORD = {0x01: np.float32, 0x02: np.uint16, 0x10: np.uint32, 0x11: np.uint16, 0x20: np.uint16}


def _groups(scheme, num_blocks, blocks):
    """(real type, parts per group, the storage as parts, as bytes)"""
    rt = np.dtype(br.real_of(blocks.dtype))
    per = scheme.group_offset * (2 if br.is_complex(blocks.dtype) else 1)
    return rt, per, blocks.view(rt), blocks.view(np.uint8)


def convert_groups(scheme, num_blocks, blocks, group_prec):
    """group by group, in place: every part of the group (padding included) becomes a word of the group's reduced
    type at the same part index, i.e. in the first part of the group; the rest of the group keeps its bytes.  A
    complex entry is its two parts"""
    out = np.array(blocks, copy=True)
    rt, per, parts, raw = _groups(scheme, num_blocks, out)
    for g in range(num_groups(scheme, num_blocks)):
        kind = storage_kind(rt, group_prec[g])
        if kind:
            words = _narrow(kind, parts[g * per:(g + 1) * per].copy())
            at = g * per * rt.itemsize
            raw[at:at + words.nbytes] = words.view(np.uint8)
    return out


def convert_storage(scheme, num_blocks, blocks, prec):
    """gkoc_jacobi_convert_storage_f64: one precision for all groups"""
    return convert_groups(scheme, num_blocks, blocks, np.full(num_groups(scheme, num_blocks), prec))


def widen_storage(scheme, num_blocks, blocks, group_prec):
    """the values the apply kernels see: part i of group g read in the group's precision (0 = the part's type)"""
    blocks = np.ascontiguousarray(blocks)
    out = blocks.copy()
    rt, per, parts, raw = _groups(scheme, num_blocks, blocks)
    outp = out.view(rt)
    for g in range(num_groups(scheme, num_blocks)):
        kind = storage_kind(rt, group_prec[g])
        if kind:
            wt = np.dtype(_WORD[kind])
            at = g * per * rt.itemsize
            outp[g * per:(g + 1) * per] = _widen(kind, raw[at:at + per * wt.itemsize].view(wt)).astype(rt)
    return out


def transpose_stored(scheme, block_ptrs, blocks, block_prec, out0):
    """gkoc_jacobi_transpose_f64 with a precision array: the entries move as raw words of their group's type.  Per
    storage type, the words of every group are laid out as one array in the scheme's own indexing and
    value_kernel_refs.jacobi_transpose moves them; the groups of that type are written back"""
    out = np.array(out0, np.float64, copy=True)
    nb = len(block_ptrs) - 1
    go = scheme.group_offset
    group_prec = [int(block_prec[g << scheme.group_power]) for g in range(num_groups(scheme, nb))]
    src, dst = np.ascontiguousarray(blocks, np.float64).view(np.uint8), out.view(np.uint8)
    for kind in sorted(set(group_prec)):
        wt = np.dtype(_WORD[kind]) if kind else np.dtype(np.float64)
        words = lambda raw: np.concatenate([raw[g * go * 8:g * go * 8 + go * wt.itemsize].view(wt)      # noqa: E731
                                            for g in range(len(group_prec))])
        moved = vr.jacobi_transpose(scheme, block_ptrs, words(src), False, words(dst))
        for g, p in enumerate(group_prec):
            if p == kind:
                dst[g * go * 8:g * go * 8 + go * wt.itemsize] = moved[g * go:(g + 1) * go].view(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------- products
def _operands(ar, b, alpha, beta, x0):
    b = ar.a(b)
    if alpha is None:
        return b, None, None, np.zeros(b.shape, ar.wt)
    return b, ar.wt(alpha), ar.wt(beta), ar.a(x0).copy()


def apply_tuned(ar, scheme, block_ptrs, blocks, b, alpha=None, beta=None, x0=None):
    """the order of the real-type kernels (jacobi_apply_kernel, the fixed and multi-column kernels): x = M b as
    sum = 0, sum += m_c b_c in column order; advanced: sum = x beta (0 if beta == 0: x is not read), then
    sum += (alpha m_c) b_c.  Multiply and add rounded separately.  b, x0: rows x nrhs"""
    b, alpha, beta, out = _operands(ar, b, alpha, beta, x0)
    blocks = ar.a(blocks)
    with np.errstate(all="ignore"):
        for ids, starts, idx in block_entries(scheme, block_ptrs):
            bs = idx.shape[1]
            rows = starts[:, None] + np.arange(bs)[None, :]
            bb = b[rows]                                        # nb x bs x nrhs
            if alpha is None or gr.is_zero(beta):
                s = np.zeros(bb.shape, ar.wt)
            else:
                s = cr.mul(ar, out[rows], beta)
            for c in range(bs):
                m = blocks[idx[:, :, c]][:, :, None]
                if alpha is not None:
                    m = cr.mul(ar, alpha, m)
                s = cr.add(ar, s, cr.mul(ar, m, bb[:, c, None, :]))
            out[rows] = s
    return out


def apply_any(ar, scheme, block_ptrs, blocks, b, alpha=None, beta=None, x0=None):
    """the order of the kernels for the other value types (lanes and thread per row): sum = 0, sum += m_c b_c, then
    x = sum, or alpha sum (+ beta x unless beta == 0)"""
    b, alpha, beta, out = _operands(ar, b, alpha, beta, x0)
    blocks = ar.a(blocks)
    with np.errstate(all="ignore"):
        for ids, starts, idx in block_entries(scheme, block_ptrs):
            bs = idx.shape[1]
            rows = starts[:, None] + np.arange(bs)[None, :]
            bb = b[rows]
            s = np.zeros(bb.shape, ar.wt)
            for c in range(bs):
                s = cr.add(ar, s, cr.mul(ar, blocks[idx[:, :, c]][:, :, None], bb[:, c, None, :]))
            if alpha is not None:
                s = cr.mul(ar, alpha, s)
                if not gr.is_zero(beta):
                    s = cr.add(ar, s, cr.mul(ar, beta, out[rows]))
            out[rows] = s
    return out


def apply_abs_sum(scheme, block_ptrs, blocks, b, alpha=None):
    """sum_c |alpha m_c b_c| per entry of x, in long double (real types)"""
    b = np.asarray(b, np.longdouble)
    blocks = np.asarray(blocks, np.longdouble)
    out = np.zeros(b.shape, np.longdouble)
    a = np.longdouble(1 if alpha is None else alpha)
    for ids, starts, idx in block_entries(scheme, block_ptrs):
        bs = idx.shape[1]
        rows = starts[:, None] + np.arange(bs)[None, :]
        bb = b[rows]
        s = np.zeros(bb.shape, np.longdouble)
        for c in range(bs):
            s = s + np.abs(a * blocks[idx[:, :, c]][:, :, None] * bb[:, c, None, :])
        out[rows] = s
    return out


def dense_blocks(scheme, block_ptrs, blocks):
    return vr.jacobi_blocks_dense(scheme, block_ptrs, blocks)


# ------------------------------------------------------------------------------------------ fused kernels
def apply_dot(ar, scheme, block_ptrs, blocks, b):
    """x = M b; the scalar <b, x> is judged against the long-double sum over the kernel's own vectors"""
    return apply_tuned(ar, scheme, block_ptrs, blocks, np.asarray(b).reshape(-1, 1)).reshape(-1)


def step2_apply(ar, scheme, block_ptrs, blocks, a):
    """cg::step_2 (x += t p, r -= t q, t = rho / beta; a no-op for beta == 0 or a stopped column), then z = M r on
    the new r.  a: x, r, p, q (n), beta, rho, stop_status (1) -> dict(x, r, z)"""
    col = {k: np.asarray(v).reshape(-1, 1) if k in "xrpq" else np.asarray(v) for k, v in a.items()}
    s2 = ks.apply(ar, "cg", "step_2", {n: col[n] for n, _ in ks.CG_ABI["cg"]["step_2"]})
    z = apply_tuned(ar, scheme, block_ptrs, blocks, s2["r"])
    return dict(x=s2["x"].reshape(-1), r=s2["r"].reshape(-1), z=z.reshape(-1))


def pipe_steps(ar, scheme, block_ptrs, blocks, a):
    """pipe_cg::step_2, step_1 with the new beta (krylov_step_refs.x_step_2_step_1), then m = M w on the new w; f
    was formed from the old m.  -> dict(x, r, z, w, p, q, f, g, m, beta_out)"""
    out = ks.x_step_2_step_1(ar, a)
    out["m"] = apply_tuned(ar, scheme, block_ptrs, blocks, np.asarray(out["w"]).reshape(-1, 1)).reshape(-1)
    return out


def fused_dot_depth(scheme, num_blocks, value_size, rows_fold=False):
    """additions on the longest path of a reduced scalar of the three fused kernels.  A thread adds the products
    of its GPW groups in turn to zero (GPW); block_sum<256>: 6 butterfly levels and 2 for the four wave sums (8);
    then nb = ceil(groups / (4 GPW)) partials.  fold_partials / fold_partials2 (apply_dot, step_2 + apply): up to
    fold_single_max = 16384 partials one block of 1024 threads adds ceil(nb / 1024) in turn and block_sum<1024>
    adds 6 + 4 levels; above that fold_chunks(2)_kernel first folds chunks of ceil(nb / 1024) partials (256
    threads: ceil(chunk / 256) in turn, block_sum<256>: 8), and the single block folds the <= 1024 chunk sums
    (1 + 10).  fold_rows_kernel (the PipeCg kernel): ceil(nb / 1024) in turn, block_sum<1024>: 10"""
    gpw = groups_per_wave(scheme.block_offset, value_size)
    nb = fixed_workgroups(scheme, num_blocks, value_size)
    if rows_fold or nb <= 16384:
        return gpw + 8 + -(-nb // 1024) + 10
    chunk = -(-nb // 1024)
    return gpw + 8 + -(-chunk // 256) + 8 + 1 + 10


def dots_hp(pairs):
    """long-double sums and sums of |terms| of the products (u, v) in `pairs`"""
    terms = [np.asarray(u, np.longdouble) * np.asarray(v, np.longdouble) for u, v in pairs]
    return np.array([np.sum(t) for t in terms], np.longdouble), np.array([np.sum(np.abs(t)) for t in terms],
                                                                         np.longdouble)


# ------------------------------------------------------------------------------------- inputs of the tests
def _rand(rng, shape, t):
    return gr.rand(rng, shape, t)


def special_blocks(max_block_size, t):
    """integer-valued blocks (name, dense): a zero leading entry, an exact tie (real: +-2; complex: entries with
    identical |re|, |im|), an exactly singular block; from three rows on a tie of three rows and a singular 3 x 3
    that dies at its last step; last a singular block whose first column is a tie (second row = minus the first):
    all its arithmetic is exact, so the half-transformed block it is left as shows which row was the pivot, in any
    value type.  Singular complex blocks are the integers times i (Smith's other branch), the last one times 1 + i"""
    cx = br.is_complex(t)
    if max_block_size == 1:
        return [("singular", np.array([[0]], t)), ("one", np.array([[2]], t))]
    tie = np.array([[3 + 4j, 1], [-3 - 4j, 2]], t) if cx else np.array([[2, 1], [-2, 3]], t)
    out = [("zero_lead", np.array([[0, 2], [1, 1]], t)), ("tie", tie),
           ("singular", np.array([[1, 2], [2, 4]], t) * (t(1j) if cx else t(1)))]
    if max_block_size >= 3:
        tie3 = np.array([[1, 2, 0], [-1, 1, 1], [1, 0, 3]], t)
        if cx:
            tie3 = tie3 * t(1 + 1j)
        out += [("tie3", tie3), ("singular", np.array([[1, 2, 3], [2, 4, 6], [1, 1, 1]], t) * (t(1j) if cx else t(1)))]
    out.append(("singular", np.array([[1, 2], [-1, -2]], t) * (t(1 + 1j) if cx else t(1))))
    return out


def margins_ok(run, margin=PIVOT_MARGIN):
    """every step's largest candidate beats the runner-up by the relative margin, or ties with it through
    identical parts"""
    for top, second, tie in run["margins"]:
        if second is None or top == 0:
            continue
        if not (top - second >= margin * top or (top == second and tie)):
            return False
    return True


def _random_block(rng, t, bs):
    """uniform entries in (-1, 1) (both parts), about a tenth of the off-diagonal ones missing.  Complex: drawn
    again until the long-double run keeps the pivot margin (twice the margin the tests assert) at every step and
    the value-type run picks the same pivots"""
    for _ in range(200):
        B = _rand(rng, (bs, bs), t)
        present = rng.random((bs, bs)) >= 0.1
        present[np.arange(bs), np.arange(bs)] = True
        B = np.where(present, B, t(0)).astype(t)
        if not br.is_complex(t):
            return B, present
        run = gauss_jordan(br.hp(t), B)
        if run["dead"] is None and margins_ok(run, 2 * PIVOT_MARGIN) and \
                gauss_jordan(br.plain(t), B)["pivots"] == run["pivots"]:
            return B, present
    raise AssertionError("no block with a clear pivot order found")


GENERATE_SIZES = {"f64": (1, 2, 3, 4, 8, 13, 16, 32, 64), "f32": (1, 2, 3, 4, 8, 13, 16, 32, 64),
                  "c128": (1, 2, 3, 4, 8, 13, 16, 32), "c64": (1, 2, 3, 4, 8, 13, 16, 32)}
_CASES = {}


def generate_case(tn, max_block_size):
    """a matrix for gkoc_jacobi_generate: per_wave * k + 1 blocks (per_wave = 64 / subwarp blocks share a wave) of
    mixed sizes 1 .. max_block_size, the special blocks first; entries outside the blocks, missing entries inside
    them, columns of every row shuffled.  dict(n, row_ptrs, cols, vals, block_ptrs, names, scheme, per_wave)"""
    key = (tn, max_block_size)
    if key in _CASES:
        return _CASES[key]
    t = br.TYPES[tn]
    rng = np.random.default_rng([23, _TN_ID[tn], max_block_size])
    scheme = storage_scheme(max_block_size)
    per_wave = 64 // subwarp_of(scheme)
    count = per_wave * max(2, -(-8 // per_wave)) + 1
    dense, names = [], []
    for name, B in special_blocks(max_block_size, t):
        dense.append((B, np.ones(B.shape, bool)))
        names.append(name)
    sizes = [max_block_size, 1] + [1 + (7 * i + 3) % max_block_size for i in range(count)]
    for bs in sizes[:count - len(dense)]:
        dense.append(_random_block(rng, t, bs))
        names.append("random")
    ptrs = np.concatenate([[0], np.cumsum([B.shape[0] for B, _ in dense])]).astype(np.int64)
    n = int(ptrs[-1])
    row_ptrs, cols, vals = [0], [], []
    for b, (B, present) in enumerate(dense):
        start, bs = int(ptrs[b]), B.shape[0]
        outside = np.setdiff1d(np.arange(n), np.arange(start, start + bs))
        for r in range(bs):
            c = list(start + np.flatnonzero(present[r]))
            v = list(B[r, present[r]])
            if outside.size:
                extra = rng.choice(outside, min(2, outside.size), replace=False)
                c += list(extra)
                v += list(_rand(rng, (extra.size,), t) + t(5))
            order = rng.permutation(len(c))
            cols += [int(c[i]) for i in order]
            vals += [v[i] for i in order]
            row_ptrs.append(len(cols))
    case = dict(n=n, row_ptrs=np.array(row_ptrs, np.int64), cols=np.array(cols, np.int64), vals=np.array(vals, t),
                block_ptrs=ptrs, names=names, scheme=scheme, per_wave=per_wave, dense=[B for B, _ in dense])
    _CASES[key] = case
    return case


def block_sizes(max_block_size, num_blocks, last=None):
    """sizes 1 .. max_block_size in turn, the first one full, the last one `last` rows (default: shorter than
    block_offset where that is possible)"""
    sizes = [max_block_size] + [1 + (5 * i + 2) % max_block_size for i in range(1, num_blocks)]
    sizes[-1] = max(1, max_block_size - 1) if last is None else last
    return np.concatenate([[0], np.cumsum(sizes[:num_blocks])]).astype(np.int64)


def apply_case(tn, max_block_size, num_blocks, nrhs, seed=0, uniform=False, fill=np.nan, ints=False, last=None):
    """operands of the products: block pointers (`block_sizes`; uniform: every block full), a storage whose block
    entries are uniform in (-1, 1) and whose padding is `fill`, b and x0 (n x nrhs), alpha, beta.
    ints: small integers everywhere, alpha = 2, beta = -1"""
    t = br.TYPES[tn]
    rng = np.random.default_rng([29, _TN_ID[tn], max_block_size, num_blocks, nrhs, seed])
    scheme = storage_scheme(max_block_size)
    if uniform:
        ptrs = np.arange(num_blocks + 1, dtype=np.int64) * max_block_size
    else:
        ptrs = block_sizes(max_block_size, num_blocks, last)
    n = int(ptrs[-1])
    size = storage_size(scheme, num_blocks)
    gen = gr.ints if ints else gr.rand
    blocks = np.full(size, fill, t)
    mask = entry_mask(scheme, ptrs, size)
    blocks[mask] = gen(rng, (int(mask.sum()),), t)
    s = (lambda v: np.array([v], t))
    return dict(scheme=scheme, block_ptrs=ptrs, n=n, blocks=blocks, b=gen(rng, (n, nrhs), t), x0=gen(rng, (n, nrhs), t),
                alpha=s(2.0 if ints else 0.75), beta=s(-1.0 if ints else -1.5), max_block_size=max_block_size,
                num_blocks=num_blocks)


def fused_case(tn, max_block_size, num_blocks, state="run", exact=False, seed=0, last=None):
    """operands of the three fused kernels on the blocks of `apply_case`: the vectors x r z w p q f g m n, the
    scalars of krylov_step_refs.x_case (same states) and beta / rho of cg::step_2"""
    t = br.TYPES[tn]
    a = apply_case(tn, max_block_size, num_blocks, 1, seed=seed + 100, ints=exact, last=last)
    v = ks.x_case(tn, a["n"], True, exact=exact, state=state if state != "cg_beta0" else "run")
    s = (lambda val: np.array([val], t))
    v["beta"] = s(0.0 if state in ("beta0", "cg_beta0") else (1.0 if exact else 1.5))
    a["vec"] = v
    return a
