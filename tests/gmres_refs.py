"""numpy restatements of the GMRES kernels of ginkgo_amd/csrc/gmres.hip: common_gmres::{initialize, hessenberg_qr,
solve_krylov}, gmres::{restart, multi_axpy, multi_dot} and the two fused steps gkoc_x_gmres_multi_sub_scaled and
gkoc_x_gmres_mgs_step, with the operand layouts of include/gko_cdna4.h.

Same conventions as tests/binding_refs.py, whose `Arith` this file uses: `hp(T)` = long double is the expected
value; `plain(T)` = the value type with every real operation rounded on its own is what gmres.hip promises to
match bit for bit for real types, and what sizes rule R where it does not.  Complex types: the product is the
textbook one (ac - bd, ad + bc), a quotient by a real divides both parts, a quotient by a complex is Smith's
(csrc/complex_type.hpp), the modulus is hypot(re, im) - the one operation that the device's math library and the
host's round differently, so everything downstream of `abs_v` (the new rotation of hessenberg_qr) is compared by
rule R and everything else bit for bit.

Arrays are tight: basis (num, rows, nrhs), small matrices (k, nrhs); the tests cut the strided views.  The two
tree sums have an emulation each (`multi_dot_tree`, `mgs_dot_tree`) and a function that returns the number of
additions on the longest path of the tree.  tests/test_gmres_refs_cpu.py checks all of it against independent
formulations; nothing here touches a GPU."""
import numpy as np

import binding_refs as br
import csr_struct_refs as cr
import value_kernel_refs as vr

STOPPED, FINALIZED = 0x81, 0xC2          # has_stopped (converged, id 1); stopped and finalized (id 2)


def _is_hp(ar):
    return ar.wt in (np.longdouble, np.clongdouble)


def mul(ar, x, y):
    return cr.mul(ar, x, y)


def div(ar, a, b):
    """a / b with b of the value type: IEEE for reals, Smith's quotient for complex values"""
    a, b = np.asarray(a, ar.wt), np.asarray(b, ar.wt)
    if np.iscomplexobj(a):
        return vr.smith(ar, a, b)
    with np.errstate(all="ignore"):
        return np.asarray(a / b, ar.wt)


def div_real(ar, a, r):
    """a / r with a real r: both parts divided"""
    with np.errstate(all="ignore"):
        return np.asarray(br.div_by_real(np.asarray(a, ar.wt), np.asarray(r, ar.rt)), ar.wt)


def abs_v(ar, x):
    """|x|: fabs, or hypot(re, im)"""
    x = np.asarray(x, ar.wt)
    if np.iscomplexobj(x) and not _is_hp(ar):
        return np.asarray(np.hypot(x.real, x.imag), ar.rt)
    return np.asarray(np.abs(x), ar.rt)


def is_zero(x):
    """x == T(0): both parts compare equal to zero (-0.0 does, NaN does not)"""
    x = np.asarray(x)
    return (x.real == 0) & (x.imag == 0)


# ------------------------------------------------------------------------------ element-wise kernels
def initialize(b, krylov_dim):
    """residual = b (a copy: bits kept), the krylov_dim x nrhs sine / cosine blocks zeroed, stop status 0"""
    b = np.asarray(b)
    nrhs = b.shape[1]
    z = np.zeros((krylov_dim, nrhs), b.dtype)
    return b.copy(), z, z.copy(), np.zeros(nrhs, np.uint8)


def restart(ar, residual, residual_norm):
    """krylov[0:n] = residual / norm (both parts by the real norm), rnc[0] = norm, final_iter_nums = 0"""
    residual = ar.a(residual)
    norm = np.asarray(residual_norm, ar.rt)
    k0 = div_real(ar, residual, norm.reshape(1, -1))
    return k0, np.asarray(norm, ar.wt), np.zeros(residual.shape[1], np.uint64)


def finalize(stop):
    """stopped, not finalized columns get the finalized bit"""
    stop = np.array(stop, np.uint8)
    hit = ((stop & 0x40) == 0) & ((stop & 0x3f) != 0)
    stop[hit] |= np.uint8(0x40)
    return stop


def multi_axpy(ar, basis, y, final_iter_nums, stop, out0):
    """out(:, k) = 0, then += basis_j(:, k) * y(j, k) for j < final_iter_nums[k], product and sum rounded
    separately; finalized columns keep what out0 holds; returns (out, stop after finalize)"""
    basis, y = ar.a(basis), ar.a(y)
    out = ar.a(out0).copy()
    for k in range(out.shape[1]):
        if int(stop[k]) & 0x40:
            continue
        acc = np.zeros(out.shape[0], ar.wt)
        for j in range(int(final_iter_nums[k])):
            acc = cr.add(ar, acc, mul(ar, basis[j, :, k], y[j, k]))
        out[:, k] = acc
    return out, finalize(stop)


def multi_sub_scaled(ar, basis, h, w0):
    """w = w - (h_d * v_d) in d order; a zero h_d is skipped only when nrhs == 1 (with more columns the term
    0 * v_d is subtracted: a NaN or infinity in v_d reaches w, and w = -0.0 becomes +0.0 when the product is
    -0.0)"""
    basis, h = ar.a(basis), ar.a(h)
    w = ar.a(w0).copy()
    nrhs = w.shape[1]
    for d in range(h.shape[0]):
        for k in range(nrhs):
            if nrhs == 1 and is_zero(h[d, k]):
                continue
            with np.errstate(all="ignore"):
                w[:, k] = np.asarray(w[:, k] - mul(ar, h[d, k], basis[d, :, k]), ar.wt)
    return w


def mgs_step(ar, w0, v_cur, h_cur, v_next):
    """w = w - h_cur * v_cur (skipped when h_cur == 0), h_next = sum conj(v_next) * w_new; returns (w, h_next,
    sum |terms|)"""
    w = ar.a(w0).copy()
    h_cur = ar.wt(h_cur)
    if not is_zero(h_cur):
        with np.errstate(all="ignore"):
            w = np.asarray(w - mul(ar, h_cur, ar.a(v_cur)), ar.wt)
    terms = mul(ar, np.conj(ar.a(v_next)), w)
    ones = np.ones(terms.shape, ar.wt)
    return w, ar.dot(terms, ones), np.sum(np.abs(terms.astype(np.clongdouble)))


def multi_dot(ar, basis, nxt):
    """h(d, k) = sum_i conj(basis_d(i, k)) * next(i, k); returns (h, sum |terms|), both num x nrhs"""
    basis, nxt = ar.a(basis), ar.a(nxt)
    num, _, nrhs = basis.shape
    h = np.zeros((num, nrhs), ar.wt)
    s = np.zeros((num, nrhs), np.longdouble)
    for d in range(num):
        for k in range(nrhs):
            terms = mul(ar, np.conj(basis[d, :, k]), nxt[:, k])
            h[d, k] = ar.dot(terms, np.ones(terms.shape, ar.wt))
            s[d, k] = np.sum(np.abs(terms.astype(np.clongdouble)))
    return h, s


# ------------------------------------------------------------------------------- the small dense part
def hessenberg_qr(ar, gsin, gcos, residual_norm, rnc, hcol, it, final_iter_nums, stop):
    """one call of common_gmres::hessenberg_qr on the (it + 2) x nrhs column hcol: the replay of the `it`
    earlier rotations, the new rotation (c = 0, s = 1 on a zero pivot, else from the scaled hypotenuse), the
    next residual norm and the final_iter_nums increment; stopped columns keep everything.  Returns new
    (gsin, gcos, residual_norm, rnc, hcol, final_iter_nums)"""
    gsin, gcos, rnc, h = (ar.a(z).copy() for z in (gsin, gcos, rnc, hcol))
    rn = np.array(residual_norm, ar.rt).copy()
    fin = np.array(final_iter_nums, np.uint64).copy()
    act = (np.asarray(stop, np.uint8) & 0x3f) == 0
    if not np.any(act):
        return gsin, gcos, rn, rnc, h, fin
    fin[act] += np.uint64(1)
    for j in range(it):
        c, s = gcos[j, act], gsin[j, act]
        hj, hj1 = h[j, act], h[j + 1, act]
        temp = cr.add(ar, mul(ar, c, hj), mul(ar, s, hj1))
        h[j + 1, act] = cr.add(ar, mul(ar, -np.conj(s), hj), mul(ar, np.conj(c), hj1))
        h[j, act] = temp
    this_h, next_h = h[it, act], h[it + 1, act]
    zero = is_zero(this_h)
    with np.errstate(all="ignore"):
        scale = np.asarray(abs_v(ar, this_h) + abs_v(ar, next_h), ar.rt)
        a, b = abs_v(ar, div_real(ar, this_h, scale)), abs_v(ar, div_real(ar, next_h, scale))
        hyp = np.asarray(scale * np.sqrt(np.asarray(a * a + b * b, ar.rt)), ar.rt)
        c = np.where(zero, ar.wt(0), div_real(ar, np.conj(this_h), hyp)).astype(ar.wt)
        s = np.where(zero, ar.wt(1), div_real(ar, np.conj(next_h), hyp)).astype(ar.wt)
    gcos[it, act], gsin[it, act] = c, s
    h[it, act] = cr.add(ar, mul(ar, c, this_h), mul(ar, s, next_h))
    h[it + 1, act] = 0
    r = rnc[it, act]
    nxt = mul(ar, -np.conj(s), r)
    rnc[it + 1, act] = nxt
    rnc[it, act] = mul(ar, c, r)
    rn[act] = abs_v(ar, nxt)
    return gsin, gcos, rn, rnc, h, fin


def solve_krylov(ar, rnc, hess, final_iter_nums, stop, y0):
    """back substitution per column k with m = final_iter_nums[k] unknowns.  hess[j, i, k] = H(i, j) of column
    k - the krylov_dim x (krylov_dim + 1) nrhs layout reshaped to (krylov_dim, krylov_dim + 1, nrhs).
    Finalized columns and rows >= m keep what y0 holds"""
    rnc, hess = ar.a(rnc), ar.a(hess)
    y = ar.a(y0).copy()
    for k in range(y.shape[1]):
        if int(stop[k]) & 0x40:
            continue
        m = int(final_iter_nums[k])
        for i in range(m - 1, -1, -1):
            temp = rnc[i:i + 1, k].copy()
            for j in range(i + 1, m):
                temp = np.asarray(temp - mul(ar, hess[j, i, k:k + 1], y[j, k:k + 1]), ar.wt)
            y[i, k] = div(ar, temp, hess[i, i, k:k + 1])[0]
    return y


def sweep(ar, hraw, beta, stop_from=None, finalized=()):
    """krylov_dim steps of hessenberg_qr on the raw Hessenberg columns hraw[it] ((it + 2) x nrhs), started from
    rnc[0] = beta, then solve_krylov.  stop_from: {column: first iteration at which it counts as stopped}.
    Returns dict(gsin, gcos, rn, rnc, hess (kd, kd + 1, nrhs), fin, y)"""
    kd, nrhs = len(hraw), hraw[0].shape[1]
    gsin, gcos = np.zeros((kd, nrhs), ar.wt), np.zeros((kd, nrhs), ar.wt)
    rnc = np.zeros((kd + 1, nrhs), ar.wt)
    rnc[0] = ar.a(beta)
    rn = np.asarray(np.abs(np.asarray(beta)), ar.rt)
    fin = np.zeros(nrhs, np.uint64)
    hess = np.zeros((kd, kd + 1, nrhs), ar.wt)
    for it in range(kd):
        stop = np.zeros(nrhs, np.uint8)
        for col, first in (stop_from or {}).items():
            if it >= first:
                stop[col] = STOPPED
        gsin, gcos, rn, rnc, h, fin = hessenberg_qr(ar, gsin, gcos, rn, rnc, hraw[it], it, fin, stop)
        hess[it, :it + 2] = h
    stop = np.zeros(nrhs, np.uint8)
    for col in finalized:
        stop[col] = FINALIZED
    y = solve_krylov(ar, rnc, hess, fin, stop, np.zeros((kd, nrhs), ar.wt))
    return dict(gsin=gsin, gcos=gcos, rn=rn, rnc=rnc, hess=hess, fin=fin, y=y)


def hessenberg_case(seed, t, kd, nrhs, zero_pivot=None):
    """raw upper-Hessenberg columns hraw[it] ((it + 2) x nrhs, value type t), uniform in [-1, 1] (both parts for
    complex types), with the diagonal entry (it, it) pushed away from zero by 3 in the direction of its real part,
    which keeps the least-squares problems well conditioned, and beta (nrhs, real positive).
    zero_pivot = (it, column): that column's entry (it, it) is made to rotate to exactly zero, by zeroing its
    whole leading part: hraw[it][:it + 1, column] = 0"""
    rng = np.random.default_rng(seed)
    cx = br.is_complex(t)
    hraw = []
    for it in range(kd):
        v = rng.uniform(-1, 1, (it + 2, nrhs))
        if cx:
            v = v + 1j * rng.uniform(-1, 1, (it + 2, nrhs))
        v[it] += 3 * np.sign(v[it].real)
        if zero_pivot is not None and zero_pivot[0] == it:
            v[:it + 1, zero_pivot[1]] = 0
        hraw.append(v.astype(t))
    beta = rng.uniform(0.5, 2, nrhs).astype(br.real_of(t))
    return hraw, beta


def dense_hessenberg(hraw, k):
    """the (kd + 1) x kd matrix H of column k (long double)"""
    kd = len(hraw)
    H = np.zeros((kd + 1, kd), np.clongdouble if np.iscomplexobj(hraw[0]) else np.longdouble)
    for it in range(kd):
        H[:it + 2, it] = hraw[it][:, k]
    return H


def lstsq_hp(H, rhs):
    """min ||rhs - H y|| in long double by Householder reflections (no rotation, no code shared with the
    restatements above); returns (y, ||rhs - H y||)"""
    cx = np.iscomplexobj(H) or np.iscomplexobj(rhs)
    wt = np.clongdouble if cx else np.longdouble
    R, q = np.array(H, wt), np.array(rhs, wt)
    rows, cols = R.shape
    for j in range(cols):
        x = R[j:, j].copy()
        alpha = np.sqrt(np.sum(np.abs(x) ** 2))
        if alpha == 0:
            continue
        phase = x[0] / np.abs(x[0]) if x[0] != 0 else wt(1)
        x[0] += phase * alpha
        v = x / np.sqrt(np.sum(np.abs(x) ** 2))
        R[j:, j:] -= 2 * np.outer(v, np.conj(v) @ R[j:, j:])
        q[j:] -= 2 * v * (np.conj(v) @ q[j:])
    y = np.zeros(cols, wt)
    for i in range(cols - 1, -1, -1):
        y[i] = (q[i] - R[i, i + 1:cols] @ y[i + 1:]) / R[i, i]
    return y, np.longdouble(np.sqrt(np.sum(np.abs(q[cols:]) ** 2)))


# --------------------------------------------------------------------------------- the two tree sums
def _wave_sum(v):
    """wave_sum of common.hpp on an array (..., 64): v += shfl_xor(v, off) for off = 32 .. 1; lane 0's value"""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ off]).astype(v.dtype)
    return v[..., 0]


def _block_sum(v):
    """block_sum<BLOCK> on an array (..., BLOCK): wave_sum per wave, then wave_sum of the BLOCK / 64 wave sums
    padded with zeros to 64 lanes"""
    waves = v.shape[-1] // 64
    w = _wave_sum(v.reshape(v.shape[:-1] + (waves, 64)))
    pad = np.zeros(w.shape[:-1] + (64,), v.dtype)
    pad[..., :waves] = w
    return _wave_sum(pad)


def multi_dot_depth(rows):
    """additions on the longest path of gkoc_gmres_multi_dot.  Stage 1: a block takes 1024 rows, every thread
    adds its md_items = 4 products in turn to acc = 0 (4 additions); block_sum<256> is wave_sum (6 butterfly
    levels) and one more wave_sum over the four wave sums, of which only 2 levels add non-zero values (8).  Stage
    2: a thread adds its ceil(nb / 256) partials in turn, nb = ceil(rows / 1024), then block_sum<256> again (8)"""
    nb = -(-max(rows, 1) // 1024)
    return 4 + 8 + -(-nb // 256) + 8


def mgs_blocks(rows):
    return min(-(-rows // 2048), 2048)


def mgs_step_depth(rows, width, vec_ok=True):
    """additions on the longest path of h_next of gkoc_x_gmres_mgs_step.  The kernel starts nb = min(ceil(rows /
    2048), 2048) blocks of 256 threads.  With aligned pointers a thread takes every (256 nb)-th vector of `width`
    = 16 / sizeof(T) entries and adds their products in turn: width * ceil((rows / width) / (256 nb)) additions,
    and at most one more for the scalar tail rows % width; otherwise ceil(rows / (256 nb)).  block_sum<256> adds
    8 levels; fold_partials (fused.hpp) folds the nb <= 2048 <= fold_single_max partials in one block of 1024
    threads: ceil(nb / 1024) in turn, then block_sum<1024>: 6 levels and 4 for the sixteen wave sums.

    The constant c of the acceptance |got - hp| <= (depth + c) eps sum |terms| covers the roundings inside one
    term (`term_roundings`)."""
    nb = mgs_blocks(max(rows, 1))
    per = 256 * nb
    if vec_ok:
        mine = width * -(-(rows // width) // per) + (1 if rows % width else 0)
    else:
        mine = -(-rows // per)
    return mine + 8 + -(-nb // 1024) + 10


def term_roundings(t):
    """c: the error of one computed term in units of eps |term|, rounded up to an integer.  Real: one rounded
    product, eps / 2 -> 1.  Complex: each part of the textbook product is two rounded products and one rounded
    sum, at most (eps / 2)(2 + eps) (|ac| + |bd|) <= about eps |x| |y| per part by Cauchy-Schwarz, so sqrt(2)
    eps in modulus -> 2.  (Every addition of the tree is charged a whole eps of sum |terms| although it rounds
    by eps / 2 of a partial sum: that factor of two absorbs the second-order terms.)"""
    return 2 if br.is_complex(t) else 1


def dot_bound(t, depth, sum_abs_terms):
    return (depth + term_roundings(t)) * br.eps_of(t) * np.longdouble(sum_abs_terms)


def multi_dot_tree(t, basis_d, nxt):
    """emulation of the two stages for one (dot, column) in the value type: returns the kernel's sum"""
    t = np.dtype(t).type
    ar = br.plain(t)
    rows = nxt.shape[0]
    nb = -(-rows // 1024)
    terms = np.zeros(nb * 1024, t)
    terms[:rows] = mul(ar, np.conj(ar.a(basis_d)), ar.a(nxt))
    terms = terms.reshape(nb, 4, 256)
    acc = np.zeros((nb, 256), t)
    for u in range(4):
        acc = (acc + terms[:, u]).astype(t)
    partial = _block_sum(acc)
    trips = -(-nb // 256)
    p = np.zeros(trips * 256, t)
    p[:nb] = partial
    p = p.reshape(trips, 256)
    acc = np.zeros(256, t)
    for i in range(trips):
        acc = (acc + p[i]).astype(t)
    return _block_sum(acc)


def vec_width(t):
    return 16 // np.dtype(t).itemsize


def mgs_dot_tree(t, w_new, v_next, vec_ok=True):
    """emulation of h_next of gmres_mgs_step_kernel + fold_partials in the value type, from the updated w"""
    t = np.dtype(t).type
    ar = br.plain(t)
    n = w_new.shape[0]
    W = vec_width(t)
    nb = mgs_blocks(n)
    per = 256 * nb
    terms = mul(ar, np.conj(ar.a(v_next)), ar.a(w_new))
    acc = np.zeros(per, t)
    done = 0
    if vec_ok:
        n_vec = n // W
        trips = -(-n_vec // per)
        tv = np.zeros(trips * per * W, t)
        tv[:n_vec * W] = terms[:n_vec * W]
        tv = tv.reshape(trips, per, W)
        for i in range(trips):
            for e in range(W):
                acc = (acc + tv[i, :, e]).astype(t)
        done = n_vec * W
    rest = terms[done:]
    trips = -(-rest.shape[0] // per)
    tr = np.zeros(trips * per, t)
    tr[:rest.shape[0]] = rest
    for row in tr.reshape(trips, per):
        acc = (acc + row).astype(t)
    partial = _block_sum(acc.reshape(nb, 256))
    trips = -(-nb // 1024)
    p = np.zeros(trips * 1024, t)
    p[:nb] = partial
    acc = np.zeros(1024, t)
    for row in p.reshape(trips, 1024):
        acc = (acc + row).astype(t)
    return _block_sum(acc)


# ------------------------------------------------------------------------------- inputs of the tests
MULTI_DOT_ROWS = (0, 1, 1023, 1024, 1025, 2049, 100003, 263169)
MGS_ROWS = (0, 1, 2, 3, 5, 2047, 2048, 100003, 4196353)
MGS_BIG_TYPES = ("f32", "c128")           # the block cap: two types are enough
SINGLE_TEETH_LIMIT = 100003               # above it, in single precision, the bound exceeds one product


def rand(rng, shape, t):
    v = rng.uniform(-1, 1, shape)
    return (v + 1j * rng.uniform(-1, 1, shape)).astype(t) if br.is_complex(t) else v.astype(t)


def ints(rng, shape, t):
    """entries in {-1, 0, 1}, or Gaussian integers with such parts"""
    v = rng.integers(-1, 2, shape).astype(np.float64)
    return (v + 1j * rng.integers(-1, 2, shape)).astype(t) if br.is_complex(t) else v.astype(t)


_TN_ID = {"f64": 1, "f32": 2, "c128": 3, "c64": 4}


def multi_dot_case(tn, rows, num, nrhs, exact=False):
    """basis (num, rows, nrhs) and next (rows, nrhs) of the multi_dot tests"""
    t = br.TYPES[tn]
    rng = np.random.default_rng([11, _TN_ID[tn], rows, num, nrhs, int(exact)])
    gen = ints if exact else rand
    return gen(rng, (num, rows, nrhs), t), gen(rng, (rows, nrhs), t)


def mgs_case(tn, rows, zero_h=False, exact=False):
    """w, v_cur, h_cur, v_next of the mgs_step tests"""
    t = br.TYPES[tn]
    rng = np.random.default_rng([13, _TN_ID[tn], rows, int(zero_h), int(exact)])
    gen = ints if exact else rand
    w, v_cur, v_next = (gen(rng, (rows,), t) for _ in range(3))
    if zero_h:
        h = t(0)
    elif exact:
        h = t(1 - 1j) if br.is_complex(t) else t(2)
    else:
        h = rand(rng, (1,), t)[0]
    return w, v_cur, h, v_next


def needs_exact(tn, rows):
    """single precision above SINGLE_TEETH_LIMIT rows: the depth bound is wider than a product of median size,
    so these (type, size) pairs also get an integer-valued case that demands equality"""
    return tn in ("f32", "c64") and rows > SINGLE_TEETH_LIMIT
