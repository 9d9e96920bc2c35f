"""The arithmetic contract of the batched solvers (include/gko_cdna4.h, "Batched solvers") restated in numpy:
the product, the reduction R_W with W as a parameter, scalar Jacobi, Cg, Bicgstab and the values-only
conversions.  Everything is vectorised over the items and over the W lanes, every operation stays in the value
type of its inputs, and nothing is fused, so the kernels' results can be compared with np.array_equal.
Not a test module: tests/test_batch_refs_cpu.py checks it, tests/test_batch_gpu.py uses it."""
import numpy as np


def width(n):
    """the W of a system with n rows (what gkoc_batch_plan reports)"""
    return 64 if n <= 64 else 128 if n <= 128 else 256 if n <= 768 else 512


def reduce_w(t, w):
    """R_W over the last axis: p_l = ((+0 + t_l) + t_{l+W}) + ..., then p_l = p_l + p_{l+d} for d = W/2 .. 1.
    The lanes that run out of terms early are padded with +0, which changes no bit: a partial is never -0."""
    t = np.asarray(t)
    n = t.shape[-1]
    terms = max(-(-n // w), 1)
    pad = np.zeros(t.shape[:-1] + (terms * w,), t.dtype)
    pad[..., :n] = t
    pad = pad.reshape(t.shape[:-1] + (terms, w))
    p = np.zeros(t.shape[:-1] + (w,), t.dtype)
    for j in range(terms):
        p = p + pad[..., j, :]
    d = w // 2
    while d >= 1:
        p = p[..., :d] + p[..., d:2 * d]
        d //= 2
    return p[..., 0]


def dot(u, v, w):
    return reduce_w(u * v, w)


def nrm(u, w):
    return np.sqrt(reduce_w(u * u, w))


class CsrPattern:
    """one pattern for all items; values: items x nnz"""
    format = "csr"

    def __init__(self, n_rows, n_cols, row_ptrs, col_idxs):
        self.size = (int(n_rows), int(n_cols))
        self.rp, self.ci = np.asarray(row_ptrs, np.int64), np.asarray(col_idxs, np.int64)
        self.stored = len(self.ci)
        self.lens = np.diff(self.rp)

    def slots(self):
        """for k = 0, 1, ...: (rows that have a k-th stored entry, its position in the values, its column)"""
        for k in range(int(self.lens.max()) if len(self.lens) else 0):
            rows = np.flatnonzero(self.lens > k)
            at = self.rp[rows] + k
            yield rows, at, self.ci[at]


class EllPattern:
    """col_idxs: slots x stride, column-major storage (entry (row, k) at row + k * stride), padding -1;
    values: items x (slots * stride)"""
    format = "ell"

    def __init__(self, n_rows, n_cols, col_idxs, num_stored_per_row, stride):
        self.size = (int(n_rows), int(n_cols))
        self.k, self.stride = int(num_stored_per_row), int(stride)
        self.cols = np.asarray(col_idxs, np.int64).reshape(self.k, self.stride)
        self.stored = self.k * self.stride

    def slots(self):
        for k in range(self.k):
            rows = np.flatnonzero(self.cols[k, :self.size[0]] >= 0)
            yield rows, rows + k * self.stride, self.cols[k, rows]


def product(pat, vals, u):
    """y = A u for every item: vals items x stored, u items x n_cols (x cols); the sequential sum from +0 over
    the stored entries of a row in storage order"""
    y = np.zeros((vals.shape[0], pat.size[0]) + u.shape[2:], vals.dtype)
    for rows, at, cols in pat.slots():
        v = vals[:, at]
        if u.ndim == 3:
            v = v[:, :, None]
        y[:, rows] = y[:, rows] + v * u[:, cols]
    return y


def advanced_product(pat, vals, alpha, u, beta, x):
    """x = (alpha * (A u)) + (beta * x), alpha and beta one per item"""
    shape = (-1,) + (1,) * (x.ndim - 1)
    return alpha.reshape(shape) * product(pat, vals, u) + beta.reshape(shape) * x


def jacobi(pat, vals):
    """dinv: 1 / a_ii of the first stored entry (i, i); 1 where none is stored or it is 0"""
    d = np.zeros((vals.shape[0], pat.size[0]), vals.dtype)
    found = np.zeros(pat.size[0], bool)
    for rows, at, cols in pat.slots():
        hit = (cols == rows) & ~found[rows]
        d[:, rows[hit]] = vals[:, at[hit]]
        found[rows[hit]] = True
    with np.errstate(all="ignore"):
        return np.where(d == 0, vals.dtype.type(1), vals.dtype.type(1) / d)


def _threshold(b, w, tol, tol_type):
    t = b.dtype.type(tol)
    if tol_type == "relative":
        return t * nrm(b, w)
    assert tol_type == "absolute"
    return np.full(b.shape[0], t, b.dtype)


def _stop(res, tau, it, max_it):
    return (res <= tau) | np.isnan(res) | (it == max_it)


def cg(pat, vals, b, x0, w, tol, tol_type, max_it, precond=None):
    """-> x, iteration counts, residual norms, converged; b, x0: items x n"""
    with np.errstate(all="ignore"):
        dinv = jacobi(pat, vals) if precond == "jacobi" else None
        m = (lambda r, a: dinv[a] * r) if dinv is not None else (lambda r, a: r)
        everyone = np.arange(vals.shape[0])
        x = x0.copy()
        tau = _threshold(b, w, tol, tol_type)
        r = b - product(pat, vals, x)
        z = m(r, everyone)
        p = z.copy()
        rho = dot(r, z, w)
        res = nrm(r, w)
        it = np.zeros(vals.shape[0], np.int32)
        active = ~_stop(res, tau, it, max_it)
        while active.any():
            a = np.flatnonzero(active)
            t = product(pat, vals[a], p[a])
            alpha = rho[a] / dot(p[a], t, w)
            x[a] = x[a] + alpha[:, None] * p[a]
            r[a] = r[a] - alpha[:, None] * t
            res[a] = nrm(r[a], w)
            it[a] += 1
            active[a] = ~_stop(res[a], tau[a], it[a], max_it)
            a = a[active[a]]
            z = m(r[a], a)
            rho_new = dot(r[a], z, w)
            beta = rho_new / rho[a]
            p[a] = z + beta[:, None] * p[a]
            rho[a] = rho_new
        return x, it, res, (res <= tau).astype(np.int32)


def bicgstab(pat, vals, b, x0, w, tol, tol_type, max_it, precond=None):
    with np.errstate(all="ignore"):
        dinv = jacobi(pat, vals) if precond == "jacobi" else None
        m = (lambda r, a: dinv[a] * r) if dinv is not None else (lambda r, a: r)
        one = vals.dtype.type(1)
        items = vals.shape[0]
        x = x0.copy()
        tau = _threshold(b, w, tol, tol_type)
        r = b - product(pat, vals, x)
        r_hat = r.copy()
        p, v = np.zeros_like(r), np.zeros_like(r)
        rho_old, alpha, omega = (np.full(items, one, vals.dtype) for _ in range(3))
        res = nrm(r, w)
        it = np.zeros(items, np.int32)
        active = ~_stop(res, tau, it, max_it)
        while active.any():
            a = np.flatnonzero(active)
            rho = dot(r_hat[a], r[a], w)
            beta = (rho / rho_old[a]) * (alpha[a] / omega[a])
            p[a] = r[a] + beta[:, None] * (p[a] - omega[a][:, None] * v[a])
            p_hat = m(p[a], a)
            v[a] = product(pat, vals[a], p_hat)
            alpha[a] = rho / dot(r_hat[a], v[a], w)
            s = r[a] - alpha[a][:, None] * v[a]
            res[a] = nrm(s, w)
            early = (res[a] <= tau[a]) | np.isnan(res[a])
            e = a[early]
            x[e] = x[e] + alpha[e][:, None] * p_hat[early]
            it[e] += 1
            active[e] = False
            go = ~early
            a, s, p_hat, rho = a[go], s[go], p_hat[go], rho[go]
            s_hat = m(s, a)
            t = product(pat, vals[a], s_hat)
            omega[a] = dot(t, s, w) / dot(t, t, w)
            x[a] = (x[a] + alpha[a][:, None] * p_hat) + omega[a][:, None] * s_hat
            r[a] = s - omega[a][:, None] * t
            res[a] = nrm(r[a], w)
            rho_old[a] = rho
            it[a] += 1
            active[a] = ~_stop(res[a], tau[a], it[a], max_it)
        return x, it, res, (res <= tau).astype(np.int32)


SOLVERS = {"cg": cg, "bicgstab": bicgstab}


# ---------------------------------------------------------------------------------- conversions
def csr_to_ell(pat, vals, stride=None):
    """-> EllPattern, values items x (slots * stride): the k-th stored entry of row i at i + k * stride, padding
    column -1 and value 0"""
    n = pat.size[0]
    stride = n if stride is None else stride
    k = int(pat.lens.max()) if n else 0
    cols = np.full((k, stride), -1, np.int32)
    out = np.zeros((vals.shape[0], k, stride), vals.dtype)
    for j, (rows, at, c) in enumerate(pat.slots()):
        cols[j, rows] = c
        out[:, j, rows] = vals[:, at]
    return EllPattern(n, pat.size[1], cols, k, stride), out.reshape(vals.shape[0], k * stride)


def ell_to_csr(pat, vals):
    """-> CsrPattern, values items x nnz: the stored slots of a row in slot order, padding skipped"""
    n = pat.size[0]
    stored = pat.cols[:, :n] >= 0                        # slots x rows
    rp = np.concatenate([[0], np.cumsum(stored.sum(axis=0))]).astype(np.int32)
    k_of, row_of = np.nonzero(stored.T)[1], np.nonzero(stored.T)[0]     # row-major over (row, slot)
    ci = pat.cols[k_of, row_of].astype(np.int32)
    return CsrPattern(n, pat.size[1], rp, ci), vals[:, row_of + k_of * pat.stride]


# ---------------------------------------------------------------------------------- test problems
def tridiagonal(n, items, dtype, seed=0, dominance=2.5, symmetric=False):
    """the per-item perturbed 3-point stencil: CsrPattern and items x nnz values, diagonally dominant"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), 3)
    cols = rows + np.tile([-1, 0, 1], n)
    keep = (cols >= 0) & (cols < n)
    rows, cols = rows[keep], cols[keep]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    vals = np.where(rows == cols, dominance, -1.0)[None, :] * (1 + 0.2 * rng.uniform(0, 1, (items, len(rows))))
    if symmetric:
        # the entry (i, i+1) takes the value of (i+1, i)
        lower = np.flatnonzero(cols == rows - 1)
        upper = np.flatnonzero(cols == rows + 1)
        vals[:, upper] = vals[:, lower]
        vals[:, rows == cols] += 0.5
    return CsrPattern(n, n, rp, cols.astype(np.int32)), np.ascontiguousarray(vals.astype(dtype))


def random_pattern(n_rows, n_cols, density, seed, empty_rows=()):
    """a random CsrPattern with unsorted rows and the given rows empty"""
    rng = np.random.default_rng(seed)
    mask = rng.uniform(0, 1, (n_rows, n_cols)) < density
    mask[list(empty_rows)] = False
    rp, ci = [0], []
    for i in range(n_rows):
        c = np.flatnonzero(mask[i])
        rng.shuffle(c)
        ci.extend(c)
        rp.append(len(ci))
    return CsrPattern(n_rows, n_cols, np.array(rp, np.int32), np.array(ci, np.int32))
