"""Matrices, exact reference and error bound of tests/test_csr_spmv_branches_gpu.py (checked on the CPU by
tests/test_csr_spmv_cases_cpu.py).

Rows of at most GKOC_CSR_LONG_ROW = 4096 entries are summed in entry order by every CSR kernel and compared bit
for bit with the sequential oracle.  Longer rows ("hub rows") are summed in another order by two of the kernels:

  * the wave path (csr_spmv_pipe.hpp / csr_spmv_multi.hpp, `is_long`): lane l adds the products l, l + 64, ...
    of the row - ceil(len / 64) additions - and wave_sum adds 6 levels;
  * the flagged path (csr_long_rows.hpp): the row is cut into 64 chunks, a thread adds at most
    ceil(len / 16384) products, the workgroup tree adds 8 levels, the fold adds the 64 chunk sums.

With one rounding for a product, one for alpha, one for beta c and one for the last addition either path stays
within D = ceil(len / 64) + 80 roundings of the value type, each at most eps times the sum S of the magnitudes:

    |got - exact| <= D eps S,   S = |alpha| sum_k |v_k b_k| + |beta c_i|,   D = ceil(len / 64) + 80.

The file is compiled with -ffp-contract=off, so no product is fused into an addition.  `exact` is the sum of the
products of the exactly widened factors, accumulated in np.longdouble.
"""
import functools
from collections import namedtuple

import numpy as np

LONG_ROW = 4096            # GKOC_CSR_LONG_ROW
LONG_MAX_PER_SEG = 8       # csr_long_rows.hpp: long rows of one segment that are cut into chunks
LONG_LIST_CAP = 4096       # csr_structure.hip long_list_cap
LONG_CACHE_CAP = 128       # csr_structure.hip long_cache_cap

Mat = namedtuple("Mat", "rp ci v lens shape")
Ref = namedtuple("Ref", "seq hubs exact S")     # seq (n, k); hubs (h,); exact, S (h, k) in np.longdouble


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def hub_rows(m):
    return np.flatnonzero(m.lens > LONG_ROW)


# ------------------------------------------------------------------ builders
def hub_matrix(seed, n, ncols, hubs, dtype=np.float64, idx=np.int32, max_short=13):
    """rows of 0 .. max_short entries, `hubs` = ((row, length), ...); sorted distinct columns per row"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_short + 1, n)
    for r, l in hubs:
        lens[r] = l
    rp = np.concatenate(([0], np.cumsum(lens))).astype(idx)
    ci = np.concatenate([np.sort(rng.choice(ncols, l, replace=False)) for l in lens]).astype(idx)
    v = rng.uniform(-1, 1, len(ci)).astype(dtype)
    return Mat(rp, ci, v, lens, (n, ncols))


def banded_matrix(seed, n, max_len, hubs=(), dtype=np.float64, idx=np.int32):
    """square, row r holds the columns r, r + 3, r + 6, ... (mod n; a row that wraps is not sorted, which
    csr::spmv does not ask for); built with arrays, for the sizes where a loop over the rows is too slow"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n)
    for r, l in hubs:
        lens[r] = l
    rp64 = np.concatenate(([0], np.cumsum(lens)))
    off = np.arange(rp64[-1]) - np.repeat(rp64[:-1], lens)
    ci = ((np.repeat(np.arange(n), lens) + 3 * off) % n).astype(idx)
    v = rng.uniform(-1, 1, len(ci)).astype(dtype)
    return Mat(rp64.astype(idx), ci, v, lens, (n, n))


A_ROWS, A_COLS = 64 * 5 + 11, 12000
A_HUBS = ((3, 4097), (4, 4096), (64 * 2 + 63, 9000), (A_ROWS - 1, 5000))


@functools.lru_cache(maxsize=None)
def case_a(dtype=np.float64, idx=np.int32):
    """cases a and b: 331 rows, 4097 entries at row 3, 4096 (NOT long) at row 4, 9000 at the last row of
    segment 2, 5000 at the last row of the matrix (a last segment of 11 rows)"""
    return hub_matrix(101, A_ROWS, A_COLS, A_HUBS, dtype, idx)


C_ROWS, C_COLS = 64 * 3 + 20, 12000
# ten rows beyond 4096 in segment 1 (rows 64 .. 127), the ninth and tenth in row order are 120 (4097 entries, one
# round of the stage and one entry) and 127 (9000 entries, three rounds); one hub in the last segment of 20 rows
C_HUBS = ((64, 4097), (69, 4200), (70, 5000), (71, 4097), (84, 6000), (85, 4100), (104, 8193), (105, 4300),
          (120, 4097), (127, 9000), (66, 4096), (67, 170), (64 * 3 + 7, 4500))
C_STAGED = (120, 127)


@functools.lru_cache(maxsize=None)
def case_c(dtype=np.float64, idx=np.int32):
    return hub_matrix(102, C_ROWS, C_COLS, C_HUBS, dtype, idx)


def case_d(n_seg, dtype=np.float32, idx=np.int32):
    """64 * n_seg rows, row 64 s + (s % 64) has the columns 0 .. 4096, every other row is empty"""
    n = 64 * n_seg
    lens = np.zeros(n, np.int64)
    lens[64 * np.arange(n_seg) + np.arange(n_seg) % 64] = LONG_ROW + 1
    rp = np.concatenate(([0], np.cumsum(lens))).astype(idx)
    ci = np.tile(np.arange(LONG_ROW + 1, dtype=idx), n_seg)
    v = (np.random.default_rng(104).random(len(ci), dtype=np.float32) * 2 - 1).astype(dtype)
    return Mat(rp, ci, v, lens, (n, LONG_ROW + 1))


E_ROWS, E_COLS = 64 * 5 + 7, 12000
E_HUBS = (
    ((64 * 0 + 9, 5000), (64 * 3 + 63, 4097)),                                   # 1: segments 0 and 3
    (),                                                                          # 2: none
    ((64 * 1 + 2, 4500), (64 * 4 + 0, 6000)),                                    # 3: segments 1 and 4 only
    tuple((r, 4097 + 100 * i) for i, r in enumerate((0, 1, 5, 17, 18, 30, 31, 40, 62, 63))),   # 4: ten in segment 0
    ((64 * 2 + 1, 7000), (E_ROWS - 1, 4200)),                                    # 5: another matrix, same n_rows
)
E_STAGED = (62, 63)      # the ninth and tenth long row of matrix 4


@functools.lru_cache(maxsize=None)
def case_e(which, dtype=np.float64, idx=np.int32):
    return hub_matrix(200 + which, E_ROWS, E_COLS, E_HUBS[which], dtype, idx)


@functools.lru_cache(maxsize=None)
def case_evict(i, dtype=np.float64, idx=np.int32):
    """64 rows, one hub of 4097 entries at row i % 64, values of their own"""
    return hub_matrix(1000 + i, 64, 6000, ((i % 64, LONG_ROW + 1),), dtype, idx)


@functools.lru_cache(maxsize=None)
def case_capture(which):
    """like case_a, with a number of rows no other matrix of the suite has: the cache's key holds n_rows, so an
    entry left by an earlier matrix at the same address cannot stand in for this one"""
    n = 64 * 5 + 13 + which
    return hub_matrix(400 + which, n, A_COLS, ((3, 4097), (4, 4096), (64 * 2 + 63, 9000), (n - 1, 5000)))


F_ROWS = 64 * 150 + 11


@functools.lru_cache(maxsize=None)
def case_f(dtype=np.float64, idx=np.int32):
    """square (the fused product and dot), hubs in the first, a middle and the last (short) segment"""
    hubs = ((2, 4097), (64 * 70 + 63, 9000), (F_ROWS - 1, 5000))
    return hub_matrix(106, F_ROWS, F_ROWS, hubs, dtype, idx)


H_ROWS_AUTO = 64 * 8192


@functools.lru_cache(maxsize=None)
def case_h_auto():
    """8192 segments = 8192 waves and two hubs: the automatic XCD-contiguous wave order"""
    return banded_matrix(108, H_ROWS_AUTO, 5, ((70, 5000), (H_ROWS_AUTO - 3, 4097)))


# ------------------------------------------------------------------ reference and bound
def depth(lens):
    return -(-np.asarray(lens, np.int64) // 64) + 80


def exact_rows(m, rows, b, alpha=None, beta=None, c=None):
    """(exact, S) of the rows `rows` of alpha A b + beta c in np.longdouble, one column per column of b;
    beta == 0 does not read c"""
    b2 = np.asarray(b).reshape(len(b), -1)
    exact = np.zeros((len(rows), b2.shape[1]), np.longdouble)
    mag = np.zeros_like(exact)
    for i, r in enumerate(rows):
        k0, k1 = int(m.rp[r]), int(m.rp[r + 1])
        p = m.v[k0:k1].astype(np.longdouble)[:, None] * b2[m.ci[k0:k1]].astype(np.longdouble)
        exact[i], mag[i] = p.sum(axis=0), np.abs(p).sum(axis=0)
    if alpha is not None:
        exact *= np.longdouble(alpha)
        mag *= abs(np.longdouble(alpha))
        if beta != 0:
            bc = np.longdouble(beta) * np.asarray(c).reshape(m.shape[0], -1)[rows].astype(np.longdouble)
            exact += bc
            mag += np.abs(bc)
    return exact, mag


def reference(oracle, m, b, alpha=None, beta=None, c=None):
    """the sequential oracle in the arithmetic type (values narrower than b are widened first: the mixed
    product) and the exact value of the hub rows"""
    v = m.v if m.v.dtype == np.asarray(b).dtype else m.v.astype(np.asarray(b).dtype)
    seq = oracle.csr_spmv(m.rp, m.ci, v, b, alpha=alpha, beta=beta, c=c)
    hubs = hub_rows(m)
    exact, mag = exact_rows(m, hubs, b, alpha, beta, c)
    return Ref(seq.reshape(m.shape[0], -1), hubs, exact, mag)


def bound(m, ref, eps):
    return depth(m.lens[ref.hubs])[:, None] * np.longdouble(eps) * ref.S


def judge(got, ref, m, bitwise=()):
    """got (n, k) against ref: every row of at most 4096 entries and every row in `bitwise` equal to the
    sequential oracle bit for bit, every other hub row within the bound.  Returns the largest
    |got - exact| / (eps S) over the bounded rows (0.0 if there are none)."""
    got = np.asarray(got).reshape(m.shape[0], -1)
    eps = eps_of(got.dtype)
    exact_rows_ = np.ones(m.shape[0], bool)
    sel = np.array([r not in bitwise for r in ref.hubs], bool)
    exact_rows_[ref.hubs[sel]] = False
    assert np.array_equal(got[exact_rows_], ref.seq[exact_rows_]), \
        ("rows summed in entry order differ from the oracle",
         np.flatnonzero((got != ref.seq).any(axis=1) & exact_rows_)[:8])
    if not sel.any():
        return 0.0
    err = np.abs(got[ref.hubs].astype(np.longdouble) - ref.exact)[sel]
    lim = bound(m, ref, eps)[sel]
    ratio = err / (np.longdouble(eps) * ref.S[sel])
    assert np.all(err <= lim), ("hub rows outside D eps S", ref.hubs[sel], np.asarray(ratio, float),
                                depth(m.lens[ref.hubs[sel]]))
    return float(ratio.max())


def judge_statistical(got, ref, m, b, c=None, advanced=False):
    """the tighter bound of tests/test_spmv_gpu.py and tests/test_flan_like_gpu.py on double hub rows, against the
    sequential oracle: 1e-15 scale sqrt(len), advanced 2e-15 (scale + |c|) sqrt(len), scale = sum |v_k b_k|"""
    got = np.asarray(got).reshape(m.shape[0], -1)
    _, scale = exact_rows(m, ref.hubs, b)
    scale = np.asarray(scale, np.float64)
    root = np.sqrt(m.lens[ref.hubs])[:, None]
    if advanced:
        if c is not None:
            scale = scale + np.abs(np.asarray(c).reshape(m.shape[0], -1)[ref.hubs])
        lim = 2e-15 * scale * root
    else:
        lim = 1e-15 * scale * root
    assert np.all(np.abs(got[ref.hubs] - ref.seq[ref.hubs]) <= lim)


def drop_median_product(m, row, b):
    """one-row matrix: hub row `row` without its product of median magnitude (one column of b)"""
    k0, k1 = int(m.rp[row]), int(m.rp[row + 1])
    p = np.abs(m.v[k0:k1].astype(np.longdouble) * np.asarray(b)[m.ci[k0:k1]].astype(np.longdouble))
    keep = np.ones(k1 - k0, bool)
    keep[np.argsort(p)[len(p) // 2]] = False
    rp = np.array([0, keep.sum()], m.rp.dtype)
    return Mat(rp, m.ci[k0:k1][keep], m.v[k0:k1][keep], np.array([keep.sum()]), (1, m.shape[1]))
