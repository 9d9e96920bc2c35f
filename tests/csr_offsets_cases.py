"""Host model, matrices and shared helpers of the tests of the CSR column-offset plan (csrc/csr_offsets.hpp, the
launcher in csrc/csr_spmv.hip, the plan cache in csrc/csr_structure.hip): tests/test_csr_offsets_gpu.py,
tests/test_csr_offsets_routes_gpu.py.  The model and the builders are checked on the CPU by tests/test_csr_offsets_cases_cpu.py, so that a bug in a builder cannot make
a device case vacuous.

plan_model is the definition of csr_offsets.hpp:3-15 in plain loops: a 64-row segment is ELIGIBLE if every row
of it has strictly ascending columns and the union of `col - row` over the segment has 1 .. 32 values; D is that
number (0: not eligible - a segment without entries included), the offsets are the union in ascending order, a
row's mask has bit d set where it stores column row + off_d.  The launcher accepts the plan (state 1) iff
eligible > 0 and eligible * 100 >= segments * 50 (offsets_min_share), else it rejects it for good (state 2).

Nothing at module level needs a device; the helpers of the second half import the package when called.
"""
import contextlib
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

OFFS_MAX = 32              # csr_offsets.hpp: offsets per segment = bits of a row's mask
SEG = 64
MIN_SHARE = 50             # csr_structure.hip offsets_min_share, per cent
CACHE_CAP = 128            # csr_structure.hip offsets_cache_cap
CAP = SEG * OFFS_MAX       # entries of a segment's stage

KEY = 18                   # GKOC_TUNE_CSR_OFFSETS
KEY_LONG_ROWS = 12         # GKOC_TUNE_CSR_LONG_ROWS
KEY_SEGS_PER_WAVE = 13     # GKOC_TUNE_CSR_SEGS_PER_WAVE

Plan = namedtuple("Plan", "D offsets mask eligible segments state")


# ---------------------------------------------------------------- the model
def plan_model(rp, ci):
    n_rows = len(rp) - 1
    n_seg = -(-n_rows // SEG)
    D, offsets = [], []
    mask = np.zeros(n_rows, np.uint32)
    eligible = 0
    for s in range(n_seg):
        rows = range(s * SEG, min((s + 1) * SEG, n_rows))
        ok = True
        union = []
        for r in rows:
            last = None
            for k in range(int(rp[r]), int(rp[r + 1])):
                c = int(ci[k])
                if last is not None and c <= last:
                    ok = False
                last = c
                if c - r not in union:
                    union.append(c - r)
        union.sort()
        if not ok or len(union) == 0 or len(union) > OFFS_MAX:
            D.append(0)
            offsets.append([])
            continue
        for r in rows:
            m = 0
            for k in range(int(rp[r]), int(rp[r + 1])):
                m |= 1 << union.index(int(ci[k]) - r)
            mask[r] = m
        D.append(len(union))
        offsets.append(union)
        eligible += 1
    state = 1 if eligible > 0 and eligible * 100 >= n_seg * MIN_SHARE else 2
    return Plan(D, offsets, mask, eligible, n_seg, state)


# ---------------------------------------------------------------- matrices (host, int32)
def from_rows(rows, n_cols, dtype, seed=0):
    """rows: list of column lists in STORAGE order; values uniform in +-[0.5, 1.5)"""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c in r], np.int32)
    rng = np.random.default_rng(seed)
    v = (rng.uniform(0.5, 1.5, len(ci)) * rng.choice([-1.0, 1.0], len(ci))).astype(dtype)
    return (len(rows), n_cols), rp, ci, v


def band_rows(n, n_cols, offsets, first=0):
    return [[r + o for o in offsets if 0 <= r + o < n_cols] for r in range(first, first + n)]


def rows_of(m):
    _, rp, ci, _ = m
    return [[int(c) for c in ci[rp[r]:rp[r + 1]]] for r in range(len(rp) - 1)]


BANDED_D = (1, 7, 8, 9, 16, 17, 24, 25, 31, 32, 33)


def banded_offsets(D):
    """D distinct offsets, negative ones among them, not contiguous"""
    return [3 * i - 20 for i in range(D)]


def banded_rows(D):
    """192 rows x 320 columns.  Segments 0 and 2: tridiagonal.  Segment 1 (rows 64 .. 127): the union of col - row is
    exactly banded_offsets(D); row 64 + j stores a subset of 1 .. min(D, 32) of them (drawn per row), row 70 stores
    the first min(D, 32) and row 71 the last min(D, 32) (for D <= 32 both store ALL of them), row 100 is empty."""
    n, n_cols = 192, 320
    offs = banded_offsets(D)
    most = min(D, OFFS_MAX)
    rng = np.random.default_rng(100 + D)
    rows = band_rows(n, n_cols, (-1, 0, 1))
    for r in range(64, 128):
        count = int(rng.integers(1, most + 1))
        pick = sorted(rng.choice(D, count, replace=False).tolist())
        rows[r] = [r + offs[i] for i in pick]
    rows[70] = [70 + o for o in offs[:most]]
    rows[71] = [71 + o for o in offs[D - most:]]
    rows[100] = []
    return rows, n_cols


def banded(D, dtype=np.float64):
    rows, n_cols = banded_rows(D)
    return from_rows(rows, n_cols, dtype, seed=D)


MIXED_D = (3, 27, 0, 0, 8, 9, 0, 5)       # what plan_model must find, segment by segment


def mixed_segments(dtype=np.float64):
    """7 segments and a last one of 37 rows, 485 x 540: D = 3; D = 27; not eligible (row 150 is not sorted);
    entirely empty; D = 8; D = 9; entirely empty; 37 rows with D = 5.  Five of eight are eligible.  Under two
    segments per wave the pairs are (3, 27), (unsorted, empty), (8, 9), (empty, 5): the last one is the wave whose
    first segment has nothing to load and whose second has."""
    n, n_cols = 7 * 64 + 37, 540
    rows = []
    spec = [(-1, 0, 1), tuple(range(-13, 14)), (-1, 0, 1), None, tuple(range(0, 16, 2)), tuple(range(-4, 5)), None,
            (-2, -1, 0, 1, 2)]
    for s, offs in enumerate(spec):
        count = min(64, n - 64 * s)
        rows += [[] for _ in range(count)] if offs is None else band_rows(count, n_cols, offs, first=64 * s)
    rows[150] = [151, 149, 150]
    return from_rows(rows, n_cols, dtype, seed=77)


def full_stage_leads(dtype):
    return range(16 // np.dtype(dtype).itemsize)


def full_stage(dtype, lead):
    """138 x 180.  Segment 0 holds 192 + lead entries (rows of 3, the first `lead` rows of 4), so that segment 1
    starts at k0 = 192 + lead, k0 % E = lead (E = 16 / sizeof(T) entries per load); segment 1 is 64 rows x the 32
    offsets 0 .. 31 = 2048 entries = the stage's capacity, streamed from the aligned k0 - lead: len = CAP + lead;
    segment 2 has 10 tridiagonal rows, so that the full segment is not the array's end."""
    n, n_cols = 138, 180
    assert 0 <= lead < 16 // np.dtype(dtype).itemsize
    rows = band_rows(64, n_cols, (0, 1, 2))
    for r in range(lead):
        rows[r].append(r + 3)
    rows += band_rows(64, n_cols, tuple(range(32)), first=64)
    rows += band_rows(10, n_cols, (-1, 0, 1), first=128)
    return from_rows(rows, n_cols, dtype, seed=40 + lead)


def tall(n_rows=300, first=200, dtype=np.float64):
    """n_rows x 100, rows first .. first + 99 store the columns r - first - 1 and r - first (the first of them
    column 0 only), every other row is empty.  An eligible segment's offsets are -first - 1 and -first: for its
    empty rows in front of `first` row + off is below 0, and for the lanes behind the last row it is above
    n_cols - 1 = 99 - both are absent slots whose load must be clamped.
    tall() = (300, 200): segments 0 .. 2 are empty, 2 of 5 are eligible - BELOW the 50 % share, the plan is
    rejected (state 2) and the row-segment kernel multiplies; tall(164, 64): 2 of 3, the plan is used."""
    assert first + 100 == n_rows
    rows = [[] for _ in range(n_rows)]
    for r in range(first, n_rows):
        rows[r] = [c for c in (r - first - 1, r - first) if c >= 0]
    return from_rows(rows, 100, dtype, seed=31)


def rows_n(n, dtype=np.float64):
    """tridiagonal n x n (n = 1, 63, 64, 65)"""
    return from_rows(band_rows(n, n, (-1, 0, 1)), n, dtype, seed=n)


ROW_COUNTS = (1, 63, 64, 65)
SHARES = ((2, 4), (1, 3), (1, 4), (0, 2))       # (2, 4) is accepted (exactly 50 %), the others are rejected


def share(k, n, dtype=np.float64):
    """64 n x 64 n tridiagonal; the first k segments are eligible, each of the others has one row out of order"""
    rows = band_rows(64 * n, 64 * n, (-1, 0, 1))
    for s in range(k, n):
        r = 64 * s + 20
        rows[r] = [r + 1, r - 1, r]
    return from_rows(rows, 64 * n, dtype, seed=10 * n + k)


HUB_ROW, HUB_LEN = 70, 4097


def hub(dtype=np.float64, square=False):
    """256 x 5000 tridiagonal, but row 70 stores the 4097 ascending columns 3, 4, .. 4099 (one more than
    GKOC_CSR_LONG_ROW): segment 1 has far more than 32 offsets and is long-flagged (csr_long_rows.hpp), the
    other three are eligible.  square: 4160 x 4160, for the fused product and dot: 64 of 65 segments eligible."""
    n, n_cols = (4160, 4160) if square else (256, 5000)
    rows = band_rows(n, n_cols, (-1, 0, 1))
    rows[HUB_ROW] = list(range(3, 3 + HUB_LEN))
    return from_rows(rows, n_cols, dtype, seed=70)


FUZZ_SEEDS = tuple(range(40))


def fuzz(seed, dtype=np.float64):
    """n_rows in 1 .. 700; per segment an offset set of 1 .. 36 values in [-n, n], every row a random subset of it
    (entries outside the matrix dropped; the density of the subset is drawn per segment), and with probability 0.1 one row of the segment gets a duplicated column
    or a descending pair"""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(1, 701))
    n_cols = n + int(rng.integers(0, 50))
    rows = []
    for s in range(-(-n // SEG)):
        count = min(SEG, n - SEG * s)
        # (half of the segments draw from the offsets that lie inside the matrix for at least one of their rows:
        # of a set drawn from all of [-n, n] about half is dropped, and more than 32 would never survive)
        pool = np.arange(-n, n + 1)
        if rng.random() < 0.5:
            pool = pool[(pool > -(SEG * s + count)) & (pool < n_cols - SEG * s)]
        offs = np.sort(rng.choice(pool, min(int(rng.integers(1, 37)), len(pool)), replace=False))
        density = rng.uniform(0.05, 1.0)
        seg_rows = []
        for r in range(SEG * s, SEG * s + count):
            keep = offs[rng.random(len(offs)) < density]
            seg_rows.append([int(r + o) for o in keep if 0 <= r + o < n_cols])
        if rng.random() < 0.1:
            victims = [i for i, row in enumerate(seg_rows) if len(row) >= 2]
            if victims:
                row = seg_rows[victims[int(rng.integers(len(victims)))]]
                if rng.random() < 0.5:
                    row[1] = row[0]                   # a duplicate
                else:
                    row[0], row[1] = row[1], row[0]   # a descending pair
        rows += seg_rows
    return from_rows(rows, n_cols, dtype, seed=seed)


def two_structures(dtype):
    """130 x 138 tridiagonal, and the same row pointers and entry count with other columns"""
    n = 130
    first = band_rows(n, n + 8, (-1, 0, 1))
    second = [[c + 2 if c > r else c for c in row] for r, row in enumerate(first)]
    return from_rows(first, n + 8, dtype, seed=1), from_rows(second, n + 8, dtype, seed=1)


def is_csr(rp, ci, shape):
    """(rp, ci) as read back from a device is a CSR structure of this shape with len(ci) entries"""
    n, n_cols = shape
    return (len(rp) == n + 1 and rp[0] == 0 and rp[-1] == len(ci) and bool(np.all(np.diff(rp.astype(np.int64)) >= 0))
            and bool(np.all((ci >= 0) & (ci < n_cols))))


@functools.lru_cache(maxsize=None)
def builders():
    """name -> builder(dtype) of every matrix of section 2 of the device file"""
    out = {}
    for D in BANDED_D:
        out["banded-%d" % D] = functools.partial(banded, D)
    out["mixed"] = mixed_segments
    out["tall-300"] = functools.partial(tall, 300, 200)
    out["tall-164"] = functools.partial(tall, 164, 64)
    for n in ROW_COUNTS:
        out["rows-%d" % n] = functools.partial(rows_n, n)
    for k, n in SHARES:
        out["share-%d-%d" % (k, n)] = functools.partial(share, k, n)
    return out


def full_stage_names():
    return ["full-%s-%d" % (np.dtype(t).name, lead) for t in (np.float64, np.float32) for lead in full_stage_leads(t)]


# ================================================================ device helpers (import the package lazily)
BITS = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}


def torch_type(dtype):
    import torch
    return {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}[np.dtype(dtype)]


@contextlib.contextmanager
def key(value, which=KEY):
    from ginkgo_amd import _lib
    was = C.c_int64(0)
    _lib.call("gkoc_tune_get", C.c_int(which), C.byref(was))
    _lib.call("gkoc_tune_set", C.c_int(which), C.c_int64(value))
    try:
        yield
    finally:
        _lib.call("gkoc_tune_set", C.c_int(which), C.c_int64(was.value))


def arena_tensor(ex, arr, role):
    """a tensor over a gkoc_malloc_role allocation of its own, whatever its size (executor._ArenaBlock)"""
    import torch
    from ginkgo_amd.executor import _ArenaBlock, _TYPESTR
    arr = np.ascontiguousarray(arr)
    if arr.size == 0:         # (nothing to allocate: an empty view of a block, whose data pointer is null)
        return arena_tensor(ex, np.zeros(1, arr.dtype), role)[:0]
    src = torch.from_numpy(arr)
    with torch.cuda.device(ex.device):
        block = _ArenaBlock(arr.nbytes, role, arr.shape, _TYPESTR[src.dtype])
        t = torch.as_tensor(block, device=ex.device)
    assert t.data_ptr() == block.ptr
    t.copy_(src)
    return t


def arena_csr(ex, shape, rp, ci, v):
    import ginkgo_amd as g
    from ginkgo_amd.executor import MEM_INDICES, MEM_VALUES
    return g.Csr(ex, shape, arena_tensor(ex, v, MEM_VALUES), arena_tensor(ex, ci.astype(np.int32), MEM_INDICES),
                 arena_tensor(ex, rp.astype(np.int32), MEM_INDICES))


def plan_info(a):
    return plan_info_at(a.row_ptrs.data_ptr(), a.col_idxs.data_ptr())


def plan_info_at(row_ptrs, col_idxs):
    from ginkgo_amd import _lib
    st, el, ns, by, pr = C.c_int(-9), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.call("gkoc_csr_plan_info", C.c_void_p(row_ptrs), C.c_void_p(col_idxs),
              C.byref(st), C.byref(el), C.byref(ns), C.byref(by), C.byref(pr))
    return {"state": st.value, "eligible": el.value, "segments": ns.value, "bytes": by.value, "products": pr.value}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(BITS[x.dtype])


MODES = ("plain", "adv", "beta0", "dot")


def run(ex, a, b, mode, c0):
    """one product, twice from the same input (the same bits): the result"""
    import ginkgo_amd as g
    n, dtype = a.size[0], b.dtype
    db = g.Dense.from_numpy(ex, b.reshape(-1, 1))
    outs = []
    for _ in range(2):
        if mode == "dot":
            from ginkgo_amd import _lib
            es = dtype.itemsize
            nbytes = _lib.lib().gkoc_x_workspace_bytes(C.c_int64(n), C.c_size_t(es))
            work = ex.alloc(((nbytes + es - 1) // es,), torch_type(dtype))
            dc = g.Dense.from_numpy(ex, np.full((n, 1), np.nan, dtype))
            dot = g.Dense.from_numpy(ex, np.full((1, 1), np.nan, dtype))
            a.apply_dot(db, dc, dot, work)
            outs.append(np.concatenate((dc.to_numpy().reshape(-1), dot.to_numpy().reshape(-1))))
            continue
        c_init = np.full((n, 1), np.nan, dtype) if mode in ("plain", "beta0") else c0.reshape(-1, 1)
        dc = g.Dense.from_numpy(ex, c_init)
        if mode == "plain":
            a.apply(db, dc)
        else:
            alpha, beta = (-0.75, 1.5) if mode == "adv" else (-0.75, 0.0)
            a.apply(g.scalar(ex, alpha, dc.dtype), db, g.scalar(ex, beta, dc.dtype), dc)
        outs.append(dc.to_numpy().reshape(-1))
    assert np.array_equal(bits(outs[0]), bits(outs[1])), "the same product twice: different bits"
    return outs[0]


def reference(oracle, m, b, mode, c0):
    _, rp, ci, v = m
    if mode in ("plain", "dot"):
        return oracle.csr_spmv(rp, ci, v, b)
    alpha, beta = (-0.75, 1.5) if mode == "adv" else (-0.75, 0.0)
    c = c0 if mode == "adv" else np.zeros_like(c0)      # beta = 0 never reads c
    return oracle.csr_spmv(rp, ci, v, b, alpha, beta, c)


def plain(ex, a, b):
    return run(ex, a, b, "plain", None)


def check_all_modes(ex, oracle, m, eligible=None, modes=MODES, b=None):
    """every mode through the plan (built by the first product: key 1), against the oracle and against key 2.
    What the plan must report - segments, eligible segments, state - comes from plan_model, the products from a
    running count: a rejected plan (state 2) has none, and the fused dot goes through the plan only where the
    matrix is square and every segment is eligible.  `eligible`, where given, is what the CALLER expects of the
    model.  A matrix without entries comes with null col_idxs / vals and is never keyed: state -1, all figures 0."""
    shape, rp, ci, v = m
    model = plan_model(rp, ci)
    if len(ci) == 0:
        model = Plan(model.D, model.offsets, model.mask, 0, 0, -1)
    if eligible is not None:
        assert model.eligible == eligible and model.state == 1, (model.eligible, eligible, model.state)
    rng = np.random.default_rng(5)
    if b is None:
        b = rng.uniform(-1, 1, shape[1]).astype(v.dtype)
    c0 = rng.uniform(-1, 1, shape[0]).astype(v.dtype)
    a = arena_csr(ex, shape, rp, ci, v)
    done = 0
    for mode in modes:
        if mode == "dot" and (shape[0] != shape[1] or model.eligible != model.segments):
            continue        # (square matrices; the fused entry takes the plan where every segment is eligible)
        with key(1):
            got = run(ex, a, b, mode, c0)
            info = plan_info(a)
        if model.state == 1:
            done += 2
        assert info["state"] == model.state and info["segments"] == model.segments, (mode, info, model.state)
        assert info["eligible"] == model.eligible, (mode, info, model.eligible)
        assert info["products"] == done and (info["bytes"] > 0) == (model.state == 1), (mode, info)
        with key(2):
            old = run(ex, a, b, mode, c0)
        assert plan_info(a)["products"] == done
        assert np.array_equal(bits(got), bits(old)), mode
        ref = reference(oracle, m, b, mode, c0)
        assert np.array_equal(bits(got[:shape[0]]), bits(ref)), mode
    return a
