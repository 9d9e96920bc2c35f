"""csr_spmv_pipe3_kernel_offsets (csrc/csr_offsets.hpp) sized by its slot count: the launcher (csrc/csr_spmv.hip) picks
the kernel with ND = 8, 16, 28 or 32 diagonal slots, the smallest that holds the plan's largest D; the value stream
(NL = ND / E + 1 loads of E = 16 / sizeof(T) entries per lane), the stage (NL x 64 x E entries) and the x loads follow
ND, and a row's start in the stage is the lead of the stream plus the wave's exclusive prefix sum of popc(mask) - the
row pointer of the row is not read.

Every case is a matrix of a few hundred rows.  As in tests/test_csr_offsets_gpu.py every product is compared BIT FOR
BIT with the sequential oracle and with the row-segment kernel (GKOC_TUNE_CSR_OFFSETS = 2), in double and float, with
one and two segments per wave (GKOC_TUNE_CSR_SEGS_PER_WAVE), plain, advanced, beta = 0 and - where the matrix is square
and every segment eligible - the fused <b, c> entry (csr_offsets_cases.check_all_modes).

The builders are checked on the CPU by tests/test_csr_offsets_shapes_cases_cpu.py.
"""
import numpy as np
import pytest

import csr_offsets_cases as oc
from csr_offsets_cases import (KEY_SEGS_PER_WAVE, arena_csr, band_rows, bits, check_all_modes, from_rows, key, plan_info,
                               reference, run)

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SPW = [1, 2]
SLOTS = (8, 16, 28, 32)            # the kernels' slot counts, csr_spmv.hip launch_offsets_kernel


def slots_for(max_d):
    return next(nd for nd in SLOTS if nd >= max_d)


def entries_per_load(dtype):
    return 16 // np.dtype(dtype).itemsize


def check(gexec, oracle, m, spw, eligible=None, modes=oc.MODES):
    with key(spw, KEY_SEGS_PER_WAVE):
        return check_all_modes(gexec, oracle, m, eligible=eligible, modes=modes)


# ---------------------------------------------------------------- builders (host)
def d_pair(d_first, d_second, dtype):
    """128 x 128: segment 0 has exactly the d_first offsets 0 .. d_first - 1, segment 1 exactly the d_second offsets
    -(d_second - 1) .. 0; every row stores all of them (all lie in the matrix)"""
    rows = band_rows(64, 128, tuple(range(d_first))) + band_rows(64, 128, tuple(range(1 - d_second, 1)), first=64)
    return from_rows(rows, 128, dtype, seed=100 * d_first + d_second)


# the plan's largest D on both sides of every step of the kernel choice, beside a segment of 3 offsets (27 beside 3:
# the stencil's D under its kernel, the 28-slot one) and, at the kernels' own widths, beside one of 1; both orders
D_EDGES = [(d, 3) for d in (8, 9, 16, 17, 27, 28, 29, 32)] + [(d, 1) for d in (16, 28)]
D_PAIRS = D_EDGES + [(b, a) for a, b in D_EDGES]


def full_stage_nd(nd, lead, wider, dtype):
    """138 x 180, as csr_offsets_cases.full_stage but for the kernel with nd slots.  Segment 0 holds 192 + lead
    entries (rows of 3, the first `lead` rows of 4), so segment 1 starts at k0 = 192 + lead, k0 % E = lead; segment
    1 is 64 rows x the nd offsets 0 .. nd - 1, all stored: 64 nd entries = the capacity of the nd-slot kernel's
    group, streamed from the aligned k0 - lead: len = 64 nd + lead.  Segment 2 has 10 rows, so the full segment is
    not the array's end: tridiagonal, or (wider) of nd + 1 offsets, which puts the whole plan under the next wider
    kernel."""
    n_cols = 180
    assert 0 <= lead < entries_per_load(dtype) and nd + 1 <= oc.OFFS_MAX
    rows = band_rows(64, n_cols, (0, 1, 2))
    for r in range(lead):
        rows[r].append(r + 3)
    rows += band_rows(64, n_cols, tuple(range(nd)), first=64)
    rows += band_rows(10, n_cols, tuple(range(nd + 1)) if wider else (-1, 0, 1), first=128)
    return from_rows(rows, n_cols, dtype, seed=300 + 10 * nd + lead)


FULL_ND = (8, 16, 28)
TAILS = (1, 37, 63)


def mask_shapes_offsets(nd):
    return [i - nd // 2 for i in range(nd)]


def mask_shapes(nd, tail, dtype):
    """(256 + tail) x (256 + tail), five segments over the nd offsets -nd / 2 .. nd / 2 - 1 (an entry outside the
    matrix is dropped), what the row starts are summed from:
      0: every row a drawn subset of 1 .. nd offsets (rows 0 .. 15, where the offsets below the diagonal leave the
         matrix, with the diagonal), row 40 all nd;
      1: rows 64 (lane 0), 127 (lane 63), 80 .. 89 and 100 .. 102 empty, the others drawn subsets;
      2: only row 191 (lane 63) stores anything: all nd offsets;
      3: only row 192 (lane 0) stores anything: all nd offsets;
      4: `tail` rows, drawn subsets with the diagonal (the offsets above it leave the matrix in the last rows).
    Under two segments per wave the pairs are (0, 1), (2, 3) and the last segment alone."""
    n = 256 + tail
    offs = mask_shapes_offsets(nd)
    rng = np.random.default_rng(1000 * nd + tail)

    def drawn(r, diagonal=False):
        count = int(rng.integers(1, nd + 1))
        pick = sorted(set(rng.choice(nd, count, replace=False).tolist()) | ({nd // 2} if diagonal else set()))
        return [r + offs[i] for i in pick if 0 <= r + offs[i] < n]

    def full(r):
        return [r + o for o in offs if 0 <= r + o < n]

    rows = [drawn(r, diagonal=r < 16) for r in range(64)]
    rows[40] = full(40)
    empty = {64, 127} | set(range(80, 90)) | set(range(100, 103))
    rows += [[] if r in empty else drawn(r) for r in range(64, 128)]
    rows += [full(r) if r == 191 else [] for r in range(128, 192)]
    rows += [full(r) if r == 192 else [] for r in range(192, 256)]
    rows += [drawn(r, diagonal=True) for r in range(256, n)]
    return from_rows(rows, n, dtype, seed=7 * nd + tail)


def stencil_band(dtype):
    """256 x 256, four segments of the 27 offsets -13 .. 13 (an entry outside the matrix is dropped)"""
    return from_rows(band_rows(256, 256, tuple(range(-13, 14))), 256, dtype, seed=27)


# ---------------------------------------------------------------- 1. kernel choice at its edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("d_first,d_second", D_PAIRS)
def test_kernel_choice(gexec, oracle, d_first, d_second, spw, dtype):
    """the plan's largest D is 8 | 9, 16 | 17, 28 | 29 and 32: the last D a kernel takes and the first it does not;
    the narrow neighbour runs under the same kernel with offset 0 and mask bit 0 in the slots it lacks"""
    m = d_pair(d_first, d_second, np.dtype(dtype))
    assert oc.plan_model(m[1], m[2]).D == [d_first, d_second]
    check(gexec, oracle, m, spw, eligible=2)


# ---------------------------------------------------------------- 2. each stage at capacity
@pytest.mark.parametrize("dtype,lead", [(t, lead) for t in DTYPES for lead in range(entries_per_load(t))])
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("wider", [False, True])
@pytest.mark.parametrize("nd", FULL_ND)
def test_stage_at_capacity(gexec, oracle, nd, wider, spw, dtype, lead):
    """64 x nd entries behind a lead of 0 .. E - 1: every chunk of the nd-slot kernel's stage holds values and the
    last row's last entry sits at index lead + 64 nd - 1, the largest a row phase reads; the same segment under the
    next wider kernel (wider), where the stage has room to spare.  (32 slots: csr_offsets_cases.full_stage.)"""
    m = full_stage_nd(nd, lead, wider, np.dtype(dtype))
    assert int(m[1][64]) == 192 + lead and int(m[1][128]) - int(m[1][64]) == 64 * nd
    assert slots_for(max(oc.plan_model(m[1], m[2]).D)) == (slots_for(nd + 1) if wider else nd)
    check(gexec, oracle, m, spw, eligible=3)


# ---------------------------------------------------------------- 3. row starts from the masks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("nd", SLOTS)
def test_row_starts_from_masks(gexec, oracle, nd, tail, spw, dtype):
    """rows of every length 0 .. nd in one wave, empty rows at both ends of the wave and in runs, all of a
    segment's entries in lane 63 (its start is the sum over 63 empty rows) or in lane 0, and a last segment of 1,
    37 and 63 rows, whose lanes behind the last row must add nothing; square and fully eligible: the fused dot
    runs too"""
    m = mask_shapes(nd, tail, np.dtype(dtype))
    assert slots_for(max(oc.plan_model(m[1], m[2]).D)) == nd
    check(gexec, oracle, m, spw, eligible=5)


# ---------------------------------------------------------------- 4. poisoned neighbours, D = 27
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("victim", [0, 1, 2, 3])
def test_poisoned_neighbours_27(gexec, oracle, victim, spw, dtype):
    """test_poisoned_neighbours of tests/test_csr_offsets_pipeline_gpu.py under the 28-slot kernel: the values of
    every segment but `victim` are NaN and Inf in turn - what is prefetched during the victim's row phase, what was
    in the registers and in the stage before it, and the entries of the neighbour that share the victim's first
    and last 16 bytes.  The victim's rows are finite and have the oracle's and the row-segment kernel's bits."""
    dtype = np.dtype(dtype)
    n = 256
    shape, rp, ci, v = stencil_band(dtype)
    mine = slice(int(rp[64 * victim]), int(rp[64 * victim + 64]))
    poisoned = np.where(np.arange(len(v)) % 2 == 0, np.nan, np.inf).astype(dtype)
    poisoned[mine] = v[mine]
    m = (shape, rp, ci, poisoned)
    rng = np.random.default_rng(80 + victim)
    b, c0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
    rows = slice(64 * victim, 64 * victim + 64)
    a = arena_csr(gexec, *m)
    done = 0
    with key(spw, KEY_SEGS_PER_WAVE):
        for mode in oc.MODES:
            with key(1):
                got = run(gexec, a, b, mode, c0)
                done += 2
                info = plan_info(a)
                assert (info["state"], info["eligible"], info["products"]) == (1, 4, done), (mode, info)
            with key(2):
                old = run(gexec, a, b, mode, c0)
            ref = reference(oracle, m, b, mode, c0)
            assert np.all(np.isfinite(got[rows])), mode
            assert np.array_equal(bits(got[rows]), bits(ref[rows])), mode
            assert np.array_equal(bits(got[rows]), bits(old[rows])), mode
            assert np.array_equal(np.isfinite(got[:n]), np.isfinite(ref)), mode
            assert not np.isfinite(got[:n][np.r_[0:64 * victim, 64 * victim + 64:n]]).any(), mode
