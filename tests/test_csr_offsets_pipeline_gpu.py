"""The hand-over between the groups of a wave in csr_spmv_pipe3_kernel_offsets (csrc/csr_offsets.hpp): a wave loops
over its groups that have a successor - the successor being the wave's next group WITH values, whose value loads are
issued before the row phase of the current one - and runs its last group behind that loop; the next unit's D, row
pointers and offsets are read one group ahead (behind the wave's end: the last unit's again); the stage takes every
chunk of every lane.  The launcher picks the kernel with 8 or with 32 diagonal slots from the plan's largest D.

Every case is the smallest matrix at which that hand-over can go wrong, a few hundred rows.  As in
tests/test_csr_offsets_gpu.py every product is compared BIT FOR BIT with the sequential oracle and with the
row-segment kernel (GKOC_TUNE_CSR_OFFSETS = 2), in double and float, plain, advanced (alpha, beta != 0), beta = 0 and
- where the matrix is square and every segment eligible, which is where that entry takes the plan - the fused
<b, c> entry; the plan's counters show that the offsets kernel did the work (csr_offsets_cases.check_all_modes).

A wave owns one or two segments (GKOC_TUNE_CSR_SEGS_PER_WAVE, which the plain, the advanced and the fused entry all
read; two by default only from 65536 segments on).  So "within one wave" below means the two segments 2w, 2w + 1 under
the key = 2, and every case also runs with one segment per wave, where every group is a wave's first and last.
test_fused_dot_really_runs_two_segments_per_wave shows that the key reaches the fused entry.

The builders are checked on the CPU by tests/test_csr_offsets_pipeline_cases_cpu.py.
"""
import numpy as np
import pytest

import csr_offsets_cases as oc
from csr_offsets_cases import (KEY_SEGS_PER_WAVE, arena_csr, band_rows, bits, check_all_modes, from_rows, key, plan_info,
                               reference, run)

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SPW = [1, 2]


def check(gexec, oracle, m, spw, eligible=None, modes=oc.MODES):
    with key(spw, KEY_SEGS_PER_WAVE):
        return check_all_modes(gexec, oracle, m, eligible=eligible, modes=modes)


# ---------------------------------------------------------------- builders (host)
def tri(n, dtype):
    return from_rows(band_rows(n, n, (-1, 0, 1)), n, dtype, seed=n)


def unsorted_segment(rows, s):
    """segment s keeps its entries but is not eligible: one row out of order (D = 0, the row-segment kernel's)"""
    r = 64 * s + 20
    rows[r] = [r + 1, r - 1, r]


def pattern(spec, dtype):
    """64 len(spec) rows, square, one segment per letter: B a tridiagonal band, 0 no entries at all, I a band with
    an unsorted row, W sorted rows of three entries whose offsets are 33 between them (0 .. 32; in the last segment
    -32 .. 0, so that every column lies in the matrix)"""
    n = 64 * len(spec)
    rows = band_rows(n, n, (-1, 0, 1))
    for s, kind in enumerate(spec):
        if kind == "0":
            rows[64 * s:64 * s + 64] = [[] for _ in range(64)]
        elif kind == "I":
            unsorted_segment(rows, s)
        elif kind == "W":
            shift = -32 if s == len(spec) - 1 else 0
            for j in range(64):
                r = 64 * s + j
                rows[r] = [r + shift + o for o in sorted({j % 33, (j + 11) % 33, (j + 22) % 33})]
    return from_rows(rows, n, dtype, seed=len(spec))


def d_pair(d_first, d_second, dtype):
    """128 x 128: segment 0 has exactly d_first offsets (0 .. d_first - 1), segment 1 exactly d_second
    (-(d_second - 1) .. 0); every row stores all of its segment's offsets that lie in the matrix, and row 0 / row
    127 store all of them"""
    rows = band_rows(64, 128, tuple(range(d_first))) + band_rows(64, 128, tuple(range(1 - d_second, 1)), first=64)
    return from_rows(rows, 128, dtype, seed=100 * d_first + d_second)


def stage_edges(full_first, dtype):
    """128 x 128: a full group (64 rows x 32 offsets = the stage's capacity) beside a group of ONE entry"""
    one = [[] for _ in range(64)]
    if full_first:
        one[5] = [64 + 5]
        rows = band_rows(64, 128, tuple(range(32))) + one
    else:
        one[5] = [5]
        rows = one + band_rows(64, 128, tuple(range(-31, 1)), first=64)
    return from_rows(rows, 128, dtype, seed=7 + full_first)


def unaligned(lead, dtype):
    """128 x 128: segment 0 holds 192 + lead entries (rows of (0, 1, 2), rows 0 .. lead - 1 one more), segment 1
    is tridiagonal and starts at k0 = row_ptrs[64] = 192 + lead"""
    rows = band_rows(64, 128, (0, 1, 2))
    for r in range(lead):
        rows[r].append(r + 3)
    rows += band_rows(64, 128, (-1, 0, 1), first=64)
    return from_rows(rows, 128, dtype, seed=50 + lead)


# ---------------------------------------------------------------- 1. no successor
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("n", [64, 65, 127, 128, 192])
def test_no_successor(gexec, oracle, n, spw, dtype):
    """n = 64: one segment.  128, 192 with two segments per wave: the wave's second unit is its last / the second
    wave owns one unit.  65, 127: a last segment of one row (2 entries: every lane's loads read the same 16
    bytes) / of 63 rows.  The array ends with the last group, and nnz = 3 n - 2 is no multiple of E for 65 and
    127."""
    m = tri(n, np.dtype(dtype))
    if n in (65, 127):
        assert len(m[3]) % (16 // np.dtype(dtype).itemsize) != 0
    check(gexec, oracle, m, spw, eligible=-(-n // 64))


# ---------------------------------------------------------------- 2. nothing to prefetch / not eligible
PATTERNS = ["B0BB", "0B0BB", "IEIE", "EIEI", "IEIEE", "I0EE", "E0IE", "WEWE", "EWEW", "WEWEE", "EIEW"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("spec", PATTERNS)
def test_segments_without_values_or_plan(gexec, oracle, spec, spw, dtype):
    """B0BB: an empty segment between non-empty ones (under two segments per wave the wave's second unit has
    nothing: no successor); 0B0BB the reverse (the wave's FIRST unit has nothing: the loads in front of the loop
    take the second).  I = not eligible (an unsorted row; D = 0 with entries, multiplied by the row-segment kernel
    in the same product): as a wave's first unit (IEIE), as its second (EIEI), on both sides of an eligible one
    (IEIEE; a wave owns at most two segments, so one of the two neighbours is the next wave's), beside an empty
    one.  W = not eligible for its 33 offsets, in the same places.  At least half of the segments stay eligible, so
    the plan is used."""
    m = pattern(spec.replace("E", "B"), np.dtype(dtype))
    check(gexec, oracle, m, spw, eligible=sum(k in "BE" for k in spec), modes=("plain", "adv", "beta0"))


# ---------------------------------------------------------------- 3. 8 and 32 diagonal slots
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("d_first,d_second", [(3, 9), (9, 3), (8, 9), (9, 8), (1, 32), (32, 1), (1, 8), (8, 1)])
def test_slots_hand_over(gexec, oracle, d_first, d_second, spw, dtype):
    """a segment of at most 8 offsets followed by one of more than 8 and the reverse, within one wave; the same
    with D = 1 and D = 32.  (1, 8) and (8, 1): the plan's largest D is 8, the 8-slot kernel multiplies; in all
    others the 32-slot kernel does, and the narrow segment's missing slots are offset 0 with mask bit 0."""
    m = d_pair(d_first, d_second, np.dtype(dtype))
    assert oc.plan_model(m[1], m[2]).D == [d_first, d_second]
    check(gexec, oracle, m, spw, eligible=2)


# ---------------------------------------------------------------- 4. stage edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("full_first", [True, False])
def test_stage_edges(gexec, oracle, full_first, spw, dtype):
    """a full group (2048 entries: every chunk of the stage holds values) beside a group of one entry (every
    chunk but the first is a copy of it that no row reads), in both orders"""
    m = stage_edges(full_first, np.dtype(dtype))
    assert sorted(oc.plan_model(m[1], m[2]).D) == [1, 32] and len(m[3]) == 2049
    check(gexec, oracle, m, spw, eligible=2)


# ---------------------------------------------------------------- 5. unaligned start
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("lead", [1, 2, 3])
def test_unaligned_start(gexec, oracle, lead, spw, dtype):
    """row_ptrs[row0] of the second segment = 192 + lead: odd for double (lead 1, 3), 1, 2, 3 mod 4 for float - the
    stream starts `lead % E` entries early, inside the previous group.  Under two segments per wave that group is
    prefetched during the first one's row phase, under one it is loaded in front of the loop."""
    m = unaligned(lead, np.dtype(dtype))
    assert int(m[1][64]) == 192 + lead
    check(gexec, oracle, m, spw, eligible=2)


# ---------------------------------------------------------------- 6. poisoned neighbours
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("victim", [0, 1, 2, 3])
def test_poisoned_neighbours(gexec, oracle, victim, spw, dtype):
    """256 x 256 tridiagonal, four segments: the values of every segment but `victim` are NaN and Inf in turn - what
    is prefetched during the victim's row phase, what was in the registers and in the stage before it.  The
    victim's rows are finite and have the oracle's and the row-segment kernel's bits (a value
    of another group never reaches this group's sums); the other rows are not finite, in the same places."""
    dtype = np.dtype(dtype)
    n = 256
    shape, rp, ci, v = tri(n, dtype)
    mine = slice(int(rp[64 * victim]), int(rp[64 * victim + 64]))
    poisoned = np.where(np.arange(len(v)) % 2 == 0, np.nan, np.inf).astype(dtype)
    poisoned[mine] = v[mine]
    m = (shape, rp, ci, poisoned)
    rng = np.random.default_rng(60 + victim)
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


# ---------------------------------------------------------------- 7. the fused entry under two segments per wave
def dot_model(term, spw, dtype):
    """<b, c> as the fused entry folds it from term = b * c (rounded), 128 rows: lane = row % 64 adds the terms of
    its wave's segments in turn, the wave's butterfly (offsets 32 .. 1) gives the wave's part, the parts are added"""
    def butterfly(x):
        x = x.copy()
        o = 32
        while o > 0:
            x = (x + x[np.arange(64) ^ o]).astype(dtype)
            o >>= 1
        return x[0]

    if spw == 2:
        return butterfly((term[:64] + term[64:]).astype(dtype))
    return dtype.type(butterfly(term[:64]) + butterfly(term[64:]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_dot_really_runs_two_segments_per_wave(gexec, oracle, dtype):
    """The fused <b, c> entry reads GKOC_TUNE_CSR_SEGS_PER_WAVE, so the dot cases above do put two segments into one
    wave.  128 rows, D = 32 and 9 (the 32-slot kernel): under the key = 2 ONE wave adds both segments' terms lane
    by lane before its butterfly, under the key = 1 two waves' parts are added - another association of the same
    terms, which differs in the last bits for this b (asserted on the host).  The dot has the bits of dot_model for
    the key in force; c has the oracle's bits either way."""
    dtype = np.dtype(dtype)
    m = d_pair(32, 9, dtype)
    shape, rp, ci, v = m
    n = shape[0]
    b = np.random.default_rng(71).uniform(-1, 1, n).astype(dtype)
    ref = oracle.csr_spmv(rp, ci, v, b)
    term = (b * ref).astype(dtype)
    want = {spw: dot_model(term, spw, dtype) for spw in SPW}
    assert want[1] != want[2], "this b does not tell the two groupings apart"
    a = arena_csr(gexec, *m)
    for spw in SPW:
        with key(spw, KEY_SEGS_PER_WAVE), key(1):
            got = run(gexec, a, b, "dot", None)
        assert np.array_equal(bits(got[:n]), bits(ref)), spw
        assert bits(got[n:])[0] == bits(np.array([want[spw]], dtype))[0], (spw, got[n], want)
    assert plan_info(a)["products"] == 4
