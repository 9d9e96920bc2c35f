"""tests/csr_offsets_cases.py on the CPU: plan_model (plain loops) against an independent formulation with sets and
numpy on every matrix the device tests use, and the builders against what their docstrings promise - the D of every
segment, k0 % E of the full stage, sortedness - so that a bug in a builder cannot make a device case vacuous."""
import numpy as np
import pytest

import csr_offsets_cases as oc


def model_by_sets(rp, ci):
    """(D per segment, offsets per segment, masks, eligible, segments, state) without a loop over entries"""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    n = len(rp) - 1
    row_of = np.repeat(np.arange(n), np.diff(rp))
    off = ci - row_of
    # an entry is "bad" if it does not exceed its predecessor in the same row
    bad = np.zeros(len(ci), bool)
    if len(ci) > 1:
        bad[1:] = (row_of[1:] == row_of[:-1]) & (ci[1:] <= ci[:-1])
    n_seg = -(-n // 64)
    D, offsets = [], []
    mask = np.zeros(n, np.uint32)
    for s in range(n_seg):
        sel = (row_of // 64) == s
        union = sorted(set(off[sel].tolist()))
        if bad[sel].any() or not 1 <= len(union) <= 32:
            D.append(0)
            offsets.append([])
            continue
        D.append(len(union))
        offsets.append(union)
        slot = np.searchsorted(np.array(union), off[sel])
        np.bitwise_or.at(mask, row_of[sel], (np.uint32(1) << slot.astype(np.uint32)))
    eligible = sum(d > 0 for d in D)
    state = 1 if eligible > 0 and 2 * eligible >= n_seg else 2
    return D, offsets, mask, eligible, n_seg, state


def all_matrices():
    out = [(name, b(np.float64)) for name, b in oc.builders().items()]
    out += [("full-%s-%d" % (np.dtype(t).name, lead), oc.full_stage(t, lead))
            for t in (np.float64, np.float32) for lead in oc.full_stage_leads(t)]
    out.append(("hub", oc.hub()))
    out.append(("hub-square", oc.hub(square=True)))
    out += [("fuzz-%d" % s, oc.fuzz(s)) for s in oc.FUZZ_SEEDS]
    out += [("two-%d" % i, m) for i, m in enumerate(oc.two_structures(np.float64))]
    return out


ALL = all_matrices()


@pytest.mark.parametrize("name,m", ALL, ids=[n for n, _ in ALL])
def test_model_against_sets(name, m):
    shape, rp, ci, v = m
    assert oc.is_csr(rp, ci, shape) and len(v) == len(ci) and rp.dtype == ci.dtype == np.int32
    got = oc.plan_model(rp, ci)
    D, offsets, mask, eligible, n_seg, state = model_by_sets(rp, ci)
    assert got.D == D and got.offsets == offsets
    assert np.array_equal(got.mask, mask)
    assert (got.eligible, got.segments, got.state) == (eligible, n_seg, state)
    # a row's mask has as many bits as the row has entries, in an eligible segment
    for s, d in enumerate(D):
        rows = slice(64 * s, min(64 * s + 64, shape[0]))
        lens = np.diff(rp)[rows]
        pop = np.array([bin(int(x)).count("1") for x in got.mask[rows]])
        assert np.array_equal(pop, lens if d > 0 else np.zeros_like(lens))


def test_model_on_hand_cases():
    """the definition's edges, by hand: 32 / 33 offsets, a duplicate, a descending pair, an empty segment, and the
    50 % share from both sides"""
    def one_segment(rows, n_cols=200):
        return oc.from_rows(rows + [[] for _ in range(64 - len(rows))], n_cols, np.float64)
    _, rp, ci, _ = one_segment([list(range(32))])
    p = oc.plan_model(rp, ci)
    assert p.D == [32] and p.offsets == [list(range(32))] and p.mask[0] == 0xffffffff and p.state == 1
    _, rp, ci, _ = one_segment([list(range(32)), [34]])
    assert oc.plan_model(rp, ci).D == [0] and oc.plan_model(rp, ci).state == 2
    _, rp, ci, _ = one_segment([list(range(32)), [33]])          # row 1, column 33: offset 32, the 33rd
    assert oc.plan_model(rp, ci).D == [0]
    _, rp, ci, _ = one_segment([list(range(32)), [32]])          # row 1, column 32: offset 31 again
    assert oc.plan_model(rp, ci).D == [32]
    for row in ([4, 4], [5, 4]):
        _, rp, ci, _ = one_segment([[0, 1], row])
        assert oc.plan_model(rp, ci).D == [0]
    _, rp, ci, _ = one_segment([])
    p = oc.plan_model(rp, ci)
    assert p.D == [0] and p.eligible == 0 and p.state == 2
    # offsets -1, 3; row 2 stores only the second: bit 1
    _, rp, ci, _ = one_segment([[], [0, 4], [5]])
    p = oc.plan_model(rp, ci)
    assert p.offsets == [[-1, 3]] and list(p.mask[:3]) == [0, 3, 2]


@pytest.mark.parametrize("D", oc.BANDED_D)
def test_banded(D):
    shape, rp, ci, _ = oc.banded(D)
    assert shape == (192, 320)
    p = oc.plan_model(rp, ci)
    rows = oc.rows_of(oc.banded(D))
    union = sorted({c - r for r in range(64, 128) for c in rows[r]})
    assert union == oc.banded_offsets(D) and len(union) == D
    assert p.D == [3, D if D <= 32 else 0, 3]
    lens = [len(rows[r]) for r in range(64, 128)]
    most = min(D, 32)
    assert min(lens) == 0 and lens[100 - 64] == 0 and sorted(lens)[1] >= 1 and max(lens) == most
    assert len(rows[70]) == most and len(rows[71]) == most
    if D <= 32:
        assert int(p.mask[70]) == int(p.mask[71]) == (1 << D) - 1
    assert all(row == sorted(set(row)) for row in rows)
    assert p.state == 1


def test_mixed_segments():
    shape, rp, ci, _ = oc.mixed_segments()
    assert shape[0] == 7 * 64 + 37
    p = oc.plan_model(rp, ci)
    assert tuple(p.D) == oc.MIXED_D == (3, 27, 0, 0, 8, 9, 0, 5)
    assert (p.eligible, p.segments, p.state) == (5, 8, 1)
    lens = np.diff(rp)
    assert lens[64:128].max() == 27                              # a row with every offset of the D = 27 segment
    assert lens[128:192].min() > 0 and lens[192:256].sum() == 0 and lens[384:448].sum() == 0
    rows = oc.rows_of(oc.mixed_segments())
    assert [r for r, row in enumerate(rows) if row != sorted(set(row))] == [150]
    # the ND = 8 / ND = 32 dispatch: a segment on either side of D = 8, next to each other
    assert p.D[4] == 8 and p.D[5] == 9


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_full_stage(dtype):
    E = 16 // np.dtype(dtype).itemsize
    assert list(oc.full_stage_leads(dtype)) == list(range(E))
    for lead in oc.full_stage_leads(dtype):
        shape, rp, ci, v = oc.full_stage(dtype, lead)
        assert v.dtype == dtype and shape == (138, 180)
        p = oc.plan_model(rp, ci)
        assert p.D == [4 if lead else 3, 32, 3] and p.state == 1
        k0, k1 = int(rp[64]), int(rp[128])
        assert k0 % E == lead and k1 - k0 == oc.CAP == 2048
        assert k1 - (k0 - k0 % E) == oc.CAP + lead               # len of unit_of: CAP + E - 1 at the last lead
        assert np.all(np.diff(rp)[64:128] == 32) and np.all(p.mask[64:128] == 0xffffffff)
        assert rp[-1] > k1                                       # the full segment is not the array's end
    with pytest.raises(AssertionError):
        oc.full_stage(dtype, E)


def test_tall():
    for (n, first), want in (((300, 200), (2, 5, 2)), ((164, 64), (2, 3, 1))):
        shape, rp, ci, _ = oc.tall(n, first)
        assert shape == (n, 100)
        p = oc.plan_model(rp, ci)
        assert (p.eligible, p.segments, p.state) == want
        assert np.diff(rp)[:first].sum() == 0 and list(np.diff(rp)[first:first + 3]) == [1, 2, 2]
        assert ci.max() == 99 and ci.min() == 0
        for s, offs in enumerate(p.offsets):
            if offs:
                assert offs == [-first - 1, -first]
                # absent slots on both sides of the vector: below 0 and above n_cols - 1
                assert 64 * s + offs[0] < 0 or s > first // 64
        assert 64 * (p.segments - 1) + 63 - first > 99           # a lane behind the last row points beyond x
        assert (first // 64) * 64 - first - 1 < 0                # an empty row of an eligible segment points below it


@pytest.mark.parametrize("n", oc.ROW_COUNTS)
def test_row_counts(n):
    shape, rp, ci, _ = oc.rows_n(n)
    p = oc.plan_model(rp, ci)
    assert shape == (n, n) and p.segments == -(-n // 64) == p.eligible and p.state == 1
    assert p.D == ([1] if n == 1 else [3] * p.segments if n != 65 else [3, 2])


@pytest.mark.parametrize("k,n", oc.SHARES)
def test_share(k, n):
    shape, rp, ci, _ = oc.share(k, n)
    p = oc.plan_model(rp, ci)
    assert shape == (64 * n, 64 * n)
    assert (p.eligible, p.segments) == (k, n) and [d > 0 for d in p.D] == [s < k for s in range(n)]
    assert p.state == (1 if (k, n) == (2, 4) else 2)
    assert np.all(np.diff(rp)[64 * k:] > 0)          # the segments that are not eligible are not empty either


def test_hub():
    shape, rp, ci, _ = oc.hub()
    p = oc.plan_model(rp, ci)
    assert shape == (256, 5000) and tuple(p.D) == (3, 0, 3, 3) and p.state == 1
    lens = np.diff(rp)
    assert lens[oc.HUB_ROW] == 4097 > 4096 and np.all(np.delete(lens, oc.HUB_ROW) <= 3)
    cols = ci[rp[oc.HUB_ROW]:rp[oc.HUB_ROW + 1]]
    assert np.all(np.diff(cols) > 0) and cols.max() < 5000
    shape, rp, ci, _ = oc.hub(square=True)
    p = oc.plan_model(rp, ci)
    assert shape == (4160, 4160) and (p.eligible, p.segments, p.state) == (64, 65, 1) and p.D[1] == 0
    assert np.diff(rp)[oc.HUB_ROW] == 4097 and ci.max() < 4160


def test_fuzz_covers_its_edges():
    """over the 40 seeds: sizes on both sides of a segment, segments with more than 32 offsets, spoiled rows, both
    states, partial last segments"""
    seen = {"over": 0, "spoiled": 0, "state1": 0, "state2": 0, "partial": 0, "single": 0, "d_le_8": 0, "d_gt_8": 0}
    for seed in oc.FUZZ_SEEDS:
        shape, rp, ci, _ = oc.fuzz(seed)
        assert 1 <= shape[0] <= 700 and shape[0] <= shape[1] < shape[0] + 50
        p = oc.plan_model(rp, ci)
        rows = oc.rows_of(oc.fuzz(seed))
        for s in range(p.segments):
            seg = rows[64 * s:64 * s + 64]
            union = {c - (64 * s + i) for i, row in enumerate(seg) for c in row}
            spoiled = any(row != sorted(set(row)) for row in seg)
            seen["over"] += len(union) > 32 and not spoiled
            seen["spoiled"] += spoiled
            seen["d_le_8"] += 0 < p.D[s] <= 8
            seen["d_gt_8"] += p.D[s] > 8
        seen["state%d" % p.state] += 1
        seen["partial"] += shape[0] % 64 != 0
        seen["single"] += p.segments == 1
    assert all(v > 0 for v in seen.values()), seen


def test_two_structures():
    m1, m2 = oc.two_structures(np.float64)
    assert m1[0] == (130, 138) and np.array_equal(m1[1], m2[1]) and not np.array_equal(m1[2], m2[2])
    for m in (m1, m2):
        p = oc.plan_model(m[1], m[2])
        assert (p.eligible, p.segments, p.state) == (3, 3, 1)
