"""The builders of tests/test_csr_offsets_shapes_gpu.py on the CPU, against csr_offsets_cases.plan_model: the D of every
segment, the kernel the plan's largest D selects, the entry counts, stream starts and row lengths their docstrings
promise - so that a bug in a builder cannot make a device case vacuous."""
import numpy as np
import pytest

import csr_offsets_cases as oc
import test_csr_offsets_shapes_gpu as sg


def model(m):
    shape, rp, ci, v = m
    assert oc.is_csr(rp, ci, shape) and len(v) == len(ci) and rp.dtype == ci.dtype == np.int32
    return oc.plan_model(rp, ci)


def popcount(mask):
    return np.array([bin(int(x)).count("1") for x in mask])


def test_slots_for():
    assert [sg.slots_for(d) for d in (1, 8, 9, 16, 17, 27, 28, 29, 32)] == [8, 8, 16, 16, 28, 28, 28, 32, 32]


def test_d_pairs_cover_every_step():
    tops = {max(p) for p in sg.D_PAIRS}
    assert tops == {8, 9, 16, 17, 27, 28, 29, 32}
    assert (27, 3) in sg.D_PAIRS and (3, 27) in sg.D_PAIRS
    assert all((b, a) in sg.D_PAIRS for a, b in sg.D_PAIRS) and all(min(p) in (1, 3) for p in sg.D_PAIRS)


@pytest.mark.parametrize("d_first,d_second", sg.D_PAIRS)
def test_d_pairs(d_first, d_second):
    m = sg.d_pair(d_first, d_second, np.dtype(np.float32))
    got = model(m)
    assert got.D == [d_first, d_second] and got.state == 1 and got.eligible == 2
    assert got.offsets == [list(range(d_first)), list(range(1 - d_second, 1))]
    assert len(m[3]) == 64 * (d_first + d_second)
    assert popcount(got.mask).tolist() == [d_first] * 64 + [d_second] * 64


@pytest.mark.parametrize("dtype", sg.DTYPES)
@pytest.mark.parametrize("wider", [False, True])
@pytest.mark.parametrize("nd", sg.FULL_ND)
def test_full_stage_nd(nd, wider, dtype):
    E = sg.entries_per_load(dtype)
    for lead in range(E):
        m = sg.full_stage_nd(nd, lead, wider, np.dtype(dtype))
        got = model(m)
        rp = m[1]
        assert got.D == [4 if lead else 3, nd, nd + 1 if wider else 3] and got.state == 1 and got.eligible == 3
        k0, k1 = int(rp[64]), int(rp[128])
        assert k0 % E == lead and k1 - k0 == 64 * nd and int(rp[-1]) > k1
        # the stream from the aligned start: len = 64 nd + lead, within the nd-slot kernel's clamp and stage
        length = k1 - (k0 & ~(E - 1))
        assert length == 64 * nd + lead <= 64 * nd + E - 1 <= (nd // E + 1) * 64 * E
        assert popcount(got.mask[64:128]).tolist() == [nd] * 64
        assert sg.slots_for(max(got.D)) == (sg.slots_for(nd + 1) if wider else nd)
        assert sg.slots_for(nd + 1) > nd


@pytest.mark.parametrize("tail", sg.TAILS)
@pytest.mark.parametrize("nd", sg.SLOTS)
def test_mask_shapes(nd, tail):
    m = sg.mask_shapes(nd, tail, np.dtype(np.float64))
    shape, rp, ci, v = m
    got = model(m)
    n = 256 + tail
    assert shape == (n, n) and got.segments == 5 and got.eligible == 5 and got.state == 1
    assert got.D[0] == nd and got.D[2] == nd and got.D[3] == nd and max(got.D) == nd
    assert got.offsets[0] == sg.mask_shapes_offsets(nd)
    lengths = np.diff(rp)
    assert np.array_equal(lengths, popcount(got.mask)), "one mask bit per stored entry"
    # segment 0: no empty row, a row of every offset, rows of different lengths
    assert lengths[:64].min() >= 1 and lengths[40] == nd and len(set(lengths[:64].tolist())) > 3
    # segment 1: empty at lane 0, at lane 63 and in two runs; entries in front of and behind every run
    empty = [64, 127] + list(range(80, 90)) + list(range(100, 103))
    assert not lengths[empty].any() and lengths[65] > 0 and lengths[79] > 0 and lengths[90] > 0 and lengths[126] > 0
    assert np.count_nonzero(lengths[64:128]) == 64 - len(empty)
    # segments 2 and 3: everything in lane 63 / in lane 0
    assert lengths[128:192].tolist() == [0] * 63 + [nd] and lengths[192:256].tolist() == [nd] + [0] * 63
    # the last segment
    assert len(lengths) - 256 == tail and lengths[256:].min() >= 1


def test_stencil_band():
    m = sg.stencil_band(np.dtype(np.float64))
    got = model(m)
    assert got.D == [27] * 4 and got.state == 1 and got.eligible == 4 and sg.slots_for(27) == 28
    assert np.diff(m[1])[13:243].tolist() == [27] * 230
    # the groups do not start on a 16-byte boundary everywhere: neighbours share a load
    assert any(int(m[1][64 * s]) % 2 for s in (1, 2, 3))
