"""The builders of tests/test_csr_offsets_pipeline_gpu.py on the CPU, against csr_offsets_cases.plan_model: the D of
every segment, the share of eligible segments, the entry counts and stream starts their docstrings promise - so that
a bug in a builder cannot make a device case vacuous."""
import numpy as np
import pytest

import csr_offsets_cases as oc
import test_csr_offsets_pipeline_gpu as pg


def model(m):
    shape, rp, ci, v = m
    assert oc.is_csr(rp, ci, shape) and len(v) == len(ci) and rp.dtype == ci.dtype == np.int32
    return oc.plan_model(rp, ci)


@pytest.mark.parametrize("spec", pg.PATTERNS)
def test_patterns(spec):
    m = pg.pattern(spec.replace("E", "B"), np.dtype(np.float64))
    got = model(m)
    assert [d > 0 for d in got.D] == [k in "BE" for k in spec]
    for seg, kind in enumerate(spec):
        if kind == "W":
            r0 = 64 * seg
            union = {c - r for r in range(r0, r0 + 64) for c in oc.rows_of(m)[r]}
            assert len(union) == 33 and all(row == sorted(row) and len(row) == 3 for row in oc.rows_of(m)[r0:r0 + 64])
    assert got.state == 1, "at least half of the segments are eligible: the plan is used"
    rp = m[1]
    for s, kind in enumerate(spec):
        assert (rp[64 * s + 64] == rp[64 * s]) == (kind == "0")


@pytest.mark.parametrize("d_first,d_second", [(3, 9), (9, 3), (8, 9), (9, 8), (1, 32), (32, 1), (1, 8), (8, 1)])
def test_d_pairs(d_first, d_second):
    m = pg.d_pair(d_first, d_second, np.dtype(np.float32))
    got = model(m)
    assert got.D == [d_first, d_second] and got.state == 1
    assert got.offsets == [list(range(d_first)), list(range(1 - d_second, 1))]
    assert len(m[3]) == 64 * (d_first + d_second)


@pytest.mark.parametrize("full_first", [True, False])
def test_stage_edges(full_first):
    m = pg.stage_edges(full_first, np.dtype(np.float64))
    got = model(m)
    assert got.D == ([32, 1] if full_first else [1, 32]) and got.state == 1
    assert np.diff(m[1][[0, 64, 128]]).tolist() == ([oc.CAP, 1] if full_first else [1, oc.CAP])


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_unaligned(lead):
    m = pg.unaligned(lead, np.dtype(np.float32))
    got = model(m)
    assert got.D == [4, 3] and got.state == 1 and int(m[1][64]) == 192 + lead


@pytest.mark.parametrize("n", [64, 65, 127, 128, 192])
def test_tri(n):
    got = model(pg.tri(n, np.dtype(np.float64)))
    assert got.D == [3 if n - 64 * s > 1 else 2 for s in range(-(-n // 64))] and got.state == 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dot_model_tells_the_groupings_apart(oracle, dtype):
    """the matrix and vector of test_fused_dot_really_runs_two_segments_per_wave: one wave of two segments and two
    waves of one fold <b, c> to different bits, both within rounding of the exact sum"""
    dtype = np.dtype(dtype)
    _, rp, ci, v = pg.d_pair(32, 9, dtype)
    b = np.random.default_rng(71).uniform(-1, 1, 128).astype(dtype)
    term = (b * oracle.csr_spmv(rp, ci, v, b)).astype(dtype)
    one, two = pg.dot_model(term, 2, dtype), pg.dot_model(term, 1, dtype)
    exact = float(np.sum(term.astype(np.longdouble)))
    bound = 128 * np.finfo(dtype).eps * float(np.abs(term).sum())
    assert one != two and abs(float(one) - exact) <= bound and abs(float(two) - exact) <= bound
