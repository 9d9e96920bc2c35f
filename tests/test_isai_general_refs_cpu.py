"""The numpy restatement of the general / spd ISAI contract (tests/isai_general_refs.py) pinned by itself:
against numpy.linalg.solve on the dense blocks in float64, by its residual where pivoting matters, and on
hand-made rows with the answers written out."""
import functools
import time

import numpy as np
import pytest

import factorization_refs as fr
import isai_general_refs as gr

WELL = [(6, 1, False), (6, 1, True), (5, 2, False), (5, 2, True)]
LONGEST = {(6, 1, True): 14, (6, 1, False): 27, (5, 2, True): 63, (5, 2, False): 125}
# measured on the restatement: max |w - w_lapack| / max |w_lapack| in eps of the dtype,
#   6^3 power 1: general 3.04 (f64) 1.43 (f32), spd 0.63 / 0.60;  5^3 power 2: general 5.17 / 5.79, spd 1.25 / 1.30
LARGEST_RATIO = 5.79
# measured on the restatement: max |(W A - I) on the pattern| / (eps * the largest row sum of |W| |A|) of the
# weak-diagonal matrix: 0.002 (f64), 0.001 (f32); the row sums reach 5.8e7 there
WEAK_C = 0.002


@functools.lru_cache(maxsize=None)
def well_case(grid, power, spd, dtype):
    rp, ci, v = fr.arrays(fr.stencil27(grid), np.int32, dtype)
    w_rp, w_ci = gr.lower_pattern_power(rp, ci, power) if spd else gr.pattern_power(rp, ci, power)
    return rp, ci, v, w_rp, w_ci, gr.general_inverse(rp, ci, v, w_rp, w_ci, spd)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("grid,power,spd", WELL, ids=["%d^3-p%d-%s" % (g_, p, "spd" if s else "general")
                                                      for g_, p, s in WELL])
def test_well_conditioned_rows_agree_with_lapack(grid, power, spd, dtype):
    """measured: 0.6 to 5.8 eps of the dtype (the table above), no identity row; the bound is 16 x the largest
    ratio, because LAPACK eliminates in another order, not because of the conditioning"""
    rp, ci, v, w_rp, w_ci, w = well_case(grid, power, spd, dtype)
    assert int(np.diff(w_rp).max()) == LONGEST[(grid, power, spd)]
    assert w.dtype == dtype and np.isfinite(w).all() and not gr.identity_rows(w_rp, w_ci, w).any()
    want = gr.lapack_inverse(rp, ci, v, w_rp, w_ci, spd)
    ratio = np.abs(w - want).max() / np.abs(want).max() / np.finfo(dtype).eps
    print("ratio %.2f eps" % ratio)
    assert ratio <= 16 * LARGEST_RATIO


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_matrix_where_pivoting_matters(dtype):
    """random 400 x 400, density 0.02, off-diagonals in [-1, 1], diagonal in [0.01, 0.1]: the longest row has
    17 entries, 369 rows take a pivot out of the diagonal order, every row is finite.  The forward difference
    to LAPACK is no yardstick here, the residual on the pattern is: measured c = 0.002 (f64) / 0.001 (f32) in
    err <= c eps scale, bound 8 x 0.002"""
    rp, ci, v = gr.weak_diagonal(dtype=dtype)
    assert len(rp) == 401 and int(np.diff(rp).max()) >= 12
    stats = {}
    w = gr.general_inverse(rp, ci, v, rp, ci, False, stats)
    assert np.isfinite(w).all() and not gr.identity_rows(rp, ci, w).any()
    assert stats["rows_pivoted_off_the_diagonal"] >= 1
    err, scale = gr.residual_on_pattern(rp, ci, v, rp, ci, w)
    print("c = %.4f, rows pivoted %d" % (err / (np.finfo(dtype).eps * scale), stats["rows_pivoted_off_the_diagonal"]))
    assert err <= 8 * WEAK_C * np.finfo(dtype).eps * scale


def full(dense, dtype=np.float64):
    """(rp, ci, v) storing EVERY entry of `dense`, zeros included"""
    return fr.on_pattern(np.array(dense, dtype), np.ones(np.shape(dense), bool), np.int32, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_tie_goes_to_the_smaller_row(dtype):
    # both rows of W see M = A^T = [[2, 1], [-2, 3]]: |2| = |-2| in column 0, row 0 is the pivot
    rp, ci, v = full([[2, -2], [1, 3]], dtype)
    stats = {}
    w = gr.general_inverse(rp, ci, v, rp, ci, False, stats)
    assert [list(q) for q in stats["pivots"]] == [[0, 1], [0, 1]]
    # A^-1 = [[3, 2], [-1, 2]] / 8, every step exact in binary
    assert np.array_equal(w, np.array([0.375, 0.25, -0.125, 0.25], dtype))
    # the larger row wins where it is larger, whatever its index
    rp, ci, v = full([[1, -2], [1, 3]], dtype)
    stats = {}
    gr.general_inverse(rp, ci, v, rp, ci, False, stats)
    assert list(stats["pivots"][0]) == [1, 0]


def test_a_permutation_needs_its_pivots():
    rp, ci, v = full([[0, 1, 0], [1, 0, 0], [0, 0, 2]])
    stats = {}
    w = gr.general_inverse(rp, ci, v, rp, ci, False, stats)
    assert np.array_equal(w, [0, 1, 0, 1, 0, 0, 0, 0, 0.5])
    assert stats["rows_pivoted_off_the_diagonal"] == 3


def test_a_zero_pivot_column_gives_the_identity_row():
    # rows 0 and 1 see the singular block [[0, 1], [0, 1]]; row 2 stores its diagonal only
    rp = np.array([0, 2, 4, 5], np.int32)
    ci = np.array([0, 1, 0, 1, 2], np.int32)
    v = np.array([0.0, 1.0, 0.0, 1.0, 4.0])
    w = gr.general_inverse(rp, ci, v, rp, ci, False)
    assert np.array_equal(w, [1, 0, 0, 1, 0.25])
    assert list(gr.identity_rows(rp, ci, w)) == [True, True, False]


def test_spd_scaling_and_a_negative_last_w():
    # the lower pattern is full (zeros are stored): rows {0}, {0, 1}, {0, 1, 2}; row 2 solves
    # M = [[2, 0, 1], [0, 8, 1], [0, 0, -4]] w = e_2: w_2 = -0.25 < 0, its root is no number, so the row is the
    # identity's; rows 0 and 1: w = 1 / a_ii divided by its own root
    rp, ci, v = full([[2, 0, 0], [0, 8, 0], [1, 1, -4]])
    w_rp, w_ci = gr.lower_pattern_power(rp, ci, 1)
    assert list(w_rp) == [0, 1, 3, 6] and list(w_ci) == [0, 0, 1, 0, 1, 2]
    w = gr.general_inverse(rp, ci, v, w_rp, w_ci, True)
    # rows 0 and 1: w = 1 / a_ii divided by its own root
    assert np.array_equal(w, [0.5 / np.sqrt(0.5), 0, 0.125 / np.sqrt(0.125), 0, 0, 1])
    # the same row with a positive diagonal: w = (-1/8, -1/32, 1/4) / sqrt(1/4), BOTH triangles of A are read
    rp, ci, v = full([[2, 0, 1], [0, 8, 1], [1, 1, 4]])
    stats = {}
    w = gr.general_inverse(rp, ci, v, w_rp, w_ci, True, stats)
    m = np.array([[2.0, 0, 1], [0, 8, 1], [1, 1, 4]])
    want = np.linalg.solve(m, [0, 0, 1.0])
    assert np.allclose(w[3:], want / np.sqrt(want[2]), rtol=4 * np.finfo(np.float64).eps, atol=0)
    assert w[3] != 0 and w[4] != 0


def test_a_nan_poisons_its_rows_only():
    rp, ci, v = (x.copy() for x in gr.convection(4))
    rows = np.repeat(np.arange(64), np.diff(rp))
    v[np.flatnonzero((rows == 21) & (ci == 22))[0]] = np.nan
    w = gr.general_inverse(rp, ci, v, rp, ci, False)
    assert np.isfinite(w).all()
    identity = gr.identity_rows(rp, ci, w)
    # every row whose block contains the entry (21, 22): the rows that store both columns
    dense = np.zeros((64, 64), bool)
    dense[rows, ci] = True
    assert np.array_equal(identity, dense[:, 21] & dense[:, 22]) and identity.sum() >= 2


def test_the_hub_references_stay_under_a_second():
    """the GPU tests compute one reference per hub length: every one must be cheap here"""
    for length in (16, 17, 32, 33, 64, 65, 128):
        for spd in (False, True):
            start = time.perf_counter()
            rp, ci, v = gr.hub(length, spd)
            w_rp, w_ci = gr.lower_pattern_power(rp, ci, 1) if spd else (rp, ci)
            assert int(np.diff(w_rp).max()) == length and np.sort(np.diff(w_rp))[-2] <= 3
            w = gr.general_inverse(rp, ci, v, w_rp, w_ci, spd)
            assert time.perf_counter() - start < 1.0
            assert np.isfinite(w).all() and not gr.identity_rows(w_rp, w_ci, w).any()
            err, scale = gr.residual_on_pattern(rp, ci, v, w_rp, w_ci, w)
            if not spd:
                assert err <= 64 * np.finfo(np.float64).eps * scale
