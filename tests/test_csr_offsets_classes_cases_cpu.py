"""The class definition of the CSR column-offset plan (csrc/csr_offsets.hpp) restated in numpy
(tests/csr_offsets_classes_cases.py), checked on the matrices of tests/test_csr_offsets_classes_gpu.py, so that a
bug in a builder or in the restatement cannot make a device case vacuous.  No device."""
import numpy as np
import pytest

import csr_offsets_cases as oc
import csr_offsets_classes_cases as cc


@pytest.mark.parametrize("grid,classes", [(8, 3), (12, 14), (16, 9)])
def test_stencil_class_counts(oracle, grid, classes):
    """the 27-point stencil: 8 / 27 / 64 segments in 3 / 14 / 9 classes"""
    _, rp, ci, _ = cc.stencil27(oracle, grid)
    assert len(cc.class_keys(rp, ci)) == grid ** 3 // 64
    assert cc.class_count(rp, ci) == classes


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_cases_have_the_classes_they_are_built_for(oracle, name):
    build, classes = cc.CASES[name]
    shape, rp, ci, v = build(oracle, np.float64)
    assert oc.is_csr(rp, ci, shape) and len(v) == len(ci)
    keys = cc.class_keys(rp, ci)
    assert all(len(k) == 97 for k in keys)
    assert cc.class_count(rp, ci) == classes
    assert max(cc.class_ids(rp, ci)) == classes - 1
    # with every hash equal the leader is segment 0: between the true count and one class per segment
    assert classes <= cc.class_count_all_collide(rp, ci) <= len(keys)


@pytest.mark.parametrize("grid,rows_last", [(5, 61), (7, 23)])
def test_partial_last_segment_carries_zero_masks(oracle, grid, rows_last):
    """125 and 343 rows: the last segment's key has mask 0 for the rows at or behind n_rows, and is eligible"""
    _, rp, ci, _ = cc.stencil27(oracle, grid)
    key = cc.class_keys(rp, ci)[-1]
    assert (grid ** 3) % 64 == rows_last and key[0] > 0
    masks = key[oc.OFFS_MAX + 1:]
    assert all(m != 0 for m in masks[:rows_last]) and all(m == 0 for m in masks[rows_last:])


def test_tridiagonal_classes():
    """segments 1 and 2 share a class, 0 and 3 do not; a hole in segment 2 splits them: same offsets, other masks"""
    _, rp, ci, _ = cc.tridiagonal()
    assert cc.class_ids(rp, ci) == [0, 1, 1, 2]
    _, rp, ci, _ = cc.tridiagonal(hole=True)
    keys = cc.class_keys(rp, ci)
    assert cc.class_ids(rp, ci) == [0, 1, 2, 3]
    assert keys[1][:oc.OFFS_MAX + 1] == keys[2][:oc.OFFS_MAX + 1] and keys[1] != keys[2]


def test_two_bands_differ_in_their_offsets_alone():
    _, rp, ci, _ = cc.two_bands()
    keys = cc.class_keys(rp, ci)
    assert cc.class_ids(rp, ci) == [0, 1, 2, 1, 2, 3]
    assert keys[1][oc.OFFS_MAX + 1:] == keys[2][oc.OFFS_MAX + 1:], "equal masks"
    assert keys[1][:4] == (3, -2, 0, 2) and keys[2][:4] == (3, -1, 0, 1)


def test_unsorted_row_makes_one_ineligible_class():
    _, rp, ci, _ = cc.one_unsorted_row()
    model = oc.plan_model(rp, ci)
    assert (model.eligible, model.segments, model.state) == (4, 5, 1) and model.D[2] == 0
    assert cc.class_keys(rp, ci)[2] == (0,) * 97
    assert cc.class_ids(rp, ci) == [0, 1, 2, 1, 3]


def test_plan_bytes_formula(oracle):
    _, rp, ci, _ = cc.stencil27(oracle, 12)
    assert cc.plan_bytes(rp, ci, 14) == 4 * 27 + 388 * 14
    _, rp, ci, _ = cc.one_unsorted_row()
    assert cc.plan_bytes(rp, ci, 4) == 4 * 5 + 388 * 4 + 4
