"""The numpy reference of the triangular ISAI (tests/isai_refs.py) is itself checked, without a device: it
solves (W A)(i, S_i) = e_i(S_i) to a few ulps, reproduces hand-computed inverses, applies the non-finite rule,
and the stencil factor's pattern rows have the lengths that take the GPU tests through all three kernel paths."""
import numpy as np
import pytest

import factorization_refs as fr
import isai_refs as ir


def stencil_factor(kind, dtype=np.float64):
    """(rp, ci, v, lower) of the IC(0) L or of the ILU(0) U of the 27-point stencil on 12^3 points"""
    rp, ci, v = fr.arrays(fr.stencil27(12), np.int32, dtype)
    if kind == "ic":
        return fr.ic_factor(rp, ci, v) + (True,)
    return fr.ilu_factors(rp, ci, v)[3:] + (False,)


@pytest.fixture(scope="module")
def factors():
    return {(kind, dt): stencil_factor(kind, dt) for kind in ("ic", "ilu") for dt in (np.float64, np.float32)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["ic", "ilu"])
@pytest.mark.parametrize("power", [1, 2])
def test_reference_solves_the_isai_equations_on_the_stencil_factors(factors, kind, dtype, power):
    rp, ci, v, lower = factors[kind, dtype]
    w_rp, w_ci = ir.pattern_power(rp, ci, power)
    w_v = ir.tri_inverse(rp, ci, v, w_rp, w_ci, lower)
    assert w_v.dtype == dtype and np.isfinite(w_v).all()
    err, scale = ir.residual_on_pattern(rp, ci, v, w_rp, w_ci, w_v)
    print("%s %s power %d: max |(W A - I)| on the pattern = %.3g, bound = %.3g"
          % (kind, np.dtype(dtype).name, power, err, 64 * np.finfo(dtype).eps * scale))
    assert err <= 64 * np.finfo(dtype).eps * scale


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_reference_solves_the_isai_equations_on_a_random_pattern(dtype, lower):
    rp, ci, v = ir.lower_from_pattern(fr.random_pattern(600, np.random.default_rng(5), 3), np.random.default_rng(6), dtype)
    if not lower:
        rp, ci, v = ir.transposed(rp, ci, v)
    for power in (1, 2):
        w_rp, w_ci = ir.pattern_power(rp, ci, power)
        w_v = ir.tri_inverse(rp, ci, v, w_rp, w_ci, lower)
        err, scale = ir.residual_on_pattern(rp, ci, v, w_rp, w_ci, w_v)
        print("power %d: %.3g against %.3g" % (power, err, 64 * np.finfo(dtype).eps * scale))
        assert np.isfinite(w_v).all() and err <= 64 * np.finfo(dtype).eps * scale


def test_hand_computed_lower():
    # A = [[2, 0, 0], [1, 4, 0], [0, 2, 8]] on its own pattern
    rp, ci = np.array([0, 1, 3, 5], np.int32), np.array([0, 0, 1, 1, 2], np.int32)
    v = np.array([2.0, 1.0, 4.0, 2.0, 8.0])
    # row 1: w_11 = 1/4, w_10 = (0 - w_11 * 1) / 2 = -1/8;  row 2: w_22 = 1/8, w_21 = (0 - 1/8 * 2) / 4 = -1/16
    want = np.array([0.5, -0.125, 0.25, -0.0625, 0.125])
    assert np.array_equal(ir.tri_inverse(rp, ci, v, rp, ci, True), want)
    # power 2 fills (2, 0): w_20 = (0 - w_21 * a_10) / a_00 = 1/32, the exact inverse
    w_rp, w_ci = ir.pattern_power(rp, ci, 2)
    assert w_rp.tolist() == [0, 1, 3, 6] and w_ci.tolist() == [0, 0, 1, 0, 1, 2]
    want = np.array([0.5, -0.125, 0.25, 0.03125, -0.0625, 0.125])
    assert np.array_equal(ir.tri_inverse(rp, ci, v, w_rp, w_ci, True), want)
    dense = fr.dense_of(w_rp, w_ci, want) @ fr.dense_of(rp, ci, v)
    assert np.array_equal(dense, np.eye(3))


def test_hand_computed_upper():
    # A = [[2, 1, 0], [0, 4, 2], [0, 0, 8]] on its own pattern
    rp, ci = np.array([0, 2, 4, 5], np.int32), np.array([0, 1, 1, 2, 2], np.int32)
    v = np.array([2.0, 1.0, 4.0, 2.0, 8.0])
    # row 0: w_00 = 1/2, w_01 = (0 - w_00 * 1) / 4 = -1/8;  row 1: w_11 = 1/4, w_12 = (0 - 1/4 * 2) / 8 = -1/16
    want = np.array([0.5, -0.125, 0.25, -0.0625, 0.125])
    assert np.array_equal(ir.tri_inverse(rp, ci, v, rp, ci, False), want)
    w_rp, w_ci = ir.pattern_power(rp, ci, 2)
    assert w_ci.tolist() == [0, 1, 2, 1, 2, 2]
    # w_02 = (0 - w_01 * a_12) / a_22 = (1/8 * 2) / 8 = 1/32
    want = np.array([0.5, -0.125, 0.03125, 0.25, -0.0625, 0.125])
    assert np.array_equal(ir.tri_inverse(rp, ci, v, w_rp, w_ci, False), want)


def test_longest_pattern_rows_of_the_stencil_factor(factors):
    """14 / 56 / 144 entries for the powers 1 / 2 / 3: groups of 16 lanes, a wave per row, streamed rows"""
    for kind in ("ic", "ilu"):
        rp, ci, _, _ = factors[kind, np.float64]
        assert [int(np.diff(ir.pattern_power(rp, ci, p)[0]).max()) for p in (1, 2, 3)] == [14, 56, 144]


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_a_zero_pivot_gives_the_identity_row(lower):
    rp, ci, v = ir.lower_from_pattern(fr.random_pattern(50, np.random.default_rng(2)), np.random.default_rng(3))
    diag = rp[1:] - 1
    v[diag[20]] = 0.0
    if not lower:
        rp, ci, v = ir.transposed(rp, ci, v)
    w = ir.tri_inverse(rp, ci, v, rp, ci, lower)
    assert np.isfinite(w).all()
    rows = np.repeat(np.arange(50), np.diff(rp))
    hit = [i for i in range(50) if 20 in ci[rp[i]:rp[i + 1]]]
    assert 20 in hit and len(hit) > 1
    for i in hit:
        assert np.array_equal(w[rows == i], (ci[rows == i] == i).astype(float)), i
    # every other row is untouched by the rule: its diagonal is the reciprocal of A's
    for i in (k for k in range(50) if k not in hit):
        assert w[(rows == i) & (ci == i)][0] == 1.0 / v[(rows == i) & (ci == i)][0]
