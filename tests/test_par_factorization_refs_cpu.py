"""The two consequences of the ParIlu / ParIc contract that include/gko_cdna4.h states, on the numpy
restatement alone (no device): after as many sweeps as the lower solve has levels the sweeps ARE the exact
ILU(0) / IC(0), bit for bit, and stay it; after one and two sweeps they are not - so a device result that
matches the restatement at few sweeps cannot have come from the exact kernel."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import factorization_refs as fr
import par_factorization_refs as pr

KINDS = ["ilu", "ic"]
DTYPES = [np.float64, np.float32]
CASES = {"chain": 40, "stencil": 36, "random": None}      # the number of levels where the shape fixes it


@functools.lru_cache(maxsize=None)
def case(name, kind, dtype):
    """(rp, ci, v) the sweeps work on: the matrix (ilu) or its lower triangle (ic); read-only"""
    rng = np.random.default_rng(300)
    if name == "chain":
        a = fr.from_lower_pattern(fr.chain_pattern(40), rng, kind == "ic")
    elif name == "stencil":
        a = fr.stencil27(6)
    else:
        a = fr.from_lower_pattern(fr.random_pattern(300, rng, 3), rng, kind == "ic")
    out = fr.arrays(sp.tril(a, format="csr") if kind == "ic" else a, np.int32, dtype)
    for x in out:
        x.setflags(write=False)
    return out


def sweeps(kind, rp, ci, v, iterations):
    return (pr.ilu_sweeps if kind == "ilu" else pr.ic_sweeps)(rp, ci, v, iterations)


def exact(kind, rp, ci, v):
    return (fr.ilu0 if kind == "ilu" else fr.ic0)(rp, ci, v)


def test_num_levels():
    assert pr.num_levels(np.array([0]), np.array([], np.int32)) == 0
    assert pr.num_levels(np.arange(6), np.arange(5)) == 1
    for name, want in CASES.items():
        for kind in KINDS:
            rp, ci, _ = case(name, kind, np.float64)
            levels = pr.num_levels(rp, ci)
            assert levels == (want or levels) and 1 < levels <= len(rp) - 1
    # the full matrix and its lower triangle have the same schedule
    assert pr.num_levels(*case("random", "ilu", np.float64)[:2]) == pr.num_levels(*case("random", "ic", np.float64)[:2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_exact_after_as_many_sweeps_as_levels_and_not_before(kind, name, dtype):
    rp, ci, v = case(name, kind, dtype)
    want = exact(kind, rp, ci, v)
    assert np.isfinite(want).all()
    levels = pr.num_levels(rp, ci)
    for iterations in (levels, levels + 1):
        got, changes = sweeps(kind, rp, ci, v, iterations)
        assert got.dtype == dtype and np.array_equal(got, want), iterations
        # ilu: a row without lower entries is its input, so all rows are exact after levels - 1 sweeps and
        # sweep `levels` changes nothing.  ic: such a row still takes the root of its diagonal in sweep 1, so
        # the induction alone promises 0 only at levels + 1; on these matrices (more than one level) the
        # last level's rows have converged in floating point before, and 0 holds at `levels` as well.
        assert changes == 0, iterations
    for iterations in (1, 2):
        got, changes = sweeps(kind, rp, ci, v, iterations)
        assert not np.array_equal(got, want) and changes > 0, iterations
        assert np.isfinite(got).all()
    # the input is left alone
    assert np.array_equal(v, case(name, kind, dtype)[2])


@pytest.mark.parametrize("kind", KINDS)
def test_the_sweeps_contract(kind):
    """the largest relative error against the exact factor falls with every sweep (stencil on 6^3 points)"""
    rp, ci, v = case("stencil", kind, np.float64)
    want = exact(kind, rp, ci, v)
    err = [np.abs((sweeps(kind, rp, ci, v, k)[0] - want) / want).max() for k in (1, 2, 3, 5)]
    print(kind, err)
    assert err[0] > err[1] > err[2] > err[3] > 0


def test_the_contraction_figures_of_the_header():
    """include/gko_cdna4.h: ILU on the stencil on 12^3 points, largest relative error of an entry 9.7e-2,
    2.1e-2, 4.3e-3, 1.6e-4 after 1, 2, 3, 5 sweeps (two digits are stated, so 5 % is their rounding)"""
    rp, ci, v = fr.arrays(fr.stencil27(12))
    want = fr.ilu0(rp, ci, v)
    swept = pr.ilu_sweeps_at(rp, ci, v, (1, 2, 3, 5))
    for iterations, stated in ((1, 9.7e-2), (2, 2.1e-2), (3, 4.3e-3), (5, 1.6e-4)):
        err = np.abs((swept[iterations][0] - want) / want).max()
        print(iterations, err)
        assert abs(err - stated) <= 0.05 * stated


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_split_of_the_sweep_result(dtype):
    rp, ci, v = case("random", "ilu", dtype)
    swept, changes = pr.ilu_sweeps(rp, ci, v, 2)
    factors, changes_2 = pr.par_ilu_factors(rp, ci, v, 2)
    assert changes == changes_2
    for got, want in zip(factors, fr.split_l_u(rp, ci, swept)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    # ic: the split comes first, the sweeps run on L's values
    (l_rp, l_ci, l_v), _ = pr.par_ic_factor(rp, ci, v, 2)
    low = fr.split_l(rp, ci, v)
    assert np.array_equal(l_rp, low[0]) and np.array_equal(l_ci, low[1])
    assert np.array_equal(l_v, pr.ic_sweeps(*low, 2)[0])
