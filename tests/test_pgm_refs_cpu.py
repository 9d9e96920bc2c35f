"""The numpy restatement of the Pgm contract (tests/pgm_refs.py) reproduces the checkpoints of the prototype the
contract was written from, in f64, and keeps the invariants of an aggregation on every case.  No device."""
import numpy as np
import pytest
import scipy.sparse as sp

import pgm_refs as pr

# case -> (matrix, aggregate() parameters, rounds, leftover rows, aggregates, largest aggregate)
CASES = {
    "stencil12": (lambda: pr.stencil27(12), {}, 5, 29, 826, 4),
    "chain": (lambda: pr.chain(2500), {}, 2, 81, 1078, None),
    "chain_one_round": (lambda: pr.chain(2500), {"max_iterations": 1}, 1, 850, 932, None),
    "star": (lambda: pr.star(700), {}, 2, 0, 1, 701),
    "identity": (lambda: sp.identity(300, format="csr"), {}, 1, 0, 300, 1),
}
_RESULTS = {}


def result(name):
    if name not in _RESULTS:
        make, params = CASES[name][:2]
        a = make()
        rp, ci, v = pr.triple(a)
        _RESULTS[name] = (a, pr.aggregate(rp, ci, v, np.float64, **params))
    return _RESULTS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_prototype_checkpoints(name):
    _, params, rounds, leftover, aggregates, largest = CASES[name]
    _, res = result(name)
    assert (res["rounds"], res["leftover"], res["n_coarse"]) == (rounds, leftover, aggregates)
    if largest is not None:
        assert np.bincount(res["agg"]).max() == largest
    if name == "chain":
        assert leftover < 0.05 * 2500      # the ratio stop, not the count


@pytest.mark.parametrize("name", list(CASES))
def test_invariants(name):
    a, res = result(name)
    n, nc, agg = a.shape[0], res["n_coarse"], res["agg"]
    assert agg.shape == (n,) and agg.min() >= 0                       # every row is assigned
    assert np.array_equal(np.unique(agg), np.arange(nc))              # exactly 0 .. n_c - 1
    assert np.array_equal(res["roots"][res["roots"]], res["roots"])   # a root is its own root
    rp, ci, v = pr.triple(a)
    c_rp, c_ci, c_v = pr.coarse_operator(rp, ci, v, agg, nc, np.float64)
    p = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))
    want = (p.T @ a @ p).tocsr()
    want.sort_indices()
    got = sp.csr_matrix((c_v, c_ci, c_rp), shape=(nc, nc))
    assert np.array_equal(c_rp, want.indptr) and np.array_equal(c_ci, want.indices)
    np.testing.assert_allclose(got.data, want.data, rtol=1e-13, atol=0)
    # the transfers are P^T and P
    r = np.random.default_rng(5).uniform(-1, 1, (n, 2))
    np.testing.assert_allclose(pr.restrict(agg, nc, r), p.T @ r, rtol=1e-13, atol=1e-15)
    e = np.random.default_rng(6).uniform(-1, 1, (nc, 2))
    assert np.array_equal(pr.prolong_add(agg, e, r), r + p @ e)


def test_weights_are_symmetric_and_exact_on_an_unsymmetric_pattern():
    rng = np.random.default_rng(11)
    a = sp.random(200, 200, density=0.02, random_state=rng, format="csr") + sp.identity(200, format="csr")
    a.sort_indices()
    rp, ci, v = pr.triple(a)
    w_rp, w_ci, w_v, d = pr.weights(rp, ci, v, np.float64)
    w = sp.csr_matrix((w_v, w_ci, w_rp), shape=a.shape)
    want = (0.5 * abs(a) + 0.5 * abs(a).T).tocsr()
    assert (w != w.T).nnz == 0 and abs(w - want).max() == 0
    assert np.array_equal(d, w.diagonal())


def test_hash_is_symmetric_and_32_bit():
    i, j = np.arange(0, 5000, 7), np.arange(5000, 0, -7)
    h = pr.pair_hash(i, j)
    assert np.array_equal(h, pr.pair_hash(j, i)) and h.max() < 2 ** 32
    # the spelled-out formula on one pair
    def spelled(lo, hi, m=0xFFFFFFFF):
        x = ((lo * 0x9E3779B1) & m) ^ ((hi * 0x85EBCA77) & m)
        x ^= x >> 15
        x = (x * 0x2C1B3C6D) & m
        return x ^ (x >> 12)
    assert int(pr.pair_hash(np.array([9]), np.array([3]))[0]) == spelled(3, 9)
    # min and max are taken of the whole indices, then both are truncated to 32 bits
    assert int(pr.pair_hash(np.array([3 + 2 ** 32]), np.array([9]))[0]) == spelled(9, 3)


def test_level_list_and_host_pcg_counts_on_the_model_problem():
    a = pr.stencil27(12)
    rp, ci, v = pr.triple(a)
    levels = pr.hierarchy(rp, ci, v, np.float64)
    assert [len(lv["rp"]) - 1 for lv in levels] == [1728, 826, 391, 184, 88, 41]
    b = np.random.default_rng(3).uniform(-1, 1, 12 ** 3)
    diag = a.diagonal()
    assert pr.pcg_iterations(a, b, lambda r: pr.cycle(levels, r[:, None])[:, 0]) == 12
    assert pr.pcg_iterations(a, b, lambda r: r / diag) == 32
    assert pr.pcg_iterations(a, b, lambda r: pr.cycle(levels, r[:, None], kind="w")[:, 0]) <= 12
