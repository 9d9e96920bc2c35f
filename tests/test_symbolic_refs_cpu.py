"""tests/symbolic_refs.py is the yardstick of tests/test_symbolic_gpu.py and tests/test_direct_gpu.py, so it is
pinned here without a device: the forest on hand-written cases, the row-mark pattern against boolean dense
elimination on every case of at most 600 rows, and the skeleton rule of the device kernels against both."""
import numpy as np
import pytest
import scipy.sparse as sp

import factorization_refs as fr
import symbolic_refs as sr


def _cases():
    rng = np.random.default_rng(5)
    return {
        "one": [[]],
        "diagonal": [[] for _ in range(9)],
        "blocks": sr.blocks(sr.arrow_first(6), fr.chain_pattern(5)),
        "chain200": fr.chain_pattern(200),
        "arrow_first70": sr.arrow_first(70),
        "arrow_last70": sr.arrow_last(70),
        "stencil5": sr.lower_rows(sr.symmetrized(fr.stencil27(5))),
        "stencil6": sr.lower_rows(sr.symmetrized(fr.stencil27(6))),
        "stencil8": sr.lower_rows(sr.symmetrized(fr.stencil27(8))),
        "random300": fr.random_pattern(300, rng, deps=3),
        "unsymmetric200": sr.lower_rows(sr.symmetrized(sr.unsymmetric())),
        "hub": fr.hub_pattern(120, 70, 64, 3),
    }


CASES = _cases()


def test_forest_of_a_chain():
    parent, post, first = sr.forest(fr.chain_pattern(5))
    assert parent.tolist() == [1, 2, 3, 4, -1]
    assert post.tolist() == [0, 1, 2, 3, 4] and first.tolist() == [0, 0, 0, 0, 0]


def test_forest_of_a_star():
    # the hub last: every leaf is its child, visited in ascending index
    parent, post, first = sr.forest(sr.arrow_last(5))
    assert parent.tolist() == [4, 4, 4, 4, -1]
    assert post.tolist() == [0, 1, 2, 3, 4] and first.tolist() == [0, 1, 2, 3, 0]
    # the hub first: elimination turns the star into a chain
    parent, post, first = sr.forest(sr.arrow_first(5))
    assert parent.tolist() == [1, 2, 3, 4, -1] and first.tolist() == [0, 0, 0, 0, 0]


def test_forest_of_two_trees_and_isolated_vertices():
    #   tree A: 0 -> 3, 1 -> 3, 3 -> 6        tree B: 2 -> 5        isolated: 4, 7
    lower = [[], [], [], [0, 1], [], [2], [3], []]
    parent, post, first = sr.forest(lower)
    assert parent.tolist() == [3, 3, 5, 6, -1, -1, -1, -1]
    # roots ascending: 4, then 5 (after its child 2), then 6 (after 0, 1, 3), then 7
    assert post.tolist() == [3, 4, 1, 5, 0, 2, 6, 7]
    assert first.tolist() == [3, 4, 1, 3, 0, 1, 3, 7]


def test_path_compression_does_not_change_the_forest():
    # 0 - 2, 1 - 2 ... a pattern where a compressed ancestor is reached twice
    lower = [[], [0], [0], [1], [0, 2], [3, 4]]
    parent = sr.forest(lower)[0]
    fill = sr.dense_fill(sr.matrix_of_lower(lower).toarray())
    for v in range(len(lower)):
        below = np.nonzero(fill[v + 1:, v])[0]
        assert parent[v] == (below[0] + v + 1 if len(below) else -1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_row_marks_equal_dense_elimination(name):
    lower = CASES[name]
    n = len(lower)
    assert n <= 600
    rows = sr.cholesky_rows(lower)
    fill = sr.dense_fill(sr.matrix_of_lower(lower).toarray())
    assert rows == [np.nonzero(fill[i])[0].tolist() for i in range(n)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_forest_invariants_and_the_skeleton_rule(name):
    lower = CASES[name]
    n = len(lower)
    parent, post, first = sr.forest(lower)
    assert sorted(post.tolist()) == list(range(n))
    assert all(parent[v] == -1 or parent[v] > v for v in range(n))
    assert all(parent[v] == -1 or (first[parent[v]] <= first[v] and post[v] < post[parent[v]]) for v in range(n))
    rows = sr.cholesky_rows(lower, parent)
    walked, lookups = sr.skeleton_rows(lower, parent, post, first)
    assert walked == rows
    assert lookups == sum(len(r) for r in rows) - n


def test_sizes_the_device_tests_rely_on():
    longest = {k: max(len(r) for r in sr.cholesky_rows(CASES[k])) for k in ("stencil5", "stencil8", "random300")}
    nnz = {k: sum(len(r) for r in sr.cholesky_rows(CASES[k])) for k in ("stencil5", "stencil8", "random300")}
    assert (longest["stencil5"], nnz["stencil5"]) == (32, 3225)
    assert (longest["stencil8"], nnz["stencil8"]) == (74, 33216)
    assert longest["random300"] > 64
    assert [len(r) for r in sr.cholesky_rows(sr.arrow_first(70))] == list(range(1, 71))
    assert sum(len(r) for r in sr.cholesky_rows(sr.arrow_last(70))) == 69 + 70


def test_patterns_of_a_matrix():
    a = sr.unsymmetric()
    assert (a != a.T).nnz > 0
    rp, ci = sr.cholesky_pattern(a)
    fill = sr.dense_fill((abs(a) + abs(a.T)).toarray() != 0)
    assert np.array_equal(ci, np.nonzero(fill)[1]) and rp[-1] == fill.sum()
    m_rp, m_ci = sr.lu_pattern(a)
    full = fill | fill.T
    assert np.array_equal(m_ci, np.nonzero(full)[1]) and m_rp[-1] == full.sum()
    v = sr.on_filled_pattern(a, m_rp, m_ci, np.float64)
    assert np.array_equal(sp.csr_matrix((v, m_ci, m_rp), shape=a.shape).toarray(), a.toarray())
