"""The nested-dissection contract (include/gko_cdna4.h, "Nested dissection") pinned on its numpy restatement,
tests/reorder_refs.py, without a device: the recursion is a permutation with the properties the contract claims,
the stages that the device entries expose compose to the same permutation, and the ordering does what it is for -
fewer levels in the factor's lower solve."""
import numpy as np
import pytest
import scipy.sparse as sp

import reorder_refs as rr
import symbolic_refs as sr

CASES = rr.edge_cases()
GRIDS = {
    "27p_4": (rr.stencil27(4), 8),
    "27p_5": (rr.stencil27(5), 8),
    "5p_20": (rr.stencil5(20), 8),
    "chain_200": (rr.chain(200), 8),
    "27p_5_leaf1": (rr.stencil27(5), 1),
    "5p_20_leaf64": (rr.stencil5(20), 64),
}
ALL = {**CASES, **GRIDS}


@pytest.fixture(scope="module")
def runs():
    """name -> (perm, trace) of the recursion, computed once"""
    out = {}
    for name, (a, leaf) in ALL.items():
        trace = []
        out[name] = (rr.nested_dissection(a, leaf, trace), trace)
    return out


@pytest.mark.parametrize("name", sorted(ALL))
def test_result_is_a_permutation(runs, name):
    perm = runs[name][0]
    assert np.array_equal(np.sort(perm), np.arange(ALL[name][0].shape[0]))


@pytest.mark.parametrize("name", sorted(ALL))
def test_every_split_separates(runs, name):
    """A, B, S are non-empty and partition R; no stored edge joins A and B (brute force over the edges); S is
    ascending; the size bounds of the contract"""
    a, leaf = ALL[name]
    adj = rr.neighbours(a)
    for d in runs[name][1]:
        r, pa, pb, ps = d["R"], d["A"], d["B"], d["S"]
        assert pa and pb and ps
        assert sorted(pa + pb + ps) == r and len(set(pa + pb + ps)) == len(r)
        assert ps == sorted(ps) and len(r) > leaf
        in_b = set(pb)
        assert not any(u in in_b for v in pa for u in adj[v])
        assert 1 <= d["m"] <= d["h"] - 1
        if d["m"] == d["mstar"]:
            # |A| itself has no bound: test_a_itself_has_no_size_bound
            assert d["below"] < (len(r) + 1) // 2
            assert len(pb) <= len(r) // 2


def test_a_itself_has_no_size_bound(runs):
    """the counter-example of the header: a wide level m outside the separator goes to A"""
    d = runs["wide_level"][1][0]
    assert (d["m"], d["mstar"], d["S"]) == (2, 2, [1]) and len(d["A"]) == 12 and len(d["R"]) == 14


@pytest.mark.parametrize("name", sorted(ALL))
def test_separator_follows_what_it_separates(runs, name):
    """positions: order(A) ++ order(B) ++ ascending(S) inside R's own contiguous segment"""
    perm, trace = runs[name]
    pos = np.empty(len(perm), np.int64)
    pos[perm] = np.arange(len(perm))
    for d in trace:
        start = min(pos[v] for v in d["R"])
        assert sorted(pos[v] for v in d["R"]) == list(range(start, start + len(d["R"])))
        assert max(pos[v] for v in d["A"]) < min(pos[v] for v in d["B"])
        assert [pos[v] for v in d["S"]] == list(range(start + len(d["R"]) - len(d["S"]), start + len(d["R"])))


@pytest.mark.parametrize("name", sorted(ALL))
def test_stages_compose_to_the_recursion(runs, name):
    a, leaf = ALL[name]
    rp, ci = rr.csr_arrays(a, np.int64)
    perm, rounds, _ = rr.by_rounds(rp, ci, a.shape[0], leaf)
    assert np.array_equal(perm, runs[name][0])
    depth = max((d["depth"] for d in runs[name][1]), default=-1) + 1
    assert rounds in (depth, depth + 1) or a.shape[0] <= leaf


# (nnz(L), levels) in natural order and after the ordering: what the restatement gives, leaf_size 8
PINNED = {
    "27p_4": ((1072, 64), (942, 38)),
    "5p_20": ((8019, 400), (4443, 53)),
    "chain_200": ((399, 200), (583, 11)),
    "arrow_first": ((5050, 100), (199, 2)),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_fewer_levels_than_natural_order(runs, name):
    a = ALL[name][0]
    natural, reordered = rr.factor_shape(a), rr.factor_shape(rr.permuted(a, runs[name][0]))
    assert (natural, reordered) == PINNED[name]
    assert reordered[1] < natural[1]


def test_fewer_levels_on_the_8_cube():
    a = rr.stencil27(8)
    perm = rr.nested_dissection(a, 8)
    assert rr.factor_shape(a) == (33216, 512)
    assert rr.factor_shape(rr.permuted(a, perm)) == (35231, 226)


def test_edge_cases_by_hand(runs):
    assert len(runs["empty"][0]) == 0 and list(runs["single"][0]) == [0]
    # nothing to divide: the identity
    for name in ("diagonal", "clique40"):
        assert np.array_equal(runs[name][0], np.arange(ALL[name][0].shape[0])) and not runs[name][1]
    # leaf_size >= n: ascending(R) at once, the components are NOT grouped (step 1 comes before step 2)
    assert np.array_equal(runs["leaf_all"][0], np.arange(40))
    # two interleaved chains of 30: the even component first, each dissected on its own
    perm = runs["interleaved"][0]
    assert sorted(perm[:30]) == list(range(0, 60, 2)) and sorted(perm[30:]) == list(range(1, 60, 2))
    # the hub is the only separator of an arrow, wherever it stands, and the leaves are left in ascending order
    assert list(runs["arrow_first"][0]) == list(range(1, 100)) + [0]
    assert list(runs["arrow_last"][0]) == [1, 0] + list(range(2, 100))      # the second sweep starts at 1: A = {1}
    assert [d["S"] for d in runs["arrow_first"][1]] == [[0]] and [d["S"] for d in runs["arrow_last"][1]] == [[99]]
    # leaf_size 1 on the 7 x 7 grid: nine splits, the rest ends as single vertices or undivided (h < 2)
    assert len(runs["leaf1"][1]) == 9


def test_components_between_grouping_and_leaves():
    """a region larger than the leaf size that is disconnected: components ordered by their smallest vertex, and
    a component of at most leaf_size vertices ascending"""
    a = rr.interleaved(20)
    perm = rr.nested_dissection(a, 10)
    assert list(perm) == list(range(0, 20, 2)) + list(range(1, 20, 2))


def test_region_that_falls_into_many_components():
    a, leaf = CASES["star_of_chains"]
    trace = []
    rr.nested_dissection(a, leaf, trace)
    adj = rr.neighbours(a)
    assert max(len(rr.components_of(adj, d["A"])) for d in trace) >= 3 or \
        max(len(rr.components_of(adj, d["B"])) for d in trace) >= 3


def test_unsymmetric_pattern_is_symmetrised():
    a = sr.unsymmetric()
    assert (a != a.T).nnz > 0
    perm = rr.nested_dissection(a, 8)
    s = sp.csr_matrix(sr.symmetrized(a), dtype=np.float64)
    assert np.array_equal(perm, rr.nested_dissection(s, 8))


def test_stage_counts():
    """what the device's loops are pinned against: a chain of n needs n sweeps and n steps, the bound exactly"""
    n = 9
    rp, ci = rr.csr_arrays(rr.chain(n), np.int64)
    region = np.zeros(n, np.int64)
    label, sweeps = rr.components(rp, ci, region)
    assert not label.any() and sweeps == n
    level, steps = rr.levels(rp, ci, region, np.arange(n))
    assert list(level) == list(range(n)) and steps == n
    assert rr.far_roots(region, level)[0] == n - 1
    cls = rr.split(rp, ci, np.arange(n), region, level)
    assert list(cls) == [0, 0, 0, 0, 2, 1, 1, 1, 1]
