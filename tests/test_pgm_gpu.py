"""Pgm on the device against the numpy restatement of tests/pgm_refs.py.  The aggregation is integers only and the
coarse operator and the transfers promise the restatement's rounding, so everything is compared with
np.array_equal, in all four (value, index) type pairs."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ginkgo_amd as g
import pgm_refs as pr
from ginkgo_amd._lib import _conv, lib
from test_factorization_gpu import TYPES, TYPE_IDS, csr_arrays, shuffled, strided

pytestmark = pytest.mark.gpu

LIMITS = g.multigrid.row_limits()
HUBS = ["hub%d" % (L + d) for L in LIMITS for d in (-1, 0, 1)]
# case -> Pgm parameters
CASES = {"one": {}, "identity": {}, "chain": {}, "chain_one_round": {"max_iterations": 1}, "stencil": {},
         "star": {}, "scaled": {}, "random": {}, **{h: {} for h in HUBS}}
_MATRICES, _REFS = {}, {}       # computed once per key; the tests do not change them


def hub_matrix(length, rng):
    """symmetric, distinct weights; row 0 of W has `length` entries (its diagonal and length - 1 neighbours),
    every other row at most 2"""
    n = length + 40
    k = np.arange(1, length)
    off = rng.uniform(0.5, 1.5, length - 1)
    a = sp.coo_matrix((np.concatenate([rng.uniform(2, 3, n), -off, -off]),
                       (np.concatenate([np.arange(n), np.zeros(length - 1, int), k]),
                        np.concatenate([np.arange(n), k, np.zeros(length - 1, int)]))), shape=(n, n)).tocsr()
    a.sort_indices()
    return a


def matrix(name):
    """the case's matrix as scipy CSR in f64, rows sorted"""
    base = "chain" if name == "chain_one_round" else name
    if base not in _MATRICES:
        rng = np.random.default_rng(len(base) * 13 + 5)
        if base == "one":
            a = sp.csr_matrix(np.array([[2.0]]))
        elif base == "identity":
            a = sp.identity(300, format="csr")
        elif base == "chain":
            a = pr.chain(2500)
        elif base == "stencil":
            a = pr.stencil27(12)
        elif base == "star":
            a = pr.star(700)
        elif base == "scaled":
            # a random symmetric positive scaling: the weights are distinct, the hash decides nothing
            s = sp.diags(rng.uniform(0.5, 2.0, 12 ** 3))
            a = (s @ pr.stencil27(12) @ s).tocsr()
        elif base == "random":
            # unsymmetric PATTERN, about 3 entries per row and a diagonal: W's pattern is A u A^T
            n = 4000
            rows = np.repeat(np.arange(n), 3)
            a = sp.coo_matrix((rng.uniform(-1, 1, 3 * n), (rows, rng.integers(0, n, 3 * n))), shape=(n, n)).tocsr()
            a.sum_duplicates()
            a = (a - sp.diags(a.diagonal()) + sp.diags(rng.uniform(1, 2, n))).tocsr()
            a.eliminate_zeros()
            assert ((a != 0) != (a != 0).T).nnz > 0
        elif base.startswith("hub"):
            a = hub_matrix(int(base[3:]), rng)
        else:
            raise KeyError(name)
        a.sort_indices()
        _MATRICES[base] = a
    return _MATRICES[base]


def reference(name, vt):
    """the restatement's aggregation and coarse operator of a case in the value type vt"""
    key = (name, vt)
    if key not in _REFS:
        rp, ci, v = pr.triple(matrix(name), vt)
        res = pr.aggregate(rp, ci, v, vt, **CASES[name])
        res["coarse"] = pr.coarse_operator(rp, ci, v, res["agg"], res["n_coarse"], vt)
        for x in (res["agg"],) + res["coarse"]:
            x.setflags(write=False)
        _REFS[key] = res
    return _REFS[key]


def device_matrix(gexec, name, vt, it):
    rp, ci, v = pr.triple(matrix(name), vt, it)
    n = len(rp) - 1
    return g.Csr.from_arrays(gexec, (n, n), rp, ci, v)


def generate(gexec, a, **params):
    f = g.Pgm.build()
    for k, val in params.items():
        f = getattr(f, "with_" + k)(val)
    return f.on(gexec).generate(a)


def rc(name, *args):
    """the return code of an entry, no exception"""
    return getattr(lib(), name)(*[_conv(a) for a in args])


# ------------------------------------------------------------------ the aggregation
@pytest.mark.parametrize("vt,it", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_aggregation_equals_the_restatement(gexec, name, vt, it):
    ref = reference(name, vt)
    level = generate(gexec, device_matrix(gexec, name, vt, it), **CASES[name])
    agg = level.get_agg().cpu().numpy()
    assert agg.dtype == it
    assert (level.rounds, level.num_leftover, level.get_num_aggregates()) == \
        (ref["rounds"], ref["leftover"], ref["n_coarse"])
    assert np.array_equal(agg, ref["agg"])
    # the member lists: the rows of every aggregate, ascending
    order = np.argsort(ref["agg"], kind="stable")
    assert np.array_equal(level.members.cpu().numpy(), order)
    assert np.array_equal(level.member_ptrs.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(ref["agg"]))]))


def test_the_checkpoints_hold_on_the_device(gexec):
    """the figures the contract was accepted with (f64): stencil 5 rounds / 29 left / 826, star one aggregate"""
    level = generate(gexec, device_matrix(gexec, "stencil", np.float64, np.int32))
    assert (level.rounds, level.num_leftover, level.get_num_aggregates()) == (5, 29, 826)
    level = generate(gexec, device_matrix(gexec, "star", np.float64, np.int32))
    assert (level.rounds, level.get_num_aggregates()) == (2, 1)
    assert level.get_fine_op().size == (701, 701) and level.get_coarse_op().size == (1, 1)


# ------------------------------------------------------------------ coarse operator and transfers
@pytest.mark.parametrize("vt,it", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["stencil", "scaled", "random", "star"])
def test_coarse_operator_and_transfers_are_bit_identical(gexec, name, vt, it):
    ref = reference(name, vt)
    level = generate(gexec, device_matrix(gexec, name, vt, it))
    c_rp, c_ci, c_v = csr_arrays(level.get_coarse_op())
    assert c_ci.dtype == it and c_v.dtype == vt
    assert np.array_equal(c_rp, ref["coarse"][0]) and np.array_equal(c_ci, ref["coarse"][1])
    assert np.array_equal(c_v, ref["coarse"][2])
    n, nc, agg = len(ref["agg"]), ref["n_coarse"], ref["agg"]
    rng = np.random.default_rng(17)
    one = g.scalar(gexec, 1.0, torch.from_numpy(np.empty(0, vt)).dtype)
    for cols, ld in ((1, 1), (3, 3), (3, 5), (1, 2)):
        r = rng.uniform(-1, 1, (n, cols)).astype(vt)
        e = rng.uniform(-1, 1, (nc, cols)).astype(vt)
        dr, _ = strided(gexec, r, ld)
        dbc, bc_store = strided(gexec, np.zeros((nc, cols), vt), ld, fill=7.0)
        level.get_restrict_op().apply(dr, dbc)
        assert np.array_equal(dbc.to_numpy(), pr.restrict(agg, nc, r))
        assert np.all(bc_store.cpu().numpy()[:, cols:] == 7.0)         # the padding is not written
        de, _ = strided(gexec, e, ld)
        dx, x_store = strided(gexec, r, ld, fill=7.0)
        level.get_prolong_op().apply(one, de, one, dx)                  # the add kernel
        assert np.array_equal(dx.to_numpy(), pr.prolong_add(agg, e, r))
        assert np.all(x_store.cpu().numpy()[:, cols:] == 7.0)
        level.get_prolong_op().apply(de, dx)                            # overwrites
        assert np.array_equal(dx.to_numpy(), e[agg])


def test_unsorted_input_gives_the_same_hierarchy_and_is_left_alone(gexec):
    rp, ci, v = pr.triple(matrix("random"), np.float64, np.int32)
    sci, sv = shuffled(rp, ci, v, np.random.default_rng(23))
    assert not np.array_equal(sci, ci)
    a = g.Csr.from_arrays(gexec, (len(rp) - 1,) * 2, rp, sci, sv)
    level = generate(gexec, a)
    ref = reference("random", np.float64)
    assert np.array_equal(level.get_agg().cpu().numpy(), ref["agg"])
    for got, want in zip(csr_arrays(level.get_coarse_op()), ref["coarse"]):
        assert np.array_equal(got, want)
    after = csr_arrays(a)
    assert np.array_equal(after[0], rp) and np.array_equal(after[1], sci) and np.array_equal(after[2], sv)
    assert level.get_fine_op() is a


def test_fbcsr_input_equals_its_csr(gexec):
    rng = np.random.default_rng(29)
    pattern = sp.random(150, 150, density=0.03, random_state=rng, format="csr") + sp.identity(150, format="csr")
    bsr = sp.kron(pattern, np.ones((2, 2))).tobsr((2, 2))
    bsr.data[:] = rng.uniform(0.5, 1.5, bsr.data.shape)
    bsr.sort_indices()
    fb = g.Fbcsr.from_scipy(gexec, bsr)
    a, b = generate(gexec, fb), generate(gexec, fb.convert_to_csr())
    assert a.get_fine_op() is fb and a.get_num_aggregates() == b.get_num_aggregates() < 300
    assert np.array_equal(a.get_agg().cpu().numpy(), b.get_agg().cpu().numpy())
    for x, y in zip(csr_arrays(a.get_coarse_op()), csr_arrays(b.get_coarse_op())):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ invalid input: return codes only
@pytest.mark.parametrize("it", [np.int32, np.int64], ids=["i32", "i64"])
def test_invalid_input_is_refused_by_return_code(gexec, it):
    """every index an entry uses was checked by it: nothing below reads or writes out of bounds"""
    suf = "i32" if it == np.int32 else "i64"
    dev = lambda x, dt=it: gexec.to_device(np.asarray(x, dt))       # noqa: E731
    st, invalid = gexec.stream, -1
    n = 4
    rp, ci = dev([0, 2, 4, 6, 8]), dev([0, 1, 0, 1, 2, 3, 2, 3])
    wv, d = dev(np.ones(8), np.float64), dev(np.ones(4), np.float64)
    agg, prop = dev([-1] * n), dev([-9] * n)
    select = "gkoc_pgm_select_f64_" + suf
    assert rc(select, st, n, rp, ci, wv, d, agg, prop) == 0
    assert np.array_equal(prop.cpu().numpy(), [1, 0, 3, 2])
    prop.fill_(-9)
    for bad_rp in ([1, 2, 4, 6, 8], [0, 2, 1, 6, 8], [0, -1, 4, 6, 8]):
        assert rc(select, st, n, dev(bad_rp), ci, wv, d, agg, prop) == invalid
        assert rc("gkoc_pgm_leftover_f64_" + suf, st, n, dev(bad_rp), ci, wv, d, agg, prop) == invalid
    for bad_ci in ([0, 1, 0, 1, 2, 3, 2, 4], [0, 1, 0, -1, 2, 3, 2, 3]):
        assert rc(select, st, n, rp, dev(bad_ci), wv, d, agg, prop) == invalid
    assert rc(select, st, n, rp, ci, wv, d, agg, agg) == invalid       # reads what it writes
    assert rc(select, st, n, rp, ci, None, d, agg, prop) == invalid
    assert np.all(prop.cpu().numpy() == -9)                            # nothing was written
    # match: a proposal outside the matrix
    count = C.c_longlong(-5)
    for bad in ([1, 0, 4, 2], [1, 0, -7, 2]):
        assert rc("gkoc_pgm_match_" + suf, st, n, dev(bad), agg, C.byref(count)) == invalid
    assert np.all(agg.cpu().numpy() == -1)
    assert rc("gkoc_pgm_match_" + suf, st, n, dev([1, 0, 3, -2 - 0]), agg, C.byref(count)) == 0
    assert np.array_equal(agg.cpu().numpy(), [0, 0, -1, 0]) and count.value == 1
    # renumber: agg must hold roots
    coarse = C.c_longlong(-5)
    for bad in ([0, 0, -1, 0], [0, 0, 4, 0], [1, 0, 2, 2]):
        assert rc("gkoc_pgm_renumber_" + suf, st, n, dev(bad), C.byref(coarse)) == invalid
    roots = dev([0, 0, 3, 3])
    assert rc("gkoc_pgm_renumber_" + suf, st, n, roots, C.byref(coarse)) == 0
    assert coarse.value == 2 and np.array_equal(roots.cpu().numpy(), [0, 0, 1, 1])
    # map_entries: agg inside [0, n_coarse), indices inside the matrix
    rows, vals = dev([0, 0, 1, 1, 2, 2, 3, 3]), dev(np.arange(8.0), np.float64)
    width = g.entry_dtype(np.float64, it)
    entries = gexec.to_device(np.full(8 * width.itemsize, 0xAB, np.uint8))
    map_entries = "gkoc_pgm_map_entries_f64_" + suf
    assert rc(map_entries, st, 8, n, 2, dev([0, 0, 2, 1]), rows, ci, vals, entries) == invalid
    assert rc(map_entries, st, 8, n, 2, dev([0, 0, -1, 1]), rows, ci, vals, entries) == invalid
    assert rc(map_entries, st, 8, n, 2, roots, dev([0, 0, 1, 1, 2, 2, 3, 4]), ci, vals, entries) == invalid
    assert rc(map_entries, st, 8, n, 2, roots, rows, dev([0, 1, 0, 1, 2, 3, 2, -1]), vals, entries) == invalid
    assert np.all(entries.cpu().numpy() == 0xAB)                       # nothing was written
    assert rc(map_entries, st, 8, n, 2, roots, rows, ci, vals, entries) == 0
    got = entries.cpu().numpy().view(width)
    assert np.array_equal(got["row"], [0, 0, 0, 0, 1, 1, 1, 1]) and np.array_equal(got["column"], got["row"])
    assert np.array_equal(got["value"], np.arange(8.0))
    # check_transfers
    check = "gkoc_pgm_check_transfers_" + suf
    ptrs, members = dev([0, 2, 4]), dev([0, 1, 2, 3])
    assert rc(check, st, n, 2, roots, ptrs, members) == 0
    assert rc(check, st, n, 2, dev([0, 0, 1, 2]), ptrs, members) == invalid
    for bad in ([0, 2, 5], [1, 2, 4], [0, 3, 2], [0, 2, 3]):
        assert rc(check, st, n, 2, roots, dev(bad), members) == invalid
    assert rc(check, st, n, 2, roots, ptrs, dev([0, 1, 2, 4])) == invalid
    assert rc(check, st, n, 5, roots, ptrs, members) == invalid        # more aggregates than rows
    # the transfers check their host arguments
    r, bc = dev(np.ones((4, 2)), np.float64), dev(np.zeros((2, 2)), np.float64)
    assert rc("gkoc_pgm_restrict_f64_" + suf, st, 2, 2, ptrs, members, r, 1, bc, 2) == invalid
    assert rc("gkoc_pgm_prolong_add_f64_" + suf, st, n, 2, roots, bc, 2, r, 1) == invalid
    assert rc("gkoc_pgm_restrict_f64_" + suf, st, 2, 2, ptrs, members, r, 2, bc, 2) == 0
    assert np.array_equal(bc.cpu().numpy(), [[2, 2], [2, 2]])
    gexec.synchronize()
