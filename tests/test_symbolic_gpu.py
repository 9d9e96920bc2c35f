"""The symbolic Cholesky factorization on the device (gkoc_symbolic_*, ginkgo_amd/csrc/symbolic.hip) against the
row-mark restatement of tests/symbolic_refs.py: patterns are compared integer-exact, in both index types, on the
smallest shapes that reach every path of the kernels - the thresholds come from gkoc_symbolic_row_limits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ginkgo_amd as g
from ginkgo_amd._lib import lib
import factorization_refs as fr
import symbolic_refs as sr

pytestmark = pytest.mark.gpu

ITYPES = [np.int32, np.int64]
ITYPE_IDS = ["i32", "i64"]
GKOC_E_INVALID = -1


def limits():
    out = g.factorization.symbolic_row_limits()
    assert 1 <= len(out) <= 4 and out == sorted(set(out)) and out[0] >= 2
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """a scipy matrix per case; the values only have to be there"""
    rng = np.random.default_rng(5)
    lower = {
        "one": lambda: [[]],
        "diagonal": lambda: [[] for _ in range(9)],
        "blocks": lambda: sr.blocks(sr.arrow_first(6), fr.chain_pattern(5)),
        "chain200": lambda: fr.chain_pattern(200),
        "arrow_first70": lambda: sr.arrow_first(70),
        "arrow_last70": lambda: sr.arrow_last(70),
        "random300": lambda: fr.random_pattern(300, rng, deps=3),
    }
    if name in lower:
        return fr.from_lower_pattern(lower[name](), rng, True)
    if name.startswith("stencil"):
        return fr.stencil27(int(name[7:]))
    if name == "unsymmetric200":
        return sr.unsymmetric()
    if name == "missing_diagonals":
        a = fr.from_lower_pattern(fr.random_pattern(40, rng, deps=2), rng, True).tolil()
        for i in (0, 7, 39):
            a[i, i] = 0
        a = a.tocsr()
        a.eliminate_zeros()
        assert a.diagonal()[7] == 0
        return a
    if name.startswith("hub"):
        n_lower = int(name[3:])
        return fr.from_lower_pattern(fr.hub_pattern(n_lower + 8, n_lower + 2, n_lower, 3), rng, True)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    rp, ci = sr.cholesky_pattern(case(name), np.int64)
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci


def device_matrix(gexec, a, itype):
    rp, ci, v = fr.arrays(a, itype, np.float64)
    return g.Csr.from_arrays(gexec, a.shape, rp, ci, v)


def check_pattern(gexec, name, itype):
    a = case(name)
    dev = device_matrix(gexec, a, itype)
    before = [t.cpu().numpy().copy() for t in (dev.row_ptrs, dev.col_idxs, dev.values)]
    fact = g.factorization.Cholesky.build().with_both_factors(False).on(gexec).generate(dev)
    pattern = fact.get_symbolic()
    rp, ci = pattern.row_ptrs.cpu().numpy(), pattern.col_idxs.cpu().numpy()
    want_rp, want_ci = reference(name)
    assert rp.dtype == itype and ci.dtype == itype
    assert np.array_equal(rp, want_rp) and np.array_equal(ci, want_ci)
    assert np.array_equal(pattern.values.cpu().numpy(), np.ones(len(ci)))
    assert fact.get_l_factor().col_idxs is pattern.col_idxs and fact.get_lt_factor() is None
    for got, kept in zip((dev.row_ptrs, dev.col_idxs, dev.values), before):
        assert np.array_equal(got.cpu().numpy(), kept), "generate changed the caller's matrix"
    return want_rp, want_ci


SHAPES = ["one", "diagonal", "blocks", "chain200", "arrow_first70", "arrow_last70", "stencil5", "stencil8",
          "random300", "unsymmetric200", "missing_diagonals"]


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
@pytest.mark.parametrize("name", SHAPES)
def test_pattern_of_l(gexec, name, itype):
    rp, ci = check_pattern(gexec, name, itype)
    rows = np.diff(rp)
    lim = limits()
    if name == "arrow_first70":
        # fills completely from one stored entry per row: walks of every length up to 69
        assert rows.tolist() == list(range(1, 71)) and 70 - 1 > lim[-1]
    if name == "arrow_last70":
        assert rp[-1] == 69 + 70 and rows.max() - 1 > lim[-1]     # one streamed row, walks of one node
    if name == "chain200":
        assert rp[-1] == 200 + 199
    if name == "stencil5":
        assert (rows.max(), rp[-1]) == (32, 3225)
    if name == "stencil8":
        assert (rows.max(), rp[-1]) == (74, 33216)
    if name == "random300":
        assert rows.max() > 4 * lim[-1]       # three stored entries per row, walks of hundreds of nodes


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
def test_hub_rows_at_every_limit(gexec, itype):
    lim = limits()
    # the last and the first length of every path, and a row that is streamed in several rounds
    for n_lower in sorted({x for limit in lim for x in (limit - 1, limit, limit + 1)} | {3 * lim[-1] + 8}):
        rp, _ = check_pattern(gexec, "hub%d" % n_lower, itype)
        assert np.diff(rp).max() - 1 == n_lower


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
def test_combined_pattern_of_lu(gexec, itype):
    for name in ("unsymmetric200", "stencil5", "missing_diagonals"):
        a = case(name)
        fact = g.factorization.Lu.build().on(gexec).generate(device_matrix(gexec, a, itype))
        m = fact.get_combined()
        want_rp, want_ci = sr.lu_pattern(a, itype)
        assert np.array_equal(m.row_ptrs.cpu().numpy(), want_rp)
        assert np.array_equal(m.col_idxs.cpu().numpy(), want_ci)


# ------------------------------------------------------------------ the entries themselves
def dev(gexec, array):
    return gexec.to_device(np.ascontiguousarray(array))


def raw(name, *args):
    """the status of an entry, without the exception of call()"""
    from ginkgo_amd._lib import _conv
    return getattr(lib(), name)(*[_conv(a) for a in args])


def entry_width(vt, itype):
    return g.entry_dtype(np.float64 if vt == "f64" else np.float32, itype).itemsize


def walk_inputs(lower, itype):
    """host arrays (rp, keys, parent, post, first, inv_post) as the count / expand entries take them"""
    n = len(lower)
    parent, post, first = sr.forest(lower)
    inv = np.zeros(n, np.int64)
    inv[post] = np.arange(n)
    rows = [sorted(int(post[j]) for j in lower[i]) + [int(post[i])] for i in range(n)]
    rp, keys = sr.csr_of_rows(rows, itype)
    return [rp, keys] + [x.astype(itype) for x in (parent, post, first, inv)]


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
def test_forest_and_keys_entries(gexec, itype):
    it = "i32" if itype == np.int32 else "i64"
    lower = sr.lower_rows(sr.symmetrized(case("unsymmetric200")))
    n = len(lower)
    rows = [r + [i] for i, r in enumerate(lower)]
    rp, ci = sr.csr_of_rows(rows, itype)
    d_rp, d_ci = dev(gexec, rp), dev(gexec, ci)
    out = [gexec.alloc((n,), d_rp.dtype).fill_(-7) for _ in range(3)]
    g._lib.call("gkoc_symbolic_forest_" + it, gexec.stream, n, len(ci), d_rp, d_ci, *out)
    parent, post, first = sr.forest(lower)
    for got, want in zip(out, (parent, post, first)):
        assert np.array_equal(got.cpu().numpy(), want.astype(itype))
    keys, inv = gexec.alloc((len(ci),), d_rp.dtype).fill_(-7), gexec.alloc((n,), d_rp.dtype).fill_(-7)
    g._lib.call("gkoc_symbolic_post_keys_" + it, gexec.stream, n, len(ci), d_rp, d_ci, out[1], keys, inv)
    gexec.synchronize()
    assert np.array_equal(keys.cpu().numpy(), post[ci].astype(itype))
    assert np.array_equal(post[inv.cpu().numpy()], np.arange(n))
    # n = 0
    assert raw("gkoc_symbolic_forest_" + it, gexec.stream, 0, 0, None, None, None, None, None) == 0
    assert raw("gkoc_symbolic_post_keys_" + it, gexec.stream, 0, 0, None, None, None, None, None) == 0
    total = C.c_longlong(-5)
    assert raw("gkoc_symbolic_cholesky_count_" + it, gexec.stream, 0, 0, None, None, None, None, None, None, None,
               C.byref(total)) == 0 and total.value == 0
    assert raw("gkoc_symbolic_cholesky_expand_f64_" + it, gexec.stream, 0, 0, None, None, None, None, None, None,
               None, 0, None) == 0


def corrupted(which, arrays, n):
    """the walk inputs with one of the listed defects"""
    rp, keys, parent, post, first, inv = [a.copy() for a in arrays]
    if which == "row pointers descend":
        rp[3] = rp[2] - 1
    elif which == "row pointers do not start at 0":
        rp[0] = 1
    elif which == "row pointers do not end at nnz":
        rp[-1] -= 1
    elif which == "key outside the matrix":
        keys[rp[5]] = n
    elif which == "negative key":
        keys[rp[5]] = -2
    elif which == "parent not above its vertex":
        parent[4] = 4
    elif which == "parent outside the matrix":
        parent[n - 1] = n
    elif which == "post twice":
        post[1] = post[0]
    elif which == "post outside the matrix":
        post[2] = n
    elif which == "inverse does not fit post":
        inv[[0, 1]] = inv[[1, 0]]
    else:
        raise KeyError(which)
    return rp, keys, parent, post, first, inv


DEFECTS = ["row pointers descend", "row pointers do not start at 0", "row pointers do not end at nnz",
           "key outside the matrix", "negative key", "parent not above its vertex", "parent outside the matrix",
           "post twice", "post outside the matrix", "inverse does not fit post"]


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
def test_invalid_inputs_are_refused_before_any_walk(gexec, itype):
    it = "i32" if itype == np.int32 else "i64"
    lower = fr.random_pattern(40, np.random.default_rng(2), deps=3)
    n = len(lower)
    good = walk_inputs(lower, itype)
    nnz = len(good[1])
    want_total = sum(len(r) for r in sr.cholesky_rows(lower))

    def run(arrays):
        d = [dev(gexec, a) for a in arrays]
        offsets = gexec.alloc((n + 1,), torch.int64).fill_(-7)
        total = C.c_longlong(-7)
        rc = raw("gkoc_symbolic_cholesky_count_" + it, gexec.stream, n, nnz, *d, offsets, C.byref(total))
        gexec.synchronize()
        return rc, offsets, total.value, d

    rc, offsets, total, d = run(good)
    assert rc == 0 and total == want_total and int(offsets[-1].item()) == want_total
    for which in DEFECTS:
        bad = corrupted(which, good, n)
        rc, bad_offsets, bad_total, bad_d = run(bad)
        assert rc == GKOC_E_INVALID, which
        assert bad_total == -7 and bool((bad_offsets == -7).all()), which + ": count wrote an output"
        for vt in ("f64", "f32"):
            entries = gexec.alloc((want_total * entry_width(vt, itype),), torch.uint8).fill_(0x5a)
            rc = raw("gkoc_symbolic_cholesky_expand_%s_%s" % (vt, it), gexec.stream, n, nnz, *bad_d, offsets,
                     want_total, entries)
            gexec.synchronize()
            assert rc == GKOC_E_INVALID, which
            assert bool((entries == 0x5a).all()), which + ": expand wrote an output"
    # post_keys and forest: the lower pattern itself, and post
    rows_of = [r + [i] for i, r in enumerate(lower)]
    rp, ci = sr.csr_of_rows(rows_of, itype)
    post = good[3]
    for which, (b_rp, b_ci, b_post) in {
            "row pointers descend": (np.r_[rp[:3], rp[2] - 1, rp[4:]].astype(itype), ci, post),
            "column outside the matrix": (rp, np.r_[ci[:-1], n].astype(itype), post),
            "post twice": (rp, ci, np.r_[post[1], post[1:]].astype(itype))}.items():
        keys, inv = gexec.alloc((len(ci),), d[0].dtype).fill_(-7), gexec.alloc((n,), d[0].dtype).fill_(-7)
        rc = raw("gkoc_symbolic_post_keys_" + it, gexec.stream, n, len(ci), dev(gexec, b_rp), dev(gexec, b_ci),
                 dev(gexec, b_post), keys, inv)
        gexec.synchronize()
        assert rc == GKOC_E_INVALID, which
        assert bool((keys == -7).all()) and bool((inv == -7).all()), which + ": post_keys wrote an output"
        if which != "post twice":
            out = [gexec.alloc((n,), d[0].dtype).fill_(-7) for _ in range(3)]
            rc = raw("gkoc_symbolic_forest_" + it, gexec.stream, n, len(ci), dev(gexec, b_rp), dev(gexec, b_ci), *out)
            gexec.synchronize()
            assert rc == GKOC_E_INVALID, which
            assert all(bool((o == -7).all()) for o in out), which + ": forest wrote an output"


@pytest.mark.parametrize("vt", ["f64", "f32"])
@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
def test_expand_emits_every_entry_once(gexec, itype, vt):
    """the entries before any sort: row i's lie in [offsets[i], offsets[i + 1]) and are its columns, each once,
    with the value 1, in the layout of matrix_data entries"""
    it = "i32" if itype == np.int32 else "i64"
    lower = sr.arrow_first(70)
    n = len(lower)
    arrays = walk_inputs(lower, itype)
    d = [dev(gexec, a) for a in arrays]
    offsets, total = gexec.alloc((n + 1,), torch.int64), C.c_longlong(0)
    g._lib.call("gkoc_symbolic_cholesky_count_" + it, gexec.stream, n, len(arrays[1]), *d, offsets, C.byref(total))
    assert total.value == 70 * 71 // 2
    layout = g.entry_dtype(np.float64 if vt == "f64" else np.float32, itype)
    entries = gexec.alloc((total.value * layout.itemsize,), torch.uint8)
    g._lib.call("gkoc_symbolic_cholesky_expand_%s_%s" % (vt, it), gexec.stream, n, len(arrays[1]), *d, offsets,
                total.value, entries)
    gexec.synchronize()
    off, got = offsets.cpu().numpy(), entries.cpu().numpy().view(layout)
    assert off.tolist() == [i * (i + 1) // 2 for i in range(n + 1)]
    assert (got["value"] == 1).all()
    for i in range(n):
        assert (got["row"][off[i]:off[i + 1]] == i).all()
        assert sorted(got["column"][off[i]:off[i + 1]].tolist()) == list(range(i + 1))
