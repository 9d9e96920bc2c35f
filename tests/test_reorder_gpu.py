"""The nested dissection on the device (gkoc_reorder_*, ginkgo_amd/csrc/reorder.hip, reorder.NestedDissection)
against the restatement of tests/reorder_refs.py, integer-exact in both index types: every entry alone on the
states the restatement passes through, the class on the edge cases and the grids, rows around every limit of
gkoc_reorder_row_limits with the one deciding neighbour stored last (and first), more vertices than one pass of
the grid covers, and the checks."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ginkgo_amd as g
from ginkgo_amd._lib import _conv, lib
import factorization_refs as fr
import reorder_refs as rr
import symbolic_refs as sr

pytestmark = pytest.mark.gpu

ITYPES = [np.int32, np.int64]
ITYPE_IDS = ["i32", "i64"]
GKOC_OK, GKOC_E_INVALID = 0, -1


def raw(name, itype, *args):
    """the status of gkoc_reorder_<name>_<itype>"""
    fn = getattr(lib(), f"gkoc_reorder_{name}_{'i32' if itype == np.int32 else 'i64'}")
    return fn(*[_conv(a) for a in args])


def dev(gexec, array, itype):
    return gexec.to_device(np.ascontiguousarray(np.asarray(array).astype(itype)))


def host(t):
    return t.cpu().numpy().astype(np.int64)


class Device:
    """the five entries on numpy arrays: outputs come back as int64 arrays"""

    def __init__(self, gexec, rp, ci, itype):
        self.ex, self.itype, self.n = gexec, itype, len(rp) - 1
        self.rp, self.ci = dev(gexec, rp, itype), dev(gexec, ci, itype)
        self.pattern = (gexec.stream, self.n, len(ci), self.rp, self.ci)

    def out(self, fill=-7):
        return dev(self.ex, np.full(self.n, fill), self.itype)

    def components(self, region):
        label, sweeps = self.out(), C.c_longlong(-1)
        assert raw("components", self.itype, *self.pattern, dev(self.ex, region, self.itype), label,
                   C.byref(sweeps)) == GKOC_OK
        return host(label), sweeps.value

    def levels(self, region, root):
        level, steps = self.out(), C.c_longlong(-1)
        assert raw("levels", self.itype, *self.pattern, dev(self.ex, region, self.itype),
                   dev(self.ex, root, self.itype), level, C.byref(steps)) == GKOC_OK
        return host(level), steps.value

    def far_roots(self, region, level):
        far = self.out()
        assert raw("far_roots", self.itype, self.ex.stream, self.n, dev(self.ex, region, self.itype),
                   dev(self.ex, level, self.itype), far) == GKOC_OK
        return host(far)

    def split(self, order, region, level):
        cls = self.out()
        assert raw("split", self.itype, *self.pattern, dev(self.ex, order, self.itype),
                   dev(self.ex, region, self.itype), dev(self.ex, level, self.itype), cls) == GKOC_OK
        return host(cls)

    def regroup(self, leaf, final_from, key, order, region):
        o, r, live = dev(self.ex, order, self.itype), dev(self.ex, region, self.itype), C.c_longlong(-1)
        assert raw("regroup", self.itype, self.ex.stream, self.n, leaf, final_from, dev(self.ex, key, self.itype),
                   o, r, C.byref(live)) == GKOC_OK
        return host(o), host(r), live.value


@functools.lru_cache(maxsize=None)
def stage_states(name):
    """every state the restatement passes through on a small pattern: a list of (stage, inputs, outputs)"""
    a, leaf = {"grid7": (rr.stencil5(7), 4), "two_chains": (rr.interleaved(24), 3),
               "star": (rr.star_of_chains(4, 6), 3), "cube3": (rr.stencil27(3), 2)}[name]
    rp, ci = rr.csr_arrays(a, np.int64)
    n = a.shape[0]
    order, region = rr.initial_state(n, leaf)
    out, live = [], n
    while live:
        label, sweeps = rr.components(rp, ci, region)
        out.append(("components", (region,), (label, sweeps)))
        new = rr.regroup(leaf, n, label, order, region)
        out.append(("regroup", (leaf, n, label, order, region), new))
        order, region, live = new
        if not live:
            break
        l0, steps = rr.levels(rp, ci, region, order)
        out.append(("levels", (region, order), (l0, steps)))
        far = rr.far_roots(region, l0)
        out.append(("far_roots", (region, l0), far))
        level, steps = rr.levels(rp, ci, region, far)
        out.append(("levels", (region, far), (level, steps)))
        cls = rr.split(rp, ci, order, region, level)
        out.append(("split", (order, region, level), cls))
        new = rr.regroup(leaf, 2, cls, order, region)
        out.append(("regroup", (leaf, 2, cls, order, region), new))
        order, region, live = new
    return rp, ci, out


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
@pytest.mark.parametrize("name", ["grid7", "two_chains", "star", "cube3"])
def test_every_entry_alone(gexec, name, itype):
    rp, ci, states = stage_states(name)
    d = Device(gexec, rp, ci, itype)
    seen = set()
    for stage, inputs, want in states:
        got = getattr(d, stage)(*inputs)
        seen.add(stage)
        if isinstance(want, tuple):
            assert len(got) == len(want)
            for x, y in zip(got, want):
                assert np.array_equal(x, y), (stage, x, y)
        else:
            assert np.array_equal(got, want), (stage, got, want)
    assert seen == {"components", "levels", "far_roots", "split", "regroup"}


def test_row_limits(gexec):
    lim = g.reorder.row_limits()
    assert 1 <= len(lim) <= 4 and lim == sorted(set(lim)) and lim[0] >= 2


# ------------------------------------------------------------------ the class
@functools.lru_cache(maxsize=None)
def class_case(name):
    cases = rr.edge_cases()
    if name in cases:
        return cases[name]
    rng = np.random.default_rng(5)
    grids = {"27p_4": lambda: rr.stencil27(4), "27p_5": lambda: rr.stencil27(5), "27p_8": lambda: rr.stencil27(8),
             "5p_20": lambda: rr.stencil5(20),
             "random300": lambda: fr.from_lower_pattern(fr.random_pattern(300, rng, deps=3), rng, True)}
    kind, leaf = name.rsplit("_leaf", 1)
    return grids[kind](), int(leaf)


@functools.lru_cache(maxsize=None)
def class_reference(name):
    a, leaf = class_case(name)
    perm = rr.nested_dissection(a, leaf)
    perm.setflags(write=False)
    return perm


def device_matrix(gexec, a, itype):
    a = sp.csr_matrix(a)
    a.sort_indices()
    return g.Csr.from_arrays(gexec, a.shape, a.indptr.astype(itype), a.indices.astype(itype),
                             a.data.astype(np.float64))


def run_class(gexec, a, leaf, itype):
    nd = g.reorder.NestedDissection(g.NestedDissection.build().with_leaf_size(leaf).on(gexec),
                                    device_matrix(gexec, a, itype))
    perm = nd.permutation.get_permutation().cpu().numpy()
    assert perm.dtype == itype
    return perm, nd


CLASS_CASES = sorted(rr.edge_cases()) + ["27p_4_leaf8", "27p_5_leaf8", "27p_8_leaf8", "5p_20_leaf8", "random300_leaf8",
                                         "27p_5_leaf1", "27p_5_leaf64", "5p_20_leaf1", "5p_20_leaf64",
                                         "random300_leaf1", "random300_leaf64"]


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
@pytest.mark.parametrize("name", CLASS_CASES)
def test_class_against_the_recursion(gexec, name, itype):
    a, leaf = class_case(name)
    dm = device_matrix(gexec, a, itype)
    before = [t.cpu().numpy().copy() for t in (dm.row_ptrs, dm.col_idxs, dm.values)]
    p = g.NestedDissection.build().with_leaf_size(leaf).on(gexec).generate(dm)
    assert isinstance(p, g.Permutation)
    assert np.array_equal(p.get_permutation().cpu().numpy(), class_reference(name))
    for got, kept in zip((dm.row_ptrs, dm.col_idxs, dm.values), before):
        assert np.array_equal(got.cpu().numpy(), kept), "generate changed the caller's matrix"


def test_rounds_and_launches_of_the_class(gexec):
    """the class waits for exactly the sweeps and steps the restatement counts"""
    a = rr.stencil5(20)
    rp, ci = rr.csr_arrays(a, np.int64)
    perm, rounds, waits = rr.by_rounds(rp, ci, 400, 8)
    got, nd = run_class(gexec, a, 8, np.int32)
    assert np.array_equal(got, perm) and (nd.rounds, nd.launches) == (rounds, waits)


# ------------------------------------------------------------------ rows around the limits
def decisive(d, first):
    """H has d neighbours: d - 1 twigs and c.  G - twigs - H - c - d tail vertices.  From a tail vertex the only
    neighbour of H with a level when H is found is c; from G the median level is H's alone (m = 2) and the only
    neighbour of H at level m + 1 is c.  c is the FIRST stored entry of H's row or the LAST.
    Returns (matrix, H, c, G, a tail vertex)."""
    if first:
        c, h, twigs = 0, 1, list(range(2, d + 1))
    else:
        twigs, h, c = list(range(d - 1)), d - 1, d
    big = d + 1
    tail = list(range(d + 2, 2 * d + 2))
    edges = [(big, t) for t in twigs] + [(t, h) for t in twigs] + [(h, c)] + [(c, t) for t in tail]
    a = rr.of_edges(2 * d + 2, edges)
    row = sr.symmetrized(a)[h].indices
    assert len(row) == d + 1 and (row[0] if first else row[-1]) == c
    return a, h, c, big, tail[0]


def limit_lengths():
    lim = g.reorder.row_limits()
    return sorted({x + k for x in lim for k in (-1, 0, 1, 2)} | {151})


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
@pytest.mark.parametrize("first", [False, True], ids=["last", "first"])
def test_rows_around_the_limits(gexec, first, itype):
    """a vertex whose row has L - 1, L, L + 1, L + 2 entries for every limit L, and 151 (three rounds of 64): a
    streaming round that is dropped, or a group that stops early, loses the deciding neighbour"""
    for length in limit_lengths():
        d = length - 1
        a, h, c, big, tail = decisive(d, first)
        n = a.shape[0]
        rp, ci = rr.csr_arrays(a, np.int64)
        dv = Device(gexec, rp, ci, itype)
        region, order = np.zeros(n, np.int64), np.arange(n)
        # levels: H is found through c alone
        root = np.full(n, tail)
        want, steps = rr.levels(rp, ci, region, root)
        assert (want[c], want[h]) == (1, 2)
        got = dv.levels(region, root)
        assert np.array_equal(got[0], want) and got[1] == steps, length
        # split: H is the separator because of c alone
        level, _ = rr.levels(rp, ci, region, np.full(n, big))
        assert (level[h], level[c]) == (2, 3)
        cls = rr.split(rp, ci, order, region, level)
        assert cls[h] == 2 and list(cls).count(2) == 1
        assert np.array_equal(dv.split(order, region, level), cls), length
        # components: the smallest label reaches H through its row
        label, sweeps = rr.components(rp, ci, region)
        got = dv.components(region)
        assert np.array_equal(got[0], label) and got[1] == sweeps, length
        perm, _ = run_class(gexec, a, 4, itype)
        assert np.array_equal(perm, rr.nested_dissection(a, 4)), length


# ------------------------------------------------------------------ more vertices than one pass of the grid
def test_more_rows_than_one_pass(gexec):
    """the row kernels give a row to a group of 16 lanes here (5 entries at most): 16 rows per workgroup, at most
    4 * 2048 workgroups (stream_grid), so one pass covers 131072 rows.  3700 disjoint 6 x 6 five-point grids are
    133200 vertices: all of them are dissected at once, in the rounds one block needs, and the restatement is run
    on one block."""
    copies, leaf = 3700, 8
    block = rr.stencil5(6)
    assert copies * 36 > 4 * 2048 * 16
    one = rr.nested_dissection(block, leaf)
    rp, ci = rr.csr_arrays(block, np.int64)
    _, rounds, waits = rr.by_rounds(rp, ci, 36, leaf)
    a = sp.block_diag([block] * copies, format="csr")
    perm, nd = run_class(gexec, a, leaf, np.int32)
    want = (one[None, :] + 36 * np.arange(copies)[:, None]).ravel()
    assert np.array_equal(perm, want)
    # the first components pass labels all blocks at once: the sweeps are those of one block
    assert nd.rounds == rounds and nd.launches == waits and rounds <= 5


# ------------------------------------------------------------------ the checks
@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
def test_invalid_input_is_refused_and_nothing_written(gexec, itype):
    a = rr.stencil5(5)
    n = 25
    rp, ci = rr.csr_arrays(a, np.int64)
    region, order = np.zeros(n, np.int64), np.arange(n)
    level, _ = rr.levels(rp, ci, region, order)
    descending = rp.copy()
    descending[3], descending[4] = rp[4], rp[3]
    bad_column = ci.copy()
    bad_column[7] = n
    bad_region = region.copy()
    bad_region[5] = n
    bad_level = level.copy()
    bad_level[6] = n
    unlevelled = level.copy()
    unlevelled[6] = -1
    bad_order = order.copy()
    bad_order[2] = 3
    bad_key = np.zeros(n, np.int64)
    bad_key[4] = n
    count = C.c_longlong(-5)

    def refused(name, arrays, host_result=True, with_pattern=True, scalars=()):
        """arrays: name -> (numpy array, is output).  Outputs are filled with -7 and must keep it."""
        x = {k: dev(gexec, np.full(n, -7) if is_out and v is None else v, itype) for k, (v, is_out) in arrays.items()}
        before = {k: host(t).copy() for k, t in x.items()}
        args = [gexec.stream, n]
        if with_pattern:
            args += [len(ci), x.pop("rp"), x.pop("ci")]
        args += list(scalars) + list(x.values()) + ([C.byref(count)] if host_result else [])
        assert raw(name, itype, *args) == GKOC_E_INVALID, (name, list(arrays))
        assert lib().gkoc_last_error()
        for k, t in x.items():
            assert np.array_equal(host(t), before[k]), (name, k)

    for bad_rp, bad_ci, bad_reg in ((descending, ci, region), (rp, bad_column, region), (rp, ci, bad_region)):
        pat = {"rp": (bad_rp, False), "ci": (bad_ci, False)}
        refused("components", {**pat, "region": (bad_reg, False), "label": (None, True)})
        refused("levels", {**pat, "region": (bad_reg, False), "root": (order, False), "level": (None, True)})
        refused("split", {**pat, "order": (order, False), "region": (bad_reg, False), "level": (level, False),
                          "cls": (None, True)}, host_result=False)
    pat = {"rp": (rp, False), "ci": (ci, False)}
    refused("levels", {**pat, "region": (region, False), "root": (np.full(n, -1), False), "level": (None, True)})
    for lv in (bad_level, unlevelled):
        refused("split", {**pat, "order": (order, False), "region": (region, False), "level": (lv, False),
                          "cls": (None, True)}, host_result=False)
        refused("far_roots", {"region": (region, False), "level": (lv, False), "far": (None, True)},
                host_result=False, with_pattern=False)
    refused("split", {**pat, "order": (bad_order, False), "region": (region, False), "level": (level, False),
                      "cls": (None, True)}, host_result=False)
    refused("far_roots", {"region": (bad_region, False), "level": (level, False), "far": (None, True)},
            host_result=False, with_pattern=False)
    # regroup works in place: order and region must come back as they went in
    for key, o, r in ((bad_key, order, region), (np.zeros(n, np.int64), bad_order, region),
                      (np.zeros(n, np.int64), order, bad_region)):
        refused("regroup", {"key": (key, False), "order": (o, True), "region": (r, True)}, with_pattern=False,
                scalars=(4, 2))
    assert raw("regroup", itype, gexec.stream, n, 0, 2, dev(gexec, np.zeros(n), itype), dev(gexec, order, itype),
               dev(gexec, region, itype), C.byref(count)) == GKOC_E_INVALID        # leaf_size < 1


@pytest.mark.parametrize("itype", ITYPES, ids=ITYPE_IDS)
def test_empty_graph(gexec, itype):
    count = C.c_longlong(-5)
    assert raw("components", itype, gexec.stream, 0, 0, None, None, None, None, C.byref(count)) == GKOC_OK
    assert raw("levels", itype, gexec.stream, 0, 0, None, None, None, None, None, C.byref(count)) == GKOC_OK
    assert raw("far_roots", itype, gexec.stream, 0, None, None, None) == GKOC_OK
    assert raw("split", itype, gexec.stream, 0, 0, None, None, None, None, None, None) == GKOC_OK
    assert raw("regroup", itype, gexec.stream, 0, 8, 2, None, None, None, C.byref(count)) == GKOC_OK
    assert count.value == 0
    p = g.NestedDissection.build().on(gexec).generate(device_matrix(gexec, sp.csr_matrix((0, 0)), itype))
    assert p.get_permutation().numel() == 0


def test_the_chain_needs_exactly_the_bound(gexec):
    """the loops stop with an error after n sweeps or steps that all changed something; no valid state gets
    there, and the chain, which needs exactly n of either (tests/test_reorder_refs_cpu.py::test_stage_counts),
    is accepted"""
    n = 9
    rp, ci = rr.csr_arrays(rr.chain(n), np.int64)
    d = Device(gexec, rp, ci, np.int32)
    assert d.components(np.zeros(n, np.int64))[1] == n
    assert d.levels(np.zeros(n, np.int64), np.zeros(n, np.int64))[1] == n
