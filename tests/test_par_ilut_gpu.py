"""ParIlut / ParIct on the device (factorization.ParIlut / ParIct, the gkoc_par_ilut_* / gkoc_par_ict_* entries and
gkoc_par_ilu_sweeps_from_* / gkoc_par_ic_sweeps_from_*) against the numpy restatement of tests/par_ilut_refs.py.
Everything is compared bit for bit (np.array_equal, thresholds by their bit pattern): the loop is specified that
way in include/gko_cdna4.h."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import ginkgo_amd as g
import factorization_refs as fr
import isai_refs as ir
import par_factorization_refs as pr
import par_ilut_refs as tr
from ginkgo_amd._lib import call
from test_factorization_gpu import (KINDS, TYPES, TYPE_IDS, csr_arrays, device_csr, factors_of, same, shuffled,
                                    solve_with, transposed)
from test_par_factorization_gpu import csr_of, entries_of, host_pcg

pytestmark = pytest.mark.gpu

VT = {np.float64: "f64", np.float32: "f32"}
IT = {np.int32: "i32", np.int64: "i64"}


def suffix(dtype, itype):
    return "%s_%s" % (VT[dtype], IT[itype])


def to_dev(gexec, *arrays):
    return [gexec.to_device(np.ascontiguousarray(x)) for x in arrays]


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def select_bytes():
    f = g._lib.lib().gkoc_par_ilut_select_workspace_bytes
    f.restype = C.c_size_t
    return int(f())


# ------------------------------------------------------------------ sweeps_from
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_sweeps_from_a_given_iterate(gexec, kind, dtype, itype):
    """4^3 27-point stencil, v0 != a: one sweep and two (the second reads the first from the work buffer); and
    from(a, a) is the existing entry"""
    a = fr.stencil27(4)
    rp, ci, v = fr.arrays(sp.tril(a, format="csr") if kind == "ic" else a, itype, dtype)
    n, nnz = len(rp) - 1, len(ci)
    rng = np.random.default_rng(5)
    v0 = (v * rng.uniform(0.5, 1.5, nnz)).astype(dtype)
    first = tr.sweep_from(kind, rp, ci, v, v0)
    second = tr.sweep_from(kind, rp, ci, v, first)
    assert not np.array_equal(first, tr.sweep_from(kind, rp, ci, v, v)) and not np.array_equal(first, second)
    d_rp, d_ci, d_v, d_v0 = to_dev(gexec, rp, ci, v, v0)
    out, work = to_dev(gexec, np.zeros(nnz, dtype), np.zeros(nnz, dtype))
    changed = gexec.to_device(np.array([77], np.int64))
    name = "gkoc_par_%s_sweeps_from_%s" % (kind, suffix(dtype, itype))
    plain = "gkoc_par_%s_sweeps_%s" % (kind, suffix(dtype, itype))
    call(name, gexec.stream, n, nnz, d_rp, d_ci, d_v, d_v0, 1, None, out, changed)
    assert np.array_equal(out.cpu().numpy(), first)
    assert int(changed.item()) == np.count_nonzero(bits(first) != bits(v0))
    call(name, gexec.stream, n, nnz, d_rp, d_ci, d_v, d_v0, 2, work, out, changed)
    assert np.array_equal(out.cpu().numpy(), second) and np.array_equal(work.cpu().numpy(), first)
    assert int(changed.item()) == np.count_nonzero(bits(second) != bits(first))
    assert np.array_equal(d_v.cpu().numpy(), v) and np.array_equal(d_v0.cpu().numpy(), v0)
    for sweeps in (1, 3):
        call(name, gexec.stream, n, nnz, d_rp, d_ci, d_v, d_v, sweeps, work, out, None)
        got = out.cpu().numpy().copy()
        call(plain, gexec.stream, n, nnz, d_rp, d_ci, d_v, sweeps, work, out, None)
        assert np.array_equal(got, out.cpu().numpy())
        assert np.array_equal(got, (pr.ilu_sweeps if kind == "ilu" else pr.ic_sweeps)(rp, ci, v, sweeps)[0])


# ------------------------------------------------------------------ gather
def masked(dense, mask, dtype, itype):
    return fr.on_pattern(dense, mask, itype, dtype)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_gather(gexec, dtype, itype):
    """source pattern equal to the target, a subset of it, disjoint from it, with empty rows on either side, a
    long row (several rounds of the group), and n = 1"""
    rng = np.random.default_rng(7)
    n = 70
    dense = rng.uniform(1, 2, (n, n))
    target = rng.random((n, n)) < 0.2
    target[3] = False
    target[20] = True                       # 70 positions: 5 rounds of 16 lanes
    sub = target & (rng.random((n, n)) < 0.5)
    sub[5] = False
    other = ~target & (rng.random((n, n)) < 0.2)
    mixed = rng.random((n, n)) < 0.3
    cases = [(n, target, m) for m in (target, sub, other, mixed, np.zeros((n, n), bool))]
    cases += [(1, np.ones((1, 1), bool), np.ones((1, 1), bool)), (1, np.ones((1, 1), bool), np.zeros((1, 1), bool))]
    for size, p_mask, s_mask in cases:
        p_rp, p_ci, _ = masked(dense[:size, :size], p_mask, dtype, itype)
        s_rp, s_ci, s_v = masked(dense[:size, :size], s_mask, dtype, itype)
        want = tr.gather(p_rp, p_ci, s_rp, s_ci, s_v)
        assert np.array_equal(want, np.where(s_mask, dense[:size, :size], 0)[p_mask].astype(dtype))
        out = gexec.to_device(np.full(len(p_ci) + 1, 9, dtype))
        d = to_dev(gexec, p_rp, p_ci, s_rp, s_ci, s_v)
        call("gkoc_par_ilut_gather_" + suffix(dtype, itype), gexec.stream, size, len(p_ci), d[0], d[1], len(s_ci),
             d[2], d[3] if len(s_ci) else None, d[4] if len(s_ci) else None, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:-1], want) and got[-1] == 9
        assert not np.signbit(got[:-1][want == 0]).any()


# ------------------------------------------------------------------ candidate values
def candidate_entry(kind, dtype, itype):
    return "gkoc_par_%s_candidate_values_%s" % ("ilut" if kind == "ilu" else "ict", suffix(dtype, itype))


def check_candidates(gexec, kind, p, a, m, dtype, itype):
    """p = (rp, ci), a and m = (rp, ci, v)"""
    want = (tr.ilut_candidates if kind == "ilu" else tr.ict_candidates)(*p, *a, *m)
    out = gexec.to_device(np.full(len(p[1]) + 1, 9, dtype))
    d_p, d_a, d_m = to_dev(gexec, *p), to_dev(gexec, *a), to_dev(gexec, *m)
    call(candidate_entry(kind, dtype, itype), gexec.stream, len(p[0]) - 1, len(p[1]), *d_p, len(a[1]), *d_a,
         len(m[1]), *d_m, out)
    got = out.cpu().numpy()
    assert np.array_equal(got[:-1], want, equal_nan=True) and got[-1] == 9
    for dev, host in zip(d_a + d_m, a + m):
        assert np.array_equal(dev.cpu().numpy(), host), "an input was written"
    return want


def small_candidate_case(kind, dtype, itype):
    """12 x 12.  A' is dense (ic: its lower triangle), M has lost about half of its off-diagonal entries, among
    them (5, 0) and (0, 11) (ilu) resp. (11, 0) (ic); row 3 of M has lost upper entries only and row 4 lower ones
    only (ilu).  P = the pattern of L U (L L^T) + A'."""
    n = 12
    rng = np.random.default_rng(11)
    dense = rng.uniform(0.5, 1.5, (n, n)) * rng.choice([-1.0, 1.0], (n, n)) + 6 * np.eye(n)
    a_mask = np.ones((n, n), bool)
    m_mask = (rng.random((n, n)) < 0.5) | np.eye(n, dtype=bool)
    m_mask[5, 0] = m_mask[0, 11] = m_mask[11, 0] = False
    m_mask[3, :3], m_mask[3, 4:] = True, rng.random(n - 4) < 0.4
    m_mask[4, :4], m_mask[4, 5:] = rng.random(4) < 0.4, True
    m_mask[3, 11] = m_mask[4, 0] = False
    if kind == "ic":
        a_mask, m_mask = np.tril(a_mask), np.tril(m_mask)
    a = masked(dense, a_mask, dtype, itype)
    m = masked(dense * rng.uniform(0.8, 1.2, (n, n)), m_mask, dtype, itype)
    p = (tr.ilut_pattern if kind == "ilu" else tr.ict_pattern)(m[0], m[1], a[0], a[1])
    return p, a, m, m_mask


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_candidate_values(gexec, kind, dtype, itype):
    p, a, m, m_mask = small_candidate_case(kind, dtype, itype)
    n = len(p[0]) - 1
    assert len(p[1]) == (n * n if kind == "ilu" else n * (n + 1) // 2), "A' is dense: so is P"
    got = fr.dense_of(p[0], p[1], check_candidates(gexec, kind, p, a, m, dtype, itype))
    a_d, m_d = fr.dense_of(*a), fr.dense_of(*m)
    assert np.array_equal(got[m_mask], m_d[m_mask]), "a stored entry is not the factor's value"
    # the candidate in column 0 has no k < 0 and A' stores it: a' / m_00; the one in column n - 1 of row 0 likewise
    # has no matching k, and is not divided
    row = 5 if kind == "ilu" else 11
    assert not m_mask[row, 0] and got[row, 0] == dtype(a_d[row, 0] / m_d[0, 0])
    if kind == "ilu":
        assert not m_mask[0, n - 1] and got[0, n - 1] == a_d[0, n - 1]
        assert m_mask[3, :3].all() and not m_mask[3, 4:].all() and m_mask[4, 5:].all() and not m_mask[4, :4].all()
    # P = pattern(M): no candidate, the values of M
    want = check_candidates(gexec, kind, m[:2], a, m, dtype, itype)
    assert np.array_equal(want, m[2])
    # A' stores nothing off the diagonal: every candidate starts from +0
    eye = masked(np.eye(n), np.eye(n, dtype=bool), dtype, itype)
    check_candidates(gexec, kind, p, eye, m, dtype, itype)
    # a candidate whose row of M is only the diagonal: nothing to subtract
    lone = masked(fr.dense_of(*m), np.eye(n, dtype=bool) | (np.arange(n)[:, None] == 0), dtype, itype) \
        if kind == "ilu" else masked(fr.dense_of(*m), np.eye(n, dtype=bool), dtype, itype)
    check_candidates(gexec, kind, p, a, lone, dtype, itype)


def hub_candidate_case(kind, length, dtype, itype):
    """a band of half-width 3 and one hub row of P with exactly `length` positions, about 60 % of which M stores:
    the candidates of the hub row find their k in the band"""
    rng = np.random.default_rng(length)
    n_lower = (length - 1) // 2 if kind == "ilu" else length - 1
    n_upper = length - 1 - n_lower
    n, hub = n_lower + n_upper + 30, n_lower + 10
    i, j = np.indices((n, n))
    eye = i == j
    p_mask = np.abs(i - j) <= 3
    p_mask[hub, hub - n_lower:hub + n_upper + 1] = True
    if kind == "ic":
        p_mask &= j <= i
    m_mask = (p_mask & (rng.random((n, n)) < 0.6)) | eye
    a_mask = (p_mask & (rng.random((n, n)) < 0.6)) | eye
    dense = rng.uniform(0.5, 1.5, (n, n)) * rng.choice([-1.0, 1.0], (n, n)) + 6 * np.eye(n)
    p = masked(dense, p_mask, dtype, itype)[:2]
    lengths = np.diff(p[0])
    assert lengths.max() == lengths[hub] == length and np.sort(lengths)[-2] <= 7
    return p, masked(dense, a_mask, dtype, itype), masked(dense * rng.uniform(0.8, 1.2, (n, n)), m_mask, dtype, itype)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_candidate_values_at_every_path_boundary(gexec, kind, dtype, itype):
    """the lanes per row come from the LONGEST row of P: on, one below and one above every limit, and rows that
    are streamed in three and in five rounds"""
    limits = g.factorization.row_limits()
    lengths = sorted({x for limit in limits for x in (limit - 1, limit, limit + 1)}
                     | {2 * limits[-1] + 22, 5 * limits[-1] - 20})
    assert max(lengths) > 4 * 64
    for length in lengths:
        p, a, m = hub_candidate_case(kind, length, dtype, itype)
        want = check_candidates(gexec, kind, p, a, m, dtype, itype)
        assert not np.array_equal(want, tr.gather(*p, *m)), "no candidate changed anything"


# ------------------------------------------------------------------ threshold select
def parts_matrix(lower, upper, width, dtype, itype):
    """a matrix whose strictly-lower entries are `lower` and whose strictly-upper ones are `upper`, at most
    `width` of either per row, with a diagonal of 1e30 that belongs to no part"""
    lower, upper = np.asarray(lower, dtype), np.asarray(upper, dtype)
    t_l, t_u = np.arange(len(lower)), np.arange(len(upper))
    rows_l = width + t_l // width
    rows_u = t_u // width
    n = int(max(rows_l.max(initial=0) + 1, rows_u.max(initial=0) + width + 1, 1))
    rows = np.concatenate([rows_l, rows_u, np.arange(n)])
    cols = np.concatenate([rows_l - 1 - t_l % width, rows_u + 1 + t_u % width, np.arange(n)])
    vals = np.concatenate([lower, upper, np.full(n, 1e30, dtype)])
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, itype)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rp, cols[order].astype(itype), vals[order]


def device_threshold(gexec, m, part, keep, dtype, itype, work, thr):
    thr.fill_(-7)
    call("gkoc_par_ilut_threshold_select_" + suffix(dtype, itype), gexec.stream, len(m[0]) - 1, m[3], m[4], m[5],
         C.c_int(part), keep, work, C.c_size_t(work.numel()), thr)
    return thr.cpu().numpy()[0]


def check_thresholds(gexec, lower, upper, keeps, dtype, itype, width=3):
    rp, ci, v = parts_matrix(lower, upper, width, dtype, itype)
    rows = tr.rows_of(rp)
    assert np.array_equal(np.sort(tr.u_of(v[ci < rows])), np.sort(tr.u_of(np.asarray(lower, dtype))))
    m = (rp, ci, v) + tuple(to_dev(gexec, rp, ci, v))
    work = gexec.alloc((select_bytes(),), torch.uint8)
    thr = gexec.to_device(np.zeros(1, dtype))
    out = []
    for part, values in ((0, lower), (1, upper)):
        for keep in keeps(len(values)):
            want = tr.part_threshold(rp, ci, v, part, keep)
            got = device_threshold(gexec, m, part, keep, dtype, itype, work, thr)
            assert bits(np.array([got]))[0] == bits(np.array([want]))[0], (part, keep, got, want)
            assert not np.signbit(got)
            out.append(got)
    assert np.array_equal(m[5].cpu().numpy(), v, equal_nan=True)
    return out


def usual_keeps(count):
    return sorted({k for k in (1, 2, count // 2, count - 1, count, count + 1, count + 5) if k >= 1})


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_threshold_select_by_count(gexec, dtype, itype):
    """0, 1 and 2 entries, the sizes around one 256-bin table, and more rows than one pass of the grid takes
    (2048 workgroups of 16 rows); keep from 1 to beyond the count"""
    rng = np.random.default_rng(13)
    for count in (0, 1, 2, 255, 256, 257):
        lower, upper = rng.standard_normal(count), rng.standard_normal((count * 2) // 3) * 1e-3
        check_thresholds(gexec, lower, upper, usual_keeps, dtype, itype)
    count = 2048 * 16 + 1500
    lower, upper = rng.standard_normal(count) * 1e5, rng.standard_normal(count)
    rp, _, _ = parts_matrix(lower, upper, 1, dtype, itype)
    assert len(rp) - 1 > 2048 * 16
    got = check_thresholds(gexec, lower, upper, lambda c: (1, 1000, c - 1, c), dtype, itype, width=1)
    assert got[0] > 1e5 and got[3] == 0 and 0 < got[4] < 10, "the two parts have thresholds of their own"


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_threshold_select_by_value(gexec, dtype, itype):
    every = lambda count: range(1, count + 2)       # noqa: E731
    nan, inf = np.nan, np.inf
    tiny = np.finfo(dtype).tiny
    cases = [[2.5] * 7,                                             # all equal
             [1.0, 2.0, -2.0, 2.0, 3.0, 2.0, -1.0],                 # duplicates straddling the rank
             [-5.0, 1.0, 3.0, -4.0, -0.5, 0.25],                    # negative values
             [-0.0, 0.0, 1.0, -0.0, -1.0],                          # the two zeros are one value
             [1.0, inf, nan, -inf, 2.0, -nan, 0.0, -3.0],           # NaN above inf
             [tiny, -tiny / 2, tiny / 4, 0.0, np.finfo(dtype).max],  # subnormals and the largest number
             [1.0 + k * np.finfo(dtype).eps for k in range(40)]]    # differ in the last digit only: every pass
    for values in cases:
        check_thresholds(gexec, values, values[::-1][:3], every, dtype, itype)


def test_threshold_select_refuses_bad_arguments(gexec):
    rp, ci, v = parts_matrix([1.0, 2.0, 3.0], [4.0], 2, np.float64, np.int32)
    d = to_dev(gexec, rp, ci, v)
    work = gexec.alloc((select_bytes(),), torch.uint8)
    thr = gexec.to_device(np.array([-7.0]))
    n, name = len(rp) - 1, "gkoc_par_ilut_threshold_select_f64_i32"
    size = C.c_size_t(work.numel())
    bad = [(n, d[0], d[1], d[2], 0, 0, work, size, thr), (n, d[0], d[1], d[2], 1, -3, work, size, thr),
           (n, d[0], d[1], d[2], 2, 1, work, size, thr), (n, d[0], d[1], d[2], -1, 1, work, size, thr),
           (-1, d[0], d[1], d[2], 0, 1, work, size, thr), (n, None, d[1], d[2], 0, 1, work, size, thr),
           (n, d[0], None, d[2], 0, 1, work, size, thr), (n, d[0], d[1], None, 0, 1, work, size, thr),
           (n, d[0], d[1], d[2], 0, 1, None, size, thr), (n, d[0], d[1], d[2], 0, 1, work, size, None),
           (n, d[0], d[1], d[2], 0, 1, work, C.c_size_t(work.numel() - 1), thr)]
    for n_, rp_, ci_, v_, part, keep, work_, size_, thr_ in bad:
        with pytest.raises(g.GkoError):
            call(name, gexec.stream, n_, rp_, ci_, v_, C.c_int(part), keep, work_, size_, thr_)
        assert thr.cpu().numpy()[0] == -7.0, "the threshold was written before the refusal"
    call(name, gexec.stream, n, *d, C.c_int(0), 1, work, size, thr)
    assert thr.cpu().numpy()[0] == 3.0
    call(name, gexec.stream, 0, None, None, None, C.c_int(0), 1, None, C.c_size_t(0), thr)
    assert thr.cpu().numpy()[0] == 0.0


# ------------------------------------------------------------------ keep mask
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_keep_mask(gexec, dtype, itype):
    """ties at the threshold are kept, the diagonal is kept even when it is 0, thresholds of +0 keep everything
    (-0 among it), NaN thresholds keep NaNs only; without an upper threshold nothing right of the diagonal"""
    nan, inf = np.nan, np.inf
    lower = [1.0, 2.0, -2.0, 2.0, 3.0, -0.0, 0.0, nan, -inf, 0.5] * 4
    upper = [-4.0, 4.0, 0.25, -0.0, inf, -nan, 1.0] * 5
    rp, ci, v = parts_matrix(lower, upper, 5, dtype, itype)
    rows = tr.rows_of(rp)
    v[rows == ci] = np.resize(np.array([0.0, -0.0, 1e-30, 5.0], dtype), len(rp) - 1)
    d = to_dev(gexec, rp, ci, v)
    nnz = len(ci)
    for thr_l, thr_u in ((2.0, 4.0), (0.0, 0.0), (2.0, None), (nan, inf), (inf, nan), (3.0, 0.25), (0.0, None)):
        want = tr.keep_mask(rp, ci, v, dtype(thr_l), None if thr_u is None else dtype(thr_u))
        thr = gexec.to_device(np.array([thr_l, 0.0 if thr_u is None else thr_u], dtype))
        mask = gexec.to_device(np.full(nnz + 1, 9, dtype))
        call("gkoc_par_ilut_keep_mask_" + suffix(dtype, itype), gexec.stream, len(rp) - 1, nnz, *d, thr[0:1],
             None if thr_u is None else thr[1:2], mask)
        got = mask.cpu().numpy()
        assert np.array_equal(got[:-1], want) and got[-1] == 9, (thr_l, thr_u)
        assert want[rows == ci].all() and not np.signbit(got[:-1]).any()
        if thr_u is None:
            assert not want[ci > rows].any()
    want = tr.keep_mask(rp, ci, v, dtype(2.0), dtype(4.0))
    assert want[(ci < rows) & (np.abs(v) == 2.0)].all() and want[(ci < rows) & (np.abs(v) == 2.0)].size == 12
    assert not want[(ci < rows) & (np.abs(v) < 2.0)].any()


# ------------------------------------------------------------------ the classes
def generate(gexec, kind, a, iterations=None, limit=None, **params):
    f = (g.factorization.ParIlut if kind == "ilu" else g.factorization.ParIct).build()
    if iterations is not None:
        f = f.with_iterations(iterations)
    if limit is not None:
        f = f.with_fill_in_limit(limit)
    for k, val in params.items():
        f = getattr(f, "with_" + k)(val)
    return f.on(gexec).generate(a)


NAMES = ["stencil4", "stencil5", "nonsymmetric2d", "random", "arrow"]
COUNTS = (1, 2, 5)
LIMITS = (1.0, 2.0, 100.0)


@functools.lru_cache(maxsize=None)
def case_matrix(name, spd):
    rng = np.random.default_rng(len(name) * 17 + 1)
    if name == "stencil4":
        return fr.stencil27(4)
    if name == "stencil5":
        return fr.stencil27(5)
    if name == "stencil6":
        return fr.stencil27(6)
    if name == "laplace6":
        t, eye = sp.diags([-np.ones(5), 2 * np.ones(6), -np.ones(5)], [-1, 0, 1]), sp.identity(6)
        return (sp.kron(sp.kron(t, eye), eye) + sp.kron(sp.kron(eye, t), eye) + sp.kron(sp.kron(eye, eye), t)).tocsr()
    if name == "nonsymmetric2d":
        # 5-point convection-diffusion on 9 x 7 points: a symmetric PATTERN with other values left and right
        tx = sp.diags([np.full(8, -1.5), np.full(9, 4.0), np.full(8, -0.5)], [-1, 0, 1])
        ty = sp.diags([np.full(6, -1.25), np.full(6, -0.75)], [-1, 1])
        a = (sp.kron(sp.identity(7), tx) + sp.kron(ty, sp.identity(9))).tocsr()
        return ((a + a.T) * 0.5).tocsr() if spd else a
    if name == "random":
        return fr.from_lower_pattern(fr.random_pattern(150, rng, 3), rng, spd)     # tie-free values
    if name == "arrow":
        return sp.csr_matrix(tr.arrow(8, spd))
    raise KeyError(name)


_REFS = {}      # {(case, kind, value type, limit): {iterations: the factors}}, computed once, read-only


def reference(name, kind, a, dtype, limit, counts=COUNTS):
    key = (name, kind, dtype, limit)
    have = _REFS.setdefault(key, {})
    if not set(counts) <= set(have):
        rp, ci, v = fr.arrays(a, np.int32, dtype)
        todo = tuple(sorted(set(counts) | set(have)))
        if kind == "ilu":
            new = {k: fr.split_l_u(*m) for k, m in tr.par_ilut_at(rp, ci, v, todo, limit).items()}
        else:
            new = tr.par_ict_at(rp, ci, v, todo, limit)
        for k, arrays in new.items():
            for arr in arrays:
                arr.setflags(write=False)
            have[k] = arrays
    return have


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_factors_match_the_restatement(gexec, kind, name, dtype, itype):
    a = case_matrix(name, kind == "ic")
    rp, ci, v = fr.arrays(a, itype, dtype)
    dev = device_csr(gexec, rp, ci, v)
    sizes = {}
    for limit in LIMITS:
        refs = reference(name, kind, a, dtype, limit)
        for iterations in COUNTS:
            fact = generate(gexec, kind, dev, iterations, limit)
            assert fact.iterations == iterations and fact.fill_in_limit == limit and fact.get_size() == dev.size
            assert fact.keep == tr.keep_counts(rp, ci, limit)
            want = refs[iterations]
            # (pivots are not checked: ParIct with limit 1.0 breaks down on the 5^3 stencil, NaN for NaN)
            same(factors_of(kind, fact), want, itype, equal_nan=True)
            sizes[limit, iterations] = len(want[1])
    for got, kept in zip(csr_arrays(dev), (rp, ci, v)):
        assert np.array_equal(got, kept), "generate changed the caller's matrix"
    if name == "arrow":
        # the closure anchor on the device: nothing is dropped, the exact factors on the full pattern
        n = a.shape[0]
        full = fr.on_pattern(a.toarray(), np.ones((n, n), bool) if kind == "ilu" else np.tril(np.ones((n, n), bool)),
                             np.int32, dtype)
        exact = fr.split_l_u(full[0], full[1], fr.ilu0(*full)) if kind == "ilu" else \
            (full[0], full[1], fr.ic0(*full))
        same(reference(name, kind, a, dtype, 100.0)[5], exact, np.int32)
    else:
        assert sizes[100.0, 2] >= sizes[2.0, 2] > sizes[1.0, 2], "the limit does not bind: the case shows nothing"


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_parameters_and_refusals(gexec, kind):
    a = case_matrix("random", kind == "ic")
    dev = device_csr(gexec, *fr.arrays(a))
    cls = g.factorization.ParIlut if kind == "ilu" else g.factorization.ParIct
    want = reference("random", kind, a, np.float64, 2.0)[5]
    fact = cls.build().on(gexec).generate(dev)
    assert fact.iterations == 5 and fact.fill_in_limit == 2.0
    same(factors_of(kind, fact), want, np.int32)
    # the selection is always exact: the sampling parameters are accepted without effect
    fact = generate(gexec, kind, dev, approximate_select=True, deterministic_sample=True)
    same(factors_of(kind, fact), want, np.int32)
    same(factors_of(kind, generate(gexec, kind, dev, approximate_select=False)), want, np.int32)
    for limit in (0.99, 0.0, -1.0, float("nan")):
        with pytest.raises(g.GkoError):
            cls.build().with_fill_in_limit(limit)
    for iterations in (0, -1):
        with pytest.raises(g.GkoError):
            cls.build().with_iterations(iterations)
    if kind == "ic":
        both = generate(gexec, kind, dev, 2, 2.0, both_factors=True)
        same(csr_arrays(both.get_lt_factor()), transposed(*csr_arrays(both.get_l_factor())), np.int32)
        assert generate(gexec, kind, dev, 2, 2.0, both_factors=False).get_lt_factor() is None
    with pytest.raises(g.NotSupported):
        cls.build().on(gexec).generate(g.Dense.create(gexec, (4, 4)))
    with pytest.raises(g.NotSupported):
        cls.build().on(gexec).generate(dev.convert_to_ell())
    wide = g.Csr.from_arrays(gexec, (2, 3), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.ones(2))
    with pytest.raises(g.DimensionMismatch):
        cls.build().on(gexec).generate(wide)
    cplx = g.Csr.from_arrays(gexec, (2, 2), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32),
                             np.ones(2, np.complex128))
    with pytest.raises(g.NotSupported):
        cls.build().on(gexec).generate(cplx)
    other = (g.Ic if kind == "ilu" else g.Ilu).build().with_factorization(cls.build())
    with pytest.raises(g.NotSupported):
        other.on(gexec).generate(dev)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_missing_diagonals_become_explicit_zeros(gexec, dtype, itype):
    """rows 5, 57 and 99 lose their diagonal entry, as in the ParIlu test: the loop runs on the matrix with
    explicit zeros there, and inf / NaN sit where the restatement has them"""
    a = case_matrix("random", True)
    rp, ci, v = fr.arrays(a, itype, dtype)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    gone = np.isin(rows, (5, 57, 99)) & (rows == ci)
    assert gone.sum() == 3
    zeroed = v.copy()
    zeroed[gone] = 0
    rp_m = np.zeros_like(rp)
    rp_m[1:] = np.cumsum(np.bincount(rows[~gone], minlength=n))
    dev = device_csr(gexec, rp_m, ci[~gone], v[~gone])
    ref = tr.par_ilut_factors(rp, ci, zeroed, 2, 2.0)
    assert not all(np.isfinite(x).all() for x in ref)
    same(factors_of("ilu", generate(gexec, "ilu", dev, 2, 2.0)), ref, itype, equal_nan=True)
    ref = tr.par_ict_factor(rp, ci, zeroed, 2, 2.0)
    assert np.isnan(ref[2]).any()
    same(factors_of("ic", generate(gexec, "ic", dev, 2, 2.0)), ref, itype, equal_nan=True)
    assert np.array_equal(dev.values.cpu().numpy(), v[~gone]), "generate changed the caller's matrix"


@pytest.mark.parametrize("kind", KINDS)
def test_unsorted_input_is_sorted_unless_told_not_to(gexec, kind):
    a = case_matrix("random", kind == "ic")
    rp, ci, v = fr.arrays(a)
    ref = reference("random", kind, a, np.float64, 2.0)[2]
    ci_u, v_u = shuffled(rp, ci, v, np.random.default_rng(8))
    assert not np.array_equal(ci_u, ci)
    dev = device_csr(gexec, rp, ci_u, v_u)
    same(factors_of(kind, generate(gexec, kind, dev, 2, 2.0)), ref, np.int32)
    assert np.array_equal(dev.col_idxs.cpu().numpy(), ci_u) and np.array_equal(dev.values.cpu().numpy(), v_u), \
        "generate changed the caller's matrix"
    same(factors_of(kind, generate(gexec, kind, device_csr(gexec, rp, ci, v), 2, 2.0, skip_sorting=True)), ref,
         np.int32)


def test_an_fbcsr_system_matrix(gexec):
    rng = np.random.default_rng(12)
    blocks = sp.random(30, 30, 0.1, random_state=rng, format="csr")
    blocks = blocks + blocks.T + sp.eye(30)
    a = sp.kron(blocks, np.ones((3, 3)), format="csr")
    a.data = rng.uniform(-1, 1, a.nnz)
    a = (a + a.T + sp.diags(np.full(90, 40.0))).tocsr()
    fb = g.Fbcsr.from_scipy(gexec, sp.bsr_matrix(a, blocksize=(3, 3)))
    for kind in KINDS:
        want = (tr.par_ilut_factors if kind == "ilu" else tr.par_ict_factor)(*fr.arrays(a), 2, 1.5)
        same(factors_of(kind, generate(gexec, kind, fb, 2, 1.5)), want, np.int32)
        factory = (g.factorization.ParIlut if kind == "ilu" else g.factorization.ParIct).build() \
            .with_iterations(2).with_fill_in_limit(1.5)
        m = (g.Ilu if kind == "ilu" else g.Ic).build().with_factorization(factory).on(gexec).generate(fb)
        same(factors_of(kind, m.factorization), want, np.int32)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_pivot_gives_the_restatement_s_non_finite_entries(gexec, kind, dtype, itype):
    a = case_matrix("random", kind == "ic")
    rp, ci, v = fr.arrays(a, itype, dtype)
    rows = tr.rows_of(rp)
    v[(rows == ci) & np.isin(rows, (0, 3))] = 0
    want = (tr.par_ilut_factors if kind == "ilu" else tr.par_ict_factor)(rp, ci, v, 2, 2.0)
    assert not all(np.isfinite(x).all() for x in want) and np.isfinite(want[2]).any()
    same(factors_of(kind, generate(gexec, kind, device_csr(gexec, rp, ci, v), 2, 2.0)), want, itype, equal_nan=True)
    # the calls succeeded; the next one on this executor is right
    good = case_matrix("arrow", kind == "ic")
    same(factors_of(kind, generate(gexec, kind, device_csr(gexec, *fr.arrays(good, itype, dtype)), 2, 100.0)),
         reference("arrow", kind, good, dtype, 100.0)[2], itype)


# ------------------------------------------------------------------ invalid arguments
def test_invalid_arguments_are_refused_before_a_value_is_touched(gexec):
    p, a, m, _ = small_candidate_case("ilu", np.float64, np.int32)
    p_ic, a_ic, m_ic, _ = small_candidate_case("ic", np.float64, np.int32)
    n = len(p[0]) - 1
    st = gexec.stream

    def without(rp, ci, row, col, *v):
        rows = tr.rows_of(rp)
        keep = ~((rows == row) & (ci == col))
        out = np.zeros_like(rp)
        out[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
        return (out, ci[keep]) + tuple(x[keep] for x in v)

    def broken(rp, ci, how):
        rp, ci = rp.copy(), ci.copy()
        if how == "descend":
            rp[4], rp[5] = rp[5], rp[4]
        elif how == "first":
            rp[0] = 1
        elif how == "out":
            ci[rp[6]] = n
        elif how == "negative":
            ci[rp[6]] = -1
        return rp, ci

    out = gexec.to_device(np.full(len(p[1]) + 1, 9.0))
    d_p, d_a, d_m = to_dev(gexec, *p), to_dev(gexec, *a), to_dev(gexec, *m)
    d_pic, d_aic, d_mic = to_dev(gexec, *p_ic), to_dev(gexec, *a_ic), to_dev(gexec, *m_ic)
    ilut, ict = "gkoc_par_ilut_candidate_values_f64_i32", "gkoc_par_ict_candidate_values_f64_i32"

    def cand(name, p_, a_, m_, out_=out, n_=n, p_nnz=None, a_nnz=None, m_nnz=None):
        return (name, (n_, len(p[1]) if p_nnz is None else p_nnz, *p_, len(a[1]) if a_nnz is None else a_nnz, *a_,
                       len(m[1]) if m_nnz is None else m_nnz, *m_, out_))

    bad = [("a negative size", cand(ilut, d_p, d_a, d_m, n_=-1)),
           ("no pattern row pointers", cand(ilut, [None, d_p[1]], d_a, d_m)),
           ("no pattern columns", cand(ilut, [d_p[0], None], d_a, d_m)),
           ("no values of a", cand(ilut, d_p, d_a[:2] + [None], d_m)),
           ("no factor values", cand(ilut, d_p, d_a, d_m[:2] + [None])),
           ("no factor columns", cand(ilut, d_p, d_a, [d_m[0], None, d_m[2]])),
           ("no output", cand(ilut, d_p, d_a, d_m, out_=None)),
           ("pattern row pointers that do not end at nnz", cand(ilut, d_p, d_a, d_m, p_nnz=len(p[1]) - 1)),
           ("factor row pointers that do not end at nnz", cand(ilut, d_p, d_a, d_m, m_nnz=len(m[1]) + 1)),
           ("row pointers of a that do not end at nnz", cand(ilut, d_p, d_a, d_m, a_nnz=len(a[1]) - 1))]
    for how in ("descend", "first", "out", "negative"):
        bad.append(("pattern: " + how, cand(ilut, to_dev(gexec, *broken(*p, how)), d_a, d_m)))
        bad.append(("factor: " + how, cand(ilut, d_p, d_a, to_dev(gexec, *broken(*m[:2], how)) + [d_m[2]])))
        bad.append(("a: " + how, cand(ilut, d_p, to_dev(gexec, *broken(*a[:2], how)) + [d_a[2]], d_m)))
    no_diag_m = without(m[0], m[1], 7, 7, m[2])
    bad.append(("a factor row without its diagonal", cand(ilut, d_p, d_a, to_dev(gexec, *no_diag_m),
                                                          m_nnz=len(no_diag_m[1]))))
    no_diag_p = without(p[0], p[1], 7, 7)
    bad.append(("a pattern row without its diagonal", cand(ilut, to_dev(gexec, *no_diag_p), d_a, d_m,
                                                           p_nnz=len(no_diag_p[1]))))
    stored = int(m[1][m[0][9]])             # the first column of row 9 of the factor, not its diagonal
    assert stored != 9
    smaller = without(p[0], p[1], 9, stored)
    bad.append(("a pattern that lacks an entry of the factor", cand(ilut, to_dev(gexec, *smaller), d_a, d_m,
                                                                    p_nnz=len(smaller[1]))))
    bad.append(("ict: a full pattern and factor", cand(ict, d_p, d_a, d_m)))
    bad.append(("ict: a full factor", (ict, (n, len(p_ic[1]), *d_pic, len(a_ic[1]), *d_aic, len(m[1]), *d_m, out))))
    bad.append(("ict: a full pattern", (ict, (n, len(p[1]), *d_p, len(a_ic[1]), *d_aic, len(m_ic[1]), *d_mic, out))))
    # gather and keep_mask
    gather, mask = "gkoc_par_ilut_gather_f64_i32", "gkoc_par_ilut_keep_mask_f64_i32"
    thr = gexec.to_device(np.array([1.0, 1.0]))
    bad += [("gather: no source row pointers", (gather, (n, len(p[1]), *d_p, len(m[1]), None, d_m[1], d_m[2], out))),
            ("gather: no source values", (gather, (n, len(p[1]), *d_p, len(m[1]), d_m[0], d_m[1], None, out))),
            ("gather: no output", (gather, (n, len(p[1]), *d_p, len(m[1]), *d_m, None))),
            ("gather: a negative size", (gather, (n, -1, *d_p, len(m[1]), *d_m, out))),
            ("gather: wrong nnz", (gather, (n, len(p[1]), *d_p, len(m[1]) - 1, *d_m, out))),
            ("gather: a column out of range", (gather, (n, len(p[1]), *to_dev(gexec, *broken(*p, "out")), len(m[1]),
                                                        *d_m, out))),
            ("gather: source pointers that descend", (gather, (n, len(p[1]), *d_p, len(m[1]),
                                                               *to_dev(gexec, *broken(*m[:2], "descend")), d_m[2], out))),
            ("mask: no lower threshold", (mask, (n, len(m[1]), *d_m, None, thr[1:2], out))),
            ("mask: no values", (mask, (n, len(m[1]), d_m[0], d_m[1], None, thr[0:1], thr[1:2], out))),
            ("mask: no mask", (mask, (n, len(m[1]), *d_m, thr[0:1], thr[1:2], None))),
            ("mask: wrong nnz", (mask, (n, len(m[1]) + 1, *d_m, thr[0:1], thr[1:2], out))),
            ("mask: a negative column", (mask, (n, len(m[1]), *to_dev(gexec, *broken(*m[:2], "negative")), d_m[2],
                                                thr[0:1], thr[1:2], out)))]
    # the sweeps from an iterate: what the plain sweeps refuse, and an iterate that is missing or overlaps
    nnz = len(m[1])
    work, v0 = gexec.to_device(np.full(nnz + 1, 9.0)), gexec.to_device(np.ones(nnz + 1))
    sweeps = "gkoc_par_ilu_sweeps_from_f64_i32"
    bad += [("sweeps: no iterate", (sweeps, (n, nnz, *d_m, None, 1, None, out, None))),
            ("sweeps: the iterate is the output", (sweeps, (n, nnz, *d_m, out, 1, None, out, None))),
            ("sweeps: the iterate is the work buffer", (sweeps, (n, nnz, *d_m, work, 2, work, out, None))),
            ("sweeps: the iterate overlaps the output", (sweeps, (n, nnz, *d_m, out[1:], 1, None, out, None))),
            ("sweeps: no sweep", (sweeps, (n, nnz, *d_m, v0, 0, work, out, None))),
            ("sweeps: no work buffer", (sweeps, (n, nnz, *d_m, v0, 2, None, out, None))),
            ("sweeps: a row without its diagonal", (sweeps, (n, len(no_diag_m[1]), *to_dev(gexec, *no_diag_m), v0, 1,
                                                             None, out, None))),
            ("sweeps: a full matrix for ic", ("gkoc_par_ic_sweeps_from_f64_i32", (n, nnz, *d_m, v0, 1, None, out,
                                                                                  None)))]
    kept = [x.cpu().numpy().copy() for x in d_a + d_m]
    for what, (name, args) in bad:
        with pytest.raises(g.GkoError):
            call(name, st, *args)
        assert (out.cpu().numpy() == 9.0).all(), what + ": the output was written before the refusal"
        assert (work.cpu().numpy() == 9.0).all(), what + ": work was written before the refusal"
    for x, y in zip(d_a + d_m, kept):
        assert np.array_equal(x.cpu().numpy(), y)
    # nothing of the above reached the device: valid calls on the same arrays are right
    check_candidates(gexec, "ilu", p, a, m, np.float64, np.int32)
    check_candidates(gexec, "ic", p_ic, a_ic, m_ic, np.float64, np.int32)
    # no rows: nothing to do
    call(ilut, st, 0, 0, None, None, 0, None, None, None, 0, None, None, None, None)
    call(ict, st, 0, 0, None, None, 0, None, None, None, 0, None, None, None, None)
    call(gather, st, 0, 0, None, None, 0, None, None, None, None)
    call(mask, st, 0, 0, None, None, None, None, None, None)
    call(sweeps, st, 0, 0, None, None, None, None, 1, None, None, None)


# ------------------------------------------------------------------ no schedule
def test_no_level_schedule_is_built(gexec):
    dev = device_csr(gexec, *fr.arrays(case_matrix("stencil4", True)))
    ilut = lambda: g.factorization.ParIlut.build().with_iterations(2)      # noqa: E731
    ict = lambda: g.factorization.ParIct.build().with_iterations(2)        # noqa: E731
    runs = {
        "ParIlut": lambda: ilut().on(gexec).generate(dev),
        "ParIct": lambda: ict().on(gexec).generate(dev),
        "Ilu": lambda: g.Ilu.build().with_factorization(ilut()).with_l_solver(g.LowerIsai.build())
        .with_u_solver(g.UpperIsai.build()).on(gexec).generate(dev),
        "Ic": lambda: g.Ic.build().with_factorization(ict()).with_l_solver(g.LowerIsai.build())
        .on(gexec).generate(dev),
    }
    for what, fn in runs.items():
        names = entries_of(fn)
        lower = "Ic" in what
        stem = "gkoc_par_ic_sweeps_from_" if lower else "gkoc_par_ilu_sweeps_from_"
        assert sum(name.startswith(stem) for name in names) == 4, what          # two sweeps per iteration
        assert sum(name.startswith("gkoc_par_ilut_threshold_select_") for name in names) == (2 if lower else 4)
        assert sum("_candidate_values_" in name for name in names) == 2
        assert not [name for name in names if "trs_generate" in name or "_factorize_" in name], what
    # the default triangular solvers do build theirs, from the same factors
    names = entries_of(lambda: g.Ilu.build().with_factorization(ilut()).on(gexec).generate(dev))
    assert any("trs_generate" in name for name in names) and not [x for x in names if "_factorize_" in x]


# ------------------------------------------------------------------ the solvers
GRID = 6
LAMBDA_MIN = 27.0 - (1.0 + 2.0 * np.cos(np.pi / (GRID + 1))) ** 3
REDUCTION = 1e-10
ITERATIONS, LIMIT = 3, 2.0


def host_gmres(a, b, precond):
    """right-preconditioned GMRES without a restart (the Krylov dimension is never reached here), x_0 = 0,
    modified Gram-Schmidt and Givens rotations; stops once the rotated residual norm is <= REDUCTION ||b||.
    Returns (x, Arnoldi steps)."""
    n = len(b)
    beta = np.linalg.norm(b)
    basis, z = [b / beta], []
    h = np.zeros((102, 101))
    cs, sn, rhs = np.zeros(101), np.zeros(101), np.zeros(102)
    rhs[0] = beta
    k = 0
    while abs(rhs[k]) > REDUCTION * beta and k < 100:
        z.append(precond(basis[k]))
        w = a @ z[k]
        for i in range(k + 1):
            h[i, k] = basis[i] @ w
            w = w - h[i, k] * basis[i]
        h[k + 1, k] = np.linalg.norm(w)
        basis.append(w / h[k + 1, k])
        for i in range(k):
            h[i, k], h[i + 1, k] = cs[i] * h[i, k] + sn[i] * h[i + 1, k], -sn[i] * h[i, k] + cs[i] * h[i + 1, k]
        r = np.hypot(h[k, k], h[k + 1, k])
        cs[k], sn[k] = h[k, k] / r, h[k + 1, k] / r
        h[k, k], h[k + 1, k] = r, 0.0
        rhs[k + 1], rhs[k] = -sn[k] * rhs[k], cs[k] * rhs[k]
        k += 1
    y = np.linalg.solve(np.triu(h[:k, :k]), rhs[:k])
    return sum((y[i] * z[i] for i in range(k)), np.zeros(n)), k


# the 7-point Laplacian on 6^3 points: the smallest eigenvalue is 3 (2 - 2 cos(pi / 7))
LAMBDA_MIN_LAPLACE = 6.0 * (1.0 - np.cos(np.pi / (GRID + 1)))


@functools.lru_cache(maxsize=None)
def problem(gexec, name):
    a_host = case_matrix(name, True)
    rp, ci, v = fr.arrays(a_host)
    return device_csr(gexec, rp, ci, v), a_host, np.ones(GRID ** 3)


@functools.lru_cache(maxsize=None)
def host_preconditioners(kind, name="stencil6"):
    """{inner solver: r -> M^-1 r on the host} with the restatement's factors: exact triangular solves for the
    default pair, the reference W of tests/isai_refs.py for the ISAI solvers"""
    arrays = fr.arrays(case_matrix(name, True))
    if kind == "ic":
        l_rp, l_ci, l_v = tr.par_ict_factor(*arrays, ITERATIONS, LIMIT)
        lower = csr_of(l_rp, l_ci, l_v)
        upper = lower.T.tocsr()
        w = csr_of(l_rp, l_ci, ir.tri_inverse(l_rp, l_ci, l_v, l_rp, l_ci, True))
        wt = w.T.tocsr()
        return {"trs": lambda r: spla.spsolve_triangular(upper, spla.spsolve_triangular(lower, r, lower=True),
                                                         lower=False),
                "isai": lambda r: wt @ (w @ r)}
    l_rp, l_ci, l_v, u_rp, u_ci, u_v = tr.par_ilut_factors(*arrays, ITERATIONS, LIMIT)
    lower, upper = csr_of(l_rp, l_ci, l_v), csr_of(u_rp, u_ci, u_v)
    w_l = csr_of(l_rp, l_ci, ir.tri_inverse(l_rp, l_ci, l_v, l_rp, l_ci, True))
    w_u = csr_of(u_rp, u_ci, ir.tri_inverse(u_rp, u_ci, u_v, u_rp, u_ci, False))
    return {"trs": lambda r: spla.spsolve_triangular(upper, spla.spsolve_triangular(lower, r, lower=True),
                                                     lower=False),
            "isai": lambda r: w_u @ (w_l @ r)}


def device_preconditioner(kind, inner):
    if kind == "ic":
        f = g.Ic.build().with_factorization(
            g.factorization.ParIct.build().with_iterations(ITERATIONS).with_fill_in_limit(LIMIT))
        return f.with_l_solver(g.LowerIsai.build()) if inner == "isai" else f
    f = g.Ilu.build().with_factorization(
        g.factorization.ParIlut.build().with_iterations(ITERATIONS).with_fill_in_limit(LIMIT))
    return f.with_l_solver(g.LowerIsai.build()).with_u_solver(g.UpperIsai.build()) if inner == "isai" else f


def check_solver(gexec, kind, inner, name, lambda_min):
    a, a_host, b = problem(gexec, name)
    solver_cls, host = (g.Cg, host_pcg) if kind == "ic" else (g.Gmres, host_gmres)
    x_host, its_host = host(a_host, b, host_preconditioners(kind, name)[inner])
    s, x = solve_with(gexec, solver_cls, a, b, device_preconditioner(kind, inner))
    m = s.get_preconditioner()
    assert isinstance(m.factorization, g.factorization.ParIct if kind == "ic" else g.factorization.ParIlut)
    assert m.factorization.iterations == ITERATIONS and m.factorization.fill_in_limit == LIMIT
    assert isinstance(m.get_l_solver(), g.LowerIsai if inner == "isai" else g.LowerTrs)
    print("%s + %s + %s on %s: device %d iterations, host %d" % (
        solver_cls.__name__, type(m.factorization).__name__, inner, name, s.num_iterations, its_host))
    assert s.has_converged and abs(s.num_iterations - its_host) <= 1
    assert np.linalg.norm(b - a_host @ x) <= 1.01 * REDUCTION * np.linalg.norm(b)
    assert np.linalg.norm(x - x_host) <= 2.1 * REDUCTION * np.linalg.norm(b) / lambda_min


# the system of each kind: (case, its smallest eigenvalue)
SYSTEMS = {"ilu": ("stencil6", LAMBDA_MIN), "ic": ("laplace6", LAMBDA_MIN_LAPLACE)}


@pytest.mark.parametrize("inner", ["trs", "isai"])
@pytest.mark.parametrize("kind", ["ic", "ilu"])
def test_solvers_match_the_host(gexec, kind, inner):
    """Gmres with Ilu + ParIlut on the 27-point stencil on 6^3 points and Cg with Ic + ParIct on the 7-point
    Laplacian on 6^3 points (3 iterations, limit 2.0), with the level-scheduled solvers and with ISAI, against the
    same iteration on the host with the restatement's factors.  The criteria are those of
    test_solvers_with_three_sweeps_match_the_host: both sides stop at ||r|| <= 1e-10 ||b||, so x_dev - x_host =
    A^-1 (r_host - r_dev) is at most 2e-10 ||b|| / lambda_min(A) long (2.1e-10 is asserted), and the iteration
    counts agree within one.

    Why the two kinds have a stencil each: the comparison needs a host iteration, and that needs factors of the
    RESTATEMENT that are finite.  On the 27-point stencil the restatement of ParIct holds NaN from 5^3 points on
    (test_par_ict_breaks_down_on_the_27_point_stencil), whatever the device does, so no reference exists there;
    on the 7-point Laplacian it is finite, and there PCG with the exact solves takes 9 iterations against 12 with
    IC(0)."""
    name, lambda_min = SYSTEMS[kind]
    check_solver(gexec, kind, inner, name, lambda_min)
    if (kind, inner) == ("ic", "trs"):
        a_host = case_matrix(name, True)
        assert host_pcg(a_host, np.ones(GRID ** 3), host_preconditioners("ic", name)["trs"])[1] == 9


def test_par_ict_breaks_down_on_the_27_point_stencil(gexec):
    """A property of the loop as it is specified, pinned so that it cannot go unnoticed: L_0 keeps the
    off-diagonal entries of A (-1) next to a diagonal of sqrt(26), five times what the factor holds there; the
    first sweep on the wide pattern of L L^T reads them as the other rows' values and leaves off-diagonal entries
    up to 1.8 in rows of up to 32 entries, and the second sweep of the same iteration takes the root of 26 minus
    the sum of their squares.  On 6^3 points the restatement has 52 NaN after iteration 1 and 3831 of 4096
    entries after iteration 2 (11 after iteration 1 on 5^3, none on 4^3).  Pivots are not checked and nothing is
    guarded by "is finite", a NaN ranks above every number and is kept as a tie: the device factor is the
    restatement's, NaN for NaN, generate returns, and Cg with it does not converge.  ParIlut takes no root and is
    finite on the same matrix."""
    a = case_matrix("stencil6", True)
    rp, ci, v = fr.arrays(a)
    dev = device_csr(gexec, rp, ci, v)
    at = tr.par_ict_at(rp, ci, v, (1, 2), LIMIT)
    assert int(np.isnan(at[1][2]).sum()) == 52
    assert int(np.isnan(at[2][2]).sum()) == 3831 and len(at[2][2]) == 4096
    for iterations in (1, 2):
        same(factors_of("ic", generate(gexec, "ic", dev, iterations, LIMIT)), at[iterations], np.int32, equal_nan=True)
    small = fr.arrays(case_matrix("stencil4", True))
    assert np.isfinite(tr.par_ict_factor(*small, 5, LIMIT)[2]).all()
    assert all(np.isfinite(x).all() for x in factors_of("ilu", generate(gexec, "ilu", dev, 2, LIMIT)))
