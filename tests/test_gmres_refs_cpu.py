"""Checks of tests/gmres_refs.py against formulations that share no code with it (no GPU): matrix products in
long double for the element-wise kernels, np.vdot for multi_dot, np.linalg.lstsq for the rotations and the back
substitution as a whole, and for the two tree sums an emulation of the tree in the value type, which must stay
inside the derived bound while a result that lost one product of median size does not."""
import numpy as np
import pytest

import binding_refs as br
import gmres_refs as gr
from binding_gpu import same_bits

TYPES = ("f64", "f32", "c128", "c64")


def _wide(t):
    return np.clongdouble if br.is_complex(t) else np.longdouble


def _close(a, b, t, factor=64):
    a, b = np.asarray(a).astype(_wide(t)), np.asarray(b).astype(_wide(t))
    scale = max(float(np.max(np.abs(b))) if b.size else 0.0, 1e-300)
    return a.shape == b.shape and (a.size == 0 or float(np.max(np.abs(a - b))) <= factor * br.eps_of(t) * scale)


@pytest.mark.parametrize("tn", TYPES)
def test_initialize_and_restart(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(1)
    b = gr.rand(rng, (7, 3), t)
    b[2, 1] = -0.0
    res, gs, gc, stop = gr.initialize(b, 4)
    assert same_bits(res, b) and gs.shape == gc.shape == (4, 3) and not gs.any() and not gc.any()
    assert stop.dtype == np.uint8 and not stop.any()
    norm = rng.uniform(0.5, 2, 3).astype(br.real_of(t))
    for ar in (br.hp(t), br.plain(t)):
        k0, rnc0, fin = gr.restart(ar, b, norm)
        assert _close(k0, b.astype(_wide(t)) * (1 / norm.astype(np.longdouble)), t)
        assert np.array_equal(rnc0, norm.astype(ar.wt)) and fin.dtype == np.uint64 and not fin.any()
    assert gr.restart(br.plain(t), b, norm)[0].dtype == np.dtype(t)


@pytest.mark.parametrize("tn", TYPES)
def test_multi_axpy_is_a_matrix_product(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(2)
    kd, n, nrhs = 8, 13, 7
    basis, y = gr.rand(rng, (kd + 1, n, nrhs), t), gr.rand(rng, (kd, nrhs), t)
    fin = np.array([0, 1, 3, 4, 5, 7, 8], np.uint64)
    stop = np.array([0, 0, gr.STOPPED, 0, gr.FINALIZED, 0, gr.STOPPED], np.uint8)
    out0 = np.full((n, nrhs), np.nan, t)
    wide = basis.astype(_wide(t))
    for ar in (br.hp(t), br.plain(t)):
        out, after = gr.multi_axpy(ar, basis, y, fin, stop, out0)
        for k in range(nrhs):
            m = int(fin[k])
            if k == 4:
                assert np.all(np.isnan(out[:, k]))
            else:
                assert _close(out[:, k], wide[:m, :, k].T @ y[:m, k].astype(_wide(t)), t) and \
                    not (m == 0 and out[:, k].any())
        assert list(after) == [0, 0, 0xC1, 0, 0xC2, 0, 0xC1]


@pytest.mark.parametrize("tn", TYPES)
@pytest.mark.parametrize("nrhs", (1, 3))
def test_multi_sub_scaled_is_a_matrix_product(tn, nrhs):
    t = br.TYPES[tn]
    rng = np.random.default_rng(3)
    num, n = 9, 11
    basis, h, w = gr.rand(rng, (num, n, nrhs), t), gr.rand(rng, (num, nrhs), t), gr.rand(rng, (n, nrhs), t)
    wide = _wide(t)
    for ar in (br.hp(t), br.plain(t)):
        got = gr.multi_sub_scaled(ar, basis, h, w)
        ref = w.astype(wide) - np.einsum("dnk,dk->nk", basis.astype(wide), h.astype(wide))
        assert _close(got, ref, t)
    # a zero h: skipped at one column (NaN and -0.0 stay out), subtracted at three
    h[4] = 0
    basis[4, 0] = np.nan
    basis[4, 1] = -1.0
    w[1] = -0.0
    got = gr.multi_sub_scaled(br.plain(t), basis, h, w)
    rest = gr.multi_sub_scaled(br.plain(t), np.delete(basis, 4, 0), np.delete(h, 4, 0), w)
    if nrhs == 1:
        assert same_bits(got, rest)
    else:
        assert np.all(np.isnan(got[0].real)) and same_bits(got[2:], rest[2:])


@pytest.mark.parametrize("tn", TYPES)
def test_multi_dot_and_mgs_step_against_vdot(tn):
    t = br.TYPES[tn]
    wide = _wide(t)
    basis, nxt = gr.multi_dot_case(tn, 2049, 3, 3)
    for ar in (br.hp(t), br.plain(t)):
        h, s = gr.multi_dot(ar, basis, nxt)
        for d in range(3):
            for k in range(3):
                ref = np.vdot(basis[d, :, k].astype(wide), nxt[:, k].astype(wide))
                assert abs(h[d, k] - ref) <= 2049 * br.eps_of(t) * float(s[d, k])
                assert abs(float(s[d, k]) - float(np.sum(np.abs(basis[d, :, k].astype(wide) * nxt[:, k])))) < 1e-3
    for zero_h in (False, True):
        w, v, h, vn = gr.mgs_case(tn, 2047, zero_h)
        for ar in (br.hp(t), br.plain(t)):
            w1, hn, s = gr.mgs_step(ar, w, v, h, vn)
            ref_w = w.astype(wide) - wide(h) * v.astype(wide)
            assert _close(w1, ref_w, t) and abs(hn - np.vdot(vn.astype(wide), ref_w)) <= 2047 * br.eps_of(t) * float(s)
        if zero_h:
            assert same_bits(gr.mgs_step(br.plain(t), w, v, h, vn)[0], w)


# ---------------------------------------------------------------------- rotations + back substitution
@pytest.mark.parametrize("tn", TYPES)
@pytest.mark.parametrize("kd", (1, 2, 7))
def test_sweep_solves_the_least_squares_problem(tn, kd):
    t = br.TYPES[tn]
    nrhs = 5
    zp = (min(1, kd - 1), 3)
    hraw, beta = gr.hessenberg_case(40 + kd, t, kd, nrhs, zero_pivot=zp)
    stop_from = {1: 2} if kd > 2 else None
    for ar in (br.hp(t), br.plain(t)):
        tol = 1e-15 if ar.name == "hp" else 64 * kd * br.eps_of(t)
        r = gr.sweep(ar, hraw, beta, stop_from=stop_from)
        assert r["gcos"][zp[0], zp[1]] == 0 and r["gsin"][zp[0], zp[1]] == 1           # the zero-pivot branch
        cs = np.abs(r["gcos"].astype(_wide(t))) ** 2 + np.abs(r["gsin"].astype(_wide(t))) ** 2
        for k in range(nrhs):
            m = int(r["fin"][k])
            assert m == (2 if stop_from and k == 1 else kd)
            assert np.all(np.abs(cs[:m, k] - 1) <= tol)
            assert all(r["hess"][it, it + 1, k] == 0 for it in range(m))                  # exactly zero
            H = gr.dense_hessenberg(hraw, k)[:m + 1, :m].astype(np.complex128 if br.is_complex(t) else np.float64)
            e1 = np.zeros(m + 1, H.dtype)
            e1[0] = beta[k]
            y, _, _, _ = np.linalg.lstsq(H, e1, rcond=None)
            res = float(np.linalg.norm(e1 - H @ y))
            scale = float(np.max(np.abs(y)))
            assert np.max(np.abs(r["y"][:m, k] - y)) <= max(tol, 1e-14) * 16 * scale, (k, r["y"][:m, k], y)
            if not (stop_from and k == 1):
                assert abs(float(r["rn"][k]) - res) <= max(tol, 1e-14) * 16 * float(beta[k])
            assert not r["y"][m:, k].any()
    fin_y = gr.sweep(br.plain(t), hraw, beta, finalized=(2,))["y"]
    assert not fin_y[:, 2].any() and fin_y[:, 0].any()


@pytest.mark.parametrize("cx", (False, True))
def test_householder_least_squares(cx):
    rng = np.random.default_rng(9)
    H = np.triu(rng.standard_normal((6, 5)), -1) + (1j * np.triu(rng.standard_normal((6, 5)), -1) if cx else 0)
    rhs = np.zeros(6, H.dtype)
    rhs[0] = 1.5
    y, res = gr.lstsq_hp(H, rhs)
    ref = np.linalg.lstsq(H, rhs, rcond=None)[0]
    assert np.max(np.abs(y - ref)) <= 1e-13 * np.max(np.abs(ref))
    assert abs(float(res) - np.linalg.norm(rhs - H @ ref)) <= 1e-13
    assert y.dtype == (np.clongdouble if cx else np.longdouble)


def test_stopped_column_keeps_its_bits():
    t = np.float64
    hraw, beta = gr.hessenberg_case(5, t, 3, 4)
    ar = br.plain(t)
    free = gr.sweep(ar, hraw[:2], beta)
    held = gr.sweep(ar, hraw, beta, stop_from={2: 2})
    assert held["fin"][2] == 2 and list(held["fin"][[0, 1, 3]]) == [3, 3, 3]
    assert same_bits(held["rnc"][:3, 2], free["rnc"][:3, 2]) and same_bits(held["gsin"][:2, 2], free["gsin"][:2, 2])
    assert held["rn"][2] == free["rn"][2] and held["gsin"][2, 2] == 0 and held["rnc"][3, 2] == 0


# ------------------------------------------------------------------------------------ the tree bounds
def test_depths():
    assert gr.multi_dot_depth(1) == 4 + 8 + 1 + 8 and gr.multi_dot_depth(262144) == 21
    assert gr.multi_dot_depth(263169) == 22                       # 258 chunks: the second trip of stage 2
    assert gr.mgs_step_depth(5, 2) == 2 + 1 + 8 + 1 + 10 and gr.mgs_step_depth(5, 2, False) == 1 + 8 + 1 + 10
    assert gr.mgs_blocks(4196353) == 2048 and gr.mgs_blocks(4194304) == 2048 and gr.mgs_blocks(2049) == 2
    # 4 196 353 rows of f32: 1 049 088 vectors over 524 288 threads: three vectors of four, the tail, two
    # partials per fold thread
    assert gr.mgs_step_depth(4196353, 4) == 12 + 1 + 8 + 2 + 10
    assert gr.term_roundings(np.float32) == 1 and gr.term_roundings(np.complex64) == 2


def _part_sum(terms):
    """sum |re| + sum |im| of the terms: bounds either part of every partial sum, in any order"""
    return np.sum(np.abs(terms.real)) + np.sum(np.abs(terms.imag))


def _lost_one(terms):
    """the median modulus of the terms: what a sum that dropped one typical product is off by"""
    return float(np.median(np.abs(terms)))


@pytest.mark.parametrize("tn", TYPES)
@pytest.mark.parametrize("rows", [r for r in gr.MULTI_DOT_ROWS if r])
def test_multi_dot_tree_bound(tn, rows):
    t = br.TYPES[tn]
    single = tn in ("f32", "c64")
    basis, nxt = gr.multi_dot_case(tn, rows, 1, 1)
    ref, s = gr.multi_dot(br.hp(t), basis, nxt)
    bound = float(gr.dot_bound(t, gr.multi_dot_depth(rows), s[0, 0]))
    tree = gr.multi_dot_tree(t, basis[0, :, 0], nxt[:, 0])
    assert abs(_wide(t)(tree) - ref[0, 0]) <= bound
    lost = _lost_one(basis[0, :, 0].astype(_wide(t)) * nxt[:, 0])
    if gr.needs_exact(tn, rows):
        assert single                 # the bound is about one median product or wider: the exact case has the teeth
        basis, nxt = gr.multi_dot_case(tn, rows, 1, 1, exact=True)
        ref, s = gr.multi_dot(br.hp(t), basis, nxt)
        watch = br.Exact()
        watch.see(_part_sum(basis[0, :, 0].astype(_wide(t)).conj() * nxt[:, 0]))
        assert gr.multi_dot_tree(t, basis[0, :, 0], nxt[:, 0]) == t(ref[0, 0])
        assert gr.multi_dot(br.plain(t), basis, nxt)[0][0, 0] == t(ref[0, 0])
    else:
        assert lost > bound, (lost, bound)


# (the block-cap size runs in f32 and c128, aligned)
MGS_CASES = [(tn, rows, vec_ok) for tn in TYPES for rows in gr.MGS_ROWS if rows for vec_ok in (True, False)
             if rows <= gr.SINGLE_TEETH_LIMIT or (tn in gr.MGS_BIG_TYPES and vec_ok)]


@pytest.mark.parametrize("tn,rows,vec_ok", MGS_CASES)
def test_mgs_tree_bound(tn, rows, vec_ok):
    t = br.TYPES[tn]
    w, v, h, vn = gr.mgs_case(tn, rows)
    w1, ref, s = gr.mgs_step(br.hp(t), w, v, h, vn)
    wp = gr.mgs_step(br.plain(t), w, v, h, vn)[0]
    ref = np.sum(np.conj(vn.astype(_wide(t))) * wp)              # the dot of the kernel's own (rounded) w
    bound = float(gr.dot_bound(t, gr.mgs_step_depth(rows, gr.vec_width(t), vec_ok), s))
    assert abs(_wide(t)(gr.mgs_dot_tree(t, wp, vn, vec_ok)) - ref) <= bound
    lost = _lost_one(np.conj(vn.astype(_wide(t))) * wp)
    if gr.needs_exact(tn, rows):
        assert lost <= bound                                    # no teeth here: the exact case has them
        w, v, h, vn = gr.mgs_case(tn, rows, exact=True)
        w1, ref, s = gr.mgs_step(br.hp(t), w, v, h, vn)
        watch = br.Exact()
        watch.see(w1)
        watch.see(_part_sum(np.conj(vn.astype(_wide(t))) * w1))
        assert gr.mgs_dot_tree(t, w1.astype(t), vn, vec_ok) == t(ref)
    else:
        assert lost > bound, (lost, bound)
