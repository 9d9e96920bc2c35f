"""tests/jacobi_refs.py against independent formulations (no GPU): the C oracle bit for bit in f64 (find_blocks,
generate, apply, convert_storage, apply_stored), the reference's stored results of tests/golden/jacobi_types.npz for
f32, c64 and c128, numpy.linalg.inv, dense per-block transposes and products - and the conditions on the inputs
that tests/test_jacobi_kernels_gpu.py relies on: the pivot margin of every complex block at every elimination step,
and the exactly zero pivot of the singular blocks."""
import os

import numpy as np
import pytest

import binding_refs as br
import jacobi_refs as jr
import value_kernel_refs as vr
from binding_gpu import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "jacobi_types.npz")
TYPES = ("f64", "f32", "c128", "c64")


# ------------------------------------------------------------------------------------------ find_blocks
pattern, PATTERNS = jr.pattern, jr.PATTERNS


def find_blocks_loop(row_ptrs, cols, max_bs):
    """the two passes of the reference written as the loops it runs (find_natural_blocks, agglomerate_supervariables)"""
    n = len(row_ptrs) - 1
    if n == 0:
        return [0]
    ptrs = [0]
    size = 1
    for i in range(1, n):
        a, b = cols[row_ptrs[i - 1]:row_ptrs[i]], cols[row_ptrs[i]:row_ptrs[i + 1]]
        if len(a) == len(b) and all(a == b) and size < max_bs:
            size += 1
        else:
            ptrs.append(i)
            size = 1
    ptrs.append(n)
    out = [0]
    size = ptrs[1] - ptrs[0]
    for k in range(1, len(ptrs) - 1):
        nxt = ptrs[k + 1] - ptrs[k]
        if size + nxt <= max_bs:
            size += nxt
        else:
            out.append(ptrs[k])
            size = nxt
    out.append(n)
    return out


@pytest.mark.parametrize("kind", PATTERNS)
def test_find_blocks_equals_the_oracle_and_the_loop_form(oracle, kind):
    for n in (0, 1, 2, 7, 255, 256, 257, 1000):
        for max_bs in (1, 2, 13, 32, 64):
            rp, cols = pattern(kind, n, max_bs)
            got = jr.find_blocks(rp, cols, max_bs)
            assert list(got) == find_blocks_loop(rp, cols, max_bs), (kind, n, max_bs)
            if n:
                nb, ptrs = oracle.jacobi_find_blocks(rp.astype(np.int32), cols.astype(np.int32), max_bs)
                assert nb == len(got) - 1 and np.array_equal(ptrs[:nb + 1], got), (kind, n, max_bs)
            assert np.all(np.diff(got) <= max_bs) and (n == 0 or np.all(np.diff(got) >= 1))


def test_find_blocks_patterns_are_what_they_claim():
    rp, cols = pattern("same", 100, 13)
    assert np.array_equal(np.diff(jr.find_blocks(rp, cols, 13)), [13] * 7 + [9])
    rp, cols = pattern("alternate", 9, 4)                  # single natural blocks, agglomerated to max_bs
    assert np.array_equal(np.diff(jr.find_blocks(rp, cols, 4)), [4, 4, 1])
    rp, cols = pattern("natural", 27, 4)     # natural runs of 13 rows cut at 4: 4 4 4 1 | 4 4 4 1 | 1, the last two merge
    assert np.array_equal(np.diff(jr.find_blocks(rp, cols, 4)), [4, 4, 4, 1, 4, 4, 4, 2])
    rp, cols = pattern("chain", 5, 1)
    assert np.array_equal(jr.find_blocks(rp, cols, 1), np.arange(6))


# --------------------------------------------------------------------------------------- scheme and layout
def test_scheme_equals_the_oracle(oracle):
    for max_bs in range(1, 65):
        assert jr.storage_scheme(max_bs).as_tuple() == tuple(oracle.jacobi_storage_scheme(max_bs))
    wide = [m for m in range(1, 65) if jr.wide_group_layout(jr.storage_scheme(m))]
    assert wide == [1, 2, 4, 8, 16]
    assert [m for m in range(1, 65) if jr.wave_group_layout(jr.storage_scheme(m))] == list(range(1, 33))
    assert [jr.groups_per_wave(bo, 8) for bo in (1, 2, 4, 8, 16)] == [2, 2, 2, 2, 1]
    assert [jr.groups_per_wave(bo, 4) for bo in (1, 2, 4, 8, 16)] == [2, 2, 2, 2, 2]


def test_launcher_predicates():
    s8, s4, s13 = jr.storage_scheme(8), jr.storage_scheme(4), jr.storage_scheme(13)
    assert jr.apply_branch(s8, 8, 1, 1, 1, 0, 0) == ("fixed", None)
    assert jr.apply_branch(s8, 8, 1, 3, 2, 0, 0) == ("general", None)
    assert jr.apply_branch(s8, 8, 4, 4, 4, 0, 0) == ("multi4", True)
    assert jr.apply_branch(s8, 8, 5, 6, 6, 8, 0) == ("multi8", False)
    assert jr.apply_branch(s8, 8, 8, 9, 10, 0, 0) == ("multi8", False)
    assert jr.apply_branch(s8, 8, 9, 9, 9, 0, 0) == ("mfma", None)
    assert jr.apply_branch(s8, 4, 9, 9, 9, 0, 0) == ("multi8", False)          # float: no matrix-core kernel
    assert jr.apply_branch(s4, 8, 17, 18, 18, 0, 0) == ("multi8", True)
    assert jr.apply_branch(s13, 8, 3, 3, 3, 0, 0) == ("general", None)
    # 65 536 single-row blocks under a max_block_size 16 scheme: 4096 workgroups in double, 2048 in float
    s16 = jr.storage_scheme(16)
    assert jr.fixed_workgroups(s16, 65536, 8) == 4096 and not jr.step2_apply_fits(s16, 65536, 65536, 8)
    assert jr.fixed_workgroups(s16, 65536, 4) == 2048 and jr.step2_apply_fits(s16, 65536, 65536, 4)
    # the xcd_map sizes: 2048 and 2051 workgroups
    s1 = jr.storage_scheme(1)
    assert jr.fixed_workgroups(s1, 1048576, 8) == 2048 and jr.fixed_workgroups(s1, 1050112, 8) == 2051
    assert jr.fixed_workgroups(s1, 1048576, 4) == 2048 and jr.xcd_map_applies(2048, 1)
    assert not jr.xcd_map_applies(2047, 1) and not jr.xcd_map_applies(4096, 0)


def test_fused_dot_depth():
    s8 = jr.storage_scheme(8)
    assert jr.fused_dot_depth(s8, 1, 8) == 2 + 8 + 1 + 10
    assert jr.fused_dot_depth(jr.storage_scheme(16), 9, 8) == 1 + 8 + 1 + 10
    assert jr.fused_dot_depth(jr.storage_scheme(16), 9, 4) == 2 + 8 + 1 + 10
    # above fold_single_max partials: chunks first
    s1 = jr.storage_scheme(1)
    nb = jr.fixed_workgroups(s1, 64 * 8 * 20000, 8)
    assert nb == 20000 and jr.fused_dot_depth(s1, 64 * 8 * 20000, 8) == 2 + 8 + 1 + 8 + 1 + 10
    assert jr.fused_dot_depth(s1, 64 * 8 * 20000, 8, rows_fold=True) == 2 + 8 + 20 + 10


# ------------------------------------------------------------------------------------------------ generate
@pytest.mark.parametrize("max_bs", jr.GENERATE_SIZES["f64"])
def test_generate_f64_equals_the_oracle_bit_for_bit(oracle, max_bs):
    c = jr.generate_case("f64", max_bs)
    nb = len(c["block_ptrs"]) - 1
    rp, cols, ptrs = (c[k].astype(np.int32) for k in ("row_ptrs", "cols", "block_ptrs"))
    want = oracle.jacobi_generate(rp, cols, c["vals"], nb, c["scheme"].as_tuple(), ptrs)
    got, runs = jr.generate(br.plain(np.float64), c["row_ptrs"], c["cols"], c["vals"], c["scheme"], c["block_ptrs"],
                            np.zeros(want.shape))
    sing = [b for b, nm in enumerate(c["names"]) if nm == "singular"]
    mask = jr.entry_mask(c["scheme"], c["block_ptrs"], want.shape[0])
    assert same_bits(got[mask], want[mask]), max_bs
    assert sing and all(runs[b]["dead"] is not None for b in sing)


@pytest.mark.parametrize("tn", TYPES)
def test_every_generate_input_has_a_clear_pivot_order(tn):
    """what the GPU file relies on.  Complex types: in the long-double run every elimination step of EVERY block has
    a largest candidate that beats the runner-up by 2^-10 (relative) or ties with it through identical |re|, |im|
    bits, so hypot cannot choose another row; and the value-type run picks the same rows.  All types: the blocks
    named singular reach an exactly zero pivot, in the value type and in long double, and no other block does"""
    t = br.TYPES[tn]
    for max_bs in jr.GENERATE_SIZES[tn]:
        c = jr.generate_case(tn, max_bs)
        assert len(c["block_ptrs"]) - 1 == c["per_wave"] * max(2, -(-8 // c["per_wave"])) + 1
        sizes = np.diff(c["block_ptrs"])
        assert sizes.max() == max_bs and sizes.min() == 1 and (max_bs < 3 or len(set(sizes)) >= 3)
        assert "singular" in c["names"] and (max_bs == 1 or {"tie", "zero_lead"} <= set(c["names"]))
        for b, B in enumerate(c["dense"]):
            start = int(c["block_ptrs"][b])
            assert same_bits(jr.extract_block(t, c["row_ptrs"], c["cols"], c["vals"], start, B.shape[0]), B)
            hp, pl = jr.gauss_jordan(br.hp(t), B), jr.gauss_jordan(br.plain(t), B)
            assert (hp["dead"] is not None) == (c["names"][b] == "singular") == (pl["dead"] is not None), (max_bs, b)
            if c["names"][b] == "singular":
                assert hp["dead"] == pl["dead"] and np.all(B.real == np.round(B.real)) and np.all(np.abs(B) <= 6)
            if br.is_complex(t):
                assert jr.margins_ok(hp), (tn, max_bs, b, c["names"][b])
                assert hp["pivots"] == pl["pivots"], (tn, max_bs, b)
        # unsorted columns, entries outside the blocks, missing entries inside
        rp, cols = c["row_ptrs"], c["cols"]
        assert any(np.any(np.diff(cols[rp[i]:rp[i + 1]]) < 0) for i in range(c["n"]))
        if max_bs > 1:
            assert sum(int(np.count_nonzero(B == 0)) for B in c["dense"]) > 0


def test_pivot_rule_ties_and_zero_lead():
    """the first of several rows of the largest magnitude wins; a zero leading entry is pivoted away"""
    for tn in TYPES:
        t = br.TYPES[tn]
        sp = dict(jr.special_blocks(4, t)[:2] + jr.special_blocks(4, t)[3:4])
        assert jr.gauss_jordan(br.plain(t), sp["tie"])["pivots"] == [0, 1]
        assert jr.gauss_jordan(br.plain(t), sp["tie3"])["pivots"][0] == 0
        assert jr.gauss_jordan(br.plain(t), sp["zero_lead"])["pivots"] == [1, 1]
        run = jr.gauss_jordan(br.hp(t), sp["tie"])
        assert run["margins"][0][0] == run["margins"][0][1] and run["margins"][0][2]
        # the singular block with a tie: the first row is the pivot, and the block it is left as tells
        tied = jr.special_blocks(4, t)[-1][1]
        first, last = jr.gauss_jordan(br.plain(t), tied), jr.gauss_jordan(br.plain(t), tied, pivots=[1, 1])
        assert first["pivots"] == [0, 1] and first["dead"] == 1 and last["dead"] == 1
        unit = t(1 + 1j) if br.is_complex(t) else t(1)
        assert np.array_equal(first["B"], np.array([[1 / unit, 2], [1, 0]], t)) and first["perm"] == [0, 1]
        assert not np.array_equal(first["B"][:, first["perm"]], last["B"][:, np.argsort(last["perm"])])


@pytest.mark.parametrize("tn", TYPES)
def test_inverse_against_numpy_and_the_identity(tn):
    """long double: M B = I to 1e-13; the value-type inverse within rule R of the long-double one, as is
    numpy.linalg.inv in double / complex128 for the double types (blocks up to 16 rows)"""
    t = br.TYPES[tn]
    for max_bs in (2, 3, 8, 16, 32):
        c = jr.generate_case(tn, max_bs)
        size = jr.storage_size(c["scheme"], len(c["block_ptrs"]) - 1)
        args = (c["row_ptrs"], c["cols"], c["vals"], c["scheme"], c["block_ptrs"], np.zeros(size))
        ref, runs = jr.generate(br.hp(t), *args)
        pl, _ = jr.generate(br.plain(t), *args, pivots=[r["pivots"] for r in runs])
        for b, (H, P, B) in enumerate(zip(jr.dense_blocks(c["scheme"], c["block_ptrs"], ref),
                                          jr.dense_blocks(c["scheme"], c["block_ptrs"], pl), c["dense"])):
            if runs[b]["dead"] is not None:
                continue
            eye = np.eye(B.shape[0])
            assert np.max(np.abs(H @ B.astype(H.dtype) - eye)) < 1e-13, (max_bs, b)
            cond = float(np.linalg.cond(B.astype(np.complex128)))
            assert np.max(np.abs(P.astype(H.dtype) - H)) <= 64 * B.shape[0] * cond * br.eps_of(t) * np.max(np.abs(H))
            if tn in ("f64", "c128") and B.shape[0] <= 16:
                ok, ratio = br.rule_r(np.linalg.inv(B), H, P, t, extra=8 * cond * br.eps_of(t) * float(np.max(np.abs(H))))
                assert ok, (tn, max_bs, b, ratio)


def _gold_full_cases():
    return [("f32", "8", "auto3"), ("f32", "32", "auto3"), ("c64", "13", "auto3"), ("c128", "8", "mix")]


@pytest.mark.parametrize("vt,max_bs,tag", _gold_full_cases())
def test_full_storage_products_of_the_golden_file(vt, max_bs, tag):
    """the reference's x = M b, M^T b, M^H b for float and complex blocks in full storage: float bit for bit,
    complex (the reference divides with the standard library's quotient) within rule R of the long-double result"""
    g = np.load(GOLD)
    gold = lambda k: g[f"{vt}/{max_bs}/{tag}/{k}"]      # noqa: E731
    assert not gold("prec").any()
    t = br.TYPES[vt]
    rp, ci, vals, b = (g[f"{vt}/{k}"] for k in ("row_ptrs", "col_idxs", "values", "b"))
    ptrs = gold("block_ptrs").astype(np.int64)
    scheme = jr.storage_scheme(int(max_bs))
    assert jr.wave_group_layout(scheme)
    size = jr.storage_size(scheme, len(ptrs) - 1)
    res = {}
    for name, ar in (("plain", br.plain(t)), ("hp", br.hp(t))):
        blocks, runs = jr.generate(ar, rp, ci, vals, scheme, ptrs, np.zeros(size),
                                   pivots=res["pivots"] if name == "hp" else None)
        res["pivots"] = [r["pivots"] for r in runs]
        x = jr.apply_any(ar, scheme, ptrs, blocks, b)
        xt = jr.apply_any(ar, scheme, ptrs, vr.jacobi_transpose(scheme, ptrs, blocks, False, np.zeros_like(blocks)), b)
        hb = vr.jacobi_transpose(scheme, ptrs, blocks, False, np.zeros_like(blocks))
        xh = jr.apply_any(ar, scheme, ptrs, np.conj(hb), b)
        res[name] = dict(x=x, xt=xt, xh=xh)
    for key in ("x", "xt", "xh"):
        if vt == "f32":
            assert same_bits(res["plain"][key], gold(key)), key
        else:
            ok, ratio = br.rule_r(gold(key), res["hp"][key], res["plain"][key], t)
            assert ok, (vt, key, ratio)


# ------------------------------------------------------------------------------------------------ products
@pytest.mark.parametrize("max_bs", (1, 2, 3, 4, 5, 8, 13, 16, 32, 64))
def test_apply_f64_equals_the_oracle_bit_for_bit(oracle, max_bs):
    nb = 3 * jr.storage_scheme(max_bs).group_size + 1
    for nrhs in (1, 3):
        a = jr.apply_case("f64", max_bs, nb, nrhs, fill=0.0)
        ptrs = a["block_ptrs"].astype(np.int32)
        sc = a["scheme"].as_tuple()
        want = oracle.jacobi_apply(nb, sc, ptrs, a["blocks"], a["b"])
        assert same_bits(jr.apply_tuned(br.plain(np.float64), a["scheme"], a["block_ptrs"], a["blocks"], a["b"]), want)
        for beta in (float(a["beta"][0]), 0.0):
            want = oracle.jacobi_apply(nb, sc, ptrs, a["blocks"], a["b"], float(a["alpha"][0]), beta, a["x0"])
            got = jr.apply_tuned(br.plain(np.float64), a["scheme"], a["block_ptrs"], a["blocks"], a["b"], a["alpha"][0],
                                 beta, a["x0"])
            assert same_bits(got, want), (max_bs, nrhs, beta)


@pytest.mark.parametrize("tn", TYPES)
def test_products_against_dense_blocks(tn):
    """x = M b with the blocks taken out as dense matrices (value_kernel_refs.jacobi_blocks_dense) and multiplied by
    numpy in long double: the restatement in long double agrees to 1e-17 relative, the value type within bs eps;
    NaN padding is never read; beta = 0 does not read a NaN x; the two operation orders agree in long double"""
    t = br.TYPES[tn]
    for max_bs in (1, 3, 8, 13, 32):
        nb = 2 * jr.storage_scheme(max_bs).group_size + 1
        a = jr.apply_case(tn, max_bs, nb, 2)
        wide = np.clongdouble if br.is_complex(t) else np.longdouble
        want = np.zeros(a["b"].shape, wide)
        for b, M in enumerate(jr.dense_blocks(a["scheme"], a["block_ptrs"], a["blocks"])):
            s, e = int(a["block_ptrs"][b]), int(a["block_ptrs"][b + 1])
            want[s:e] = M.astype(wide) @ a["b"][s:e].astype(wide)
        args = (a["scheme"], a["block_ptrs"], a["blocks"], a["b"])
        for fn in (jr.apply_tuned, jr.apply_any):
            assert np.max(np.abs(fn(br.hp(t), *args) - want)) <= 1e-17 * max_bs
            assert np.max(np.abs(fn(br.plain(t), *args) - want)) <= 4 * max_bs * br.eps_of(t)
            adv = fn(br.hp(t), *args, a["alpha"][0], a["beta"][0], a["x0"])
            assert np.max(np.abs(adv - (wide(a["alpha"][0]) * want + wide(a["beta"][0]) * a["x0"]))) <= 1e-17 * max_bs
            nanx = np.full(a["x0"].shape, np.nan, t)
            zero = fn(br.plain(t), *args, a["alpha"][0], t(0), nanx)
            assert np.all(np.isfinite(zero))
            assert same_bits(zero, fn(br.plain(t), *args, a["alpha"][0], t(0), a["x0"]))
        if not br.is_complex(t):
            bound = jr.apply_abs_sum(a["scheme"], a["block_ptrs"], a["blocks"], a["b"])
            assert np.all(np.abs(jr.apply_tuned(br.plain(t), *args) - want) <= max_bs * br.eps_of(t) * bound)


# ----------------------------------------------------------------------------------------- reduced storage
@pytest.mark.parametrize("prec", jr.PRECISIONS)
def test_stored_f64_equals_the_oracle_bit_for_bit(oracle, prec):
    for max_bs in (1, 2, 4, 8, 16):
        nb = 2 * jr.storage_scheme(max_bs).group_size + 1
        a = jr.apply_case("f64", max_bs, nb, 1, fill=-777.25)
        a["blocks"][::7] *= 1e-6                        # below the normal half range: signed zeros
        a["blocks"][3::11] *= 3e5                       # above it: infinities
        sc = a["scheme"].as_tuple()
        want = oracle.jacobi_convert_storage(nb, sc, a["blocks"], prec)
        got = jr.convert_storage(a["scheme"], nb, a["blocks"], prec)
        assert same_bits(got, want), (prec, max_bs)
        groups = np.full(jr.num_groups(a["scheme"], nb), prec)
        assert same_bits(jr.convert_groups(a["scheme"], nb, a["blocks"], groups), got)
        wide = jr.widen_storage(a["scheme"], nb, got, groups)
        mask = jr.entry_mask(a["scheme"], a["block_ptrs"], wide.shape[0])
        finite = np.where(mask & np.isfinite(wide), wide, 0.0)
        ptrs = a["block_ptrs"].astype(np.int32)
        got_fin = jr.convert_storage(a["scheme"], nb, np.where(np.isfinite(wide), a["blocks"], 0.0), prec)
        want_x = oracle.jacobi_apply_stored(nb, sc, ptrs, got_fin, prec, a["b"][:, 0])
        assert same_bits(jr.apply_tuned(br.plain(np.float64), a["scheme"], a["block_ptrs"], finite, a["b"])[:, 0], want_x)
        want_x = oracle.jacobi_apply_stored(nb, sc, ptrs, got_fin, prec, a["b"][:, 0], 0.75, -1.5, a["x0"][:, 0])
        got_x = jr.apply_tuned(br.plain(np.float64), a["scheme"], a["block_ptrs"], finite, a["b"], 0.75, -1.5, a["x0"])
        assert same_bits(got_x[:, 0], want_x), (prec, max_bs)


def test_storage_conversions_by_hand():
    """the five conversions on edge values against the bit patterns written out by hand"""
    v = np.array([1.0, -1.5, 1.0 + 2.0 ** -30, 3.0e-5, 6.0e-5, 65504.0, 65520.0, 1e6, -0.0, 0.1])
    f = v.astype(np.float32)
    assert same_bits(jr._narrow(0x01, v), f)
    assert same_bits(jr._narrow(0x02, v), br.f32_to_half_bits_by_hand(f))
    assert same_bits(jr._narrow(0x10, v), (v.view(np.uint64) // 2 ** 32).astype(np.uint32))
    assert same_bits(jr._narrow(0x20, v), (v.view(np.uint64) // 2 ** 48).astype(np.uint16))
    assert same_bits(jr._narrow(0x11, v), (f.view(np.uint32) // 2 ** 16).astype(np.uint16))
    for prec in jr.PRECISIONS:
        back = jr._widen(prec, jr._narrow(prec, v))
        exact = np.array([1.0, -1.5, -0.0])
        assert same_bits(jr._widen(prec, jr._narrow(prec, exact)), exact)
        rel = {0x01: 2.0 ** -24, 0x02: 2.0 ** -11, 0x10: 2.0 ** -20, 0x11: 2.0 ** -7, 0x20: 2.0 ** -4}[prec]
        ok = np.abs(v) < 6.0e4 if prec == 0x02 else np.ones(v.shape, bool)
        ok &= ~((prec == 0x02) & (np.abs(v) < 6.2e-5))
        assert np.all(np.abs(back - v)[ok] <= rel * np.abs(v)[ok]), prec
    assert jr._widen(0x02, jr._narrow(0x02, np.array([3.0e-5])))[0] == 0.0          # below 2^-14: signed zero


# ------------------------------------------------------------------------------------------ transposes
@pytest.mark.parametrize("tn", TYPES)
def test_block_transpose_is_the_dense_transpose(tn):
    for max_bs in (1, 5, 13, 32):
        a = jr.apply_case(tn, max_bs, 2 * jr.storage_scheme(max_bs).group_size + 1, 1)
        out0 = np.full(a["blocks"].shape, -3.0, a["blocks"].dtype)
        tr = vr.jacobi_transpose(a["scheme"], a["block_ptrs"], a["blocks"], False, out0)
        for M, T in zip(jr.dense_blocks(a["scheme"], a["block_ptrs"], a["blocks"]),
                        jr.dense_blocks(a["scheme"], a["block_ptrs"], tr)):
            assert same_bits(T, np.ascontiguousarray(M.T))
        mask = jr.entry_mask(a["scheme"], a["block_ptrs"], tr.shape[0])
        assert np.all(tr[~mask] == -3.0)
        back = vr.jacobi_transpose(a["scheme"], a["block_ptrs"], tr, False, a["blocks"])
        assert same_bits(back, a["blocks"])


# ------------------------------------------------------------------------------------------ fused kernels
@pytest.mark.parametrize("tn", ("f64", "f32"))
def test_fused_compositions(tn):
    """step_2 + apply and the PipeCg steps + apply are the separate restatements chained; integer-valued inputs
    stay integral and small, so their sums are exact in either type and any order"""
    t = br.TYPES[tn]
    for state in ("run", "stopped", "beta0", "prev0", "delta"):
        a = jr.fused_case(tn, 8, 19, state=state)
        v = a["vec"]
        blk = (a["scheme"], a["block_ptrs"], a["blocks"])
        got = jr.step2_apply(br.plain(t), *blk, v)
        if state in ("stopped", "beta0"):
            assert same_bits(got["x"], v["x"]) and same_bits(got["r"], v["r"])
        else:
            tmp = t(v["rho"][0] / v["beta"][0])
            assert same_bits(got["r"], (v["r"] - (tmp * v["q"]).astype(t)).astype(t))
        assert same_bits(got["z"], jr.apply_dot(br.plain(t), *blk, got["r"]))
        p = jr.pipe_steps(br.plain(t), *blk, v)
        assert same_bits(p["m"], jr.apply_dot(br.plain(t), *blk, p["w"]))
        if state == "stopped":
            assert all(same_bits(p[k], v[k]) for k in "xrzwpqfg") and same_bits(p["beta_out"], v["beta_in"])
        if state == "delta":
            assert same_bits(p["beta_out"], v["delta"])
    a = jr.fused_case(tn, 8, 19, exact=True)
    watch = br.Exact()
    blk = (a["scheme"], a["block_ptrs"], a["blocks"])
    for out in (jr.step2_apply(br.hp(t), *blk, a["vec"]), jr.pipe_steps(br.hp(t), *blk, a["vec"])):
        for k, val in out.items():
            watch.see(val)
    s2 = jr.step2_apply(br.hp(t), *blk, a["vec"])
    sums, sabs = jr.dots_hp([(s2["r"], s2["z"]), (s2["r"], s2["r"])])
    watch.see(sabs)
    assert same_bits(jr.step2_apply(br.plain(t), *blk, a["vec"])["z"], s2["z"].astype(t))


def test_transpose_of_stored_words():
    """the raw-word transpose of mixed-precision groups: widened, every block is the dense transpose of the widened
    original, whatever the group's type; twice is the identity on the bytes"""
    for max_bs in (4, 13):
        sc = jr.storage_scheme(max_bs)
        nb = 5 * sc.group_size + 1
        a = jr.apply_case("f64", max_bs, nb, 1, fill=-777.25)
        gp = np.array([0x00, 0x01, 0x02, 0x10, 0x11, 0x20])
        st = jr.convert_groups(sc, nb, a["blocks"], gp)
        bp = np.repeat(gp, sc.group_size)[:nb]
        tr = jr.transpose_stored(sc, a["block_ptrs"], st, bp, st)
        for M, T in zip(jr.dense_blocks(sc, a["block_ptrs"], jr.widen_storage(sc, nb, st, gp)),
                        jr.dense_blocks(sc, a["block_ptrs"], jr.widen_storage(sc, nb, tr, gp))):
            assert same_bits(T, np.ascontiguousarray(M.T))
        assert same_bits(jr.transpose_stored(sc, a["block_ptrs"], tr, bp, tr), st)


def test_float_and_complex_storage_kinds():
    """float parts fall on two 16-bit types; a complex entry is stored as its two parts"""
    assert [jr.storage_kind(np.float32, p) for p in (0, 1, 2, 0x10, 0x11, 0x20)] == [0, 2, 2, 0x11, 2, 0x11]
    assert [jr.storage_kind(np.float64, p) for p in (0, 1, 2, 0x10, 0x11, 0x20, 0x33)] == [0, 1, 2, 0x10, 0x11, 0x20, 0]
    sc = jr.storage_scheme(4)
    a = jr.apply_case("c128", 4, sc.group_size + 1, 1, fill=-777.25)
    st = jr.convert_groups(sc, sc.group_size + 1, a["blocks"], [0x01, 0x00])
    wide = jr.widen_storage(sc, sc.group_size + 1, st, [0x01, 0x00])
    go = sc.group_offset
    assert same_bits(wide[:go], a["blocks"][:go].astype(np.complex64).astype(np.complex128))
    assert same_bits(wide[go:], a["blocks"][go:])
    f = jr.apply_case("f32", 4, sc.group_size + 1, 1, fill=-777.25)
    st = jr.convert_groups(sc, sc.group_size + 1, f["blocks"], [0x10, 0x01])
    wide = jr.widen_storage(sc, sc.group_size + 1, st, [0x10, 0x01])
    assert same_bits(wide[:go], (f["blocks"][:go].view(np.uint32) & np.uint32(0xffff0000)).view(np.float32))
    assert same_bits(wide[go:], f["blocks"][go:].astype(np.float16).astype(np.float32))
