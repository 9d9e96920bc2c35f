"""tests/krylov_step_refs.py checked on its own, without a GPU: the plain restatement in f64 / f32 against the C
oracle bit for bit, the loop form against the array form, the complex restatement against the real one and against
numpy's own complex arithmetic in long double, the invariants of the MINRES rotation, the two square root formulas
against long double on the sweep of the GPU test, and the emulation of the fused kernels' tree sums against their
depth bound."""
import numpy as np
import pytest

import binding_refs as br
import gmres_refs as gr
import krylov_family_cases as kc
import krylov_step_refs as ks
from krylov_family_abi import KERNELS

ALL = [(s, k) for s, ks_ in KERNELS.items() for k in ks_]
EVERY = [(s, k) for s, ks_ in ks.ALL_ABI.items() for k in ks_]
TYPES = ("f64", "f32", "c128", "c64")


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "u":
        return np.array_equal(a, b)
    rt = br.real_of(a.dtype)
    ra, rb = a.reshape(-1).view(rt), b.reshape(-1).view(rt)
    both = np.isnan(ra) & np.isnan(rb)
    return np.array_equal(np.where(both, rt(0), ra).view(np.uint8), np.where(both, rt(0), rb).view(np.uint8))


@pytest.mark.parametrize("solver,kernel", ALL)
@pytest.mark.parametrize("rows,cols,dtype", [(597, 3, np.float64), (33, 5, np.float32), (7, 1, np.float64),
                                             (0, 2, np.float32)])
def test_plain_equals_oracle(oracle, solver, kernel, rows, cols, dtype):
    """every kernel of krylov_family_abi.KERNELS on krylov_family_cases.random_case inputs, with the zero_col /
    stopped_col variants of tests/test_krylov_family_gpu.py: the same bits as the C oracle"""
    for variant, (zero_col, stopped_col) in enumerate(((None, None), (0, 1), (1, 0), (0, None), (None, 2))):
        ref = kc.random_case(solver, kernel, rows, cols, dtype, 100 * rows + variant, zero_col, stopped_col)
        if kernel == "finalize":
            ref["stop_status"][:] = [kc.STOPPED, kc.FINAL, kc.RUN][variant % 3]
        mine = ks.apply(br.plain(dtype), solver, kernel, ref)
        if rows > 0:        # (the oracle's loops over rows write nothing without rows; the kernels' scalar
            #                  launches do, which the GPU test pins)
            oracle.krylov_step(f"{solver}_{kernel}", rows, cols, *ref.values())
            for name in ref:
                assert same_bits_or_nan(mine[name], ref[name]), (solver, kernel, name, variant)


@pytest.mark.parametrize("solver,kernel", EVERY)
@pytest.mark.parametrize("tn", TYPES)
def test_loop_form_equals_array_form(tn, solver, kernel):
    t = br.TYPES[tn]
    for rows in (3, 0):
        a, _ = ks.state_case(solver, kernel, tn, rows)
        arr, loop = ks.apply(br.plain(t), solver, kernel, a), ks.apply_by_element(br.plain(t), solver, kernel, a)
        for name in a:
            assert same_bits_or_nan(arr[name], loop[name]), (solver, kernel, name, rows)


@pytest.mark.parametrize("solver,kernel", EVERY)
@pytest.mark.parametrize("rt,ct", [("f64", "c128"), ("f32", "c64")])
def test_complex_with_zero_imaginary_parts_equals_real(rt, ct, solver, kernel):
    """all imaginary parts +0: the same values as the real restatement (signs of zeros are free: (-0) + (+0) i
    times a real is not the real product's zero)"""
    a, _ = ks.state_case(solver, kernel, rt, 9)
    c = {k: (v if k.startswith("_") else v.astype(br.TYPES[ct]) if v.dtype.kind == "f" and k != "Ap_norm" else v.copy())
         for k, v in a.items()}
    real, cplx = ks.apply(br.plain(br.TYPES[rt]), solver, kernel, a), ks.apply(br.plain(br.TYPES[ct]), solver, kernel, c)
    for name, v in real.items():
        w = cplx[name]
        if w.dtype.kind == "c":
            assert np.array_equal(w.real, v, equal_nan=True), (solver, kernel, name)
            assert np.all((w.imag == 0) | np.isnan(w.real)), (solver, kernel, name)
        else:
            assert np.array_equal(w, v), (solver, kernel, name)


@pytest.mark.parametrize("solver,kernel", EVERY)
@pytest.mark.parametrize("tn", ("c128", "c64"))
def test_complex_agrees_with_numpy_long_double(tn, solver, kernel):
    """well-scaled random input: the by-parts restatement and numpy's own clongdouble product / quotient / sqrt of
    the same formulas agree to a few eps.  A kernel chains at most six value operations on operands of modulus at
    most 16 (|rho / prev_rho * alpha / omega| <= 16), each within 2 sqrt(2) eps: 64 eps of the largest entry"""
    t = br.TYPES[tn]
    a = ks.random_case(solver, kernel, tn, 11, 4, outputs_nan=False)
    pl, ref = ks.apply(br.plain(t), solver, kernel, a), ks.apply(br.hp(t), solver, kernel, a)
    for name, v in ref.items():
        if v.dtype.kind not in "fc" or v.size == 0:
            assert np.array_equal(pl[name], v)
            continue
        err = np.max(np.abs(pl[name].astype(v.dtype) - v))
        assert err <= 64 * br.eps_of(t) * max(float(np.max(np.abs(v))), 1.0), (solver, kernel, name, float(err))


@pytest.mark.parametrize("tn", TYPES)
def test_minres_rotation_invariants(tn):
    """step_1 repeated over 20 steps from initialize: |c|^2 + |s|^2 = 1 within 8 eps, the new alpha is the
    hypotenuse of (a, sqrt(beta)) to rounding, eta_next = -conj(s) eta"""
    t = br.TYPES[tn]
    eps, cols = br.eps_of(t), 6
    rng = np.random.default_rng([23, TYPES.index(tn)])
    a = ks.random_case("minres", "initialize", tn, 5, cols)
    st = ks.apply(br.plain(t), "minres", "initialize", a)
    state = {k: st[k] for k in ks._MINRES_1 if k in st}
    state.update(stop_status=np.zeros(cols, np.uint8), tau=gr.rand(rng, (cols,), t))
    wide = np.clongdouble if br.is_complex(t) else np.longdouble
    for step in range(20):
        fresh = ks.random_case("minres", "step_1", tn, 0, cols, seed=step)
        state["alpha"], state["beta"] = fresh["alpha"], fresh["beta"]
        new = ks.apply(br.plain(t), "minres", "step_1", state)
        c, s = new["cos"].astype(wide), new["sin"].astype(wide)
        assert np.all(np.abs(np.abs(c) ** 2 + np.abs(s) ** 2 - 1) <= 8 * eps), (tn, step)
        o = {k: np.asarray(v).astype(wide) for k, v in state.items() if k != "stop_status"}
        bt = ks.sqrt_hp(state["beta"]) if br.is_complex(t) else np.sqrt(o["beta"])
        t1, t2 = -np.conj(o["sin"]) * o["cos_prev"] * o["gamma"], o["cos"] * o["alpha"]
        hyp = np.sqrt(np.abs(t1 + t2) ** 2 + np.abs(bt) ** 2)
        scale = np.abs(t1) + np.abs(t2) + np.abs(bt)
        assert np.all(np.abs(new["alpha"].astype(wide) - hyp) <= 16 * eps * scale), (tn, step)
        assert np.all(np.abs(new["alpha"].imag) <= 16 * eps * scale), (tn, step)
        want = -np.conj(s) * o["eta_next"]
        assert np.all(np.abs(new["eta_next"].astype(wide) - want) <= 4 * eps * np.abs(o["eta_next"])), (tn, step)
        assert same_bits_or_nan(new["eta"], state["eta_next"])
        state = new


def _sqrt_errors(tn, form):
    """|form(z) - hp| / (eps |hp|) over the sweep"""
    t = br.TYPES[tn]
    pts = ks.sqrt_sweep(tn)
    a, b = form(pts, br.real_of(t))
    ref = ks.sqrt_hp(pts)
    got = a.astype(np.longdouble) + 1j * b.astype(np.longdouble)
    return np.abs(got - ref) / (br.eps_of(t) * np.abs(ref)), pts


@pytest.mark.parametrize("tn", ("c128", "c64"))
def test_square_root_forms_on_the_sweep(tn):
    """the stable form stays within 4 eps |hp| (derived: under 2 eps); the formula the kernels had fails that"""
    ref = ks.sqrt_hp(ks.sqrt_sweep(tn))
    back = ref * ref - ks.sqrt_sweep(tn).astype(np.clongdouble)
    assert np.all(np.abs(back) <= 8 * np.finfo(np.longdouble).eps * np.abs(ref) ** 2), "the long-double root is off"
    stable, _ = _sqrt_errors(tn, ks.csqrt_stable)
    old, pts = _sqrt_errors(tn, ks.csqrt_cancelling)
    worst = int(np.argmax(old))
    print(f"sqrt | {tn} | stable form: largest error {float(stable.max()):.3f} eps; cancelling form: "
          f"{float(old.max()):.3g} eps at {pts[worst]!r}")
    assert stable.max() <= 4
    assert old.max() > 4


@pytest.mark.parametrize("tn", ("f64", "f32"))
@pytest.mark.parametrize("two", (False, True))
def test_x_dots_tree_bound(tn, two):
    """the emulation of the three tree sums in the value type stays within (depth + 1) eps sum |terms| of the
    long-double sums on the inputs of the GPU test, with either pointer alignment; the bound is below one median
    term - so that one missing or doubled term cannot pass - except in f32 above X_SINGLE_TEETH_LIMIT rows,
    which therefore get an integer-valued case with exact equality"""
    t = br.TYPES[tn]
    eps = br.eps_of(t)
    for n in ks.X_ROWS + (ks.X_BIG[tn],):
        a = ks.x_case(tn, n, two)
        v = (ks.x_step_2_step_1 if two else ks.x_step_1)(br.plain(t), a)
        hp, sums = ks.x_dots_hp(v["r"], v["z"], v["w"])
        for vec_ok in (True, False):
            depth = ks.x_dots_depth(n, t, vec_ok)
            tree = ks.x_dots_tree(t, v["r"], v["z"], v["w"], vec_ok)
            bound = (depth + 1) * eps * sums
            assert np.all(np.abs(tree.astype(np.longdouble) - hp) <= bound), (tn, n, vec_ok)
            if n:
                median = float(np.median(np.abs(v["r"] * v["z"])))
                assert (float(bound[0]) < median) == (not ks.x_needs_exact(tn, n)), (tn, n, float(bound[0]), median)
        if ks.x_needs_exact(tn, n):
            a = ks.x_case(tn, n, two, exact=True)
            v = (ks.x_step_2_step_1 if two else ks.x_step_1)(br.plain(t), a)
            watch = br.Exact()
            hp, sums = ks.x_dots_hp(v["r"], v["z"], v["w"])
            watch.see(sums)
            assert np.array_equal(ks.x_dots_tree(t, v["r"], v["z"], v["w"]).astype(np.longdouble), hp)
