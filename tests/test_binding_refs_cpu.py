"""The numpy references of tests/binding_refs.py against independent formulations, so that a wrong
reference cannot pass a wrong kernel (no GPU needed)."""
import numpy as np
import pytest

import binding_refs as br


def _rand(rng, shape, t):
    v = rng.standard_normal(shape)
    return (v + 1j * rng.standard_normal(shape)).astype(t) if br.is_complex(t) else v.astype(t)


def _system(n=40, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, n))
    a += np.diag(np.abs(a).sum(axis=1) + 1)          # diagonally dominant, nonsymmetric
    return a, rng.uniform(-1, 1, n)


@pytest.mark.parametrize("tn", ["f64", "c128", "f32"])
@pytest.mark.parametrize("mode", ["hp", "plain"])
def test_initialize_orthonormalises(tn, mode):
    t = br.TYPES[tn]
    ar = getattr(br, mode)(t)
    rng = np.random.default_rng(1)
    p0 = _rand(rng, (4, 300), t)
    m, p, stop = br.idr_initialize(ar, p0, 4, 3)
    gram = p.astype(np.clongdouble) @ np.conj(p.astype(np.clongdouble)).T
    assert np.max(np.abs(gram - np.eye(4))) < 50 * (br.eps_of(t) if mode == "plain" else 1e-18)
    # Gram-Schmidt in row order: row r stays in the span of the first r + 1 input rows
    coef = np.linalg.lstsq(p0[:2].T.astype(np.complex128), p[1].astype(np.complex128), rcond=None)
    assert np.max(np.abs(p0[:2].T @ coef[0] - p[1])) < 1e-5
    assert not stop.any() and m.shape == (4, 12)
    for r in range(4):
        for c in range(4):
            assert np.all(m[r, c * 3:(c + 1) * 3] == (r == c))


@pytest.mark.parametrize("tn", ["f64", "c128"])
def test_step_1_solves_the_lower_system(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(2)
    s, nrhs, n, k = 5, 3, 17, 2
    m = _rand(rng, (s, s * nrhs), t)
    for j in range(s):
        m[j, j * nrhs:(j + 1) * nrhs] += 4
    f, res, g = _rand(rng, (s, nrhs), t), _rand(rng, (n, nrhs), t), _rand(rng, (n, s * nrhs), t)
    c, v = br.idr_step_1(br.hp(t), k, m, f, res, g, np.zeros((s, nrhs), t), np.zeros((n, nrhs), t))
    for i in range(nrhs):
        low = np.tril(m[:, i::nrhs])
        assert np.max(np.abs(low @ c[:, i].astype(np.complex128) - f[:, i])) < 1e-13
        want = res[:, i] - g[:, i::nrhs][:, k:] @ c[k:, i].astype(np.complex128)
        assert np.max(np.abs(v[:, i] - want)) < 1e-13


def test_stopped_columns_are_left_alone():
    t = np.float64
    rng = np.random.default_rng(3)
    d = br.idr_rounding_case(rng, t, 50, 2, 1, 3)
    stop = np.array([0, br.STOPPED, 0], np.uint8)
    out = br.idr_step_3(br.plain(t), 1, d["p"], d["g"], d["g_k"], d["u"], d["m"], d["f"], d["residual"], d["x"],
                        stop)
    for key in ("g", "u", "m"):
        assert np.array_equal(out[key][:, 1::3], d[key][:, 1::3])
    assert np.array_equal(out["x"][:, 1], d["x"][:, 1]) and not np.array_equal(out["x"][:, 0], d["x"][:, 0])


@pytest.mark.parametrize("s", [1, 4])
def test_idr_loop_solves(s):
    a, b = _system()
    rng = np.random.default_rng(4)
    p = rng.standard_normal((s, 40))
    x, iters = br.idr_solve(br.plain(np.float64), lambda v: a @ v, b, p, s, 1e-13, 400)
    want = np.linalg.solve(a, b)
    assert np.max(np.abs(x - want)) <= 1e-10 * np.max(np.abs(want)), iters
    assert iters < 400


def test_idr_loop_complex_rhs():
    a, b = _system()
    b = b + 1j * b[::-1]
    p = np.random.default_rng(4).standard_normal((4, 40))
    x, iters = br.idr_solve(br.plain(np.complex128), lambda v: a @ v, b, p, 4, 1e-13, 400)
    assert np.max(np.abs(x - np.linalg.solve(a, b))) <= 1e-10


@pytest.mark.parametrize("tn,kind", [("f64", br.KEEP), ("f64", br.F32), ("f64", br.I32), ("c128", br.KEEP)])
def test_cb_gmres_loop_solves(tn, kind):
    t = br.TYPES[tn]
    a, b = _system()
    if br.is_complex(t):
        b = b + 1j * b[::-1]
    x, iters, best = br.cb_gmres_solve(br.plain(t), t, kind, lambda v: a @ v, b, 15, 1e-13, 20)
    want = np.linalg.solve(a, b)
    assert np.max(np.abs(x - want)) <= 1e-10 * np.max(np.abs(want)), (iters, best)


@pytest.mark.parametrize("tn,kind", [("f64", br.KEEP), ("c128", br.KEEP), ("f64", br.F16), ("f64", br.I16),
                                     ("f32", br.KEEP)])
def test_arnoldi_relation_and_givens(tn, kind):
    """A V_m = V_{m+1} H with the un-rotated H (V = the decompressed basis; the defect is of the size of the
    storage quantum), the rotated columns are upper triangular, unrotate() inverts the rotations, and the
    residual norm estimate equals the true minimal residual for uncompressed storage"""
    t = br.TYPES[tn]
    ar = br.hp(t)
    a, b = _system()
    a = a.astype(ar.wt)
    if br.is_complex(t):
        b = b + 1j * b[::-1]
    kd = 8
    st = br.CbGmres(ar, t, kind, 40, 1, kd)
    nxt = st.restart(ar.a(b).reshape(-1, 1))
    v = [nxt[:, 0]]
    for it in range(kd):
        w = a @ st.basis(it, 0)
        nxt = st.arnoldi(it, w.reshape(-1, 1))
        v.append(nxt[:, 0])
    vm = np.stack([st.basis(k, 0) for k in range(kd + 1)], axis=1)
    hraw = np.zeros((kd + 1, kd), ar.wt)
    for it in range(kd):
        hraw[:it + 2, it] = st.hess_raw[it][:, 0]
        back = br.unrotate(st.hess[it][:, 0], st.gcos[:, 0], st.gsin[:, 0], it)
        assert np.max(np.abs(back - st.hess_raw[it][:, 0])) < 1e-17 * np.max(np.abs(hraw))
        assert st.hess[it][it + 1, 0] == 0
    q = br.quantum(kind, t, st.scalars[1:, 0].max())
    defect = np.max(np.abs(a @ vm[:, :kd] - vm @ hraw))
    assert defect <= 4 * q * np.max(np.abs(hraw)) * np.sqrt(40), (defect, q)
    if kind == br.KEEP:
        y, dx = st.solve_krylov()
        true = np.linalg.norm((ar.a(b) - a @ dx[:, 0]).astype(np.complex128))
        assert abs(true - float(st.residual_norm[0])) <= 1e3 * br.eps_of(t) * np.linalg.norm(b)
        assert abs(abs(st.gcos[3, 0]) ** 2 + abs(st.gsin[3, 0]) ** 2 - 1) < 1e-17


def test_half_emulation_all_bit_patterns():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = bits.view(np.float16)
    f = br.half_to_f32(h)
    back = br.f32_to_half(f).view(np.uint16)
    exp, man = bits & 0x7c00, bits & 0x3ff
    normal = (exp != 0) & (exp != 0x7c00)
    assert np.array_equal(back[normal], bits[normal])
    sub = exp == 0
    assert np.array_equal(back[sub], bits[sub] & 0x8000)          # subnormals and zeros: signed zero
    assert np.all(f[sub] == 0) and np.array_equal(np.signbit(f[sub]), (bits[sub] & 0x8000) != 0)
    inf = (exp == 0x7c00) & (man == 0)
    assert np.array_equal(back[inf], bits[inf])
    assert np.all(np.isnan(f[(exp == 0x7c00) & (man != 0)]))
    # float -> half on values between the representable ones: the astype-based form against the bit form
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(200000) * 10.0 ** rng.integers(-9, 6, 200000),
                        [0.0, -0.0, 2.0 ** -14, -2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), 0),
                         65504.0, 65519.9, 65520.0, 1e9, -1e9, 2.0 ** -15, 2.0 ** -24, 1.0 + 2.0 ** -11,
                         1.0 + 3 * 2.0 ** -11, np.inf, -np.inf]]).astype(np.float32)
    assert np.array_equal(br.f32_to_half(x).view(np.uint16), br.f32_to_half_bits_by_hand(x))


@pytest.mark.parametrize("kind", [br.I64, br.I32, br.I16])
def test_integer_storage_truncates(kind):
    v = np.array([0.999, -0.999, 0.5, -0.25, 1.0, 0.0], np.float64)
    scal = np.float64(1.0 * br.correction(kind))
    st = br.store(kind, np.float64, v, scal)
    back = br.load(kind, st, np.float64, scal)
    assert np.all(np.abs(back) <= np.abs(v)) and np.max(np.abs(back - v)) <= scal
    assert st.dtype == br.storage_dtype(kind, np.float64) and st[4] == np.iinfo(st.dtype).max // 2 + (kind == br.I64)


@pytest.mark.parametrize("tn", ["f64", "f32", "c128", "c64"])
def test_gemm_small_integers(tn):
    t = br.TYPES[tn]
    rng = np.random.default_rng(7)

    def ints(shape):
        v = rng.integers(-3, 4, shape)
        return (v + 1j * rng.integers(-3, 4, shape)).astype(t) if br.is_complex(t) else v.astype(t)
    a, b, c = ints((17, 33)), ints((33, 5)), ints((17, 5))
    for ar in (br.hp(t), br.plain(t)):
        assert np.array_equal(br.gemm(ar, a, b), (a @ b).astype(ar.wt))
        assert np.array_equal(br.gemm(ar, a, b, c, 2, -3), (2 * (a @ b) - 3 * c).astype(ar.wt))
        nan_c = np.full_like(c, np.nan)
        assert np.array_equal(br.gemm(ar, a, b, nan_c, 2, 0), (2 * (a @ b)).astype(ar.wt))
    assert np.array_equal(br.gemm(br.plain(t), a[:, :0], b[:0], c, 2, -3), -3 * c)


def test_gemm_plain_is_left_to_right():
    a = np.array([[1.0, 2.0 ** -30, -1.0]], np.float32)
    b = np.ones((3, 1), np.float32)
    assert br.gemm(br.plain(np.float32), a, b)[0, 0] == 0.0          # (1 + 2^-30) rounds to 1 first
    assert br.gemm(br.hp(np.float32), a, b)[0, 0] == np.longdouble(2.0) ** -30


@pytest.mark.parametrize("tn", ["f64", "f32", "c64"])
@pytest.mark.parametrize("n,s,k,nrhs", [(257, 2, 1, 3), (1025, 8, 7, 1), (5000, 4, 3, 3)])
def test_exact_case_is_exact_in_every_precision(tn, n, s, k, nrhs):
    """the integer-valued step_3 inputs: the long-double result (whose intermediates the reference checks to
    be integral) equals a float restatement with a different summation order"""
    t = br.TYPES[tn]
    case, ref, largest = br.idr_exact_step3_case(np.random.default_rng(n + k), t, n, s, k, nrhs)
    assert largest < 2 ** 24
    beta = case["f"][k] / ref["m"][k, k * nrhs:(k + 1) * nrhs]
    assert np.all(beta == 3)

    def pairwise(a, b):
        return (a * b).astype(t)[::-1].sum(dtype=t)             # numpy's blocked pairwise sum, reversed
    got = br.idr_step_3(br.Arith(np.dtype(t).type, pairwise, "tree"), k, **case)
    for key, want in ref.items():
        assert np.array_equal(got[key].astype(want.dtype), want), key


@pytest.mark.parametrize("tn", ["f64", "f32"])
def test_rounding_case_is_well_conditioned(tn):
    t = br.TYPES[tn]
    d = br.idr_rounding_case(np.random.default_rng(0), t, 1000, 4, 3, 3)
    diag = np.array([d["m"][j, j * 3:(j + 1) * 3] for j in range(4)])
    assert np.all(np.abs(diag) >= 0.5) and np.all(np.abs(diag) <= 2)
    gram = d["p"].astype(np.float64) @ d["p"].astype(np.float64).T
    assert np.max(np.abs(gram - np.eye(4))) < 20 * br.eps_of(t)
    args = [d[key] for key in ("p", "g", "g_k", "u", "m", "f", "residual", "x")]
    ref = br.idr_step_3(br.hp(t), 3, *args)
    pl = br.idr_step_3(br.plain(t), 3, *args)
    for key in ref:
        ok, ratio = br.rule_r(pl[key], ref[key], pl[key], t)
        assert ratio <= 35, (key, ratio)


def test_compute_omega_branches():
    ar = br.hp(np.float64)
    # |thr / (sqrt(tht) rn)| = 0.5 < 0.7: omega = thr / tht * 0.7 / 0.5; 0.9 >= 0.7: omega = thr / tht
    om = br.idr_compute_omega(ar, 0.7, [4.0, 4.0], [1.0, 1.0], [1.0, 1.8])
    assert abs(om[0] - 0.25 * 1.4) < 1e-18 and abs(om[1] - 0.45) < 1e-18
    om = br.idr_compute_omega(ar, 0.7, [4.0, 4.0], [1.0, 1.0], [1.0, 1.8], np.array([br.STOPPED, 0], np.uint8))
    assert om[0] == 1.0


def test_reorthogonalisation_case_has_teeth():
    """the nearly dependent next_krylov of the GPU test: with a single Gram-Schmidt round the result misses
    the orthogonality bound (rule R on the three-round plain restatement's own defect) by more than 100"""
    for t in (np.float64, np.float32):
        rows, nb = 1025, 6
        rng = np.random.default_rng(11)
        basis, nxt = br.reorth_case(rng, t, rows, nb)
        defects = {}
        for rounds in (3, 1):
            st = br.CbGmres(br.plain(t), t, br.KEEP, rows, 1, nb, rounds=rounds)
            st.bases[:nb, :, 0] = basis
            out = st.arnoldi(nb - 1, nxt.reshape(-1, 1))
            defects[rounds] = br.orth_defect(st, nb, 0)
            assert st.rounds_taken[0] == 1 if rounds == 1 else st.rounds_taken[0] >= 2
        bound = 4 * defects[3] + 8 * br.eps_of(t)
        assert defects[1] >= 100 * bound, (defects, bound)
        hpst = br.CbGmres(br.hp(t), t, br.KEEP, rows, 1, nb)
        hpst.bases[:nb, :, 0] = basis
        hpst.arnoldi(nb - 1, nxt.reshape(-1, 1))
        assert br.orth_defect(hpst, nb, 0) <= bound
