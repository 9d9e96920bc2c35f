"""LowerIsai / UpperIsai on the device against the numpy substitution of tests/isai_refs.py, and Ilu / Ic with
ISAI solvers.  Values are compared with np.array_equal: the kernel promises the reference's rounding."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import ginkgo_amd as g
import factorization_refs as fr
import isai_refs as ir
from test_factorization_gpu import (TYPES, TYPE_IDS, criteria, csr_arrays, device_csr, model_problem,  # noqa: F401
                                    shuffled, solve_with, strided)

pytestmark = pytest.mark.gpu

SIDES = ["lower", "upper"]
POWERS = {"one": (1,), "diagonal": (1,), "chain": (1, 2, 3), "stencil": (1, 2, 3), "random": (1,), "small": (1, 2)}
CASES = [(name, p) for name in ("one", "diagonal", "chain", "stencil", "random") for p in POWERS[name]]


# ------------------------------------------------------------------ helpers
def cls_of(side):
    return g.LowerIsai if side == "lower" else g.UpperIsai


def generate(gexec, side, a, **params):
    f = cls_of(side).build()
    for k, val in params.items():
        f = getattr(f, "with_" + k)(val)
    return f.on(gexec).generate(a)


_MATRICES, _REFS = {}, {}   # computed once per key; the tests copy what they change


def case_arrays(name, side, dtype):
    """(rp, ci, v), int32 indices, of the triangular matrix of a case"""
    key = (name, side, dtype)
    if key not in _MATRICES:
        rng = np.random.default_rng(len(name) * 7 + 1)
        if name == "one":
            a = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0], dtype))
        elif name == "diagonal":
            a = (np.arange(301, dtype=np.int32), np.arange(300, dtype=np.int32), rng.uniform(1, 2, 300).astype(dtype))
        elif name == "chain":
            a = ir.lower_from_pattern(fr.chain_pattern(2500), rng, dtype)
        elif name == "random":
            a = ir.lower_from_pattern(fr.random_pattern(4000, rng), rng, dtype)
        elif name == "small":
            a = ir.lower_from_pattern(fr.random_pattern(300, rng, 3), rng, dtype)
        elif name.startswith("hub"):
            a = ir.hub_lower(int(name[3:]), rng, dtype)
        elif name == "stencil":
            # the IC(0) factor L (lower), the ILU(0) factor U (upper) of the 27-point stencil on 12^3 points
            full = fr.arrays(fr.stencil27(12), np.int32, dtype)
            a = fr.ic_factor(*full) if side == "lower" else fr.ilu_factors(*full)[3:]
        else:
            raise KeyError(name)
        if side == "upper" and name.startswith("hub"):
            a = ir.flipped(*a)          # the hub stays a ROW
        elif side == "upper" and name != "stencil":
            a = ir.transposed(*a)
        _MATRICES[key] = a
    return _MATRICES[key]


def reference(name, side, dtype, power):
    """(w_rp, w_ci, w_v) of the reference, int32 indices"""
    key = (name, side, dtype, power)
    if key not in _REFS:
        rp, ci, v = case_arrays(name, side, dtype)
        w_rp, w_ci = ir.pattern_power(rp, ci, power)
        w_v = ir.tri_inverse(rp, ci, v, w_rp, w_ci, side == "lower")
        for x in (w_rp, w_ci, w_v):
            x.setflags(write=False)
        _REFS[key] = (w_rp, w_ci, w_v)
    return _REFS[key]


def check_case(gexec, name, side, dtype, itype, power):
    rp, ci, v = case_arrays(name, side, dtype)
    rp, ci = rp.astype(itype), ci.astype(itype)
    dev = device_csr(gexec, rp, ci, v)
    m = generate(gexec, side, dev, sparsity_power=power)
    for got, kept in zip(csr_arrays(dev), (rp, ci, v)):
        assert np.array_equal(got, kept), "generate changed the caller's matrix"
    w_rp, w_ci, w_v = reference(name, side, dtype, power)
    assert np.isfinite(w_v).all()
    inv = m.get_approximate_inverse()
    assert isinstance(inv, g.Csr) and inv.size == dev.size and m.get_size() == dev.size
    got = csr_arrays(inv)
    assert got[0].dtype == got[1].dtype == itype and got[2].dtype == dtype
    # the pattern is scipy's pattern of |A|^p, sorted
    assert np.array_equal(got[0], w_rp) and np.array_equal(got[1], w_ci)
    if power == 1:
        assert np.array_equal(got[1], ci)
        assert inv.row_ptrs.data_ptr() == dev.row_ptrs.data_ptr() and inv.col_idxs.data_ptr() == dev.col_idxs.data_ptr()
    assert np.array_equal(got[2], w_v)
    return m


# ------------------------------------------------------------------ values and pattern, bit for bit
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name,power", CASES, ids=["%s-p%d" % c for c in CASES])
@pytest.mark.parametrize("side", SIDES)
def test_inverse_matches_reference(gexec, side, name, power, dtype, itype):
    check_case(gexec, name, side, dtype, itype, power)
    if name == "stencil":
        longest = int(np.diff(reference(name, side, dtype, power)[0]).max())
        assert longest == {1: 14, 2: 56, 3: 144}[power]


def boundary_lengths():
    limits = g.isai.row_limits()
    assert 1 <= len(limits) <= 4 and limits == sorted(set(limits)) and limits[0] >= 8
    # the first and the last length of every path, and rows streamed in two, three and four rounds
    return sorted({x for limit in limits for x in (limit, limit + 1)} | {65, 129, 200})


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("side", SIDES)
def test_hub_rows_at_every_path_boundary(gexec, side, dtype, itype):
    """the kernel picks its path from the LONGEST pattern row, so every length gets a matrix of its own in
    which one hub row has exactly that many entries and no other more than 3"""
    lengths = boundary_lengths()
    assert {65, 129, 200} <= set(lengths) and len(lengths) >= 5
    for length in lengths:
        name = "hub%d" % length
        stored = np.diff(case_arrays(name, side, dtype)[0])
        assert stored.max() == length and np.sort(stored)[-2] <= 3
        check_case(gexec, name, side, dtype, itype, 1)


# ------------------------------------------------------------------ input handling
@pytest.mark.parametrize("side", SIDES)
def test_unsorted_input_is_sorted_unless_told_not_to(gexec, side):
    rp, ci, v = case_arrays("small", side, np.float64)
    want = reference("small", side, np.float64, 2)
    ci_u, v_u = shuffled(rp, ci, v, np.random.default_rng(8))
    assert not np.array_equal(ci_u, ci)
    dev = device_csr(gexec, rp, ci_u, v_u)
    for power in (1, 2):
        want = reference("small", side, np.float64, power)
        got = csr_arrays(generate(gexec, side, dev, sparsity_power=power).get_approximate_inverse())
        assert all(np.array_equal(p, q) for p, q in zip(got, want))
        assert np.array_equal(dev.col_idxs.cpu().numpy(), ci_u) and np.array_equal(dev.values.cpu().numpy(), v_u), \
            "generate changed the caller's matrix"
    # sorted input and skip_sorting: the same inverse
    got = csr_arrays(generate(gexec, side, device_csr(gexec, rp, ci, v), sparsity_power=2,
                              skip_sorting=True).get_approximate_inverse())
    assert all(np.array_equal(p, q) for p, q in zip(got, want))
    # unsorted input and skip_sorting: nothing was sorted, so the diagonal is not where the entry needs it
    with pytest.raises(g.GkoError):
        generate(gexec, side, dev, skip_sorting=True)


def test_an_fbcsr_input(gexec):
    rng = np.random.default_rng(12)
    blocks = sp.tril(sp.random(40, 40, 0.1, random_state=rng, format="csr"), -1) + sp.eye(40)
    a = sp.kron(blocks, np.ones((3, 3)), format="csr")
    a.data = rng.uniform(0.1, 1, a.nnz)
    full = (a + sp.diags(np.full(120, 40.0))).tocsr()
    for side in SIDES:
        # block triangular with full 3 x 3 blocks on the diagonal is not triangular: the ABI's refusal
        # surfaces as the package's exception
        fb = g.Fbcsr.from_scipy(gexec, sp.bsr_matrix(full if side == "lower" else full.T.tocsr(), blocksize=(3, 3)))
        with pytest.raises(g.GkoError):
            generate(gexec, side, fb)
    # 1 x 1 blocks carry any triangular matrix
    rp, ci, v = case_arrays("small", "lower", np.float64)
    tri = sp.csr_matrix((v, ci, rp), shape=(300, 300))
    for side in SIDES:
        t = tri if side == "lower" else tri.T.tocsr()
        fb = g.Fbcsr.from_scipy(gexec, sp.bsr_matrix(t, blocksize=(1, 1)))
        m1, m2 = generate(gexec, side, fb, sparsity_power=2), generate(gexec, side, fb.convert_to_csr(), sparsity_power=2)
        for p, q, r in zip(csr_arrays(m1.get_approximate_inverse()), csr_arrays(m2.get_approximate_inverse()),
                           reference("small", side, np.float64, 2)):
            assert p.size and np.array_equal(p, q) and np.array_equal(p, r)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("side", SIDES)
def test_a_zero_diagonal_gives_the_reference_identity_rows(gexec, side, dtype, itype):
    rp, ci, v = case_arrays("small", side, dtype)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    v = v.copy()
    v[(rows == ci) & np.isin(rows, (40, 41, 250))] = 0
    for power in (1, 2):
        w_rp, w_ci = ir.pattern_power(rp, ci, power)
        want = ir.tri_inverse(rp, ci, v, w_rp, w_ci, side == "lower")
        w_rows = np.repeat(np.arange(len(rp) - 1), np.diff(w_rp))
        identity = [i for i in range(len(rp) - 1)
                    if np.array_equal(want[w_rows == i], (w_ci[w_rows == i] == i).astype(dtype))]
        assert {40, 41, 250} <= set(identity) and np.isfinite(want).all()
        m = generate(gexec, side, device_csr(gexec, rp.astype(itype), ci.astype(itype), v), sparsity_power=power)
        assert np.array_equal(csr_arrays(m.get_approximate_inverse())[2], want)
    # the call succeeded; the next generate on this executor is right
    check_case(gexec, "small", side, dtype, itype, 2)


def test_invalid_arguments_are_refused_and_the_device_stays_usable(gexec):
    from ginkgo_amd._lib import call
    st = gexec.stream
    rp, ci, v = (x.copy() for x in case_arrays("small", "lower", np.float64))
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    w_rp, w_ci, w_want = reference("small", "lower", np.float64, 2)

    def dev(*arrays):
        return [gexec.to_device(np.array(x)) for x in arrays]

    def without(rp_, ci_, row, col):
        """the index arrays without the entry (row, col)"""
        rows_ = np.repeat(np.arange(n), np.diff(rp_))
        keep = ~((rows_ == row) & (ci_ == col))
        assert keep.sum() == len(ci_) - 1
        out = np.zeros_like(rp_)
        out[1:] = np.cumsum(np.bincount(rows_[keep], minlength=n))
        return out, ci_[keep], keep

    a = dev(rp, ci, v)
    pattern = dev(w_rp, w_ci)
    up = dev(*ir.transposed(rp, ci, v))
    rp_m, ci_m, keep = without(rp, ci, 57, 57)
    a_missing = dev(rp_m, ci_m, v[keep])
    p_missing = dev(*without(w_rp, w_ci, 57, 57)[:2])
    ci_out = ci.copy()
    ci_out[rp[100]] = n
    ci_neg = ci.copy()
    ci_neg[rp[100]] = -1
    rp_bad = rp.copy()
    assert rp[11] > rp[10]
    rp_bad[10], rp_bad[11] = rp[11], rp[10]
    rp_first = rp.copy()
    rp_first[0] = 1
    extra = sp.csr_matrix((v, ci, rp), shape=(n, n)).tolil()
    extra[57, 58] = 0.25
    a_extra = dev(*fr.arrays(extra.tocsr()))
    w = gexec.to_device(np.full(len(w_ci), 9.0))
    w_own = gexec.to_device(np.full(len(ci), 9.0))
    bad = [("A on the wrong side", 0, a, pattern),
           ("A on the wrong side", 1, up, pattern),
           ("the pattern on the wrong side", 0, up, pattern),
           ("an entry right of the diagonal", 1, a_extra, pattern),
           ("a missing diagonal in A", 1, a_missing, pattern),
           ("a pattern row without its diagonal", 1, a, p_missing),
           ("a column out of range in A", 1, dev(rp, ci_out, v), pattern),
           ("a negative column in the pattern", 1, a, dev(rp, ci_neg)),
           ("row pointers that descend", 1, dev(rp_bad, ci, v), pattern),
           ("row pointers that start at 1", 1, a, dev(rp_first, ci)),
           ("a negative size", 1, a, pattern)]
    for what, is_lower, a_, p_ in bad:
        out = w if p_ is pattern or p_ is p_missing else w_own
        n_ = -1 if what == "a negative size" else n
        with pytest.raises(g.GkoError):
            call("gkoc_isai_generate_tri_inverse_f64_i32", st, n_, C.c_int(is_lower), *a_, *p_, out)
        assert (out.cpu().numpy() == 9.0).all(), what + ": w_v was written before the refusal"
    for k in range(6):
        args = a + pattern + [w]
        args[k] = None
        with pytest.raises(g.GkoError):
            call("gkoc_isai_generate_tri_inverse_f64_i32", st, n, C.c_int(1), *args)
    assert (w.cpu().numpy() == 9.0).all()
    # nothing of the above reached the values or the device: valid calls on the same arrays are right
    call("gkoc_isai_generate_tri_inverse_f64_i32", st, n, C.c_int(1), *a, *pattern, w)
    assert np.array_equal(w.cpu().numpy(), w_want)
    call("gkoc_isai_generate_tri_inverse_f64_i32", st, n, C.c_int(1), *a, a[0], a[1], w_own)
    assert np.array_equal(w_own.cpu().numpy(), reference("small", "lower", np.float64, 1)[2])
    call("gkoc_isai_generate_tri_inverse_f64_i32", st, 0, C.c_int(1), None, None, None, None, None, None)
    # the classes refuse what Ginkgo's refuse
    good = device_csr(gexec, rp, ci, v)
    for cls in (g.LowerIsai, g.UpperIsai):
        for power in (0, -1):
            with pytest.raises(g.GkoError):
                cls.build().with_sparsity_power(power).on(gexec).generate(good)
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(g.Dense.create(gexec, (4, 4)))
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(good.convert_to_ell())
        wide = g.Csr.from_arrays(gexec, (2, 3), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.ones(2))
        with pytest.raises(g.DimensionMismatch):
            cls.build().on(gexec).generate(wide)
        cplx = g.Csr.from_arrays(gexec, (2, 2), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32),
                                 np.ones(2, np.complex128))
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(cplx)
    # a lower matrix is no input of UpperIsai
    with pytest.raises(g.GkoError):
        g.UpperIsai.build().on(gexec).generate(good)
    check_case(gexec, "small", "lower", np.float64, np.int32, 2)


# ------------------------------------------------------------------ apply and transpose
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("side", SIDES)
def test_apply_is_the_csr_apply_of_the_reference_inverse(gexec, side, dtype, itype):
    m = check_case(gexec, "small", side, dtype, itype, 2)
    w_rp, w_ci, w_v = reference("small", side, dtype, 2)
    n = len(w_rp) - 1
    ref = g.Csr.from_arrays(gexec, (n, n), w_rp.astype(itype), w_ci.astype(itype), w_v.copy())
    alpha = g.Dense.from_numpy(gexec, np.array([[-1.5]], dtype))
    beta = g.Dense.from_numpy(gexec, np.array([[0.75]], dtype))
    t = m.transpose()
    assert type(t) is cls_of("upper" if side == "lower" else "lower") and isinstance(t, g.base.LinOp)
    assert t.get_size() == m.get_size()
    for got, want in zip(csr_arrays(t.get_approximate_inverse()), ir.transposed(w_rp, w_ci, w_v)):
        assert np.array_equal(got, want)
    ref_t = g.Csr.from_arrays(gexec, (n, n), *(x.astype(itype) if x.dtype.kind == "i" else x
                                               for x in ir.transposed(w_rp, w_ci, w_v)))
    for op, ref_op in ((m, ref), (t, ref_t)):
        for nrhs in (1, 3):
            b = np.random.default_rng(nrhs).uniform(-1, 1, (n, nrhs)).astype(dtype)
            x0 = np.random.default_rng(5).uniform(-1, 1, (n, nrhs)).astype(dtype)
            bd, _ = strided(gexec, b, nrhs + 3, fill=7.0)
            out = []
            for o in (op, ref_op):
                xd, store = strided(gexec, np.full_like(b, np.nan), nrhs + 2, fill=np.nan)
                o.apply(bd, xd)
                full = store.cpu().numpy()
                assert np.isnan(full[:, nrhs:]).all(), "the apply wrote into the padding of x"
                yd, ystore = strided(gexec, x0, nrhs + 2, fill=np.nan)
                o.apply(alpha, bd, beta, yd)
                yfull = ystore.cpu().numpy()
                assert np.isnan(yfull[:, nrhs:]).all()
                out.append((full[:, :nrhs], yfull[:, :nrhs]))
            assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
            if op is m:
                # and the product is the product: against scipy, to rounding
                want = sp.csr_matrix((w_v.astype(np.float64), w_ci, w_rp), shape=(n, n)) @ b.astype(np.float64)
                bound = sp.csr_matrix((np.abs(w_v).astype(np.float64), w_ci, w_rp), shape=(n, n)) @ np.abs(b)
                assert np.abs(out[0][0] - want).max() <= 64 * np.finfo(dtype).eps * bound.max()


# ------------------------------------------------------------------ the preconditioners
def host_pcg(a, b, w, reduction=1e-10, max_iters=1000):
    """preconditioned CG with M^-1 = W^T W, x_0 = 0; stops, like the device solver, before the iteration in
    which ||r|| <= reduction * ||r_0|| is seen.  Returns (x, iterations)."""
    wt = w.T.tocsr()
    x = np.zeros_like(b)
    r = b.copy()
    z = wt @ (w @ r)
    p = z.copy()
    rho = r @ z
    stop = reduction * np.linalg.norm(r)
    its = 0
    while np.linalg.norm(r) > stop and its < max_iters:
        q = a @ p
        alpha = rho / (p @ q)
        x += alpha * p
        r -= alpha * q
        its += 1
        z = wt @ (w @ r)
        rho, rho_old = r @ z, rho
        p = z + (rho / rho_old) * p
    return x, its


def model_reference(a_host, power):
    """the reference W of the reference IC(0) factor of the model problem's matrix"""
    if a_host.shape == (12 ** 3,) * 2 and abs(a_host - fr.stencil27(12)).max() == 0:
        return reference("stencil", "lower", np.float64, power)      # shared with the cases above
    rp, ci, v = fr.ic_factor(*fr.arrays(a_host))
    w_rp, w_ci = ir.pattern_power(rp, ci, power)
    return w_rp, w_ci, ir.tri_inverse(rp, ci, v, w_rp, w_ci, True)


def test_cg_with_ic_and_isai_solvers(gexec, model_problem):
    a, a_host, b = model_problem
    jacobi, _ = solve_with(gexec, g.Cg, a, b, g.Jacobi.build().with_max_block_size(1))
    assert jacobi.has_converged
    its = {}
    for power in (1, 2, 3):
        def factory():
            return g.Ic.build().with_l_solver(g.LowerIsai.build().with_sparsity_power(power))
        s, x = solve_with(gexec, g.Cg, a, b, factory())
        assert s.has_converged and s.num_iterations < 1000, power
        assert np.linalg.norm(b - a_host @ x) <= 1e-9 * np.linalg.norm(b), power
        m = s.get_preconditioner()
        assert isinstance(m.get_l_solver(), g.LowerIsai) and isinstance(m.get_lh_solver(), g.UpperIsai)
        # the device's W is the reference's W of the reference's IC(0) factor
        w_rp, w_ci, w_v = model_reference(a_host, power)
        for got, want in zip(csr_arrays(m.get_l_solver().get_approximate_inverse()), (w_rp, w_ci, w_v)):
            assert np.array_equal(got, want)
        n = len(w_rp) - 1
        _, host_its = host_pcg(a_host, b, sp.csr_matrix((w_v, w_ci, w_rp), shape=(n, n)))
        print("power %d: CG iterations on the device %d, host PCG %d" % (power, s.num_iterations, host_its))
        assert abs(s.num_iterations - host_its) <= 2, power
        plain, xp = solve_with(gexec, g.Cg, a, b, factory(), hip_graph=False)
        assert plain.has_converged and plain.num_iterations == s.num_iterations, power
        its[power] = s.num_iterations
    print("CG iterations: scalar Jacobi %d, Ic + ISAI %s" % (jacobi.num_iterations, its))
    assert its[3] <= its[2] <= its[1] < jacobi.num_iterations


def test_gmres_and_bicgstab_with_ilu_and_isai_solvers(gexec, model_problem):
    a, a_host, b = model_problem
    rp, ci, v = csr_arrays(a)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    # the unsymmetric perturbation of test_other_solvers_and_generated_preconditioners
    v = np.where(rows == ci, v, v * np.random.default_rng(7).uniform(0.8, 1.0, v.size))
    u, u_host = g.Csr.from_arrays(gexec, (n, n), rp, ci, v), sp.csr_matrix((v, ci, rp), shape=(n, n))
    assert abs(u_host - u_host.T).max() > 0.01
    for cls in (g.Gmres, g.Bicgstab):
        for power in (1, 2):
            f = g.Ilu.build().with_l_solver(g.LowerIsai.build().with_sparsity_power(power)) \
                .with_u_solver(g.UpperIsai.build().with_sparsity_power(power))
            s, x = solve_with(gexec, cls, u, b, f)
            m = s.get_preconditioner()
            assert isinstance(m.get_l_solver(), g.LowerIsai) and isinstance(m.get_u_solver(), g.UpperIsai)
            assert s.has_converged and s.num_iterations < 1000, cls.__name__
            assert np.linalg.norm(b - u_host @ x) <= 1e-8 * np.linalg.norm(b), cls.__name__
            print("%s with Ilu + ISAI power %d: %d iterations" % (cls.__name__, power, s.num_iterations))


def test_ic_refuses_a_trs_solver_and_ilu_with_explicit_trs_is_the_default(gexec, model_problem):
    a, _, b = model_problem
    with pytest.raises(g.NotSupported, match="transpose"):
        g.Ic.build().with_l_solver(g.LowerTrs.build()).on(gexec).generate(a)
    default = g.Ilu.build().on(gexec).generate(a)
    explicit = g.Ilu.build().with_l_solver(g.LowerTrs.build()).with_u_solver(g.UpperTrs.build()).on(gexec).generate(a)
    assert isinstance(explicit.get_l_solver(), g.LowerTrs) and isinstance(explicit.get_u_solver(), g.UpperTrs)
    assert isinstance(default.get_l_solver(), g.LowerTrs) and isinstance(default.get_u_solver(), g.UpperTrs)
    out = []
    for m in (default, explicit):
        x = g.Dense.from_numpy(gexec, np.full_like(b, np.nan))
        m.apply(g.Dense.from_numpy(gexec, b), x)
        out.append(x.to_numpy())
    assert np.isfinite(out[0]).all() and np.array_equal(out[0], out[1])
    # the reverse order keeps working with given solvers
    rev = g.Ilu.build().with_reverse_apply(True).with_l_solver(g.LowerIsai.build()).on(gexec).generate(a)
    assert isinstance(rev.get_l_solver(), g.LowerIsai) and isinstance(rev.get_u_solver(), g.UpperTrs)
    x = g.Dense.from_numpy(gexec, np.full_like(b, np.nan))
    rev.apply(g.Dense.from_numpy(gexec, b), x)
    assert np.isfinite(x.to_numpy()).all()
