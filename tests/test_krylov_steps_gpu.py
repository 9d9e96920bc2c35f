"""The Krylov step kernels of csrc/krylov_steps.hip and the CG steps of csrc/cg_stop.hip through the C ABI, in all
four value types, at the smallest shapes that select each path of launch_elementwise (csrc/elementwise.hpp) and of
the per-column scalar kernels, against the numpy restatements of tests/krylov_step_refs.py (checked on their own
by tests/test_krylov_step_refs_cpu.py); and the two fused PipeCg kernels gkoc_x_pipe_cg_step_1_dots /
gkoc_x_pipe_cg_step_2_step_1_dots (f64, f32, gate = NULL).

Every vector operand is cut from a padded array whose padding, leading and trailing canaries must survive; output-
only operands start as NaN; every input is read back and compared bit for bit; every call runs twice from the same
inputs and must give the same bits.

Acceptance.  Every vector output, stored scalar, stop byte and final_iter_nums: bit-identical to the plain
restatement (complex types: the textbook product, Smith's quotient, == on both parts), where both give NaN its sign
and payload are free.  The only exceptions, in the complex types, are the outputs that pass through abs_v (device
hypot) or the complex sqrt: beta / eta / eta_next of minres_initialize, the scalars minres_step_1 computes, beta of
pipe_cg_step_2; they obey rule R against long double from the same state (binding_refs.rule_r), and what
minres_initialize derives from its beta (q, z) is bit-identical to the restatement started from the kernel's own
beta.  The square root itself: |got - hp| <= 4 eps |hp| on the sweep of krylov_step_refs.sqrt_sweep.  The fused
kernels: vectors bit-identical to the separate kernels and to the restatement; each of the three sums within
(depth + 1) eps sum |terms| of the long-double sum over the kernel's own vectors (krylov_step_refs.x_dots_depth)
and exactly equal on integer-valued inputs.

Every rule-R ratio and every fraction of a depth bound is printed by the case that observes it, before it is
asserted (pytest -s shows them)."""
import ctypes as C
import re

import numpy as np
import pytest

import binding_refs as br
import gmres_refs as gr
import krylov_step_refs as ks
from binding_gpu import CANARY, Dev, _C128, call, padded, same_bits, sync

pytestmark = pytest.mark.gpu

TYPES = ("f64", "f32", "c128", "c64")
EVERY = [(s, k) for s, kernels in ks.ALL_ABI.items() for k in kernels]
WITH_VECTORS = [sk for sk in EVERY if any(kind in "Vv" for _, kind in ks.ALL_ABI[sk[0]][sk[1]])]
# minres_step_1 in complex types: what does not pass through hypot or sqrt stays bit-identical all the same
STRICT_ANYWAY = {("minres", "step_1"): ("cos_prev", "sin_prev", "eta", "delta", "gamma")}


def _note(kind, what, tn, v):
    """one line per observed figure: "ratio" = |kernel - ref| / (eps max |ref|) of a rule-R output, "sqrt" =
    largest |got - hp| / (eps |hp|) of a sweep, "bound" = the fraction of a depth bound that a sum used"""
    print(f"{kind:5s} | {what} | {tn} | {float(v):.3f}")


class Vec:
    """a rows x cols operand with leading dimension ld, `shift` elements behind a 16-byte-aligned address, inside a
    device array that holds canaries in front of it, in its padding and behind it"""

    def __init__(self, gexec, a, ld=None, shift=0):
        a = np.asarray(a)
        self.rows, self.cols = a.shape
        self.ld, self.shift = self.cols if ld is None else ld, shift
        fill = np.full(3, CANARY, a.dtype)
        self.host = np.concatenate([np.full(shift, CANARY, a.dtype), padded(a, self.ld).reshape(-1), fill])
        self.dev = Dev(gexec, self.host)
        self.ptr = self.dev.at(shift)

    def get(self):
        full = self.dev.get()
        keep = np.ones(full.shape, bool)
        body = keep[self.shift:self.shift + self.rows * self.ld].reshape(self.rows, self.ld)
        body[:, :self.cols] = False
        assert same_bits(full[keep], self.host[keep]), "a canary around an operand was overwritten"
        inner = full[self.shift:self.shift + self.rows * self.ld].reshape(self.rows, self.ld)
        return np.ascontiguousarray(inner[:, :self.cols])

    def unchanged(self):
        return same_bits(self.dev.get(), self.host)


class Flat:
    """a flat device array followed by three canaries"""

    def __init__(self, gexec, a):
        a = np.ascontiguousarray(a).reshape(-1)
        self.n = a.shape[0]
        canary = {1: 0x5a, 8: 0x5a5a5a5a}[a.dtype.itemsize] if a.dtype.kind == "u" else CANARY
        self.host = np.concatenate([a, np.full(3, canary, a.dtype)])
        self.dev = Dev(gexec, self.host)
        self._as_parameter_ = self.dev._as_parameter_

    def get(self):
        full = self.dev.get()
        assert same_bits(full[self.n:], self.host[self.n:]), "written behind the end"
        return full[:self.n]

    def unchanged(self):
        return same_bits(self.dev.get(), self.host)


def same_bits_or_nan(a, b):
    """bit for bit, except that where both hold a NaN its sign and payload are free; parts of complex values one
    by one"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "u":
        return same_bits(a, b)
    rt = br.real_of(a.dtype)
    ra, rb = a.reshape(-1).view(rt), b.reshape(-1).view(rt)
    both = np.isnan(ra) & np.isnan(rb)
    return same_bits(np.where(both, rt(0), ra), np.where(both, rt(0), rb))


def _first_diff(got, ref):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    bad = np.flatnonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    if not bad.size:
        return "differs in the sign of a zero only"
    i = int(bad[0])
    return f"first wrong element {i} of {got.size}: {got[i]!r}, expected {ref[i]!r}"


def _coeff(v, cx):
    if not cx:
        return C.c_double(float(v))
    v = complex(v)
    return C.byref(_C128(v.real, v.imag))


def entry(solver, kernel, tn):
    return "gkoc_ir_initialize" if solver == "ir" else f"gkoc_{solver}_{kernel}_{tn}"


def run_kernel(gexec, tn, solver, kernel, a, lds=None, shifts=None):
    """one call on fresh device copies of the operands a (name -> tight array); returns what the device holds
    afterwards, name -> array, after checking the canaries and that the inputs kept their bits"""
    spec = ks.ALL_ABI[solver][kernel]
    vec = [n for n, k in spec if k in "Vv"]
    dims = list(np.asarray(a[vec[0]]).shape) if vec else [np.asarray(a[spec[0][0]]).shape[0]]
    dev, args = {}, []
    for name, kind in spec:
        if kind in "Vv":
            dev[name] = Vec(gexec, a[name], (lds or {}).get(name), (shifts or {}).get(name, 0))
            args += [dev[name].ptr, dev[name].ld]
        else:
            dev[name] = Flat(gexec, a[name])
            args.append(dev[name])
    coeffs = []
    if solver == "chebyshev":
        cx = br.is_complex(br.TYPES[tn])
        coeffs = [_coeff(a["_alpha"], cx)] + ([_coeff(a["_beta"], cx)] if kernel == "update" else [])
    call(entry(solver, kernel, tn), gexec.stream, *dims, *coeffs, *args)
    sync()
    out = {}
    for name, kind in spec:
        out[name] = dev[name].get()
        if kind in "VSTP":
            assert dev[name].unchanged(), (solver, kernel, name, "an input was written")
    return out


def rule_r(got, ref, plain_v, t, what, tn):
    """rule R over the entries where the reference is finite; elsewhere (the NaN a stopped column keeps) the kernel
    must hold a non-finite value as well"""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (what, "finite entries differ")
    ok, ratio = br.rule_r(got[fin], ref[fin], plain_v[fin], t)
    _note("ratio", what, tn, ratio)
    assert ok, (what, ratio)
    return ratio


def check(gexec, tn, solver, kernel, a, lds=None, shifts=None):
    """two runs with the same bits; every operand compared with the plain restatement (rule R where it applies)"""
    t = br.TYPES[tn]
    got, again = (run_kernel(gexec, tn, solver, kernel, a, lds, shifts) for _ in range(2))
    for name in got:
        assert same_bits(got[name], again[name]), (solver, kernel, tn, name, "two runs differ")
    ops = {k: v for k, v in a.items()}
    ref = ks.apply(br.plain(t), solver, kernel, ops)
    key = (solver, kernel)
    loose = ks.RULE_R.get(key, ()) if br.is_complex(t) else ()
    if loose and key == ("minres", "initialize"):
        o = ks.Ops(br.plain(t))
        with np.errstate(all="ignore"):             # q and z: from the kernel's own beta, bit for bit
            ref["q"], ref["z"] = o.safe_div(a["r"], got["beta"]), o.safe_div(a["z"], got["beta"])
        assert same_bits(got["eta"], got["beta"]) and same_bits(got["eta_next"], got["beta"])
    shape = tuple(np.asarray(next(iter(got.values()))).shape)
    for name, _ in ks.ALL_ABI[solver][kernel]:
        if name not in loose or name in STRICT_ANYWAY.get(key, ()):
            assert same_bits_or_nan(got[name], ref[name]), (solver, kernel, tn, name, shape, lds, shifts,
                                                            _first_diff(got[name], ref[name]))
    if loose:
        hp = ks.apply(br.hp(t), solver, kernel, ops)
        for name in loose:
            rule_r(got[name], hp[name], ref[name], t, f"{solver}_{kernel} {name}", tn)
    return got


def release():
    """hand the device memory of a large case back, so that the tests that follow do not run next to it"""
    import torch
    torch.cuda.empty_cache()


def own_lds(solver, kernel, cols):
    """every operand with a leading dimension of its own: cols + 1 .. cols + 4"""
    vec = [n for n, k in ks.ALL_ABI[solver][kernel] if k in "Vv"]
    return {n: cols + 1 + i % 4 for i, n in enumerate(vec)}


def every(pairs, one):
    """one(solver, kernel) for each entry point of `pairs`.  A failed comparison of one entry point does not hide the
    others: all of them are reported together (any other error, a failed HIP call among them, ends the test at
    once)"""
    failed = []
    for solver, kernel in pairs:
        try:
            one(solver, kernel)
        except AssertionError as e:
            failed.append(f"{solver}_{kernel}: {str(e)[:600]}")
    assert not failed, f"{len(failed)} of {len(pairs)} entry points:\n" + "\n".join(failed)


# ------------------------------------------------------------------------------- paths of launch_elementwise
# (one test per value type; each walks over the entry points, which the failure message names)
@pytest.mark.parametrize("tn", TYPES)
def test_flat_path_vector_loop_and_tail(gexec, tn):
    """cols = 1, ld = 1, aligned: the flat path; rows below W = 16 / sizeof(T) leave its vector loop empty (thread
    0's scalar tail does all the work), 255 .. 257 and 2049 end a block, 100003 has several"""
    def one(solver, kernel):
        for rows in (0, 1, 2, 3, 5, 255, 256, 257, 2049, 100003):
            check(gexec, tn, solver, kernel, ks.random_case(solver, kernel, tn, rows, 1))
            if (solver, kernel) not in WITH_VECTORS:
                break               # no vectors: rows does not exist
    every(EVERY, one)


@pytest.mark.parametrize("tn", TYPES)
def test_general_path_by_stride(gexec, tn):
    """every operand with a leading dimension of its own"""
    def one(solver, kernel):
        for cols in (1, 2, 3, 5):
            for rows in (0, 1, 257, 2049):
                check(gexec, tn, solver, kernel, ks.random_case(solver, kernel, tn, rows, cols),
                      own_lds(solver, kernel, cols))
    every(WITH_VECTORS, one)


@pytest.mark.parametrize("tn", TYPES)
def test_general_path_by_alignment(gexec, tn):
    """cols = 1, ld = 1, rows 257: (a) all operands one element behind a 16-byte boundary, (b) only the first
    input, (c) only the last output, (d) none.  A flat candidate with one misaligned pointer falls back to the
    general kernel.  In c128 one element IS 16 bytes: the shift keeps the flat path there, and the result must be
    right all the same"""
    def one(solver, kernel):
        spec = ks.ALL_ABI[solver][kernel]
        vec = [n for n, k in spec if k in "Vv"]
        last_out = [n for n, k in spec if k == "v"][-1]
        a = ks.random_case(solver, kernel, tn, 257, 1)
        for shifts in ({n: 1 for n in vec}, {vec[0]: 1}, {last_out: 1}, {}):
            check(gexec, tn, solver, kernel, a, None, shifts)
    every(WITH_VECTORS, one)


@pytest.mark.parametrize("tn", TYPES)
def test_flat_path_with_several_columns(gexec, tn):
    """the uniform-scalar kernels take the flat path for cols > 1 when ld == cols: rows * 3 with every tail length;
    once with ld = cols + 1 (general path)"""
    def one(solver, kernel):
        for rows in (1, 3, 85, 683):
            check(gexec, tn, solver, kernel, ks.random_case(solver, kernel, tn, rows, 3))
        a = ks.random_case(solver, kernel, tn, 85, 3)
        check(gexec, tn, solver, kernel, a, {n: 4 for n, k in ks.ALL_ABI[solver][kernel] if k in "Vv"})
    every(ks.UNIFORM, one)


@pytest.mark.parametrize("tn", TYPES)
def test_per_column_states(gexec, tn):
    """one column per state (krylov_step_refs.state_case): running, stopped / converged with and without the
    finalized bit, every zero denominator, in complex types (0, 1) and (1, 0) and the underflowing prev_rho *
    omega.  Stored scalars: the restatement's value for running columns, the NaN they had for stopped ones"""
    every(EVERY, lambda solver, kernel: _states(gexec, tn, solver, kernel))


def _states(gexec, tn, solver, kernel):
    for rows in (5, 0):
        a, labels = ks.state_case(solver, kernel, tn, rows)
        cols = len(labels)
        got = check(gexec, tn, solver, kernel, a, own_lds(solver, kernel, cols))
        name = ks.STORED.get((solver, kernel))
        if name:
            for c, label in enumerate(labels):
                if label.startswith("stop") or rows == 0 and np.isnan(a[name][c].real):
                    assert np.isnan(got[name][c].real), (solver, kernel, name, label, "a skipped column's scalar")
                elif rows:
                    assert np.isfinite(got[name][c].real), (solver, kernel, name, label)


SCALAR_KERNELS = [sk for sk in EVERY if sk[1].startswith("initialize")] + \
    [("minres", "step_1"), ("bicgstab", "finalize"), ("gcr", "restart")]


@pytest.mark.parametrize("tn", TYPES)
def test_second_block_of_the_scalar_kernels(gexec, tn):
    """cols = 257: column 256 belongs to the second 256-thread block of the per-column kernels; without rows they
    still run (bicgstab_finalize does not: it leaves the stop status alone then)"""
    def one(solver, kernel):
        for rows in (3, 0):
            a = ks.random_case(solver, kernel, tn, rows, 257)
            if kernel == "finalize":
                a["stop_status"][:] = np.resize(np.array([ks.STOPPED, ks.RUN, ks.STOPPED_FINAL, ks.CONVERGED],
                                                         np.uint8), 257)
            check(gexec, tn, solver, kernel, a)
    every(SCALAR_KERNELS, one)


@pytest.mark.parametrize("solver,kernel", [("pipe_cg", "step_1"), ("bicgstab", "step_3"), ("minres", "step_2"),
                                           ("chebyshev", "update")])
@pytest.mark.parametrize("tn", ("f32", "c128"))
@pytest.mark.parametrize("path", ("flat", "general"))
def test_beyond_the_grid_caps(gexec, tn, solver, kernel, path):
    """flat: more than 2048 * 256 vectors (2 097 159 x 1 in f32, 524 545 x 1 in c128, both with a tail or an odd
    count); general: more than 8192 * 256 elements (699 137 x 3, ld = cols + 1).  Every element is compared"""
    if path == "flat":
        rows = {"f32": 2097159, "c128": 524545}[tn]
        assert rows // gr.vec_width(br.TYPES[tn]) > 2048 * 256
        check(gexec, tn, solver, kernel, ks.random_case(solver, kernel, tn, rows, 1))
    else:
        assert 699137 * 3 > 8192 * 256
        a = ks.random_case(solver, kernel, tn, 699137, 3)
        check(gexec, tn, solver, kernel, a, {n: 4 for n, k in ks.ALL_ABI[solver][kernel] if k in "Vv"})
    release()


# ----------------------------------------------------------------------------------------- the square root
def _sqrt_check(got, pts, tn, what):
    t = br.TYPES[tn]
    ref = ks.sqrt_hp(pts)
    err = np.abs(got.astype(np.clongdouble) - ref) / (br.eps_of(t) * np.abs(ref))
    worst = int(np.argmax(err))
    _note("sqrt", f"{what}: worst point {pts[worst]!r}", tn, err[worst])
    bad = np.flatnonzero(~(err <= 4))
    first = int(bad[0]) if bad.size else 0
    assert not bad.size, (what, tn, f"{bad.size} of {pts.size} points; first wrong element {first}: sqrt({pts[first]!r}) = "
                          f"{got[first]!r}, long double {complex(ref[first])!r}, error {float(err[first]):.3g} eps")


@pytest.mark.parametrize("tn", ("c128", "c64"))
def test_square_root_sweep_minres_initialize(gexec, tn):
    """beta = sqrt(<r, z>) of minres_initialize on the sweep, rows = 1, one column per point: within 4 eps |hp|
    (derived for the stable form: hypot within an ulp, one sum of non-negative terms, a halving, a square root and
    one quotient - under 2 eps normwise; the bound is twice that)"""
    pts = ks.sqrt_sweep(tn)
    a = ks.random_case("minres", "initialize", tn, 1, pts.size)
    a["beta"] = pts.copy()
    _sqrt_check(run_kernel(gexec, tn, "minres", "initialize", a)["beta"], pts, tn, "minres_initialize beta")
    check(gexec, tn, "minres", "initialize", a)


@pytest.mark.parametrize("tn", ("c128", "c64"))
def test_square_root_sweep_minres_step_1(gexec, tn):
    pts = ks.sqrt_sweep(tn)
    a = ks.random_case("minres", "step_1", tn, 0, pts.size)
    a["beta"] = pts.copy()
    _sqrt_check(run_kernel(gexec, tn, "minres", "step_1", a)["beta"], pts, tn, "minres_step_1 beta")
    check(gexec, tn, "minres", "step_1", a)


# ------------------------------------------------------------------------------------------ the fused kernels
X1 = ("x", "r", "z", "w", "p", "q", "f", "g")
X2 = X1 + ("m", "n")


def work_bytes(tn):
    return 3 * ks.X_MAX_BLOCKS * np.dtype(br.TYPES[tn]).itemsize


def run_x(gexec, tn, a, two, shifted=None, wbytes=None, alias_beta=False):
    """one call of a fused kernel; returns (vectors and scalars afterwards, out3)"""
    names = X2 if two else X1
    written = X1 if two else X1[:4]
    dev = {k: Vec(gexec, np.asarray(a[k]).reshape(-1, 1), 1, 1 if k == shifted else 0) for k in names}
    n = dev["x"].rows
    sc = {k: Flat(gexec, v) for k, v in a.items() if k not in names}
    out3 = Flat(gexec, np.full(3, np.nan, br.TYPES[tn]))
    work = Flat(gexec, np.zeros(work_bytes(tn), np.uint8))
    wb = C.c_size_t(work_bytes(tn) if wbytes is None else wbytes)
    vec = [dev[k].ptr for k in names]
    if two:
        beta_out = sc["beta_in"] if alias_beta else sc["beta_out"]
        call("gkoc_x_pipe_cg_step_2_step_1_dots_" + tn, gexec.stream, n, *vec, sc["prev_rho"], sc["rho"], sc["delta"],
             sc["beta_in"], beta_out, sc["stop_status"], out3, work, wb, None)
    else:
        call("gkoc_x_pipe_cg_step_1_dots_" + tn, gexec.stream, n, *vec, sc["rho"], sc["beta"], sc["stop_status"], out3,
             work, wb)
    sync()
    work.get()
    out = {k: dev[k].get().reshape(-1) for k in names}
    out.update({k: f.get() for k, f in sc.items()})
    for k in a:
        if k not in written and k != "beta_out":
            assert (dev[k] if k in dev else sc[k]).unchanged(), (k, "an input was written")
    return out, out3.get()


def check_x(gexec, tn, a, two, shifted=None, exact=False, what=""):
    t = br.TYPES[tn]
    (got, out3), (again, out3b) = (run_x(gexec, tn, a, two, shifted) for _ in range(2))
    assert all(same_bits(got[k], again[k]) for k in got) and same_bits(out3, out3b), "two runs differ"
    ref = (ks.x_step_2_step_1 if two else ks.x_step_1)(br.plain(t), a)
    for k, v in ref.items():
        assert same_bits_or_nan(got[k], v), (what, tn, k, _first_diff(got[k], v))
    n = a["x"].shape[0]
    if n == 0:
        assert same_bits(out3, np.zeros(3, t)), "out3 of an empty call is +0"
        return got, out3
    # the separate kernels on copies of the same input
    col = {k: np.asarray(v).reshape(-1, 1) if k in X2 else v for k, v in a.items()}
    if two:
        col["beta"] = col["beta_in"]
        s2 = run_kernel(gexec, tn, "pipe_cg", "step_2", {k: col[k] for k, _ in ks.ALL_ABI["pipe_cg"]["step_2"]})
        col.update({k: s2[k] for k in ("p", "q", "f", "g", "beta")})
        assert same_bits_or_nan(got["beta_out"], s2["beta"])
        for k in ("p", "q", "f", "g"):
            assert same_bits(got[k], s2[k].reshape(-1)), (what, tn, k, "differs from pipe_cg_step_2")
    col["z1"], col["z2"] = col["z"], np.full_like(col["z"], np.nan)
    s1 = run_kernel(gexec, tn, "pipe_cg", "step_1", {k: col[k] for k, _ in ks.ALL_ABI["pipe_cg"]["step_1"]})
    for k, k1 in (("x", "x"), ("r", "r"), ("z", "z1"), ("w", "w")):
        assert same_bits(got[k], s1[k1].reshape(-1)), (what, tn, k, "differs from pipe_cg_step_1")
    # the three sums over the kernel's own vectors
    hp, sums = ks.x_dots_hp(got["r"], got["z"], got["w"])
    if exact:
        br.Exact().see(sums)
        assert np.array_equal(out3.astype(np.longdouble), hp), (what, tn, out3, hp)
        return got, out3
    depth = ks.x_dots_depth(n, t, shifted is None)
    bound = (depth + 1) * br.eps_of(t) * sums
    err = np.abs(out3.astype(np.longdouble) - hp)
    _note("bound", f"{what} n = {n} depth {depth}", tn, np.max(err / bound))
    assert np.all(err <= bound), (what, tn, n, out3, hp)
    return got, out3


@pytest.mark.parametrize("two", (False, True), ids=("step_1_dots", "step_2_step_1_dots"))
@pytest.mark.parametrize("tn", ("f64", "f32"))
def test_fused_shapes(gexec, tn, two):
    """n = 0 (out3 = +0, nothing else touched) .. 100003, all operands aligned, and one operand one element behind
    a 16-byte boundary so that the scalar loop does all the work"""
    for n in ks.X_ROWS:
        a = ks.x_case(tn, n, two)
        check_x(gexec, tn, a, two, what="aligned")
        if n:
            names = X2 if two else X1
            check_x(gexec, tn, a, two, shifted=names[n % len(names)], what="shifted")


@pytest.mark.parametrize("two", (False, True), ids=("step_1_dots", "step_2_step_1_dots"))
@pytest.mark.parametrize("tn", ("f64", "f32"))
def test_fused_above_the_block_cap(gexec, tn, two):
    """more than 1024 blocks' worth of rows: the grid-stride loop makes a second trip.  In f32 the depth bound is
    wider than one term there (tests/test_krylov_step_refs_cpu.py::test_x_dots_tree_bound), so that size also gets
    the integer-valued case that demands equality"""
    n = ks.X_BIG[tn]
    assert n > ks.X_MAX_BLOCKS * 512 * gr.vec_width(br.TYPES[tn])
    check_x(gexec, tn, ks.x_case(tn, n, two), two, what="above the cap")
    if ks.x_needs_exact(tn, n):
        check_x(gexec, tn, ks.x_case(tn, n, two, exact=True), two, exact=True, what="above the cap, exact")
    release()


@pytest.mark.parametrize("two", (False, True), ids=("step_1_dots", "step_2_step_1_dots"))
@pytest.mark.parametrize("tn", ("f64", "f32"))
def test_fused_states_and_exact_sums(gexec, tn, two):
    """beta = 0 and a stopped column: the vectors keep their bits and the sums are those of the old vectors; the
    two-step kernel also with prev_rho = 0, beta' = 0 -> delta, and stopped (beta_out = beta_in); integer-valued
    inputs give the exact sums"""
    for n in (5, 2049):
        for state in ("beta0", "stopped") + (("prev0", "delta") if two else ()):
            a = ks.x_case(tn, n, two, state=state)
            got, _ = check_x(gexec, tn, a, two, what=state)
            if state in ("beta0", "stopped"):
                assert all(same_bits(got[k], a[k]) for k in ("x", "r", "z", "w")), (state, "step_1 is a no-op")
            if state == "stopped":
                assert all(same_bits(got[k], a[k]) for k in (X1 if two else X1[:4]))
                assert not two or same_bits(got["beta_out"], a["beta_in"])
            if state == "delta":
                assert same_bits(got["beta_out"], a["delta"])
        check_x(gexec, tn, ks.x_case(tn, n, two, exact=True), two, exact=True, what="exact")


# --------------------------------------------------------------------------------- refused before any launch
def _status(fn):
    try:
        fn()
    except Exception as e:          # ginkgo_amd._lib.GkoError
        m = re.search(r"failed with status (-?\d+):", str(e))
        return int(m.group(1)) if m else None
    return 0


INVALID, WORKSPACE = -1, -3


@pytest.mark.parametrize("tn", ("f64", "f32"))
def test_fused_refusals(gexec, tn):
    """beta_in == beta_out: GKOC_E_INVALID; a workspace one byte short of 3 * 1024 * sizeof(T) at n > 0:
    GKOC_E_WORKSPACE.  Both are refused before any launch (run_x checks that every operand kept its bits and reads
    nothing from a call that raised), and a valid call afterwards gives the right result"""
    a2, a1 = ks.x_case(tn, 257, True), ks.x_case(tn, 257, False)
    assert _status(lambda: run_x(gexec, tn, a2, True, alias_beta=True)) == INVALID
    for two, a in ((True, a2), (False, a1)):
        assert _status(lambda: run_x(gexec, tn, a, two, wbytes=work_bytes(tn) - 1)) == WORKSPACE
        check_x(gexec, tn, a, two, what="after a refusal")
    # refused calls leave every operand alone: the same device buffers before and after
    t = br.TYPES[tn]
    dev = {k: Vec(gexec, np.asarray(a2[k]).reshape(-1, 1), 1) for k in X2}
    sc = {k: Flat(gexec, v) for k, v in a2.items() if k not in X2}
    out3, work = Flat(gexec, np.full(3, np.nan, t)), Flat(gexec, np.zeros(work_bytes(tn), np.uint8))
    vec = [dev[k].ptr for k in X2]
    tail = (sc["stop_status"], out3, work)
    assert _status(lambda: call("gkoc_x_pipe_cg_step_2_step_1_dots_" + tn, gexec.stream, 257, *vec, sc["prev_rho"],
                                sc["rho"], sc["delta"], sc["beta_in"], sc["beta_in"], *tail,
                                C.c_size_t(work_bytes(tn)), None)) == INVALID
    assert _status(lambda: call("gkoc_x_pipe_cg_step_2_step_1_dots_" + tn, gexec.stream, 257, *vec, sc["prev_rho"],
                                sc["rho"], sc["delta"], sc["beta_in"], sc["beta_out"], *tail,
                                C.c_size_t(work_bytes(tn) - 1), None)) == WORKSPACE
    assert _status(lambda: call("gkoc_x_pipe_cg_step_1_dots_" + tn, gexec.stream, 257, *vec[:8], sc["rho"],
                                sc["beta_in"], *tail, C.c_size_t(work_bytes(tn) - 1))) == WORKSPACE
    sync()
    assert all(d.unchanged() for d in list(dev.values()) + list(sc.values()) + [out3, work])


@pytest.mark.parametrize("tn", TYPES)
def test_elementwise_refusals(gexec, tn):
    """ld < cols of one operand: GKOC_E_INVALID from launch_elementwise; a NULL Chebyshev coefficient in the complex
    types: GKOC_E_INVALID.  The buffers are sized for the valid layout, nothing is launched, every operand keeps its
    bits, and the valid call that follows is right"""
    t = br.TYPES[tn]
    rows, cols = 9, 3
    for solver, kernel, bad in (("cg", "step_2", "q"), ("bicgstab", "step_3", "r"), ("pipe_cg", "step_1", "x"),
                                ("chebyshev", "update", "output")):
        a = ks.random_case(solver, kernel, tn, rows, cols)
        spec = ks.ALL_ABI[solver][kernel]
        dev = {n: (Vec(gexec, a[n]) if k in "Vv" else Flat(gexec, a[n])) for n, k in spec}
        args = []
        for n, k in spec:
            args += [dev[n].ptr, cols - 1 if n == bad else cols] if k in "Vv" else [dev[n]]
        cx = br.is_complex(t)
        coeffs = [_coeff(a["_alpha"], cx), _coeff(a["_beta"], cx)] if solver == "chebyshev" else []
        assert _status(lambda: call(entry(solver, kernel, tn), gexec.stream, rows, cols, *coeffs, *args)) == INVALID
        sync()
        assert all(d.unchanged() for d in dev.values()), (solver, kernel, "a refused call wrote")
        check(gexec, tn, solver, kernel, a)
    if br.is_complex(t):
        for kernel, coeffs in (("init_update", [None]), ("update", [None, _coeff(0.5, True)]),
                               ("update", [_coeff(0.5, True), None])):
            a = ks.random_case("chebyshev", kernel, tn, rows, cols)
            spec = ks.ALL_ABI["chebyshev"][kernel]
            dev = {n: Vec(gexec, a[n]) for n, _ in spec}
            args = [x for n, _ in spec for x in (dev[n].ptr, cols)]
            assert _status(lambda: call(entry("chebyshev", kernel, tn), gexec.stream, rows, cols, *coeffs, *args)) == INVALID
            sync()
            assert all(d.unchanged() for d in dev.values())
            check(gexec, tn, "chebyshev", kernel, a)
