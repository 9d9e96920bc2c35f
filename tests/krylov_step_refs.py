"""numpy restatements of the Krylov step kernels of ginkgo_amd/csrc/krylov_steps.hip (bicgstab, cgs, fcg, pipe_cg,
bicg, gcr, minres, chebyshev, ir) and of the CG steps of csrc/cg_stop.hip, with the two fused PipeCg kernels
gkoc_x_pipe_cg_step_1_dots / gkoc_x_pipe_cg_step_2_step_1_dots, operand names and order of include/gko_cdna4.h
(tests/krylov_family_abi.py; `CG_ABI` below for the entry points that table lacks).

Same conventions as tests/binding_refs.py, whose `Arith` this file uses: `hp(T)` = long double is the expected
value where a tolerance applies, `plain(T)` = the value type with every real operation rounded on its own is what
the kernels promise to match bit for bit.  The expressions and their order are those of the op_* structs and the
scalar kernels.  Complex arithmetic follows csrc/complex_type.hpp operation for operation: the textbook product
(gmres_refs.mul), real times complex and complex over real by parts, Smith's quotient (gmres_refs.div), == on both
parts (gmres_refs.is_zero).  Two operations are NOT copied from the kernel, so that a defect of the device's
formula cannot hide in the reference: the modulus is hypot(re, im), and the complex square root is the stable form
(`csqrt_stable`: the larger part from sqrt((|z| + |re|) / 2), the other one as im / (2 * that)).

Every function takes an `Ops(ar)` and a dict name -> array (vectors tight rows x cols, scalars and stop status of
length cols) and returns the dict of what the kernel writes.  The expressions are numpy array operations in the
value type (complex by parts), scalars broadcast along the columns - the form the large shapes need;
`apply_by_element` evaluates the same kernel one element at a time (the loop form), and
tests/test_krylov_step_refs_cpu.py checks that both give the same bits, that plain(f64 / f32) equals the C oracle,
and the formulas against independent evaluations.  Nothing here touches a GPU."""
import numpy as np

import binding_refs as br
import gmres_refs as gr
from krylov_family_abi import KERNELS

STOP_MASK, FINALIZED_BIT = 0x3f, 0x40
RUN, STOPPED, STOPPED_FINAL, CONVERGED, CONVERGED_FINAL = 0x00, 0x01, 0x41, 0x82, 0xC3

# argument lists (krylov_family_abi kinds) of the entry points that table lacks
CG_ABI = {
    'cg': {
        'initialize': [('b', 'V'), ('r', 'v'), ('z', 'v'), ('p', 'v'), ('q', 'v'), ('prev_rho', 's'), ('rho', 's'),
                       ('stop_status', 't')],
        'step_1': [('p', 'v'), ('z', 'V'), ('rho', 'S'), ('prev_rho', 'S'), ('stop_status', 'T')],
        'step_2': [('x', 'v'), ('r', 'v'), ('p', 'V'), ('q', 'V'), ('beta', 'S'), ('rho', 'S'), ('stop_status', 'T')],
    },
    'chebyshev': {          # after the dimensions: the coefficients alpha (and beta): `_alpha`, `_beta` of the operand dict
        'init_update': [('inner_sol', 'V'), ('update_sol', 'v'), ('output', 'v')],
        'update': [('inner_sol', 'v'), ('update_sol', 'v'), ('output', 'v')],
    },
    'ir': {'initialize': [('stop_status', 't')]},
}
ALL_ABI = dict(KERNELS, **CG_ABI)
# kernels whose scalars do not vary per column (launch_elementwise(..., uniform_scalars = true))
UNIFORM = [(s, k) for s, ks in ALL_ABI.items() for k in ks if k.startswith("initialize")] + [("gcr", "restart")]
UNIFORM += [("chebyshev", "init_update"), ("chebyshev", "update")]
UNIFORM.remove(("ir", "initialize"))            # no vectors
UNIFORM.remove(("minres", "initialize"))        # reads beta per column: always the general path for cols > 1
# scalars written by OP::store: compared for running columns, untouched for stopped ones and when rows == 0
STORED = {("bicgstab", "step_2"): "alpha", ("cgs", "step_2"): "alpha", ("bicgstab", "step_3"): "omega",
          ("cgs", "step_1"): "beta", ("pipe_cg", "step_2"): "beta"}
# complex types: outputs downstream of abs_v (device hypot) or the complex sqrt follow rule R, not bit equality
RULE_R = {("minres", "initialize"): ("beta", "eta", "eta_next"),
          ("minres", "step_1"): ("alpha", "beta", "gamma", "delta", "cos_prev", "cos", "sin_prev", "sin", "eta",
                                 "eta_next", "tau"),
          ("pipe_cg", "step_2"): ("beta",)}


def has_stopped(stop):
    return (np.asarray(stop, np.uint8) & STOP_MASK) != 0


def csqrt_stable(z, rt):
    """principal square root of complex z, every real operation in rt: t = sqrt((|z| + |re|) / 2) is a sum of
    non-negative terms, the other part is |im| / (2 t); sqrt(+-0 + 0 i) = 0, the imaginary part has the sign of im
    (-0.0 counts as not negative)"""
    z = np.asarray(z)
    re, im = np.asarray(z.real, rt), np.asarray(z.imag, rt)
    with np.errstate(all="ignore"):
        m = np.hypot(re, im)
        t = np.sqrt((m + np.abs(re)) / rt(2))
        u = np.abs(im) / (rt(2) * t)
    neg = re < 0
    a, b = np.where(neg, u, t), np.where(neg, t, u)
    a, b = np.where(m == 0, rt(0), a), np.where(m == 0, rt(0), b)
    return a.astype(rt), np.where(im < 0, -b, b).astype(rt)


def csqrt_cancelling(z, rt):
    """the formula csrc/complex_type.hpp had before: both parts as sqrt((|z| +- re) / 2); one of them cancels when
    |im| << |re|.  Kept to show that the sweep of the tests tells the two apart"""
    z = np.asarray(z)
    re, im = np.asarray(z.real, rt), np.asarray(z.imag, rt)
    with np.errstate(all="ignore"):
        m = np.hypot(re, im)
        a, b = np.sqrt((m + re) / rt(2)), np.sqrt((m - re) / rt(2))
    return a.astype(rt), np.where(im < 0, -b, b).astype(rt)


def sqrt_sweep(tn):
    """the points of the square root sweep: beta = +-4 + 3 * 2^e i and 3 * 2^e +- 4 i with both signs of the small
    part, e = 0 .. -40 (c128) or 0 .. -20 (c64), the whole set scaled by 2^-60, 1, 2^60 (2^-30, 1, 2^30)"""
    t = br.TYPES[tn]
    emin, s = (-40, 60) if tn == "c128" else (-20, 30)
    pts = []
    for e in range(0, emin - 1, -1):
        small = 3.0 * 2.0 ** e
        for big in (4.0, -4.0):
            for sm in (small, -small):
                pts += [complex(big, sm), complex(sm, big)]
    pts = np.array(pts, np.complex128)
    return np.concatenate([pts * 2.0 ** -s, pts, pts * 2.0 ** s]).astype(t)      # powers of two: exact


def sqrt_hp(z):
    """the long-double square root (stable form) of value-type points, as a clongdouble array"""
    a, b = csqrt_stable(np.asarray(z).astype(np.clongdouble), np.longdouble)
    out = np.empty(a.shape, np.clongdouble)
    out.real, out.imag = a, b
    return out


class Ops:
    """the value arithmetic of one Arith: results are arrays of ar.wt (real ones of ar.rt)"""

    def __init__(self, ar):
        self.ar, self.wt, self.rt = ar, ar.wt, ar.rt
        self.hp = ar.wt in (np.longdouble, np.clongdouble)
        self.cx = np.dtype(ar.wt).kind == "c"

    def v(self, x):
        return np.asarray(x, self.wt)

    def mul(self, x, y):
        return gr.mul(self.ar, x, y)

    def div(self, x, y):
        return gr.div(self.ar, x, y)

    def rdiv(self, z, r):
        """value over real: both parts divided"""
        return gr.div_real(self.ar, z, r)

    def rmul(self, r, z):
        """real times value: both parts multiplied"""
        r, z = np.asarray(r, self.rt), self.v(z)
        if self.cx:
            out = np.empty(np.broadcast(r, z).shape, self.wt)
            out.real, out.imag = r * z.real, r * z.imag
            return out
        return np.asarray(r * z, self.wt)

    def add(self, x, y):
        return np.asarray(self.v(x) + self.v(y), self.wt)

    def sub(self, x, y):
        return np.asarray(self.v(x) - self.v(y), self.wt)

    def neg(self, x):
        return np.asarray(-self.v(x), self.wt)

    def conj(self, x):
        return np.asarray(np.conj(self.v(x)), self.wt)

    def abs(self, x):
        return gr.abs_v(self.ar, x)

    def sqrt(self, x):
        x = self.v(x)
        if not self.cx:
            return np.asarray(np.sqrt(x), self.wt)
        a, b = csqrt_stable(x, self.rt)
        out = np.empty(x.shape, self.wt)
        out.real, out.imag = a, b
        return out

    def safe_div(self, a, b):
        """b == 0 ? 0 : a / b"""
        return np.where(gr.is_zero(self.v(b)), self.wt(0), self.div(a, b)).astype(self.wt)

    def sel(self, mask, x, y):
        return np.where(mask, self.v(x), self.v(y)).astype(self.wt)


def _rows(a, name):
    return np.asarray(a[name]).shape[0]


def _init(o, a, copies, zeros, ones=(), zero_scalars=(), stop="stop_status", src="b"):
    b = o.v(a[src])
    cols = b.shape[1]
    out = {n: b.copy() for n in copies}
    out.update({n: np.zeros_like(b) for n in zeros})
    out.update({n: np.ones(cols, o.wt) for n in ones})
    out.update({n: np.zeros(cols, o.wt) for n in zero_scalars})
    if stop:
        out[stop] = np.zeros(cols, np.uint8)
    return out


def _stored(o, a, vec, name, stopped, new):
    """a scalar written by OP::store: by the thread of row 0 of a column that is not skipped"""
    if _rows(a, vec) == 0:
        return o.v(a[name]).copy()
    return o.sel(stopped, a[name], new)


# ---------------------------------------------------------------------------------------------- bicgstab
def bicgstab_initialize(o, a):
    return _init(o, a, ["r"], ["rr", "y", "s", "t", "z", "v", "p"],
                 ["prev_rho", "rho", "alpha", "beta", "gamma", "omega"])


def bicgstab_step_1(o, a):
    st = has_stopped(a["stop_status"])
    pr, om = o.v(a["prev_rho"]), o.v(a["omega"])
    nz = ~gr.is_zero(o.mul(pr, om))
    tmp = o.div(o.mul(o.div(a["rho"], pr), a["alpha"]), om)
    r, p = o.v(a["r"]), o.v(a["p"])
    full = o.add(r, o.mul(tmp, o.sub(p, o.mul(om, a["v"]))))
    return dict(p=o.sel(st, p, o.sel(nz, full, r)))


def bicgstab_step_2(o, a):
    st = has_stopped(a["stop_status"])
    bt = o.v(a["beta"])
    nz = ~gr.is_zero(bt)
    alpha = o.sel(nz, o.div(a["rho"], bt), 0)
    r = o.v(a["r"])
    s = o.sel(nz, o.sub(r, o.mul(alpha, a["v"])), r)
    return dict(s=o.sel(st, a["s"], s), alpha=_stored(o, a, "r", "alpha", st, alpha))


def bicgstab_step_3(o, a):
    st = has_stopped(a["stop_status"])
    bt = o.v(a["beta"])
    omega = o.sel(~gr.is_zero(bt), o.div(a["gamma"], bt), 0)
    x = o.add(a["x"], o.add(o.mul(a["alpha"], a["y"]), o.mul(omega, a["z"])))
    r = o.sub(a["s"], o.mul(omega, a["t"]))
    return dict(x=o.sel(st, a["x"], x), r=o.sel(st, a["r"], r), omega=_stored(o, a, "x", "omega", st, omega))


def bicgstab_finalize(o, a):
    stop = np.asarray(a["stop_status"], np.uint8)
    todo = has_stopped(stop) & ((stop & FINALIZED_BIT) == 0)
    x = o.sel(todo, o.add(a["x"], o.mul(a["alpha"], a["y"])), a["x"])
    if _rows(a, "x") == 0:
        return dict(x=x, stop_status=stop.copy())
    return dict(x=x, stop_status=np.where(has_stopped(stop), stop | FINALIZED_BIT, stop).astype(np.uint8))


# --------------------------------------------------------------------------------------------------- cgs
def cgs_initialize(o, a):
    return _init(o, a, ["r", "r_tld"], ["p", "q", "u", "u_hat", "v_hat", "t"],
                 ["rho_prev", "alpha", "beta", "gamma"], ["rho"])


def cgs_step_1(o, a):
    st = has_stopped(a["stop_status"])
    pr = o.v(a["rho_prev"])
    beta = o.sel(~gr.is_zero(pr), o.div(a["rho"], pr), a["beta"])
    q = o.v(a["q"])
    u = o.add(a["r"], o.mul(beta, q))
    p = o.add(u, o.mul(beta, o.add(q, o.mul(beta, a["p"]))))
    return dict(u=o.sel(st, a["u"], u), p=o.sel(st, a["p"], p), beta=_stored(o, a, "r", "beta", st, beta))


def cgs_step_2(o, a):
    st = has_stopped(a["stop_status"])
    g = o.v(a["gamma"])
    alpha = o.sel(~gr.is_zero(g), o.div(a["rho"], g), a["alpha"])
    q = o.sub(a["u"], o.mul(alpha, a["v_hat"]))
    t = o.add(a["u"], q)
    return dict(q=o.sel(st, a["q"], q), t=o.sel(st, a["t"], t), alpha=_stored(o, a, "u", "alpha", st, alpha))


def cgs_step_3(o, a):
    st = has_stopped(a["stop_status"])
    x = o.add(a["x"], o.mul(a["alpha"], a["u_hat"]))
    r = o.sub(a["r"], o.mul(a["alpha"], a["t"]))
    return dict(x=o.sel(st, a["x"], x), r=o.sel(st, a["r"], r))


# --------------------------------------------------------------------------------------------------- fcg
def fcg_initialize(o, a):
    return _init(o, a, ["r", "t"], ["z", "p", "q"], ["prev_rho", "rho_t"], ["rho"])


def _p_update(o, a, z, p, rho):
    """p = z + (rho / prev_rho) p, p = z if prev_rho == 0 (cg, fcg, bicg step_1)"""
    pr = o.v(a["prev_rho"])
    zero = gr.is_zero(pr)
    tmp = o.sel(zero, 0, o.div(a[rho], pr))
    return o.sel(has_stopped(a["stop_status"]), a[p], o.sel(zero, a[z], o.add(a[z], o.mul(tmp, a[p]))))


def fcg_step_1(o, a):
    return dict(p=_p_update(o, a, "z", "p", "rho_t"))


def _tmp_noop(o, a):
    """tmp = rho / beta; a no-op if beta == 0 or the column has stopped"""
    bt = o.v(a["beta"])
    nz = ~gr.is_zero(bt)
    return o.sel(nz, o.div(a["rho"], bt), 0), ~nz | has_stopped(a["stop_status"])


def fcg_step_2(o, a):
    tmp, noop = _tmp_noop(o, a)
    rn = o.sub(a["r"], o.mul(tmp, a["q"]))
    x = o.add(a["x"], o.mul(tmp, a["p"]))
    return dict(x=o.sel(noop, a["x"], x), r=o.sel(noop, a["r"], rn), t=o.sel(noop, a["t"], o.sub(rn, a["r"])))


# ------------------------------------------------------------------------------------------------ pipe_cg
def pipe_cg_initialize_1(o, a):
    return _init(o, a, ["r"], [], ["prev_rho"])


def pipe_cg_initialize_2(o, a):
    return dict(beta=o.v(a["delta"]).copy(), p=o.v(a["z"]).copy(), q=o.v(a["w"]).copy(), f=o.v(a["m"]).copy(),
                g=o.v(a["n"]).copy())


def pipe_cg_step_1(o, a):
    tmp, noop = _tmp_noop(o, a)
    z = o.sub(a["z1"], o.mul(tmp, a["f"]))
    out = dict(x=o.add(a["x"], o.mul(tmp, a["p"])), r=o.sub(a["r"], o.mul(tmp, a["q"])), z1=z, z2=z,
               w=o.sub(a["w"], o.mul(tmp, a["g"])))
    return {k: o.sel(noop, a[k], v) for k, v in out.items()}


def pipe_cg_step_2(o, a):
    st = has_stopped(a["stop_status"])
    pr = o.v(a["prev_rho"])
    plain = gr.is_zero(pr)
    tmp = o.sel(plain, 0, o.div(a["rho"], pr))
    m = o.abs(tmp)
    delta = o.v(a["delta"])
    b = o.sub(delta, o.rmul(np.asarray(m * m, o.rt), a["beta"]))
    b = o.sel(gr.is_zero(b), delta, b)
    out = dict(beta=_stored(o, a, "p", "beta", st, o.sel(plain, delta, b)))
    for dst, src in (("p", "z"), ("q", "w"), ("f", "m"), ("g", "n")):
        out[dst] = o.sel(st, a[dst], o.sel(plain, a[src], o.add(a[src], o.mul(tmp, a[dst]))))
    return out


# --------------------------------------------------------------------------------------------------- bicg
def bicg_initialize(o, a):
    return _init(o, a, ["r", "r2"], ["z", "p", "q", "z2", "p2", "q2"], ["prev_rho"], ["rho"])


def bicg_step_1(o, a):
    return dict(p=_p_update(o, a, "z", "p", "rho"), p2=_p_update(o, a, "z2", "p2", "rho"))


def bicg_step_2(o, a):
    tmp, noop = _tmp_noop(o, a)
    return dict(x=o.sel(noop, a["x"], o.add(a["x"], o.mul(tmp, a["p"]))),
                r=o.sel(noop, a["r"], o.sub(a["r"], o.mul(tmp, a["q"]))),
                r2=o.sel(noop, a["r2"], o.sub(a["r2"], o.mul(tmp, a["q2"]))))


# ---------------------------------------------------------------------------------------------------- gcr
def gcr_initialize(o, a):
    return _init(o, a, ["residual"], [])


def gcr_restart(o, a):
    cols = np.asarray(a["residual"]).shape[1]
    return dict(p_bases=o.v(a["residual"]).copy(), Ap_bases=o.v(a["A_residual"]).copy(),
                final_iter_nums=np.zeros(cols, np.uint64))


def gcr_step_1(o, a):
    nrm = np.asarray(a["Ap_norm"], o.rt)                    # remove_complex<T>: a real divisor
    nz = nrm != 0
    tmp = o.sel(nz, o.rdiv(a["rAp"], nrm), 0)
    noop = ~nz | has_stopped(a["stop_status"])
    return dict(x=o.sel(noop, a["x"], o.add(a["x"], o.mul(tmp, a["p"]))),
                residual=o.sel(noop, a["residual"], o.sub(a["residual"], o.mul(tmp, a["Ap"]))))


# ------------------------------------------------------------------------------------------------- minres
def minres_initialize(o, a):
    r = o.v(a["r"])
    cols = r.shape[1]
    b = o.sqrt(a["beta"])
    zero = np.zeros(cols, o.wt)
    out = dict(delta=zero, gamma=zero.copy(), cos_prev=zero.copy(), sin_prev=zero.copy(), sin=zero.copy(),
               cos=np.ones(cols, o.wt), beta=b, eta=b.copy(), eta_next=b.copy(), stop_status=np.zeros(cols, np.uint8))
    out.update(q=o.safe_div(r, b), z=o.safe_div(a["z"], b))
    out.update({n: np.zeros_like(r) for n in ("p", "p_prev", "q_prev", "q_tilde")})
    return out


_MINRES_1 = ("alpha", "beta", "gamma", "delta", "cos_prev", "cos", "sin_prev", "sin", "eta", "eta_next", "tau")


def minres_step_1(o, a):
    st = has_stopped(a["stop_status"])
    alpha, beta, gamma, _, cos_prev, cos, sin_prev, sin, _, eta_next, tau = (o.v(a[k]) for k in _MINRES_1)
    bt = o.sqrt(beta)
    delta_n = o.mul(sin_prev, gamma)
    gamma_n = o.add(o.mul(o.mul(cos_prev, cos), gamma), o.mul(sin, alpha))
    an = o.add(o.mul(o.mul(o.neg(o.conj(sin)), cos_prev), gamma), o.mul(cos, alpha))
    zero = gr.is_zero(an)
    with np.errstate(all="ignore"):
        scale = np.asarray(o.abs(an) + o.abs(bt), o.rt)
        as_, bs = o.abs(o.rdiv(an, scale)), o.abs(o.rdiv(bt, scale))
        hyp = np.asarray(scale * np.sqrt(np.asarray(as_ * as_ + bs * bs, o.rt)), o.rt)
    c = o.sel(zero, 0, o.rdiv(o.conj(an), hyp))
    sn = o.sel(zero, 1, o.rdiv(o.conj(bt), hyp))
    new = dict(alpha=o.add(o.mul(c, an), o.mul(sn, bt)), beta=bt, gamma=gamma_n, delta=delta_n, cos_prev=cos,
               cos=c, sin_prev=sin, sin=sn, eta=eta_next, eta_next=o.mul(o.neg(o.conj(sn)), eta_next),
               tau=o.mul(o.mul(sn, sn), tau))
    return {k: o.sel(st, a[k], v) for k, v in new.items()}


def minres_step_2(o, a):
    st = has_stopped(a["stop_status"])
    p = o.safe_div(o.sub(o.sub(a["z"], o.mul(a["gamma"], a["p_prev"])), o.mul(a["delta"], a["p"])), a["alpha"])
    new = dict(x=o.add(a["x"], o.mul(o.mul(a["cos"], a["eta"]), p)), p=p, z=o.safe_div(a["z_tilde"], a["beta"]),
               q=o.safe_div(a["v"], a["beta"]), q_prev=o.v(a["v"]).copy(), v=o.mul(a["q"], a["beta"]))
    return {k: o.sel(st, a[k], v) for k, v in new.items()}


# --------------------------------------------------------------------------------------------- cg, ir
def cg_initialize(o, a):
    return _init(o, a, ["r"], ["z", "p", "q"], ["prev_rho"], ["rho"])


def cg_step_1(o, a):
    return dict(p=_p_update(o, a, "z", "p", "rho"))


def cg_step_2(o, a):
    tmp, noop = _tmp_noop(o, a)
    return dict(x=o.sel(noop, a["x"], o.add(a["x"], o.mul(tmp, a["p"]))),
                r=o.sel(noop, a["r"], o.sub(a["r"], o.mul(tmp, a["q"]))))


def ir_initialize(o, a):
    return dict(stop_status=np.zeros(np.asarray(a["stop_status"]).shape[0], np.uint8))


def chebyshev_init_update(o, a):
    upd, out = cheb_init_update(o.ar, np.asarray(a["inner_sol"]).dtype, a["_alpha"], a["inner_sol"], a["output"])
    return dict(update_sol=upd, output=out)


def chebyshev_update(o, a):
    inner, upd, out = cheb_update(o.ar, np.asarray(a["inner_sol"]).dtype, a["_alpha"], a["_beta"], a["inner_sol"],
                                  a["update_sol"], a["output"])
    return dict(inner_sol=inner, update_sol=upd, output=out)


FUNCS = {(s, k): globals()[f"{s}_{k}"] for s, ks in ALL_ABI.items() for k in ks}


def apply(ar, solver, kernel, a):
    """the kernel's effect on the dict a: a new dict, the operands it writes replaced"""
    with np.errstate(all="ignore"):
        out = FUNCS[solver, kernel](Ops(ar), a)
    res = {k: np.array(v, copy=True) for k, v in a.items()}
    for k, v in out.items():
        res[k] = np.asarray(v).reshape(np.asarray(a[k]).shape)
    return res


def apply_by_element(ar, solver, kernel, a):
    """the loop form: the same kernel evaluated for one element (row, column) at a time; per-column outputs are
    taken from row 0, or from a call without rows if there are none"""
    spec = ALL_ABI[solver][kernel]
    vec = [n for n, k in spec if k in "Vv"]
    res = {k: np.array(v, copy=True) for k, v in a.items()}
    if not vec:
        return apply(ar, solver, kernel, a)
    rows, cols = np.asarray(a[vec[0]]).shape
    for c in range(cols):
        for r in ([None] if rows == 0 else range(rows)):
            one = {n: (np.asarray(a[n])[(slice(0, 0) if r is None else slice(r, r + 1)), c:c + 1]
                       if n in vec else np.asarray(a[n])[c:c + 1]) for n, _ in spec}
            one.update({k: v for k, v in a.items() if k.startswith("_")})
            got = apply(ar, solver, kernel, one)
            for n, k in spec:
                if n in vec:
                    if r is not None:
                        res[n] = res[n].astype(got[n].dtype, copy=False)
                        res[n][r, c] = got[n][0, 0]
                elif r in (None, 0):
                    res[n] = res[n].astype(got[n].dtype, copy=False)
                    res[n][c] = got[n][0]
    return res


# ---------------------------------------------------------------------------------------------- chebyshev
def _cheb_ops(ar, t):
    """Chebyshev works in coeff_type: double / complex<double> whatever the value type (long double for hp)"""
    if ar.wt in (np.longdouble, np.clongdouble):
        return Ops(ar)
    return Ops(br.plain(np.complex128 if br.is_complex(t) else np.float64))


def _narrow(ar, t, v):
    return v if ar.wt in (np.longdouble, np.clongdouble) else v.astype(t)


def cheb_init_update(ar, t, alpha, inner, output):
    """update = inner ; output += alpha inner -> (update, output)"""
    o = _cheb_ops(ar, t)
    with np.errstate(all="ignore"):
        v = o.v(inner)
        return _narrow(ar, t, v), _narrow(ar, t, o.add(output, o.mul(alpha, v)))


def cheb_update(ar, t, alpha, beta, inner, update, output):
    """val = inner + beta update ; inner = update = val ; output += alpha val -> (inner, update, output)"""
    o = _cheb_ops(ar, t)
    with np.errstate(all="ignore"):
        v = o.add(inner, o.mul(beta, update))
        return _narrow(ar, t, v), _narrow(ar, t, v), _narrow(ar, t, o.add(output, o.mul(alpha, v)))


# ------------------------------------------------------------------ the two fused PipeCg kernels (real types)
X_MAX_BLOCKS = 1024


def x_step_1(ar, a):
    """the vectors of gkoc_x_pipe_cg_step_1_dots: pipe_cg::step_1 on one column without z2"""
    col = {k: np.asarray(v).reshape(-1, 1) if k in "xrzwpqfg" else np.asarray(v) for k, v in a.items()}
    col["z1"], col["z2"] = col["z"], col["z"]
    got = apply(ar, "pipe_cg", "step_1", {n: col[n] for n, _ in KERNELS["pipe_cg"]["step_1"]})
    return {k: got[{"z": "z1"}.get(k, k)].reshape(-1) for k in "xrzw"}


def x_step_2_step_1(ar, a):
    """the vectors and beta_out of gkoc_x_pipe_cg_step_2_step_1_dots: pipe_cg::step_2, then step_1 with the new
    beta; a stopped column keeps everything and beta_out = beta_in"""
    col = {k: np.asarray(v).reshape(-1, 1) if k in "xrzwpqfgmn" else np.asarray(v) for k, v in a.items()}
    col["beta"] = col["beta_in"]
    if col["x"].shape[0] == 0:              # n = 0: the launcher zeroes out3 and touches nothing else
        return dict({k: col[k].reshape(-1) for k in "xrzwpqfg"}, beta_out=np.asarray(a["beta_out"]).copy())
    s2 = apply(ar, "pipe_cg", "step_2", {n: col[n] for n, _ in KERNELS["pipe_cg"]["step_2"]})
    nxt = dict(col, **{k: s2[k] for k in "pqfg"}, beta=s2["beta"], z1=col["z"], z2=col["z"])
    s1 = apply(ar, "pipe_cg", "step_1", {n: nxt[n] for n, _ in KERNELS["pipe_cg"]["step_1"]})
    out = {k: s2[k].reshape(-1) for k in "pqfg"}
    out.update({k: s1[{"z": "z1"}.get(k, k)].reshape(-1) for k in "xrzw"})
    out["beta_out"] = s2["beta"]
    return out


def x_blocks(n, t):
    return min(-(-n // (256 * gr.vec_width(t) * 2)), X_MAX_BLOCKS)


def x_dots_depth(n, t, vec_ok=True):
    """additions on the longest path of one of the three sums of the fused kernels.  nb = min(ceil(n / (512 W)),
    1024) blocks of 256 threads, W = 16 / sizeof(T).  With aligned pointers a thread takes every (256 nb)-th vector
    and adds its W products in turn: W * ceil((n / W) / (256 nb)) additions, and at most one more for the scalar
    tail of n % W rows; otherwise the scalar loop does all the work, ceil(n / (256 nb)) additions.  block_sum<256>
    adds 8 levels (6 butterfly levels and 2 for the four wave sums); fold_rows_kernel (fused.hpp) gives each of its
    1024 threads at most one of the nb <= 1024 partials (1 addition to acc = 0), then block_sum<1024>: 6 levels
    and 4 for the sixteen wave sums"""
    if n == 0:
        return 0
    W = gr.vec_width(t)
    per = 256 * x_blocks(n, t)
    mine = W * -(-(n // W) // per) + (1 if n % W else 0) if vec_ok else -(-n // per)
    return mine + 8 + 1 + 10


def x_dots_hp(r, z, w):
    """(<r, z>, <w, z>, <r, r>) and the sums of |terms| in long double"""
    r, z, w = (np.asarray(v, np.longdouble) for v in (r, z, w))
    terms = (r * z, w * z, r * r)
    return np.array([np.sum(v) for v in terms], np.longdouble), np.array([np.sum(np.abs(v)) for v in terms],
                                                                         np.longdouble)


def x_dots_tree(t, r, z, w, vec_ok=True):
    """emulation in the value type of the three sums: per-thread vector and tail loops, block_sum<256>, the fold"""
    t = np.dtype(t).type
    n = r.shape[0]
    if n == 0:
        return np.zeros(3, t)
    W, nb = gr.vec_width(t), x_blocks(n, t)
    per = 256 * nb
    out = []
    for u, v in ((r, z), (w, z), (r, r)):
        terms = (np.asarray(u, t) * np.asarray(v, t)).astype(t)
        acc = np.zeros(per, t)
        done = 0
        if vec_ok:
            n_vec = n // W
            trips = -(-n_vec // per)
            tv = np.zeros(trips * per * W, t)
            tv[:n_vec * W] = terms[:n_vec * W]
            tv = tv.reshape(trips, per, W)
            for i in range(trips):
                for e in range(W):
                    acc = (acc + tv[i, :, e]).astype(t)
            done = n_vec * W
        rest = terms[done:]
        trips = -(-rest.shape[0] // per)
        tr = np.zeros(trips * per, t)
        tr[:rest.shape[0]] = rest
        for row in tr.reshape(trips, per):
            acc = (acc + row).astype(t)
        partial = gr._block_sum(acc.reshape(nb, 256))
        p = np.zeros(1024, t)
        p[:nb] = partial
        out.append(gr._block_sum((np.zeros(1024, t) + p).astype(t)))
    return np.array(out, t)


# ------------------------------------------------------------------------------------- inputs of the tests
_TN_ID = {"f64": 1, "f32": 2, "c128": 3, "c64": 4}
X_ROWS = (0, 1, 2, 3, 5, 2047, 2048, 2049, 100003)
X_BIG = {"f64": 1049601, "f32": 2098177}          # above 1024 blocks of 512 W rows: the grid-stride loop's second trip
X_SINGLE_TEETH_LIMIT = 100003                     # f32 above it: the depth bound exceeds one median term


def x_needs_exact(tn, n):
    return tn == "f32" and n > X_SINGLE_TEETH_LIMIT


def x_case(tn, n, two, exact=False, state="run"):
    """operands of the fused kernels (`two`: the two-step one).  state: run, beta0 (step_1 a no-op: beta = 0, or
    in the two-step kernel beta' = delta = 0), stopped, and for the two-step kernel prev0 (prev_rho = 0) and
    delta (delta - |t2|^2 beta_in = 0, so beta' = delta).  exact: entries in {-1, 0, 1}, tmp = 1"""
    t = br.TYPES[tn]
    rng = np.random.default_rng([19, _TN_ID[tn], n, int(two), int(exact)])
    gen = gr.ints if exact else gr.rand
    a = {k: gen(rng, (n,), t) for k in ("xrzwpqfg" + ("mn" if two else ""))}
    s = (lambda v: np.array([v], t))
    a["rho"] = s(1.0 if exact else 0.75)
    a["stop_status"] = np.array([STOPPED if state == "stopped" else RUN], np.uint8)
    if not two:
        a["beta"] = s(0.0 if state == "beta0" else (1.0 if exact else 1.5))
        return a
    a["prev_rho"] = s(0.0 if state == "prev0" else (1.0 if exact else 1.25))
    a["beta_in"], a["delta"] = (s(2.0), s(3.0)) if exact else (s(0.5), s(2.0))
    if state == "delta":            # t2 = 1, 2 - 1 * 2 = 0 -> beta' = delta
        a["rho"], a["prev_rho"], a["beta_in"], a["delta"] = s(1.5), s(1.5), s(2.0), s(2.0)
    if state == "beta0":            # prev_rho = 0 -> beta' = delta = 0
        a["prev_rho"], a["delta"] = s(0.0), s(0.0)
    a["beta_out"] = np.full(1, np.nan, t)
    return a


def random_case(solver, kernel, tn, rows, cols, seed=0, outputs_nan=True):
    """well-scaled operands of one kernel: vectors uniform in (-1, 1) (both parts), scalars of modulus in
    (0.5, 2), output-only operands NaN, all columns running; Ap_norm is real and positive, the beta of minres
    (a square root is taken) has a positive real part that dominates"""
    t = br.TYPES[tn]
    rt = br.real_of(t)
    rng = np.random.default_rng([17, _TN_ID[tn], rows, cols, seed] + [ord(ch) for ch in solver + kernel])
    a = {}
    if solver == "chebyshev":       # host coefficients of coeff_type: double, or complex<double>
        a["_alpha"], a["_beta"] = (0.37 + 0.21j, -0.61 + 0.4j) if br.is_complex(t) else (0.37, -0.61)
    for name, kind in ALL_ABI[solver][kernel]:
        if kind in "Vv":
            a[name] = gr.rand(rng, (rows, cols), t)
            if kind == "v" and outputs_nan and name in OUTPUT_ONLY.get((solver, kernel), ()):
                a[name] = np.full((rows, cols), np.nan, t)
        elif kind in "Ss":
            if name == "Ap_norm":
                a[name] = rng.uniform(0.5, 2.0, cols).astype(rt)
                continue
            v = rng.uniform(0.5, 2.0, cols) * rng.choice([-1, 1], cols)
            if br.is_complex(t):
                v = v * np.exp(1j * rng.uniform(-np.pi, np.pi, cols))
            if solver == "minres" and name == "beta":
                v = np.abs(v) * (np.exp(1j * rng.uniform(-0.3, 0.3, cols)) if br.is_complex(t) else 1)
            a[name] = np.asarray(v).astype(t)
            if kind == "s" and outputs_nan and name in OUTPUT_ONLY.get((solver, kernel), ()):
                a[name] = np.full(cols, np.nan, t)
        elif kind == "U":
            a[name] = np.full(cols, 7, np.uint64)
        else:
            a[name] = np.full(cols, 0xff, np.uint8) if kind in "tp" and kernel != "finalize" else np.zeros(cols, np.uint8)
    return a


# the scalars whose being zero a kernel branches on
ZERO_DENOMS = {("bicgstab", "step_1"): ("prev_rho", "omega"), ("bicgstab", "step_2"): ("beta",),
               ("bicgstab", "step_3"): ("beta",), ("cgs", "step_1"): ("rho_prev",), ("cgs", "step_2"): ("gamma",),
               ("fcg", "step_1"): ("prev_rho",), ("fcg", "step_2"): ("beta",), ("pipe_cg", "step_1"): ("beta",),
               ("pipe_cg", "step_2"): ("prev_rho",), ("bicg", "step_1"): ("prev_rho",), ("bicg", "step_2"): ("beta",),
               ("gcr", "step_1"): ("Ap_norm",), ("minres", "initialize"): ("beta",),
               ("minres", "step_2"): ("alpha", "beta"), ("cg", "step_1"): ("prev_rho",), ("cg", "step_2"): ("beta",)}


def state_case(solver, kernel, tn, rows, seed=1):
    """random_case with one column per state: running; stopped without and with the finalized bit; converged
    without and with it; one column per zero denominator of the kernel (ZERO_DENOMS; pipe_cg step_2 also
    beta' = 0 -> delta, minres step_1 also the a == 0 rotation); bicgstab step_1: a prev_rho * omega whose product
    underflows to zero although neither factor is zero; complex types: each denominator once as (0, 1) and once
    as (1, 0), which are not zero.  Returns (operands, labels)"""
    t = br.TYPES[tn]
    cx = br.is_complex(t)
    key = (solver, kernel)
    has_stop = any(k in "TtPp" for _, k in ALL_ABI[solver][kernel]) and not kernel.startswith("initialize")
    states = [("running", None)]
    if has_stop:
        states += [(f"stop {code:#04x}", code) for code in (STOPPED, STOPPED_FINAL, CONVERGED, CONVERGED_FINAL)]
    for name in ZERO_DENOMS.get(key, ()):
        states.append((f"{name} = 0", {name: 0}))
        if cx and name != "Ap_norm":
            states += [(f"{name} = i", {name: 1j}), (f"{name} = (1, 0)", {name: 1})]
    if key == ("bicgstab", "step_1"):
        tiny = 1e-200 if br.real_of(t) == np.float64 else 1e-30
        states.append(("prev_rho omega underflows", {"prev_rho": tiny, "omega": -tiny}))
        if cx:
            states.append(("prev_rho omega underflows (i)", {"prev_rho": tiny * 1j, "omega": tiny}))
    if key == ("pipe_cg", "step_2"):
        states.append(("beta' = 0 -> delta", {"rho": 1.5, "prev_rho": 1.5, "beta": 2.0, "delta": 2.0}))
    if key == ("minres", "step_1"):
        states.append(("a = 0", {"alpha": 0, "gamma": 0}))
    a = random_case(solver, kernel, tn, rows, len(states), seed)
    for c, (_, what) in enumerate(states):
        if isinstance(what, dict):
            for name, v in what.items():
                a[name][c] = v
        elif what is not None:
            a["stop_status"][c] = what
            if key in STORED:                   # a stopped column must keep the NaN of its stored scalar
                a[STORED[key]][c] = np.nan
    return a, [s[0] for s in states]


def _output_only():
    out = {}
    for (s, k) in [(s, k) for s, ks in ALL_ABI.items() for k in ks]:
        spec = ALL_ABI[s][k]
        if k.startswith("initialize") or k == "restart":
            names = [n for n, kind in spec if kind in "vs"]
            if (s, k) == ("minres", "initialize"):
                names = [n for n in names if n not in ("z", "beta")]
            out[s, k] = tuple(names)
    out["chebyshev", "init_update"] = ("update_sol",)
    out["bicgstab", "step_2"] = ("s", "alpha")
    out["bicgstab", "step_3"] = ("r", "omega")
    out["cgs", "step_1"] = ("u",)
    out["cgs", "step_2"] = ("q", "t")
    out["fcg", "step_2"] = ("t",)
    out["pipe_cg", "step_1"] = ("z2",)
    out["minres", "step_1"] = ("delta", "eta")
    out["minres", "step_2"] = ("q_prev",)
    return out


OUTPUT_ONLY = _output_only()
