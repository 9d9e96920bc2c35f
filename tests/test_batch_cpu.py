"""What of the batched solvers can be checked without a device: the C ABI declares and the library exports the
gkoc_batch_* entry points, the launch plan is a host-only call and behaves, the host-side argument checks of every
entry answer by return code, and the package exposes the classes with their setters and defaults."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import batch_refs as R
import ginkgo_amd as g
from ginkgo_amd import batch
from ginkgo_amd._lib import lib
from test_abi import declared_symbols

VT = ("f64", "f32")
ENTRIES = (["gkoc_batch_plan", "gkoc_batch_csr_check_i32", "gkoc_batch_ell_check_i32"]
           + [f"gkoc_batch_{s}_{f}_{t}_i32" for s in ("cg", "bicgstab") for f in ("csr", "ell") for t in VT]
           + [f"gkoc_batch_{f}_{k}_{t}_i32" for f in ("csr", "ell") for k in ("apply", "advanced_apply") for t in VT]
           + [f"gkoc_batch_{k}_{t}" for k in ("scale", "add_scaled", "compute_dot", "compute_norm2") for t in VT]
           + [f"gkoc_batch_{k}_{t}_i32" for k in ("csr_to_ell_values", "ell_to_csr_values") for t in VT])
SOLVERS, FORMATS, PRECONDS = ("cg", "bicgstab"), ("csr", "ell"), (None, "jacobi")
BUDGET = 81920      # half of a CU's LDS: two workgroups per CU


def test_entry_points_are_declared_and_exported():
    declared = set(declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (gkoc_\w+)", out))
    for name in ENTRIES:
        assert name in declared and name in exported, name
    assert {s for s in declared if s.startswith("gkoc_batch_")} == set(ENTRIES)


def test_no_entry_has_a_writable_index_pointer():
    import test_csr_plan_contract_cpu as contract
    assert not [s for s in contract.scan() if s.startswith("gkoc_batch")]
    assert not [s for e in contract.header_names() for s in e if s.startswith("gkoc_batch")]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_plan_is_monotone(solver, fmt, precond, dtype):
    """with n the resident vectors never rise and the workspace never falls; W is a power of two >= 64 that depends
    on n alone; the LDS stays within the budget; the values are never cached"""
    vb = 8 if dtype == "f64" else 4
    total = {("cg", None): 4, ("cg", "jacobi"): 6, ("bicgstab", None): 7, ("bicgstab", "jacobi"): 10}[solver, precond]
    sizes = sorted(set(list(range(0, 300)) + [2 ** k + d for k in range(9, 18) for d in (-1, 0, 1)]
                       + list(range(1500, 6000, 37)) + [10 ** 6]))
    before = None
    for n in sizes:
        p = batch.plan(solver, fmt, precond, dtype, n, 3 * n)
        assert p.w == R.width(n) and p.w >= 64 and p.w & (p.w - 1) == 0
        assert p.w == batch.plan("cg", "csr", None, "f64", n, 0).w
        assert p.total_vectors == total and 0 <= p.resident_vectors <= total
        assert 2 * p.w * vb <= p.lds_bytes <= BUDGET and p.lds_bytes % 16 == 0
        assert not p.values_cached
        assert p.lds_bytes == 2 * p.w * vb + p.resident_vectors * ((n * vb + 15) // 16 * 16)
        vec = (n * vb + 15) // 16 * 16
        assert p.workspace_bytes == max(total - p.resident_vectors - 1, 0) * vec
        if before is not None:
            assert p.resident_vectors <= before.resident_vectors and p.workspace_bytes >= before.workspace_bytes
        before = p
    assert batch.plan(solver, fmt, precond, dtype, 10, 30).resident_vectors == total
    assert batch.plan(solver, fmt, precond, dtype, 10 ** 6, 3 * 10 ** 6).resident_vectors == 0
    # (81920 - 2 * 512 * 8) / 10 = 7372 bytes per vector: all ten vectors of f64 Bicgstab + Jacobi up to 920 rows,
    # all but x at 1024
    if (solver, precond, dtype) == ("bicgstab", "jacobi", "f64"):
        assert batch.plan(solver, fmt, precond, dtype, 920, 2760).resident_vectors == total
        assert batch.plan(solver, fmt, precond, dtype, 921, 2763).resident_vectors == total - 1
        assert batch.plan(solver, fmt, precond, dtype, 1024, 3072).resident_vectors == total - 1


def test_plan_refuses_bad_arguments():
    L, info = lib(), batch._PlanInfo()
    args = lambda **kw: [C.c_int(kw.get("solver", 0)), C.c_int(kw.get("fmt", 0)), C.c_int(kw.get("pre", 0)),
                         C.c_int(kw.get("vb", 8)), C.c_int64(kw.get("n", 5)), C.c_int64(kw.get("stored", 5))]
    assert L.gkoc_batch_plan(*args(), C.byref(info)) == 0
    assert L.gkoc_batch_plan(*args(), None) == -1
    for bad in ({"solver": 2}, {"fmt": -1}, {"pre": 3}, {"vb": 2}, {"n": -1}, {"stored": -1}, {"n": 2 ** 31}):
        assert L.gkoc_batch_plan(*args(**bad), C.byref(info)) == -1, bad
    with pytest.raises(g.NotSupported):
        batch.plan("cg", "csr", "ilu", "f64", 5, 5)
    with pytest.raises(g.NotSupported):
        batch.plan("cg", "csr", None, "f16", 5, 5)


def test_host_side_argument_checks_answer_by_return_code():
    """null pointers, negative sizes, short strides, unknown codes and a short workspace are refused before any
    device call; nothing to do is not an error"""
    L, null = lib(), C.c_void_p(0)
    i64, dbl, sz, ci = C.c_int64, C.c_double, C.c_size_t, C.c_int
    one, neg, zero = i64(1), i64(-1), i64(0)
    p = C.c_void_p(64)       # a non-null address that is never dereferenced: every case below is refused first
    for t in VT:
        for s in SOLVERS:
            csr = getattr(L, f"gkoc_batch_{s}_csr_{t}_i32")
            ell = getattr(L, f"gkoc_batch_{s}_ell_{t}_i32")
            tail = lambda **k: [k.get("vals", p), ci(k.get("pre", 0)), k.get("b", p), i64(k.get("ldb", 1)), k.get("x", p),
                                i64(k.get("ldx", 1)), dbl(1e-8), ci(k.get("kind", 0)), i64(k.get("max_it", 10)),
                                k.get("work", null), sz(k.get("work_bytes", 0)), k.get("it", p), k.get("res", p),
                                k.get("conv", p)]
            for bad in ({"vals": null}, {"b": null}, {"x": null}, {"it": null}, {"res": null}, {"conv": null}, {"pre": 2},
                        {"kind": 2}, {"ldb": 0}, {"ldx": 0}, {"max_it": -1}):
                assert csr(null, one, i64(4), i64(8), p, p, *tail(**bad)) == -1, (s, t, bad)
                assert ell(null, one, i64(4), i64(2), i64(4), p, *tail(**bad)) == -1, (s, t, bad)
            assert csr(null, neg, i64(4), i64(8), p, p, *tail()) == -1
            assert csr(null, one, neg, i64(8), p, p, *tail()) == -1
            assert csr(null, one, i64(4), neg, p, p, *tail()) == -1
            assert csr(null, one, i64(4), i64(8), null, p, *tail()) == -1
            assert csr(null, one, i64(4), i64(8), p, null, *tail()) == -1
            assert ell(null, one, i64(4), neg, i64(4), p, *tail()) == -1
            assert ell(null, one, i64(4), i64(2), i64(3), p, *tail()) == -1       # stride < rows
            assert ell(null, one, i64(4), i64(2), i64(4), null, *tail()) == -1
            # a system that does not fit into LDS needs its workspace
            n = 10 ** 6
            need = batch.plan(s, "csr", None, t, n, 3 * n).workspace_bytes
            assert need > 0
            assert csr(null, i64(3), i64(n), i64(3 * n), p, p, *tail(work=null)) == -1
            assert csr(null, i64(3), i64(n), i64(3 * n), p, p, *tail(work=p, work_bytes=3 * need - 1)) == -1
            assert ell(null, i64(3), i64(n), i64(3), i64(n), p, *tail(work=p, work_bytes=need)) == -1
            assert csr(null, zero, i64(4), i64(8), null, null, *tail(vals=null, b=null, x=null)) == 0
        for f in FORMATS:
            head = [i64(4), i64(4), i64(8)] if f == "csr" else [i64(4), i64(4), i64(2), i64(4)]
            idx = [p, p] if f == "csr" else [p]
            simple = getattr(L, f"gkoc_batch_{f}_apply_{t}_i32")
            adv = getattr(L, f"gkoc_batch_{f}_advanced_apply_{t}_i32")
            assert simple(null, one, *head, *idx, p, p, i64(2), null, i64(2), i64(2)) == -1      # x
            assert simple(null, one, *head, *idx, null, p, i64(2), p, i64(2), i64(2)) == -1     # values
            assert simple(null, one, *head, *idx, p, p, i64(1), p, i64(2), i64(2)) == -1        # ldb < cols
            assert simple(null, one, *head, *idx, p, p, i64(2), p, i64(1), i64(2)) == -1        # ldx < cols
            assert simple(null, neg, *head, *idx, p, p, i64(2), p, i64(2), i64(2)) == -1
            assert simple(null, one, *head, *idx, p, p, i64(2), p, i64(2), neg) == -1
            assert simple(null, one, *head, *[null] * len(idx), p, p, i64(2), p, i64(2), i64(2)) == -1
            assert simple(null, zero, *head, *idx, p, p, i64(2), p, i64(2), i64(2)) == 0
            assert adv(null, one, *head, null, *idx, p, p, i64(2), p, p, i64(2), i64(2)) == -1  # alpha
            assert adv(null, one, *head, p, *idx, p, p, i64(2), null, p, i64(2), i64(2)) == -1  # beta
            assert adv(null, one, *head, p, *idx, p, p, i64(1), p, p, i64(2), i64(2)) == -1
            assert adv(null, zero, *head, p, *idx, p, p, i64(2), p, p, i64(2), i64(2)) == 0
        ell_bad = [i64(4), i64(4), i64(2), i64(3)]                                                # stride < rows
        assert getattr(L, f"gkoc_batch_ell_apply_{t}_i32")(null, one, *ell_bad, p, p, p, i64(2), p, i64(2), i64(2)) == -1
        scale, add = getattr(L, "gkoc_batch_scale_" + t), getattr(L, "gkoc_batch_add_scaled_" + t)
        dot, norm = getattr(L, "gkoc_batch_compute_dot_" + t), getattr(L, "gkoc_batch_compute_norm2_" + t)
        assert scale(null, one, i64(4), i64(3), null, one, p, i64(3)) == -1
        assert scale(null, one, i64(4), i64(3), p, one, null, i64(3)) == -1
        assert scale(null, one, i64(4), i64(3), p, i64(2), p, i64(3)) == -1         # 2 scalars for 3 columns
        assert scale(null, one, i64(4), i64(3), p, one, p, i64(2)) == -1            # ldx < cols
        assert scale(null, one, neg, i64(3), p, one, p, i64(3)) == -1
        assert scale(null, zero, i64(4), i64(3), p, one, p, i64(3)) == 0
        assert add(null, one, i64(4), i64(3), p, i64(3), null, i64(3), p, i64(3)) == -1
        assert add(null, one, i64(4), i64(3), p, i64(3), p, i64(2), p, i64(3)) == -1
        assert add(null, one, i64(4), i64(3), p, i64(4), p, i64(3), p, i64(3)) == -1
        assert add(null, zero, i64(4), i64(3), p, i64(3), p, i64(3), p, i64(3)) == 0
        assert dot(null, one, i64(4), i64(3), p, i64(3), p, i64(3), null) == -1
        assert dot(null, one, i64(4), i64(3), null, i64(3), p, i64(3), p) == -1
        assert dot(null, one, i64(4), i64(3), p, i64(3), p, i64(2), p) == -1
        assert dot(null, neg, i64(4), i64(3), p, i64(3), p, i64(3), p) == -1
        assert dot(null, zero, i64(4), i64(3), p, i64(3), p, i64(3), p) == 0
        assert norm(null, one, i64(4), i64(3), null, i64(3), p) == -1
        assert norm(null, one, i64(4), i64(3), p, i64(2), p) == -1
        assert norm(null, one, i64(4), i64(3), p, i64(3), null) == -1
        assert norm(null, zero, i64(4), i64(3), p, i64(3), p) == 0
        to_ell = getattr(L, f"gkoc_batch_csr_to_ell_values_{t}_i32")
        to_csr = getattr(L, f"gkoc_batch_ell_to_csr_values_{t}_i32")
        assert to_ell(null, one, i64(4), i64(8), null, i64(2), i64(4), p, p) == -1
        assert to_ell(null, one, i64(4), i64(8), p, i64(2), i64(4), null, p) == -1
        assert to_ell(null, one, i64(4), i64(8), p, i64(2), i64(4), p, null) == -1
        assert to_ell(null, one, i64(4), i64(8), p, i64(2), i64(3), p, p) == -1
        assert to_ell(null, one, i64(4), neg, p, i64(2), i64(4), p, p) == -1
        assert to_ell(null, zero, i64(4), i64(8), p, i64(2), i64(4), p, p) == 0
        assert to_csr(null, one, i64(4), i64(2), i64(4), null, i64(8), p, p, p) == -1
        assert to_csr(null, one, i64(4), i64(2), i64(4), p, i64(8), null, p, p) == -1
        assert to_csr(null, one, i64(4), i64(2), i64(4), p, i64(8), p, null, p) == -1
        assert to_csr(null, one, i64(4), i64(2), i64(4), p, i64(8), p, p, null) == -1
        assert to_csr(null, one, i64(4), i64(2), i64(3), p, i64(8), p, p, p) == -1
        assert to_csr(null, zero, i64(4), i64(2), i64(4), p, i64(8), p, p, p) == 0
    assert L.gkoc_batch_csr_check_i32(null, one, one, one, null, p) == -1
    assert L.gkoc_batch_csr_check_i32(null, one, one, one, p, null) == -1
    assert L.gkoc_batch_csr_check_i32(null, neg, one, one, p, p) == -1
    assert L.gkoc_batch_ell_check_i32(null, i64(4), i64(4), i64(2), i64(4), null) == -1
    assert L.gkoc_batch_ell_check_i32(null, i64(4), i64(4), i64(2), i64(3), p) == -1
    assert L.gkoc_batch_ell_check_i32(null, i64(4), i64(4), neg, i64(4), p) == -1
    assert L.gkoc_batch_ell_check_i32(null, i64(4), i64(4), zero, i64(4), null) == 0


def test_package_exposes_the_classes_setters_and_defaults():
    assert "batch" in g.__all__ and g.batch is batch
    for name in ("MultiVector", "Csr", "Ell", "Cg", "Bicgstab", "Jacobi", "plan"):
        assert name in batch.__all__ and hasattr(batch, name)
    for name in ("create", "from_numpy", "to_numpy", "create_view_for_item", "scale", "add_scaled", "compute_dot",
                 "compute_norm2"):
        assert callable(getattr(batch.MultiVector, name))
    for cls, convert in ((batch.Csr, "convert_to_ell"), (batch.Ell, "convert_to_csr")):
        for name in ("from_numpy", "from_matrices", "duplicate", "create_view_for_item", "apply", convert):
            assert callable(getattr(cls, name))
    for cls in (batch.Cg, batch.Bicgstab):
        f = cls.build()
        assert (f.max_iterations, f.tolerance, f.tolerance_type, f.preconditioner) == (100, 1e-11, "absolute", None)
        jac = batch.Jacobi.build()
        f = (f.with_max_iterations(7).with_tolerance(1e-6).with_tolerance_type("relative").with_preconditioner(jac))
        assert (f.max_iterations, f.tolerance, f.tolerance_type, f.preconditioner) == (7, 1e-6, "relative", jac)
        assert f.with_preconditioner(None).preconditioner is None
        with pytest.raises(g.GkoError):
            f.with_tolerance_type("implicit")
        with pytest.raises(g.GkoError):
            f.with_max_iterations(-1)
        with pytest.raises(g.NotSupported):
            f.with_preconditioner(g.Jacobi.build())
        with pytest.raises(g.GkoError):
            cls.build().generate(None)            # no executor
        assert callable(cls.apply)


def test_block_jacobi_is_not_supported():
    assert batch.Jacobi.build().with_max_block_size(1).max_block_size == 1
    for size in (2, 8, 32):
        with pytest.raises(g.NotSupported):
            batch.Jacobi.build().with_max_block_size(size)


class _FakeCsr(g.Csr):
    """a Csr whose arrays live on the host: enough for the pattern comparison, which runs before any device call"""

    def __init__(self, size, row_ptrs, col_idxs, values):
        import torch
        self.exec, self.size = None, size
        self.row_ptrs, self.col_idxs = torch.tensor(row_ptrs, dtype=torch.int32), torch.tensor(col_idxs, dtype=torch.int32)
        self.values = torch.tensor(values, dtype=torch.float64)


def test_mismatched_patterns_raise():
    a = _FakeCsr((2, 2), [0, 1, 2], [0, 1], [1.0, 2.0])
    for other in (_FakeCsr((2, 2), [0, 1, 2], [1, 1], [1.0, 2.0]), _FakeCsr((2, 2), [0, 2, 2], [0, 1], [1.0, 2.0]),
                  _FakeCsr((2, 2), [0, 1, 3], [0, 1, 0], [1.0, 2.0, 3.0]), _FakeCsr((2, 3), [0, 1, 2], [0, 1], [1.0, 2.0])):
        with pytest.raises(g.GkoError, match="sparsity pattern"):
            batch.Csr.from_matrices([a, other])
    with pytest.raises(g.GkoError):
        batch.Csr.from_matrices([])
    with pytest.raises(g.GkoError):
        batch.Csr.from_matrices([a, np.eye(2)])
