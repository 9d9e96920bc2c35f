"""What of the Pgm / Multigrid feature can be checked without a device: the C ABI declares and the library exports
the gkoc_pgm_* entry points, the path limits are reported by a host-only call, host-side argument checks
answer by return code, and the package exposes the classes with their setters and defaults."""
import ctypes as C
import re
import subprocess

import pytest

import ginkgo_amd as g
from ginkgo_amd._lib import call, lib
from test_abi import HEADER, declared_symbols

PAIRS = ["f64_i32", "f64_i64", "f32_i32", "f32_i64"]
ENTRIES = (["gkoc_pgm_row_limits"]
           + [f"gkoc_pgm_{k}_{i}" for k in ("match", "renumber", "check_transfers") for i in ("i32", "i64")]
           + [f"gkoc_pgm_{k}_{p}" for k in ("select", "leftover", "map_entries", "restrict", "prolong_add")
              for p in PAIRS])


def test_entry_points_are_declared_and_exported():
    declared = set(declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (gkoc_\w+)", out))
    for name in ENTRIES:
        assert name in declared and name in exported, name
    assert {s for s in declared if s.startswith("gkoc_pgm_")} == set(ENTRIES)


def test_row_limits_are_reported_without_a_device():
    limits = g.multigrid.row_limits()
    assert 1 <= len(limits) <= 4 and limits == sorted(set(limits)) and all(8 <= x <= 64 for x in limits)
    with pytest.raises(g.GkoError):
        call("gkoc_pgm_row_limits", None, C.byref(C.c_int(0)))
    with pytest.raises(g.GkoError):
        call("gkoc_pgm_row_limits", (C.c_int * 4)(), None)


def test_host_side_argument_checks_answer_by_return_code():
    """null pointers, negative sizes and short strides are refused before any device call"""
    L, null, one = lib(), C.c_void_p(0), C.c_int64(1)
    invalid = -1
    for p in PAIRS:
        assert getattr(L, "gkoc_pgm_select_" + p)(null, one, null, null, null, null, null, null) == invalid
        assert getattr(L, "gkoc_pgm_leftover_" + p)(null, one, null, null, null, null, null, null) == invalid
        assert getattr(L, "gkoc_pgm_restrict_" + p)(null, one, one, null, null, null, one, null, one) == invalid
        assert getattr(L, "gkoc_pgm_prolong_add_" + p)(null, one, one, null, null, one, null, one) == invalid
        assert getattr(L, "gkoc_pgm_restrict_" + p)(null, C.c_int64(-1), one, null, null, null, one, null, one) == invalid
        assert getattr(L, "gkoc_pgm_map_entries_" + p)(null, one, one, one, null, null, null, null, null) == invalid
        assert getattr(L, "gkoc_pgm_map_entries_" + p)(null, one, one, C.c_int64(2), null, null, null, null, null) == invalid
        # nothing to do is not an error
        assert getattr(L, "gkoc_pgm_restrict_" + p)(null, C.c_int64(0), one, null, null, null, one, null, one) == 0
        assert getattr(L, "gkoc_pgm_select_" + p)(null, C.c_int64(0), null, null, null, null, null, null) == 0
    count = C.c_longlong(7)
    for i in ("i32", "i64"):
        assert getattr(L, "gkoc_pgm_match_" + i)(null, one, null, null, C.byref(count)) == invalid
        assert getattr(L, "gkoc_pgm_match_" + i)(null, one, null, null, null) == invalid
        assert getattr(L, "gkoc_pgm_renumber_" + i)(null, one, null, C.byref(count)) == invalid
        assert getattr(L, "gkoc_pgm_check_transfers_" + i)(null, one, one, null, null, null) == invalid
        assert getattr(L, "gkoc_pgm_renumber_" + i)(null, C.c_int64(0), null, C.byref(count)) == 0 and count.value == 0


def test_no_entry_writes_an_index_array_of_a_matrix():
    """The column-offset plan's contract (test_csr_plan_contract_cpu) lists every entry that writes a typed index
    array.  The Pgm entries write aggregation state (gkoc_pgm_i32 / _i64) and matrix_data entries (void*), and
    announce themselves as nothing else: no int32_t* / int64_t* output, and nothing added to the contract."""
    pre = subprocess.run(["gcc", "-E", "-P", HEADER], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        m = re.search(name + r"\s*\(([^)]*)\)", pre)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert not [p for p in params if re.match(r"^int(32|64)_t\s*\*", p)], (name, params)
    import test_csr_plan_contract_cpu as contract
    assert not [s for s in contract.scan() if s.startswith("gkoc_pgm")]
    assert not [s for e in contract.header_names() for s in e if s.startswith("gkoc_pgm")]
    outputs = {"select": "proposals", "leftover": "agg", "match": "agg", "renumber": "agg"}
    for kind, param in outputs.items():
        name = f"gkoc_pgm_{kind}_" + ("i32" if kind in ("match", "renumber") else "f64_i32")
        assert re.search(name + r"\s*\([^)]*gkoc_pgm_i32\s*\*\s*" + param + r"\s*[,)]", pre), name


def test_package_exposes_the_classes_setters_and_defaults():
    assert {"Pgm", "Multigrid", "multigrid"} <= set(g.__all__)
    f = g.Pgm.build()
    assert (f.max_iterations, f.max_unassign_ratio, f.skip_sorting) == (15, 0.05, False)
    assert f.with_max_iterations(3).max_iterations == 3 and f.with_max_unassign_ratio(0.2).max_unassign_ratio == 0.2
    assert f.with_skip_sorting(True).skip_sorting is True
    assert f.with_deterministic(False) is f           # accepted, without effect
    for name in ("get_agg", "get_num_aggregates", "get_fine_op", "get_coarse_op", "get_restrict_op", "get_prolong_op"):
        assert callable(getattr(g.Pgm, name))
    assert issubclass(g.Multigrid, g.solver._IterativeSolver)
    m = g.Multigrid.build()
    assert isinstance(m, g.solver._SolverFactory) and m.params == {}
    pgm = g.Pgm.build()
    m = (m.with_mg_level(pgm).with_max_levels(4).with_min_coarse_rows(10).with_cycle("w").with_smoother_relax(0.8)
         .with_smoother_iters(2).with_pre_smoother(None).with_post_smoother(None).with_coarsest_solver(None)
         .with_default_initial_guess("provided").with_criteria(g.stop.Iteration.build().with_max_iters(2)))
    assert m.params["mg_level"] is pgm and m.params["cycle"] == "w" and m.params["max_levels"] == 4
    assert callable(g.Multigrid.get_mg_level_list) and callable(g.Multigrid.get_coarsest_solver)
    # a preconditioner factory for every solver class
    for cls in (g.Cg, g.Gmres, g.Bicgstab, g.Fcg, g.Ir):
        assert cls.build().with_preconditioner(g.Multigrid.build()).preconditioner.cls is g.Multigrid
