"""What of the triangular ISAI feature can be checked without a device: the C ABI declares and the library
exports its entry points, generate_tri_inverse keeps the column-offset plan's contract by taking every index
array as const, the path limits are reported by a host-only call, and the package exposes the classes and the
new solver setters of Ilu / Ic."""
import ctypes as C
import re
import subprocess

import pytest

import ginkgo_amd as g
from test_abi import HEADER, declared_symbols

TYPES = ["f64_i32", "f64_i64", "f32_i32", "f32_i64"]
STEM = "gkoc_isai_generate_tri_inverse_"


def test_entry_points_are_declared_and_exported():
    declared = set(declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (gkoc_\w+)", out))
    for name in [STEM + t for t in TYPES] + ["gkoc_isai_row_limits"]:
        assert name in declared and name in exported, name


def test_generate_tri_inverse_takes_no_index_output():
    """it writes values only: an entry that wrote col_idxs would have to notify the column-offset plan"""
    pre = subprocess.run(["gcc", "-E", "-P", HEADER], capture_output=True, text=True, check=True).stdout
    for suffix, value, index in (("f64_i32", "double", "int32_t"), ("f32_i64", "float", "int64_t")):
        m = re.search(STEM + suffix + r"\s*\(([^)]*)\)", pre)
        assert m, suffix
        params = [p.strip() for p in m.group(1).split(",")]
        assert not [p for p in params if re.match(r"^int(32|64)_t\s*\*", p)], params
        assert len([p for p in params if re.match(r"^const\s+%s\s*\*" % index, p)]) == 4, params
        assert len([p for p in params if re.match(r"^%s\s*\*" % value, p)]) == 1, params


def test_row_limits_are_reported_without_a_device():
    limits = g.isai.row_limits()
    assert 1 <= len(limits) <= 4 and limits == sorted(set(limits)) and all(8 <= x <= 64 for x in limits)
    from ginkgo_amd._lib import call
    with pytest.raises(g.GkoError):
        call("gkoc_isai_row_limits", None, C.byref(C.c_int(0)))
    with pytest.raises(g.GkoError):
        call("gkoc_isai_row_limits", (C.c_int * 4)(), None)


def test_package_exposes_the_classes_and_the_setters():
    assert {"LowerIsai", "UpperIsai"} <= set(g.__all__)
    for cls in (g.LowerIsai, g.UpperIsai):
        assert issubclass(cls, g.base.LinOp)
        f = cls.build()
        assert f.sparsity_power == 1 and f.skip_sorting is False
        assert f.with_sparsity_power(3).sparsity_power == 3 and f.with_skip_sorting(True).skip_sorting is True
        # accepted, without effect
        assert f.with_excess_limit(7).with_excess_solver_reduction(1e-3).with_excess_solver_factory(None) is f
    lower, upper = g.LowerIsai.build().with_sparsity_power(2), g.UpperIsai.build()
    f = g.Ilu.build().with_l_solver(lower).with_u_solver(upper)
    assert f.l_solver is lower and f.u_solver is upper
    assert g.Ic.build().with_l_solver(lower).l_solver is lower
    assert g.Ilu.build().l_solver is None and g.Ilu.build().u_solver is None and g.Ic.build().l_solver is None
    assert not hasattr(g.Ic.build(), "with_u_solver")
