"""What of the ILU(0) / IC(0) feature can be checked without a device: the C ABI declares and the library
exports its entry points, the split entries keep the column-offset plan's contract by writing no index array,
the path limits are reported by a host-only call, and the package exposes the classes."""
import ctypes as C
import re
import subprocess

import pytest

import ginkgo_amd as g
from test_abi import HEADER, declared_symbols

TYPES = ["f64_i32", "f64_i64", "f32_i32", "f32_i64"]
STEMS = ["gkoc_ilu_factorize_", "gkoc_ic_factorize_", "gkoc_factorization_initialize_l_u_",
         "gkoc_factorization_initialize_l_"]


def test_entry_points_are_declared_and_exported():
    declared = set(declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (gkoc_\w+)", out))
    for name in [s + t for s in STEMS for t in TYPES] + ["gkoc_factorization_row_limits"]:
        assert name in declared and name in exported, name


def test_split_entries_take_no_index_output():
    """they write values only: an entry that wrote col_idxs would have to notify the column-offset plan"""
    pre = subprocess.run(["gcc", "-E", "-P", HEADER], capture_output=True, text=True, check=True).stdout
    for stem in STEMS:
        m = re.search(stem + r"f64_i32\s*\(([^)]*)\)", pre)
        assert m, stem
        params = [p.strip() for p in m.group(1).split(",")]
        assert not [p for p in params if re.match(r"^int(32|64)_t\s*\*", p)], (stem, params)
        assert [p for p in params if re.match(r"^double\s*\*", p)], stem


def test_row_limits_are_reported_without_a_device():
    limits = g.factorization.row_limits()
    assert 1 <= len(limits) <= 4 and limits == sorted(set(limits)) and all(0 < x <= 64 for x in limits)
    from ginkgo_amd._lib import call
    with pytest.raises(g.GkoError):
        call("gkoc_factorization_row_limits", None, C.byref(C.c_int(0)))


def test_package_exposes_the_classes():
    for cls in (g.factorization.Ilu, g.factorization.Ic, g.Ilu, g.Ic):
        assert callable(cls.build)
    assert g.Ilu is not g.factorization.Ilu and g.Ic is not g.factorization.Ic
    assert g.Ilu.build().with_reverse_apply(True).reverse_apply is True
    assert g.factorization.Ic.build().with_both_factors(False).both_factors is False
    assert g.factorization.Ilu.build().with_skip_sorting(True).skip_sorting is True
    assert {"Ilu", "Ic", "factorization"} <= set(g.__all__)
