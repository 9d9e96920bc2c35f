"""What of the general / spd ISAI feature can be checked without a device: the C ABI declares and the library
exports its entry points, the generate entry takes every index array as const (so the column-offset plan's
contract gains no writer), the path limits are reported by a host-only call, null pointers are refused before
anything touches the device, and the package exposes the classes with the factory's setters."""
import ctypes as C
import re
import subprocess

import pytest

import ginkgo_amd as g
from ginkgo_amd._lib import call
from test_abi import HEADER, declared_symbols

TYPES = ["f64_i32", "f64_i64", "f32_i32", "f32_i64"]
STEM = "gkoc_isai_generate_general_inverse_"
GKOC_OK, GKOC_E_INVALID = 0, -1        # include/gko_cdna4.h


def test_entry_points_are_declared_and_exported():
    declared = set(declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (gkoc_\w+)", out))
    for name in [STEM + t for t in TYPES] + ["gkoc_isai_general_row_limits"]:
        assert name in declared and name in exported, name


def test_generate_general_inverse_takes_no_index_output():
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
    limits = g.isai.general_row_limits()
    assert 1 <= len(limits) <= 4 and limits == sorted(set(limits))
    assert limits[0] >= 8 and limits[-1] >= 128 and 64 in limits
    with pytest.raises(g.GkoError):
        call("gkoc_isai_general_row_limits", None, C.byref(C.c_int(0)))
    with pytest.raises(g.GkoError):
        call("gkoc_isai_general_row_limits", (C.c_int * 4)(), None)
    # the triangular entry keeps its own limits: it has no cap to report
    assert max(g.isai.row_limits()) <= 64 < limits[-1]


@pytest.mark.parametrize("suffix", TYPES)
def test_null_pointers_are_invalid_before_any_device_work(suffix):
    fn = getattr(g._lib.lib(), STEM + suffix)
    fn.restype = C.c_int
    index = C.c_int32 if suffix.endswith("i32") else C.c_int64
    value = C.c_double if suffix.startswith("f64") else C.c_float
    rp, ci, v = (index * 2)(0, 1), (index * 1)(0), (value * 1)(1.0)
    good = [rp, ci, v, rp, ci, v]
    for spd in (0, 1):
        for k in range(6):
            args = [C.cast(x, C.c_void_p) for x in good]
            args[k] = C.c_void_p(None)
            assert fn(C.c_void_p(None), C.c_int64(1), C.c_int(spd), *args) == GKOC_E_INVALID, (spd, k)
        assert fn(C.c_void_p(None), C.c_int64(-1), C.c_int(spd), *[C.cast(x, C.c_void_p) for x in good]) \
            == GKOC_E_INVALID
        assert fn(C.c_void_p(None), C.c_int64(0), C.c_int(spd), *[C.c_void_p(None)] * 6) == GKOC_OK
    assert v[0] == 1.0


def test_package_exposes_the_classes_and_the_setters():
    assert {"GeneralIsai", "SpdIsai", "LowerIsai", "UpperIsai"} <= set(g.__all__)
    for cls in (g.GeneralIsai, g.SpdIsai):
        assert issubclass(cls, g.base.LinOp)
        f = cls.build()
        assert f.cls is cls and f.sparsity_power == 1 and f.skip_sorting is False
        assert f.with_sparsity_power(3).sparsity_power == 3 and f.with_skip_sorting(True).skip_sorting is True
        # accepted, without effect
        assert f.with_excess_limit(7).with_excess_solver_reduction(1e-3).with_excess_solver_factory(None) is f
        assert f.with_skip_sorting(False).with_sparsity_power(2).on(None) is f
    assert g.Cg.build().with_preconditioner(g.SpdIsai.build()) is not None
