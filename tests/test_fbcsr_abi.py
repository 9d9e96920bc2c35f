"""CPU-side checks of the Fbcsr (fixed-block CSR) entries of libgko_cdna4.so: they are
exported, and bad block sizes, sizes not divisible by the block size and null arrays are
refused before any HIP call - so these run on a machine without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

GKOC_E_INVALID, GKOC_E_NOT_SUPPORTED = -1, -2
SUFFIXES = [f"{v}_{i}" for v in ("f64", "f32") for i in ("i32", "i64")]
ENTRIES = ["gkoc_fbcsr_spmv", "gkoc_fbcsr_advanced_spmv", "gkoc_csr_convert_to_fbcsr",
           "gkoc_fbcsr_convert_to_csr", "gkoc_fbcsr_fill_in_dense", "gkoc_fbcsr_extract_diagonal",
           "gkoc_fbcsr_is_sorted_by_column_index"]


@pytest.fixture(scope="module")
def lib():
    import ginkgo_amd as g
    assert os.path.exists(g.LIB_PATH), "run __graft_entry__.build() first"
    return C.CDLL(g.LIB_PATH)


def i64(v):
    return C.c_int64(v)


DUMMY = C.c_void_p(16)     # never dereferenced: every call below fails its argument check


def test_fbcsr_entries_are_exported():
    import ginkgo_amd as g
    out = subprocess.run(["nm", "-D", "--defined-only", g.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    want = [f"{e}_{s}" for e in ENTRIES for s in SUFFIXES]
    want += ["gkoc_csr_convert_to_fbcsr_row_ptrs_i32", "gkoc_csr_convert_to_fbcsr_row_ptrs_i64"]
    missing = [w for w in want if f" T {w}\n" not in out + "\n"]
    assert not missing, missing


def test_python_class_is_exported():
    import ginkgo_amd as g
    assert "Fbcsr" in g.__all__ and g.Fbcsr.MAX_BLOCK_SIZE == 8


@pytest.mark.parametrize("suf", SUFFIXES)
@pytest.mark.parametrize("bs,code", [(0, GKOC_E_INVALID), (-3, GKOC_E_INVALID),
                                     (9, GKOC_E_NOT_SUPPORTED), (16, GKOC_E_NOT_SUPPORTED)])
def test_bad_block_size_is_refused(lib, suf, bs, code):
    f = getattr(lib, "gkoc_fbcsr_spmv_" + suf)
    assert f(None, i64(2), i64(2), i64(bs), DUMMY, DUMMY, DUMMY, DUMMY, i64(1), DUMMY, i64(1),
             i64(1)) == code
    f = getattr(lib, "gkoc_fbcsr_advanced_spmv_" + suf)
    assert f(None, i64(2), i64(2), i64(bs), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, i64(1), DUMMY,
             DUMMY, i64(1), i64(1)) == code
    f = getattr(lib, "gkoc_csr_convert_to_fbcsr_" + suf)
    assert f(None, i64(6), i64(6), i64(bs), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY) == code
    f = getattr(lib, "gkoc_fbcsr_convert_to_csr_" + suf)
    assert f(None, i64(2), i64(bs), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY) == code
    f = getattr(lib, "gkoc_fbcsr_fill_in_dense_" + suf)
    assert f(None, i64(2), i64(2), i64(bs), DUMMY, DUMMY, DUMMY, DUMMY, i64(6)) == code
    f = getattr(lib, "gkoc_fbcsr_extract_diagonal_" + suf)
    assert f(None, i64(6), i64(6), i64(bs), DUMMY, DUMMY, DUMMY, DUMMY) == code
    it = suf.split("_")[1]
    n = C.c_int64(-7)
    f = getattr(lib, "gkoc_csr_convert_to_fbcsr_row_ptrs_" + it)
    assert f(None, i64(6), i64(6), i64(bs), DUMMY, DUMMY, DUMMY, C.byref(n)) == code


@pytest.mark.parametrize("suf", SUFFIXES)
@pytest.mark.parametrize("rows,cols", [(7, 6), (6, 7), (5, 5)])
def test_sizes_not_divisible_by_the_block_size_are_refused(lib, suf, rows, cols):
    f = getattr(lib, "gkoc_csr_convert_to_fbcsr_" + suf)
    assert f(None, i64(rows), i64(cols), i64(3), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY,
             DUMMY) == GKOC_E_INVALID
    f = getattr(lib, "gkoc_fbcsr_extract_diagonal_" + suf)
    assert f(None, i64(rows), i64(cols), i64(3), DUMMY, DUMMY, DUMMY, DUMMY) == GKOC_E_INVALID
    n = C.c_int64(-7)
    f = getattr(lib, "gkoc_csr_convert_to_fbcsr_row_ptrs_" + suf.split("_")[1])
    assert f(None, i64(rows), i64(cols), i64(3), DUMMY, DUMMY, DUMMY, C.byref(n)) == GKOC_E_INVALID
    assert n.value == -7          # refused before anything was written


@pytest.mark.parametrize("suf", SUFFIXES)
def test_null_arrays_with_work_are_refused(lib, suf):
    f = getattr(lib, "gkoc_fbcsr_spmv_" + suf)
    # row pointers, b, c missing for a 2-block-row product
    assert f(None, i64(2), i64(2), i64(3), None, DUMMY, DUMMY, DUMMY, i64(1), DUMMY, i64(1),
             i64(1)) == GKOC_E_INVALID
    assert f(None, i64(2), i64(2), i64(3), DUMMY, DUMMY, DUMMY, None, i64(1), DUMMY, i64(1),
             i64(1)) == GKOC_E_INVALID
    assert f(None, i64(2), i64(2), i64(3), DUMMY, DUMMY, DUMMY, DUMMY, i64(1), None, i64(1),
             i64(1)) == GKOC_E_INVALID
    # strides below the number of right-hand sides, negative sizes
    assert f(None, i64(2), i64(2), i64(3), DUMMY, DUMMY, DUMMY, DUMMY, i64(1), DUMMY, i64(3),
             i64(3)) == GKOC_E_INVALID
    assert f(None, i64(-1), i64(2), i64(3), DUMMY, DUMMY, DUMMY, DUMMY, i64(1), DUMMY, i64(1),
             i64(1)) == GKOC_E_INVALID
    f = getattr(lib, "gkoc_fbcsr_advanced_spmv_" + suf)
    # alpha / beta missing
    assert f(None, i64(2), i64(2), i64(3), None, DUMMY, DUMMY, DUMMY, DUMMY, i64(1), DUMMY,
             DUMMY, i64(1), i64(1)) == GKOC_E_INVALID
    assert f(None, i64(2), i64(2), i64(3), DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, i64(1), None,
             DUMMY, i64(1), i64(1)) == GKOC_E_INVALID
    f = getattr(lib, "gkoc_fbcsr_is_sorted_by_column_index_" + suf)
    assert f(None, i64(2), DUMMY, DUMMY, None) == GKOC_E_INVALID
    f = getattr(lib, "gkoc_fbcsr_convert_to_csr_" + suf)
    assert f(None, i64(2), i64(3), DUMMY, DUMMY, DUMMY, None, DUMMY, DUMMY) == GKOC_E_INVALID
    f = getattr(lib, "gkoc_fbcsr_fill_in_dense_" + suf)
    # a row stride that does not cover the 2 x 3 columns would write past the rows
    assert f(None, i64(2), i64(2), i64(3), DUMMY, DUMMY, DUMMY, DUMMY, i64(5)) == GKOC_E_INVALID
    assert f(None, i64(2), i64(2), i64(3), DUMMY, DUMMY, DUMMY, None, i64(6)) == GKOC_E_INVALID


def test_python_refuses_before_the_device():
    """the block-size and divisibility checks of the Python class run before any array
    is touched (Fbcsr.__init__ / Csr.convert_to_fbcsr share them)"""
    import ginkgo_amd as g
    from ginkgo_amd import matrix
    with pytest.raises(g.NotSupported):
        matrix._fbcsr_check_block_size(9, (18, 18))
    with pytest.raises(g.DimensionMismatch):
        matrix._fbcsr_check_block_size(3, (7, 6))
    with pytest.raises(g.GkoError):
        matrix._fbcsr_check_block_size(0, (6, 6))
    assert matrix._fbcsr_check_block_size(4, (8, 12)) == 4
