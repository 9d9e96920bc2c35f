"""The column-offset plan kept by class (csrc/csr_offsets.hpp, the plan code of csrc/csr_structure.hip): segments whose
33 table words and 64 mask words are equal share one entry of the class tables.

Every case goes through check_all_modes of tests/csr_offsets_cases.py - bit for bit against the sequential oracle and
against the row-segment kernel (GKOC_TUNE_CSR_OFFSETS = 2), plain / advanced / beta = 0 / fused dot, in double and
float, with one and two segments per wave - and the number of classes the library reports (gkoc_csr_plan_classes)
must be the one of the numpy restatement of the definition (tests/csr_offsets_classes_cases.py, itself checked by
tests/test_csr_offsets_classes_cases_cpu.py).  With the hash cut to a few bits (GKOC_TUNE_CSR_OFFSETS_HASH_BITS)
unequal segments collide: the bits must stay and the classes may only get more.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import csr_offsets_cases as oc
import csr_offsets_classes_cases as cc
from csr_offsets_cases import KEY_SEGS_PER_WAVE, arena_csr, bits, check_all_modes, key, plain, plan_info, plan_info_at

pytestmark = pytest.mark.gpu


def plan_classes(a):
    from ginkgo_amd import _lib
    n = C.c_uint64(0)
    _lib.call("gkoc_csr_plan_classes", C.c_void_p(a.row_ptrs.data_ptr()), C.c_void_p(a.col_idxs.data_ptr()),
              C.byref(n))
    return n.value


# ---------------------------------------------------------------- 1. the cases
@pytest.mark.parametrize("spw", [1, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_cases(gexec, oracle, name, dtype, spw):
    """whole segments (27-point 8^3, 12^3), a last segment of 61 / 23 rows (5^3, 7^3), equal offsets with other
    masks, equal masks with other offsets, a segment that is not eligible (it stays with the row-segment kernel,
    the plan is in use)"""
    build, classes = cc.CASES[name]
    m = build(oracle, np.dtype(dtype))
    with key(spw, KEY_SEGS_PER_WAVE):
        a = check_all_modes(gexec, oracle, m)
    info = plan_info(a)
    assert info["state"] == 1, info
    got = plan_classes(a)
    assert got == classes == cc.class_count(m[1], m[2]), (got, classes)
    assert info["bytes"] == cc.plan_bytes(m[1], m[2], got), info


# ---------------------------------------------------------------- 2. hash collisions
@pytest.mark.parametrize("hash_bits", [0, 1])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["27pt-8", "tri-256"])
def test_hash_collisions(gexec, oracle, name, dtype, hash_bits):
    """a member of a run of equal hashes joins its leader's class only if all 97 words are equal.  0 bits: every
    segment's leader is segment 0, and every segment that differs from it is a class of its own; 1 bit: two runs"""
    build, classes = cc.CASES[name]
    m = build(oracle, np.dtype(dtype))
    with key(hash_bits, cc.KEY_HASH_BITS):
        a = check_all_modes(gexec, oracle, m)
        with key(2, KEY_SEGS_PER_WAVE):
            a2 = check_all_modes(gexec, oracle, m)
    for mat in (a, a2):
        info = plan_info(mat)
        got = plan_classes(mat)
        assert info["state"] == 1 and classes <= got <= info["segments"], (info, got)
        if hash_bits == 0:
            assert got == cc.class_count_all_collide(m[1], m[2]), got
        assert info["bytes"] == cc.plan_bytes(m[1], m[2], got), info


# ---------------------------------------------------------------- 3. what the plan holds
def test_plan_bytes(gexec, oracle):
    """4 bytes a segment and 388 a class on the stencil 12^3 (27 segments, 14 classes); the skip bits on top where
    a segment is not eligible"""
    m = cc.stencil27(oracle, 12)
    a = check_all_modes(gexec, oracle, m, modes=("plain",))
    info = plan_info(a)
    assert plan_classes(a) == 14 and info["segments"] == 27
    assert info["bytes"] == 4 * 27 + 388 * 14, info
    m = cc.one_unsorted_row()
    a = check_all_modes(gexec, oracle, m, modes=("plain",))
    assert plan_classes(a) == 4 and plan_info(a)["bytes"] == 4 * 5 + 388 * 4 + 4, plan_info(a)


def test_no_plan_no_classes(gexec, oracle):
    """arrays without a plan in use report 0 classes: never seen, and built under key 2"""
    m = cc.tridiagonal()
    a = arena_csr(gexec, *m)
    assert plan_classes(a) == 0
    b = np.random.default_rng(3).uniform(-1, 1, m[0][1])
    with key(2):
        plain(gexec, a, b)
    assert plan_info(a)["state"] == -1 and plan_classes(a) == 0


# ---------------------------------------------------------------- 4. release
def _allocations(ex):
    gc.collect()
    ex.synchronize()
    return ex.arena_info()["num_allocations"]


@pytest.mark.parametrize("name,buffers", [("tri-256", 3), ("unsorted-row", 4)])
@pytest.mark.parametrize("how", ["free", "structure_changed"])
def test_release(gexec, oracle, how, name, buffers):
    """a plan in use holds the class ids, the class tables, the class masks (and the skip bits where a segment is
    not eligible); the per-segment tables, the per-row masks and the scratch of the class search are gone when the
    product returns, and the rest when the plan is dropped"""
    m = cc.CASES[name][0](oracle, np.dtype(np.float64))
    b = np.random.default_rng(4).uniform(-1, 1, m[0][1])
    ref = oracle.csr_spmv(m[1], m[2], m[3], b)

    def round_():
        empty = _allocations(gexec)
        a = arena_csr(gexec, *m)
        with key(2):
            plain(gexec, a, b)          # (what a first product sets up beside the plan)
        before = _allocations(gexec)
        with key(1):
            assert np.array_equal(bits(plain(gexec, a, b)), bits(ref))
        assert plan_info(a)["state"] == 1 and plan_classes(a) == cc.CASES[name][1]
        assert _allocations(gexec) == before + buffers
        if how == "structure_changed":
            a.structure_changed()
            assert plan_info(a)["state"] == -1 and plan_classes(a) == 0
            assert _allocations(gexec) == before
        old = (a.row_ptrs.data_ptr(), a.col_idxs.data_ptr())
        del a
        assert _allocations(gexec) == empty
        assert plan_info_at(*old)["state"] == -1

    warm = arena_csr(gexec, *m)     # (a first plan and its release: what the library keeps per stream)
    with key(1):
        plain(gexec, warm, b)
    del warm
    round_()
