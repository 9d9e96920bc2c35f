"""The classes of the CSR column-offset plan (csrc/csr_offsets.hpp, "kept BY CLASS") restated in numpy, and the
matrices of tests/test_csr_offsets_classes_cases_cpu.py and tests/test_csr_offsets_classes_gpu.py.

The class key of a 64-row segment is its 33 table words (D, the offsets padded with zeros to 32) followed by its 64
mask words (0 for a row at or behind n_rows, and for every row of a segment that is not eligible); two segments are
in one class iff the 97 words are equal.  Nothing here needs a device.
"""
import numpy as np

import csr_offsets_cases as oc

KEY_HASH_BITS = 19         # GKOC_TUNE_CSR_OFFSETS_HASH_BITS
CLASS_BYTES = (oc.OFFS_MAX + 1 + oc.SEG) * 4       # a table and 64 masks


def class_keys(rp, ci):
    """one tuple of 97 words per segment, from plan_model"""
    model = oc.plan_model(rp, ci)
    n_rows = len(rp) - 1
    keys = []
    for s in range(model.segments):
        tab = [model.D[s]] + list(model.offsets[s]) + [0] * (oc.OFFS_MAX - len(model.offsets[s]))
        masks = [int(model.mask[r]) if r < n_rows else 0 for r in range(s * oc.SEG, (s + 1) * oc.SEG)]
        assert len(tab) == oc.OFFS_MAX + 1 and len(masks) == oc.SEG
        keys.append(tuple(tab + masks))
    return keys


def class_count(rp, ci):
    return len(set(class_keys(rp, ci)))


def class_ids(rp, ci):
    """the segments' classes, numbered by first appearance (a numbering of its own: only equality matters)"""
    seen = {}
    return [seen.setdefault(k, len(seen)) for k in class_keys(rp, ci)]


def class_count_all_collide(rp, ci):
    """with the hash cut to 0 bits every segment's leader is segment 0: what equals it joins its class, every
    other segment is a class of its own"""
    keys = class_keys(rp, ci)
    return 1 + sum(1 for k in keys[1:] if k != keys[0])


def plan_bytes(rp, ci, n_classes):
    model = oc.plan_model(rp, ci)
    skip = 0 if model.eligible == model.segments else 4 * -(-model.segments // 32)
    return 4 * model.segments + CLASS_BYTES * n_classes + skip


# ---------------------------------------------------------------- matrices (host, int32)
def stencil27(oracle, g, dtype=np.float64, seed=0):
    rp, ci, v = oracle.stencil_csr(3, g)
    rng = np.random.default_rng(seed)
    v = (v * rng.uniform(0.5, 1.5, len(v))).astype(dtype)
    return (g ** 3, g ** 3), rp, ci, v


def tridiagonal(dtype=np.float64, hole=False):
    """256 x 256, four segments: the first lacks the entry left of row 0 and the last the one right of row 255,
    the two in the middle are equal: 3 classes.  hole: row 140 (segment 2) loses its upper off-diagonal entry - the
    same offsets, another mask: 4 classes."""
    rows = oc.band_rows(256, 256, (-1, 0, 1))
    if hole:
        rows[140] = [139, 140]
    return oc.from_rows(rows, 256, dtype, seed=256 + hole)


def two_bands(dtype=np.float64):
    """384 x 384, six segments, offsets {-1, 0, 1} in the even and {-2, 0, 2} in the odd ones.  The rows in the
    middle of the matrix store all three, so segments 1 .. 4 have EQUAL masks (7 in every row) and differ in their
    offsets alone: segments 2 and 4 share a class, 1 and 3 share another, and the two must not be merged; the first
    and the last segment lose entries at the matrix' edge: 4 classes."""
    rows = []
    for s in range(6):
        rows += oc.band_rows(64, 384, (-1, 0, 1) if s % 2 == 0 else (-2, 0, 2), first=64 * s)
    return oc.from_rows(rows, 384, dtype, seed=384)


def one_unsorted_row(dtype=np.float64):
    """320 x 320 tridiagonal, five segments; row 150 (segment 2) is not sorted, so segment 2 is not eligible and is
    a class of its own (D = 0, masks 0) beside first / middle / last: 4 classes, 4 of 5 segments eligible"""
    rows = oc.band_rows(320, 320, (-1, 0, 1))
    rows[150] = [151, 149, 150]
    return oc.from_rows(rows, 320, dtype, seed=320)


# name -> (builder(oracle, dtype), classes): the class counts are what the definition gives, pinned by the CPU file
CASES = {
    "27pt-8": (lambda oracle, dtype: stencil27(oracle, 8, dtype), 3),
    "27pt-12": (lambda oracle, dtype: stencil27(oracle, 12, dtype), 14),
    "27pt-5": (lambda oracle, dtype: stencil27(oracle, 5, dtype), 2),
    "27pt-7": (lambda oracle, dtype: stencil27(oracle, 7, dtype), 6),
    "tri-256": (lambda oracle, dtype: tridiagonal(dtype), 3),
    "tri-256-hole": (lambda oracle, dtype: tridiagonal(dtype, hole=True), 4),
    "two-bands": (lambda oracle, dtype: two_bands(dtype), 4),
    "unsorted-row": (lambda oracle, dtype: one_unsorted_row(dtype), 4),
}
