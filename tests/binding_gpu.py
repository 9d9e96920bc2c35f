"""Device buffers for the tests that call gkoc_* entry points directly (tests/test_idr_gpu.py,
test_cb_gmres_gpu.py, test_dense_gpu.py, test_csr_struct_gpu.py, test_csr_diag_gpu.py, test_dist_partition_gpu.py, test_dist_index_gpu.py,
test_cdense_gpu.py, test_format_helpers_gpu.py, test_array_components_gpu.py, test_format_spmv_gpu.py,
test_format_setup_gpu.py): any numpy dtype
travels as bytes, strided operands are cut out of a padded array whose padding keeps a canary, flat outputs
are followed by one."""
import ctypes as C
import os
import re

import numpy as np

CANARY = -777.25


class Dev:
    """device copy of a numpy array (uploaded and read back as raw bytes, so uint16 / uint64 / float16 /
    complex work alike); pass it to ginkgo_amd._lib.call, or `at(i)` for a pointer i elements in"""

    def __init__(self, gexec, a):
        import torch
        a = np.ascontiguousarray(a)
        self.dtype, self.shape, self.nbytes = a.dtype, a.shape, a.nbytes
        raw = np.zeros(max(a.nbytes, 64), np.uint8)
        raw[:a.nbytes] = a.reshape(-1).view(np.uint8)
        self.t = torch.from_numpy(raw).to(gexec.device)
        self._as_parameter_ = C.c_void_p(self.t.data_ptr())

    def at(self, i):
        return C.c_void_p(self.t.data_ptr() + int(i) * self.dtype.itemsize)

    def get(self):
        raw = self.t.cpu().numpy()[:self.nbytes]
        return raw.view(self.dtype).reshape(self.shape).copy()


def padded(a, ld=None, canary=CANARY):
    """rows x ld array holding a in its first columns, the canary in the rest"""
    a = np.asarray(a)
    ld = a.shape[1] + 3 if ld is None else ld
    out = np.full((a.shape[0], ld), canary, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def sync():
    import torch
    torch.cuda.synchronize()


def call(name, *args):
    from ginkgo_amd._lib import call as lib_call
    lib_call(name, *args)


class DevCsr:
    """a Csr matrix (or pattern) on the device in index type it, with the host arrays it was made from"""

    def __init__(self, gexec, it, ptrs, cols, vals=None):
        self.host = [np.asarray(ptrs).astype(it), np.asarray(cols).astype(it)] + \
            ([np.ascontiguousarray(vals)] if vals is not None else [])
        self.dev = [Dev(gexec, h) for h in self.host]

    def unchanged(self):
        return all(same_bits(d.get(), h) for d, h in zip(self.dev, self.host))


def out_buf(gexec, n, t, fill=np.nan, tail=3):
    """device array of n entries `fill` followed by `tail` canaries"""
    a = np.full(n + tail, fill, t)
    a[n:] = CANARY
    return Dev(gexec, a)


def tail_ok(got, n):
    return np.all(got[n:] == got.dtype.type(CANARY))


def grid_cap_rows():
    """256 * 4 * max_stream_blocks (csrc/common.hpp): the number of threads the capped launchers start"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "ginkgo_amd", "csrc", "common.hpp")).read()
    return 256 * 4 * int(re.search(r"constexpr\s+int\s+max_stream_blocks\s*=\s*(\d+)\s*;", text).group(1))


SENTINEL = -99


def head_of(out, n, k, fill=SENTINEL):
    """the first k entries of an out_buf of n entries, after checking that entries k .. n still hold `fill`
    bit for bit and that the canaries behind them are intact"""
    got = out.get()
    assert tail_ok(got, n)
    assert same_bits(got[k:n], np.full(n - k, fill, got.dtype)), "written beyond what the operation defines"
    return got[:k]


class _C128(C.Structure):
    _fields_ = [("re", C.c_double), ("im", C.c_double)]


class _C64(C.Structure):
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


def by_value(v):
    """a numpy scalar as the ctypes object that passes it BY VALUE with its bits intact (NaN payloads
    included): float32 / float64 / int32 / int64 / gkoc_c64 / gkoc_c128"""
    a = np.ascontiguousarray(v).reshape(1)
    ct = {"float64": C.c_double, "float32": C.c_float, "int32": C.c_int32, "int64": C.c_int64,
          "complex128": _C128, "complex64": _C64}[a.dtype.name]
    return ct.from_buffer_copy(a.tobytes())


def canaries_ok(a, cols):
    """the padding columns of a `padded` array still hold the canary"""
    return bool(np.all(a[:, cols:] == a.dtype.type(CANARY)))


def raises_invalid(name, *args):
    """the call is refused with GKOC_E_INVALID (-1) before any launch"""
    import re
    from ginkgo_amd._lib import GkoError
    try:
        call(name, *args)
    except GkoError as e:
        m = re.search(r"failed with status (-?\d+):", str(e))
        return m is not None and int(m.group(1)) == -1
    return False


class PartitionStruct(C.Structure):
    """gkoc_partition of include/gko_cdna4.h: a host struct of device pointers"""
    _fields_ = [("num_ranges", C.c_int64), ("num_parts", C.c_int32), ("range_bounds", C.c_void_p),
                ("part_ids", C.c_void_p), ("range_starting_indices", C.c_void_p), ("part_sizes", C.c_void_p)]


class DevPartition:
    """a partition (bounds, pids, starts, sizes, num_parts on the host) on the device with local index type
    lt and global index type gt; `ref` is what a const gkoc_partition* parameter takes"""

    def __init__(self, gexec, lt, gt, part):
        assert part.bounds.max(initial=0) <= np.iinfo(gt).max and part.sizes.max(initial=0) <= np.iinfo(lt).max
        self.host = [part.bounds.astype(gt), part.pids.astype(np.int32), part.starts.astype(lt),
                     part.sizes.astype(lt)]
        self.dev = [Dev(gexec, h) for h in self.host]
        self.struct = PartitionStruct(len(part.pids), part.num_parts, *[d.t.data_ptr() for d in self.dev])
        self.ref = C.byref(self.struct)

    def unchanged(self):
        return all(same_bits(d.get(), h) for d, h in zip(self.dev, self.host))
