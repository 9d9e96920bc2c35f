"""Device buffers for the tests that call gkoc_* entry points directly (tests/test_idr_gpu.py,
test_cb_gmres_gpu.py, test_dense_gpu.py): any numpy dtype travels as bytes, strided operands are cut out of
a padded array whose padding keeps a canary."""
import ctypes as C

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
