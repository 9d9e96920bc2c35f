"""Fbcsr (fixed-block CSR) on the device: block SpMV bit-identical to the CSR reference loop
on the expanded matrix (entries of a scalar row in block order, then by column inside the
block), the conversions against scipy's BSR, and the Flan-like stand-in of configs[4]
(L27 (x) B3, dense 3 x 3 blocks) as the system matrix of CG + block-Jacobi(3).
Expected values come from the CSR expansion built in numpy here and the C reference loop."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

B3 = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 2.0]])


def flan_like(oracle, g):
    rp, ci, v = oracle.stencil_csr(3, g)
    n = g ** 3
    l27 = sp.csr_matrix((v, ci, rp), shape=(n, n))
    a = sp.kron(l27, sp.csr_matrix(B3), format="csr")
    a.sort_indices()
    return a, l27


def expand(rp, cols, vals, bs):
    """the scalar CSR of a block matrix, every row in block order, then column in block"""
    nbr = len(rp) - 1
    out_rp, out_c, out_v = [0], [], []
    blocks = vals.reshape(-1, bs, bs)          # [k, j, i] (column-major blocks)
    for br in range(nbr):
        k0, k1 = int(rp[br]), int(rp[br + 1])
        c = (cols[k0:k1].astype(np.int64)[:, None] * bs + np.arange(bs)[None, :]).reshape(-1)
        for i in range(bs):
            out_c.append(c)
            out_v.append(blocks[k0:k1, :, i].reshape(-1))
            out_rp.append(out_rp[-1] + c.size)
    idt = cols.dtype
    cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt))
    return np.asarray(out_rp, idt), cat(out_c, idt), cat(out_v, vals.dtype)


def to_dense(rp, cols, vals, bs, shape):
    a = np.zeros(shape, vals.dtype)
    blocks = vals.reshape(-1, bs, bs)
    for br in range(len(rp) - 1):
        for k in range(rp[br], rp[br + 1]):
            a[br * bs:(br + 1) * bs, cols[k] * bs:(cols[k] + 1) * bs] += blocks[k].T
    return a


def random_blocks(rng, nbr, nbc, bs, per_row, dtype, idt, ordered=True, empty=()):
    counts = rng.integers(1, per_row + 1, nbr)
    counts[list(empty)] = 0
    cols = []
    for br in range(nbr):
        c = rng.choice(nbc, size=min(int(counts[br]), nbc), replace=False)
        cols.append(np.sort(c) if ordered else c)
    rp = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(idt)
    ci = np.concatenate(cols).astype(idt)
    vals = rng.uniform(-1, 1, int(rp[-1]) * bs * bs).astype(dtype)
    return rp, ci, vals


def dense_on(gexec, arr, stride=None):
    import ginkgo_amd as g
    return g.Dense.from_numpy(gexec, np.ascontiguousarray(arr), stride=stride)


def check_products(gexec, oracle, fb, rp, ci, v, bs, shape, nrhs, strided, seed):
    """apply and both advanced forms of `fb` against the reference loop on the expansion"""
    import ginkgo_amd as g
    dt = v.dtype
    tdt = torch.float64 if dt == np.float64 else torch.float32
    erp, eci, ev = expand(rp, ci, v, bs)
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1, 1, (shape[1], nrhs)).astype(dt)
    c0 = rng.uniform(-1, 1, (shape[0], nrhs)).astype(dt)
    sb = nrhs + 3 if strided else None
    sx = nrhs + 2 if strided else None
    x = g.Dense.create(gexec, (shape[0], nrhs), tdt, stride=sx)
    fb.apply(dense_on(gexec, b, sb), x)
    assert np.array_equal(x.to_numpy(), oracle.csr_spmv(erp, eci, ev, b))
    for alpha, beta in ((-1.0, 2.0), (0.75, 0.0)):
        x = dense_on(gexec, c0 if beta != 0 else np.full_like(c0, np.nan), sx)
        fb.apply(g.scalar(gexec, alpha, tdt), dense_on(gexec, b, sb), g.scalar(gexec, beta, tdt), x)
        ref = oracle.csr_spmv(erp, eci, ev, b, alpha=alpha, beta=beta, c=c0)
        assert np.array_equal(x.to_numpy(), ref), (alpha, beta)


def test_known_answers(gexec):
    import ginkgo_amd as g
    # 6 x 6 Fbcsr<2>: block rows {0: cols 0, 2}, {1: col 1}, {2: cols 0, 2}; blocks column-major
    rp = np.array([0, 2, 3, 5], np.int32)
    ci = np.array([0, 2, 1, 0, 2], np.int32)
    v = np.arange(1, 21, dtype=np.float64)
    a = np.array([[1, 3, 0, 0, 5, 7],
                  [2, 4, 0, 0, 6, 8],
                  [0, 0, 9, 11, 0, 0],
                  [0, 0, 10, 12, 0, 0],
                  [13, 15, 0, 0, 17, 19],
                  [14, 16, 0, 0, 18, 20]], np.float64)
    assert np.array_equal(to_dense(rp, ci, v, 2, (6, 6)), a)
    fb = g.Fbcsr.from_arrays(gexec, (6, 6), 2, rp, ci, v)
    b = np.array([1.0, -2.0, 0.5, 3.0, -1.0, 2.0])
    x = g.Dense.create(gexec, (6, 1))
    fb.apply(dense_on(gexec, b), x)
    assert np.array_equal(x.to_numpy()[:, 0], a @ b)
    assert np.array_equal(x.to_numpy()[:, 0], [4.0, 4.0, 37.5, 41.0, 4.0, 4.0])
    c = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    x = dense_on(gexec, c)
    fb.apply(g.scalar(gexec, -1.0), dense_on(gexec, b), g.scalar(gexec, 2.0), x)
    assert np.array_equal(x.to_numpy()[:, 0], 2 * c - a @ b)
    x = dense_on(gexec, np.full(6, np.nan))
    fb.apply(g.scalar(gexec, -1.0), dense_on(gexec, b), g.scalar(gexec, 0.0), x)
    assert np.array_equal(x.to_numpy()[:, 0], -(a @ b))
    # 6 x 9 Fbcsr<3>: block row 0 holds block columns 0 and 2, block row 1 is empty
    rp = np.array([0, 2, 2], np.int64)
    ci = np.array([0, 2], np.int64)
    v = np.arange(1, 19, dtype=np.float64)
    a = np.zeros((6, 9))
    a[0:3, 0:3] = v[:9].reshape(3, 3).T
    a[0:3, 6:9] = v[9:].reshape(3, 3).T
    assert a[0, 1] == 4.0 and a[1, 0] == 2.0 and a[2, 8] == 18.0
    fb = g.Fbcsr.from_arrays(gexec, (6, 9), 3, rp, ci, v)
    assert fb.get_num_stored_blocks() == 2 and fb.get_num_stored_elements() == 18
    b = np.arange(9, dtype=np.float64) - 4.0
    x = dense_on(gexec, np.full(6, 5.0))
    fb.apply(dense_on(gexec, b), x)
    assert np.array_equal(x.to_numpy()[:, 0], a @ b)
    assert np.array_equal(x.to_numpy()[3:, 0], np.zeros(3))
    x = dense_on(gexec, np.ones(6))
    fb.apply(g.scalar(gexec, -1.0), dense_on(gexec, b), g.scalar(gexec, 2.0), x)
    assert np.array_equal(x.to_numpy()[:, 0], 2.0 - a @ b)
    x = dense_on(gexec, np.full(6, np.nan))
    fb.apply(g.scalar(gexec, -1.0), dense_on(gexec, b), g.scalar(gexec, 0.0), x)
    assert np.array_equal(x.to_numpy()[:, 0], -(a @ b))
    assert np.array_equal(fb.convert_to_dense().to_numpy(), a)


@pytest.mark.parametrize("bs", [1, 2, 3, 4, 5, 7, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("idt", [np.int32, np.int64])
@pytest.mark.parametrize("ordered", [True, False])
def test_random_products_are_bit_identical(gexec, oracle, bs, dtype, idt, ordered):
    import ginkgo_amd as g
    rng = np.random.default_rng(1000 * bs + 10 * (dtype == np.float32) + (idt == np.int64) + 7 * ordered)
    nbr, nbc = 57, 41
    rp, ci, v = random_blocks(rng, nbr, nbc, bs, 9, dtype, idt, ordered, empty=(0, 1, 28, nbr - 1))
    shape = (nbr * bs, nbc * bs)
    fb = g.Fbcsr.from_arrays(gexec, shape, bs, rp, ci, v)
    assert fb.is_sorted_by_column_index() == (ordered or all(
        np.all(np.diff(ci[rp[r]:rp[r + 1]]) >= 0) for r in range(nbr)))
    for nrhs, strided in ((1, False), (3, True), (1, True)):
        check_products(gexec, oracle, fb, rp, ci, v, bs, shape, nrhs, strided, seed=bs + nrhs)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_block_row_of_1200_blocks_is_not_chunked(gexec, oracle, dtype):
    import ginkgo_amd as g
    rng = np.random.default_rng(5)
    bs, nbc = 3, 1500
    c0 = np.sort(rng.choice(nbc, 1200, replace=False))
    ci = np.concatenate([c0, [0, 7, 1499]]).astype(np.int32)
    rp = np.array([0, 1200, 1203], np.int32)
    v = rng.uniform(-1, 1, ci.size * 9).astype(dtype)
    fb = g.Fbcsr.from_arrays(gexec, (6, nbc * bs), bs, rp, ci, v)
    check_products(gexec, oracle, fb, rp, ci, v, bs, (6, nbc * bs), 1, False, seed=9)


@pytest.mark.parametrize("bs", [2, 3, 4, 7])
@pytest.mark.parametrize("idt", [np.int32, np.int64])
def test_conversions_against_scipy_bsr(gexec, bs, idt):
    import ginkgo_amd as g
    rng = np.random.default_rng(bs)
    nbr, nbc = 23, 17
    n, m = nbr * bs, nbc * bs
    # partly filled blocks (explicit zeros after the conversion), some empty block rows
    a = sp.random(n, m, density=0.08, random_state=bs, format="csr")
    a = a.tolil()
    a[bs * 3:bs * 5, :] = 0
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    rp, ci, v = a.indptr.astype(idt), a.indices.astype(idt), a.data
    bsr = a.tobsr((bs, bs))
    bsr.sort_indices()
    csr = g.Csr.from_arrays(gexec, (n, m), rp, ci, v)
    fb = csr.convert_to_fbcsr(bs)
    assert fb.block_size == bs and fb.col_idxs.dtype == csr.col_idxs.dtype
    assert np.array_equal(fb.row_ptrs.cpu().numpy(), bsr.indptr)
    assert np.array_equal(fb.col_idxs.cpu().numpy(), bsr.indices)
    got = fb.values.cpu().numpy().reshape(-1, bs, bs).transpose(0, 2, 1)
    assert np.array_equal(got, bsr.data)
    assert fb.is_sorted_by_column_index()
    assert np.array_equal(fb.convert_to_dense().to_numpy(), a.toarray())
    # Fbcsr -> Csr: bs^2 entries per block, explicit zeros kept; -> Fbcsr again: the same arrays
    back = fb.convert_to_csr()
    erp, eci, ev = expand(bsr.indptr, bsr.indices, fb.values.cpu().numpy(), bs)
    assert np.array_equal(back.row_ptrs.cpu().numpy(), erp)
    assert np.array_equal(back.col_idxs.cpu().numpy(), eci)
    assert np.array_equal(back.values.cpu().numpy(), ev)
    again = back.convert_to_fbcsr(bs)
    for name in ("row_ptrs", "col_idxs", "values"):
        assert torch.equal(getattr(again, name).cpu(), getattr(fb, name).cpu()), name
    # diagonal of a square one
    sq = sp.random(n, n, density=0.1, random_state=bs + 1, format="csr") + sp.eye(n) * 3
    sq = sq.tocsr()
    sq.sort_indices()
    fbs = g.Csr.from_scipy(gexec, sq, idt).convert_to_fbcsr(bs)
    assert np.array_equal(fbs.extract_diagonal().cpu().numpy(), sq.diagonal())
    # from_scipy: scipy's row-major blocks transposed
    fb2 = g.Fbcsr.from_scipy(gexec, bsr, idt)
    assert np.array_equal(fb2.values.cpu().numpy(), fb.values.cpu().numpy())
    assert np.array_equal(fb2.convert_to_dense().to_numpy(), bsr.toarray())


def test_unsorted_csr_is_converted_on_a_clone(gexec):
    import ginkgo_amd as g
    a = sp.random(24, 24, density=0.2, random_state=11, format="csr")
    a.sort_indices()
    rp, ci, v = a.indptr.astype(np.int32), a.indices.astype(np.int32).copy(), a.data.copy()
    for r in range(24):          # reverse every row
        ci[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][::-1]
        v[rp[r]:rp[r + 1]] = v[rp[r]:rp[r + 1]][::-1]
    csr = g.Csr.from_arrays(gexec, (24, 24), rp, ci, v)
    assert not csr.is_sorted_by_column_index()
    fb = csr.convert_to_fbcsr(4)
    assert np.array_equal(csr.col_idxs.cpu().numpy(), ci)          # left as it was
    assert np.array_equal(csr.values.cpu().numpy(), v)
    bsr = a.tobsr((4, 4))
    bsr.sort_indices()
    assert np.array_equal(fb.col_idxs.cpu().numpy(), bsr.indices)
    assert np.array_equal(fb.convert_to_dense().to_numpy(), a.toarray())


def test_read_device_matrix_data(gexec):
    import ginkgo_amd as g
    a = sp.random(15, 12, density=0.25, random_state=4, format="coo")
    order = np.lexsort((a.col, a.row))
    ent = np.zeros(a.nnz, g.entry_dtype(np.float64, np.int32))
    ent["row"], ent["column"], ent["value"] = a.row[order], a.col[order], a.data[order]
    data = g.DeviceMatrixData.create_from_host(gexec, (15, 12), ent)
    fb = g.Fbcsr.read(data, 3)
    ref = g.Csr.read(data).convert_to_fbcsr(3)
    for name in ("row_ptrs", "col_idxs", "values"):
        assert torch.equal(getattr(fb, name).cpu(), getattr(ref, name).cpu()), name
    assert np.array_equal(fb.convert_to_dense().to_numpy(), a.toarray())


@pytest.mark.parametrize("grid", [6, 14])
def test_flan_like_blocks_spmv_and_cg(gexec, oracle, grid):
    import ginkgo_amd as g
    a, l27 = flan_like(oracle, grid)
    n = a.shape[0]
    csr = g.Csr.from_scipy(gexec, a)
    fb = csr.convert_to_fbcsr(3)
    # L27's block pattern, every block dense
    assert np.array_equal(fb.row_ptrs.cpu().numpy(), l27.indptr)
    assert np.array_equal(fb.col_idxs.cpu().numpy(), l27.indices)
    assert fb.get_num_stored_elements() == a.nnz
    xv = np.random.default_rng(grid).uniform(-1, 1, n)
    y1, y2 = g.Dense.create(gexec, (n, 1)), g.Dense.create(gexec, (n, 1))
    csr.apply(dense_on(gexec, xv), y1)
    fb.apply(dense_on(gexec, xv), y2)
    assert np.array_equal(y1.to_numpy(), y2.to_numpy())
    # the block-Jacobi of the Fbcsr is the one of the Csr
    pf = g.Jacobi.build().with_max_block_size(3).on(gexec).generate(fb)
    pc = g.Jacobi.build().with_max_block_size(3).on(gexec).generate(csr)
    assert pf.get_num_blocks() == pc.get_num_blocks() == n // 3
    assert torch.equal(pf.block_pointers.cpu(), pc.block_pointers.cpu())
    assert torch.equal(pf.blocks.cpu(), pc.blocks.cpu())
    # CG + block-Jacobi(3): the Fbcsr system matrix against the Csr without the fused spmv + dot
    rhs = np.ones(n)
    runs = []
    for op, fused in ((fb, True), (csr, False)):
        s = (g.Cg.build()
             .with_criteria(g.stop.Iteration.build().with_max_iters(1000),
                            g.stop.ResidualNorm.build().with_reduction_factor(1e-10))
             .with_preconditioner(g.Jacobi.build().with_max_block_size(3))
             .with_fused_spmv_dot(fused).on(gexec).generate(op))
        x = g.Dense.from_numpy(gexec, np.zeros(n))
        s.apply(g.Dense.from_numpy(gexec, rhs), x)
        assert s.has_converged
        runs.append((s.num_iterations, x.to_numpy()))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1])
    assert np.linalg.norm(rhs - a @ runs[0][1][:, 0]) <= 1.01e-10 * np.linalg.norm(rhs)


def test_errors(gexec):
    import ginkgo_amd as g
    a = sp.random(7, 7, density=0.3, random_state=1, format="csr")
    with pytest.raises((g.DimensionMismatch, g.GkoError)):
        g.Csr.from_scipy(gexec, a).convert_to_fbcsr(3)
    b = sp.random(18, 18, density=0.3, random_state=1, format="csr")
    with pytest.raises(g.NotSupported):
        g.Csr.from_scipy(gexec, b).convert_to_fbcsr(9)
    with pytest.raises(g.NotSupported):
        g.Fbcsr.from_arrays(gexec, (18, 18), 9, np.zeros(3, np.int32), np.zeros(0, np.int32),
                            np.zeros(0))
    with pytest.raises(g.NotSupported):
        g.Fbcsr.from_scipy(gexec, sp.bsr_matrix(np.ones((4, 6)), blocksize=(2, 3)))
    fb = g.Csr.from_scipy(gexec, b).convert_to_fbcsr(3)
    with pytest.raises(g.NotSupported):
        fb.apply(g.Dense.create(gexec, (18, 1), torch.float32), g.Dense.create(gexec, (18, 1)))
    with pytest.raises(g.NotSupported):
        fb.apply(g.scalar(gexec, 1.0, torch.float32), g.Dense.create(gexec, (18, 1)),
                 g.scalar(gexec, 0.0, torch.float32), g.Dense.create(gexec, (18, 1)))
    with pytest.raises(g.DimensionMismatch):
        fb.apply(g.Dense.create(gexec, (12, 1)), g.Dense.create(gexec, (18, 1)))
