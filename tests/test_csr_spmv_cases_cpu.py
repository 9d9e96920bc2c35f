"""The helper of tests/test_csr_spmv_branches_gpu.py on the CPU: the builders give what the launcher's branches
need, the sequential oracle stays inside the bound D eps S on every builder's hub rows, and a hub row that has
lost one product of median magnitude falls outside it - the bound has teeth on the inputs chosen."""
import numpy as np
import pytest

import csr_spmv_cases as cc

BUILDERS = {
    "a_f64": lambda: cc.case_a(np.float64, np.int32),
    "a_f32_i64": lambda: cc.case_a(np.float32, np.int64),
    "c_f64": lambda: cc.case_c(np.float64, np.int32),
    "c_f32": lambda: cc.case_c(np.float32, np.int32),
    "d_5_segments": lambda: cc.case_d(5),
    "e_1": lambda: cc.case_e(0),
    "e_3": lambda: cc.case_e(2),
    "e_4": lambda: cc.case_e(3),
    "e_5": lambda: cc.case_e(4),
    "evict_0": lambda: cc.case_evict(0),
    "evict_129_f32": lambda: cc.case_evict(129, np.float32),
    "capture_1": lambda: cc.case_capture(1),
    "f_f64": lambda: cc.case_f(np.float64),
    "f_f32": lambda: cc.case_f(np.float32),
    "h_auto": cc.case_h_auto,
}


def test_builders_have_the_rows_the_branches_need():
    a = cc.case_a()
    assert a.shape == (331, 12000) and a.lens[3] == 4097 and a.lens[4] == 4096
    assert a.lens[64 * 2 + 63] == 9000 and a.lens[330] == 5000 and a.lens.max() == 9000
    assert cc.hub_rows(a).tolist() == [3, 191, 330]
    assert np.delete(a.lens, [3, 4, 191, 330]).max() <= 13 and (a.lens == 0).any()
    for m in (a, cc.case_c(), cc.case_f()):
        for r in range(m.shape[0]):
            assert np.all(np.diff(m.ci[m.rp[r]:m.rp[r + 1]]) > 0)          # sorted, no duplicates
    c = cc.case_c()
    seg1 = cc.hub_rows(c)[(cc.hub_rows(c) >= 64) & (cc.hub_rows(c) < 128)]
    assert len(seg1) == 10 and tuple(seg1[cc.LONG_MAX_PER_SEG:]) == cc.C_STAGED
    assert c.lens[127] > 2 * 4096                                           # more than two rounds of the stage
    assert c.shape[0] % 64 != 0 and cc.hub_rows(c)[-1] >= 64 * 3            # a hub in a last segment of 20 rows
    d = cc.case_d(5)
    assert d.shape == (320, 4097) and cc.hub_rows(d).tolist() == [0, 65, 130, 195, 260]
    assert d.rp[-1] == 5 * 4097 and d.v.dtype == np.float32 and len(np.unique(d.v)) > 20000
    segs = [sorted({r // 64 for r in cc.hub_rows(cc.case_e(i))}) for i in range(5)]
    assert segs == [[0, 3], [], [1, 4], [0], [2, 5]]
    e4 = cc.hub_rows(cc.case_e(3))
    assert len(e4) == 10 and tuple(e4[cc.LONG_MAX_PER_SEG:]) == cc.E_STAGED
    assert all(cc.case_e(i).shape == cc.case_e(0).shape for i in range(5))
    assert cc.hub_rows(cc.case_evict(70)).tolist() == [6]
    assert not np.array_equal(cc.case_evict(0).v[:50], cc.case_evict(64).v[:50])
    f = cc.case_f()
    assert f.shape[0] == f.shape[1] and cc.hub_rows(f).tolist() == [2, 64 * 70 + 63, f.shape[0] - 1]
    h = cc.case_h_auto()
    assert h.shape[0] == 64 * 8192 and len(cc.hub_rows(h)) == 2 and h.ci.max() < h.shape[0]
    k0, k1 = h.rp[70], h.rp[71]
    assert len(np.unique(h.ci[k0:k1])) == 5000


def test_exact_reference_on_known_values():
    """integers: every partial sum is exact in every type, so exact == oracle == the plain sum"""
    lens = np.array([5000, 0, 3])
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    ci = np.concatenate([np.arange(l) for l in lens]).astype(np.int32)
    v = (np.arange(len(ci)) % 7 - 3).astype(np.float64)
    m = cc.Mat(rp, ci, v, lens, (3, 5000))
    b = np.stack([np.arange(5000) % 5 - 2.0, np.ones(5000)], axis=1)
    c = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    ex, mag = cc.exact_rows(m, [0, 2], b, alpha=-0.75, beta=1.5, c=c)
    want = -0.75 * np.array([v[:5000] @ b[:, 0], v[:5000] @ b[:, 1]]) + 1.5 * c[0]
    assert np.array_equal(np.asarray(ex[0], np.float64), want)
    assert np.array_equal(np.asarray(mag[0], np.float64),
                          0.75 * np.array([np.abs(v[:5000] * b[:, 0]).sum(), np.abs(v[:5000]).sum()]) + 1.5 * c[0])
    ex0, mag0 = cc.exact_rows(m, [0], b, alpha=2.0, beta=0.0, c=np.full((3, 2), np.nan))
    assert np.isfinite(np.asarray(ex0, np.float64)).all() and np.isfinite(np.asarray(mag0, np.float64)).all()
    assert cc.depth([4097, 9000, 64 * 100]).tolist() == [65 + 80, 141 + 80, 180]


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_oracle_inside_and_dropped_product_outside_the_bound(oracle, name):
    m = BUILDERS[name]()
    t = m.v.dtype
    rng = np.random.default_rng(7)
    b = rng.uniform(-1, 1, (m.shape[1], 2)).astype(t)
    c0 = rng.uniform(-1, 1, (m.shape[0], 2)).astype(t)
    hubs = cc.hub_rows(m)
    assert len(hubs) > 0
    for alpha, beta, c in ((None, None, None), (-0.75, 1.5, c0), (-0.75, 0.0, np.full_like(c0, np.nan))):
        ref = cc.reference(oracle, m, b, alpha, beta, c)
        assert cc.judge(ref.seq.copy(), ref, m) < cc.depth(m.lens[hubs]).min()
        # (and the rows asked for bit for bit are taken from the oracle, whatever their length)
        assert cc.judge(ref.seq.copy(), ref, m, bitwise=tuple(hubs)) == 0.0
    # one product less, one column, the plain product
    ref = cc.reference(oracle, m, b[:, 0].copy())
    lim = cc.bound(m, ref, cc.eps_of(t))[:, 0]
    for i, r in enumerate(hubs[:12]):
        one = cc.drop_median_product(m, r, b[:, 0])
        assert one.lens[0] == m.lens[r] - 1
        short = oracle.csr_spmv(one.rp, one.ci, one.v, b[:, 0].copy())[0]
        assert abs(np.longdouble(short) - ref.exact[i, 0]) > lim[i]
        broken = ref.seq.copy()
        broken[r, 0] = short
        with pytest.raises(AssertionError):
            cc.judge(broken, ref, m)


def test_judge_rejects_a_short_row_off_by_one_ulp_and_nan(oracle):
    m = cc.case_a()
    b = np.random.default_rng(3).uniform(-1, 1, m.shape[1])
    ref = cc.reference(oracle, m, b)
    row = int(np.flatnonzero((m.lens > 0) & (m.lens <= cc.LONG_ROW))[0])
    for bad in (np.nextafter(ref.seq[row, 0], np.inf), np.nan):
        got = ref.seq.copy()
        got[row, 0] = bad
        with pytest.raises(AssertionError):
            cc.judge(got, ref, m)
    got = ref.seq.copy()
    got[3, 0] = np.nan
    with pytest.raises(AssertionError):
        cc.judge(got, ref, m)
    cc.judge_statistical(ref.seq, ref, m, b)
