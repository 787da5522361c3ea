"""GPU: range search of the flat index (vlq.GpuFlat.range_search, csrc/scan_range_knn.hip) against fixtures made from the
reference's own IndexFlat::range_search (tests/golden/make_golden_flatrange.py) and against the restatement
(tests/knn_range_ref.py).  Against the restatement every comparison is exact -- lims, D as bits, I, order included: a range
search selects nothing, so nothing is free.  Against a fixture the rule is its kind's (test_knn_range_ref.check_result)."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_range_ref as rr
import vector_line_quantization_amd as vlq
from knn_ref import is_direct
from test_knn_range_ref import METRICS, NAMES, check_result, load, radius
from util import bits
from vector_line_quantization_amd._lib import check

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED = 1, 3
FLT_MAX = float(np.finfo(np.float32).max)


def host(got):
    l, d, i = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in got)
    assert l.dtype == np.int64 and d.dtype == np.float32 and i.dtype == np.int64
    return l, d, i


def same(got, want, what=""):
    (l, d, i), (lims, D, I) = host(got), want
    assert np.array_equal(l, lims), what + ": lims differ"
    assert d.shape == D.shape and np.array_equal(bits(d), bits(D)), what + ": D differs"
    assert np.array_equal(i, I), what + ": I differs"


@functools.lru_cache(maxsize=None)
def restated_matrix(name, metric):
    z = load(name)
    m = rr.matrix(z["xq"], z["xb"], metric)
    m.setflags(write=False)
    return m


def uneven(n):
    """three uneven pieces of range(n)"""
    a = max(1, n // 7)
    b = max(a + 1, n // 2 + 3) if n > 2 else a
    return [(0, a), (a, min(b, n)), (min(b, n), n)]


def filled(xb, metric, pieces=1):
    g = vlq.GpuFlat(xb.shape[1], metric=metric, device=0)
    for lo, hi in ([(0, xb.shape[0])] if pieces == 1 else uneven(xb.shape[0])):
        if hi > lo:
            g.add(xb[lo:hi])
    return g


def observed_radius(mat, metric, share):
    """an observed value of mat that admits about `share` of its pairs: the strict test decides the pairs at it"""
    s = np.sort(mat.ravel())
    if metric == "ip":
        s = s[::-1]
    return float(s[min(int(share * s.size), s.size - 1)])


def path_of(nq, d):
    return "path=direct kernel=range_direct_kernel" if is_direct(nq, d) else "path=gemm kernel=range_gemm_kernel"


# --- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pieces", [1, 3])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_fixture(name, metric, pieces):
    """every radius of the fixture, the store filled in one add and in three uneven ones"""
    z = load(name)
    mat = restated_matrix(name, metric)
    g = filled(z["xb"], metric, pieces)
    try:
        assert g.ntotal == z["xb"].shape[0]
        for nm in z["names"]:
            what = "%s %s %s %d" % (name, metric, nm, pieces)
            r = float(radius(z, metric, nm))
            got = host(g.range_search(z["xq"], r))
            same(got, rr.from_matrix(mat, r, metric), what)
            check_result(z, metric, nm, *got, what)
            assert path_of(z["xq"].shape[0], z["d"]) in g.last_scan_info(), g.last_scan_info()
    finally:
        g.close()


# --- forced splits ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def split_data(nq):
    """8200 vectors of d 12: 64 slices of one 128-column tile each, with two columns over; 150 queries make row tiles of 32,
    64 and 128 differ (5, 3 and 2 of them, the last ones partly empty)"""
    rng = np.random.default_rng(77 + nq)
    xb = rng.standard_normal((8200, 12)).astype(np.float32)
    xq = rng.standard_normal((nq, 12)).astype(np.float32)
    want = {}
    for metric in METRICS:
        mat = rr.matrix(xq, xb, metric)
        r = observed_radius(mat, metric, 0.01)
        want[metric] = (r, rr.from_matrix(mat, r, metric))
    return xb, xq, want


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [150, 19])
def test_forced_splits_give_identical_arrays(nq, metric):
    xb, xq, want = split_data(nq)
    r, ref = want[metric]
    assert ref[0][-1] > nq
    g = filled(xb, metric)
    try:
        for rows in (32, 64, 128):
            for slices in (1, 3, 64):
                g.scan_split(rows, slices)
                same(g.range_search(xq, r), ref, "rows %d slices %d" % (rows, slices))
                info = g.last_scan_info()
                assert path_of(nq, 12) in info
                if nq == 150:
                    assert "rows=%d S=%d " % (rows, slices) in info, info
                else:
                    assert "rows=19 S=%d " % min(slices, 8200 // 256) in info, info
        g.scan_split(0, 0)
        same(g.range_search(xq, r), ref, "the plan's own split")
    finally:
        g.close()


# --- the smallest shapes at which the tiling can go wrong -------------------------------------------------------------------
NTOTALS = (1, 127, 128, 129, 300)
NQS = (1, 19, 20, 33, 150)


@functools.lru_cache(maxsize=None)
def shape_data(d):
    rng = np.random.default_rng(9000 + d)
    return rng.standard_normal((300, d)).astype(np.float32), rng.standard_normal((150, d)).astype(np.float32)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [1, 3, 30, 64, 65, 128, 200])
def test_small_shapes(d, metric):
    """ntotal at and around one column tile, nq at and around the dispatch's 20 and a row tile's 32, d across d % 4 and the
    64-float k step.  The store grows by add from one ntotal to the next."""
    xb, xq = shape_data(d)
    mats = {False: rr.matrix(xq, xb, metric, nq_call=150)}
    if d % 4 == 0:
        mats[True] = rr.matrix(xq[:19], xb, metric, nq_call=19)
    g = vlq.GpuFlat(d, metric=metric, device=0)
    try:
        have = 0
        for nt in NTOTALS:
            g.add(xb[have:nt])
            have = nt
            for nq in NQS:
                sub = mats[is_direct(nq, d)][:nq, :nt]
                r = observed_radius(sub, metric, 0.125)
                want = rr.from_matrix(sub, r, metric)
                same(g.range_search(xq[:nq], r), want, "d %d ntotal %d nq %d" % (d, nt, nq))
                assert path_of(nq, d) in g.last_scan_info()
    finally:
        g.close()


# --- radii and store contents -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["small_d32_nq19", "blas_d30_nq20"])
def test_extreme_radii(name, metric):
    z = load(name)
    mat = restated_matrix(name, metric)
    nq, nb = mat.shape
    g = filled(z["xb"], metric)
    try:
        every = -np.inf if metric == "ip" else np.inf
        for r, n in ((float(radius(z, metric, "all")), mat.size), (float(radius(z, metric, "none")), 0), (float("nan"), 0),
                     (every, mat.size), (-every, 0)):
            got = host(g.range_search(z["xq"], r))
            same(got, rr.from_matrix(mat, r, metric), "radius %r" % r)
            assert got[0][-1] == n
            if n:
                assert np.array_equal(got[2], np.tile(np.arange(nb), nq))
    finally:
        g.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["small_ties", "int_d30_nq40"])
def test_every_vector_stored_twice(name, metric):
    """a stored duplicate comes back twice, the lower position first"""
    z = load(name)
    xb2 = np.concatenate([z["xb"], z["xb"]])
    nb = z["xb"].shape[0]
    r = float(radius(z, metric, "tight"))
    g = filled(xb2, metric, 3)
    try:
        lims, D, I = host(g.range_search(z["xq"], r))
        same((lims, D, I), rr.range_search(z["xq"], xb2, r, metric))
        assert lims[-1] == 2 * z["lims_%s_tight" % metric][-1]
        for a, b in zip(lims[:-1], lims[1:]):
            h = (b - a) // 2
            assert np.array_equal(I[a:a + h] + nb, I[a + h:b]) and np.array_equal(bits(D[a:a + h]), bits(D[a + h:b]))
    finally:
        g.close()


@pytest.mark.parametrize("metric", METRICS)
def test_more_queries_than_a_page(metric):
    """33 000 queries over 300 vectors of d 8: the count pass over both pages, one scan, the fill pass over both"""
    rng = np.random.default_rng(33)
    xb = rng.standard_normal((300, 8)).astype(np.float32)
    xq = rng.standard_normal((33000, 8)).astype(np.float32)
    mat = rr.matrix(xq, xb, metric)
    r = observed_radius(mat, metric, 0.02)
    g = filled(xb, metric)
    try:
        got = host(g.range_search(xq, r))
        same(got, rr.from_matrix(mat, r, metric))
        assert got[0][32768] < got[0][-1] and "page=32768" in g.last_scan_info()
    finally:
        g.close()


# --- handle behaviour -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_empty_calls_reset_and_held_result(metric):
    z = load("blas_d30_nq20")
    xb, xq = z["xb"], z["xq"]
    r = float(radius(z, metric, "tight"))
    mat = restated_matrix("blas_d30_nq20", metric)
    g = vlq.GpuFlat(z["d"], metric=metric, device=0)
    try:
        # an empty store: all-zero lims, both paths' n
        for q in (xq, xq[:5]):
            lims, D, I = g.range_search(q, r)
            assert np.array_equal(lims, np.zeros(q.shape[0] + 1, np.int64)) and D.shape == I.shape == (0,)
        g.add(xb[:1000])
        want = rr.from_matrix(mat[:, :1000], r, metric)
        same(g.range_search(xq, r), want)
        # the held result after an add, and read twice; either output alone
        g.add(xb[1000:])
        same((want[0],) + g.range_result(), want)
        same((want[0],) + g.range_result(), want)
        D = np.empty(want[1].shape, np.float32)
        I = np.empty(want[2].shape, np.int64)
        check(vlq.lib().vlq_flat_range_result(g._h, D.ctypes.data_as(C.c_void_p), None))
        check(vlq.lib().vlq_flat_range_result(g._h, None, I.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(bits(D), bits(want[1])) and np.array_equal(I, want[2])
        # ... the next search sees the added rows
        same(g.range_search(xq, r), rr.from_matrix(mat, r, metric))
        # n = 0: lims[0] = 0 and an empty result in the handle
        lims, D, I = g.range_search(xq[:0], r)
        assert np.array_equal(lims, [0]) and D.shape == I.shape == (0,)
        assert g.range_result()[0].shape == (0,)
        # a refused call drops the previous hits before it looks at its arguments
        same(g.range_search(xq, r), rr.from_matrix(mat, r, metric))
        total = C.c_int64(-1)
        with pytest.raises(vlq.VlqError) as e:
            check(vlq.lib().vlq_flat_range_search(g._h, C.c_int64(3), None, C.c_float(r), None, C.byref(total)))
        assert e.value.code == ERR_INVALID and total.value == 0        # (the total goes with the hits)
        total = C.c_int64(-1)
        one = np.full(1, -1, np.int64)
        check(vlq.lib().vlq_flat_range_search(g._h, C.c_int64(0), None, C.c_float(r), one.ctypes.data_as(C.c_void_p),
                                                  C.byref(total)))
        assert total.value == 0 and one[0] == 0
        # reset: an empty store again, nothing held
        same(g.range_search(xq, r), rr.from_matrix(mat, r, metric))
        g.reset()
        assert g.ntotal == 0 and g.range_result()[0].shape == (0,)
        assert g.range_search(xq, r)[0][-1] == 0
        g.add(xb[500:])
        g.add(xb[:500])
        same(g.range_search(xq, r), rr.range_search(xq, np.concatenate([xb[500:], xb[:500]]), r, metric))
        # a k-NN search in between leaves the held hits alone, and last_scan_info names the last scan
        held = g.range_result()
        g.search(xq, 5)
        assert "knn_gemm_kernel" in g.last_scan_info()
        assert np.array_equal(bits(g.range_result()[0]), bits(held[0])) and np.array_equal(g.range_result()[1], held[1])
    finally:
        g.close()


@pytest.mark.parametrize("metric", METRICS)
def test_device_tensors(metric):
    import torch
    dev = torch.device("cuda:0")
    for name in ("small_d32_nq19", "blas_d128_nq150"):
        z = load(name)
        mat = restated_matrix(name, metric)
        r = float(radius(z, metric, "tight"))
        g = vlq.GpuFlat(z["d"], metric=metric, device=0)
        try:
            xb = torch.from_numpy(z["xb"].copy()).to(dev)
            xq = torch.from_numpy(z["xq"].copy()).to(dev)
            torch.cuda.synchronize()
            g.add(xb[:300])
            g.add(xb[300:])
            lims, D, I = g.range_search(xq, r)
            assert lims.is_cuda and D.is_cuda and I.is_cuda
            assert (lims.dtype, D.dtype, I.dtype) == (torch.int64, torch.float32, torch.int64)
            want = rr.from_matrix(mat, r, metric)
            same((lims, D, I), want)
            D2, I2 = g.range_result(like=xq)
            assert D2.is_cuda and I2.is_cuda
            same((lims, D2, I2), want)
            same((want[0],) + g.range_result(), want)          # ... and to the host
        finally:
            g.close()


def test_unsupported_d_on_the_direct_path():
    """one query of d 40 000 does not fit LDS beside the row tiles; one more float takes the GEMM path, which takes any d"""
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((3, 40001)).astype(np.float32)
    g = filled(np.ascontiguousarray(xb[:, :40000]), "l2")
    try:
        with pytest.raises(vlq.VlqError) as e:
            g.range_search(np.ascontiguousarray(xb[:1, :40000]), 1.0)
        assert e.value.code == ERR_UNSUPPORTED and "LDS" in str(e.value)
    finally:
        g.close()
    g = filled(xb, "l2")
    try:
        r = 2.0 * 40001
        same(g.range_search(xb[:2], r), rr.range_search(xb[:2], xb, r, "l2"))
    finally:
        g.close()
