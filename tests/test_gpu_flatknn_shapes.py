"""GPU: the flat exact k-NN scan (csrc/scan_knn.hip under csrc/knn_plan.h) at the smallest shapes at which it can go wrong, on
random floats against the restatement (tests/knn_ref.py; L2 through the oracle), bit for bit including labels.

  ntotal  1, 63, 64, 65, 127, 128, 129 (the 128-column tile and its halves, both sides), 1000, 4999; k > ntotal among them
  nq      1, 19 | 20 (the dispatch boundary, both sides), 127, 129 (a row tile and one more), 300; 1030 (two pages of the
          matrix route)
  d       1, 3, 4, 30, 128, 132, 200 (d % 4, one staged step of 64 floats, more than one, a ragged last one)
  k       1, 10, 64 | 65, 256 | 257, 1024: one, four and sixteen keys per lane; the fused scan up to 256, the matrix route beyond
Both metrics; the inner products of centred Gaussian data are negative about as often as not.  Every value appears at least
once, every boundary is paired with the others' plain values."""
import functools

import numpy as np
import pytest

import knn_ref as kr
import vector_line_quantization_amd as vlq
from util import bits

pytestmark = pytest.mark.gpu
METRICS = ("l2", "ip")


@functools.lru_cache(maxsize=None)
def data(ntotal, nq, d, seed=0, dup=False):
    rng = np.random.default_rng(1000 * seed + 7 * ntotal + 3 * nq + d)
    xb = rng.standard_normal((ntotal, d)).astype(np.float32)
    if dup:                         # 40 % of the vectors are copies of others: exact ties everywhere
        src = rng.integers(0, ntotal, (ntotal * 2) // 5)
        dst = rng.permutation(ntotal)[: src.size]
        xb[dst] = xb[src]
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    xb.setflags(write=False)
    xq.setflags(write=False)
    return xb, xq


@functools.lru_cache(maxsize=None)
def expected(ntotal, nq, d, k, metric, seed=0, dup=False):
    xb, xq = data(ntotal, nq, d, seed, dup)
    D, I = kr.search(xq, xb, k, metric)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


def same(D, I, Dn, In, what):
    assert np.array_equal(bits(D), bits(Dn)), "%s: distances differ" % (what,)
    assert np.array_equal(I, In), "%s: labels differ" % (what,)


SHAPES = []
SHAPES += [(nt, 20, 30, 10) for nt in (1, 63, 64, 65, 127, 128, 129, 1000, 4999)]
SHAPES += [(nt, 5, 32, 10) for nt in (1, 64, 129, 4999)]                              # the direct path's row tiles
SHAPES += [(1000, nq, 128, 10) for nq in (1, 19, 20, 127, 129, 300)]
SHAPES += [(1000, 19, 30, 10)]                                                          # below 20 queries, d % 4 != 0: GEMM
SHAPES += [(1000, nq, d, 10) for d in (1, 3, 4, 30, 128, 132, 200) for nq in (5, 20)]
SHAPES += [(1000, nq, 32, k) for k in (1, 10, 64, 65, 256, 257, 1024) for nq in (5, 20)]
SHAPES += [(300, 129, 200, 65), (129, 300, 132, 256), (1000, 1030, 32, 257)]
SHAPES = sorted(set(SHAPES))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "nt%d_nq%d_d%d_k%d" % s)
def test_shape(shape, metric):
    ntotal, nq, d, k = shape
    xb, xq = data(ntotal, nq, d)
    g = vlq.GpuFlat(d, metric=metric, device=0)
    try:
        g.add(xb)
        D, I = g.search(xq, k)
        same(D, I, *expected(ntotal, nq, d, k, metric), what=(shape, metric, g.last_scan_info()))
        assert ((I == -1).sum(axis=1) == max(0, k - ntotal)).all()
    finally:
        g.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [10, 100, 300], ids=["k10_fused1", "k100_fused4", "k300_matrix"])
def test_tiling_independence(k, metric):
    """forced row tiles x slices whose ends lie off every tile multiple give the default rows bit for bit, ties included"""
    ntotal, nq, d = 4999, 300, 32
    xb, xq = data(ntotal, nq, d, seed=1, dup=True)
    Dn, In = expected(ntotal, nq, d, k, metric, seed=1, dup=True)
    assert any(np.unique(r).size < r.size for r in Dn)              # ties among the results
    g = vlq.GpuFlat(d, metric=metric, device=0)
    try:
        g.add(xb)
        D0, I0 = g.search(xq, k)
        same(D0, I0, Dn, In, ("default", g.last_scan_info()))
        routes = set()
        for rows in (32, 64, 128):
            for slices in (1, 2, 7):
                g.scan_split(rows, slices)
                D, I = g.search(xq, k)
                info = g.last_scan_info()
                routes.add(info.split()[1])
                assert "S=%d " % slices in info, info
                same(D, I, D0, I0, info)
        assert routes == ({"route=fused"} if k <= 256 else {"route=matrix"})
        # the small-batch path over the same database
        g.scan_split(0, 0)
        q5 = xq[:5]
        D5, I5 = g.search(q5, k)
        same(D5, I5, *kr.search(q5, xb, k, metric), what=g.last_scan_info())
        for slices in (1, 2, 7):
            g.scan_split(0, slices)
            D, I = g.search(q5, k)
            assert "path=direct" in g.last_scan_info() and "S=%d " % slices in g.last_scan_info()
            same(D, I, D5, I5, g.last_scan_info())
    finally:
        g.close()


@pytest.mark.parametrize("metric", METRICS)
def test_paging_keeps_the_calls_dispatch(metric):
    """one search of 32 768 + 301 queries and one of 32 768 + 5: the last page takes the GEMM path of the whole call (d % 4 == 0:
    five queries by themselves would take the small-batch path); a call of 19 queries beside them takes the other"""
    ntotal, d, k = 300, 8, 5
    xb, xq = data(ntotal, 32768 + 301, d, seed=2)
    Dn, In = expected(ntotal, 32768 + 301, d, k, metric, seed=2)
    g = vlq.GpuFlat(d, metric=metric, device=0)
    try:
        g.add(xb)
        D, I = g.search(xq, k)
        assert "path=gemm" in g.last_scan_info()
        same(D, I, Dn, In, "32768 + 301")
        n2 = 32768 + 5
        D, I = g.search(xq[:n2], k)
        same(D, I, Dn[:n2], In[:n2], "32768 + 5")
        q19 = xq[32768:32768 + 19]
        D, I = g.search(q19, k)
        assert "path=direct" in g.last_scan_info()
        same(D, I, *kr.search(q19, xb, k, metric), what="19 queries")
        if metric == "l2":          # (the two paths differ in bits on general floats: the check above is not vacuous)
            assert not np.array_equal(bits(D), bits(Dn[32768:32768 + 19]))
    finally:
        g.close()


def test_matrix_route_walks_several_chunks():
    """1024 queries make the chunk 32 768 columns: 40 000 vectors are two chunks, the second joined onto the running rows"""
    ntotal, nq, d, k = 40000, 1024, 8, 257
    xb, xq = data(ntotal, nq, d, seed=3)
    g = vlq.GpuFlat(d, metric="l2", device=0)
    try:
        g.add(xb)
        D, I = g.search(xq, k)
        info = g.last_scan_info()
        assert "route=matrix" in info and "chunk=32768" in info, info
        same(D, I, *expected(ntotal, nq, d, k, "l2", seed=3), what=info)
    finally:
        g.close()
