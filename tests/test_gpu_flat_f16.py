"""GPU: float16 vector storage of the flat exact index (vlq.GpuFlat(storage="f16"), vlq.GpuRefineFlat(base, storage="f16");
csrc/scan_knn16.hip, csrc/refine_flat16.hip).  The whole specification is one property without a tolerance: an f16 index over x
returns, bit for bit, what the fp32 index returns over x.astype(float16).astype(float32).  So every expected value is the numpy
restatement (tests/knn_ref.py, tests/refineflat_ref.py) applied to the rounded vectors; D is compared as bits, I exactly.

777 Gaussian vectors: three 256-row blocks and a partial wave of the direct kernel, six 128-column tiles of the fused kernel, the
last one partial."""
import functools

import numpy as np
import pytest

import knn_ref as kr
import refineflat_ref as rr
import vector_line_quantization_amd as vlq
from util import bits

pytestmark = pytest.mark.gpu
NTOTAL = 777
METRICS = ("l2", "ip")
DIRECT_D = (8, 64, 72, 136, 12, 4)       # one piece; exactly one; one + an 8-half tail; two + a tail; the row path twice
GEMM_D = (64, 72, 200, 30, 3)            # one k step; a step + a tail; four steps; the 2-byte fetch twice


def rounded(x):
    return x.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def data(d):
    """(x [NTOTAL][d], 33 queries)"""
    rng = np.random.default_rng(2000 + d)
    x = rng.standard_normal((NTOTAL, d)).astype(np.float32)
    xq = rng.standard_normal((33, d)).astype(np.float32)
    assert (rounded(x) != x).mean() > 0.95
    for a in (x, xq):
        a.setflags(write=False)
    return x, xq


@functools.lru_cache(maxsize=None)
def expected(nq, d, metric, k):
    x, xq = data(d)
    De, Ie = kr.search(xq[:nq], rounded(x), k, metric)
    # the case discriminates: a path that kept fp32 rows gives other bits
    assert not np.array_equal(bits(kr.search(xq[:nq], x, k, metric)[0]), bits(De))
    return De, Ie


@functools.lru_cache(maxsize=None)
def index(d, metric):
    """one filled handle per (d, metric), shared by the search cases"""
    g = vlq.GpuFlat(d, metric=metric, device=0, storage="f16")
    g.add(data(d)[0])
    return g


def read_path(d):
    return "read=tile128" if d % 8 == 0 else "read=row"


def check_search(nq, d, metric, k, kernel, split=(0, 0)):
    De, Ie = expected(nq, d, metric, k)
    g = index(d, metric)
    g.scan_split(*split)
    try:
        D, I = g.search(data(d)[1][:nq], k)
        info = g.last_scan_info()
    finally:
        g.scan_split(0, 0)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie), info
    assert "kernel=" + kernel + " " in info and "store=f16" in info and read_path(d) in info, info
    return info


@pytest.mark.parametrize("nq,d,metric,k", [(nq, d, m, 10) for nq in (1, 4, 19) for d in DIRECT_D for m in METRICS] + [(19, 72, "l2", 100)])
def test_direct(nq, d, metric, k):
    info = check_search(nq, d, metric, k, "knn_direct16_kernel")
    assert "path=direct" in info and "rows=%d " % nq in info, info


@pytest.mark.parametrize("nq,d,metric,k", [(nq, d, m, k) for nq in (20, 33) for d in GEMM_D for m in METRICS for k in (1, 10)]
                         + [(5, 30, "l2", 10), (33, 72, "ip", 100)])      # (d % 4 != 0 below 20 queries; KPL 4)
def test_fused(nq, d, metric, k):
    assert "route=fused" in check_search(nq, d, metric, k, "knn_gemm16_kernel")


@pytest.mark.parametrize("split", [(32, 0), (64, 0), (128, 0), (0, 3)])
def test_fused_forced_split(split):
    info = check_search(33, 72, "l2", 10, "knn_gemm16_kernel", split)
    assert ("rows=%d " % split[0] if split[0] else "S=3 ") in info, info


@pytest.mark.parametrize("metric,k", [("l2", 300), ("ip", 300), ("l2", 1000)])       # (k = 1000 > ntotal: padding)
def test_matrix_route(metric, k):
    info = check_search(20, 72, metric, k, "flat16_decode+coarse_dist+knn_select_kernel")
    assert "route=matrix" in info, info
    if k > NTOTAL:
        assert (expected(20, 72, metric, k)[1][:, NTOTAL:] == -1).all()


@pytest.mark.parametrize("k_base", [10, 100])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [64, 72, 12, 30])
def test_refine_and_subset(d, metric, k_base):
    x, xq = data(d)
    xq = xq[:7]
    rng = np.random.default_rng(k_base + d)
    base_I = rng.integers(0, NTOTAL, (7, k_base)).astype(np.int64)
    base_I[3, k_base // 2] = -1
    base_D = rng.standard_normal((7, k_base)).astype(np.float32)
    g = index(d, metric)
    De, Ie = rr.refine(rounded(x), xq, base_D, base_I, 10, metric)
    assert not rr.same_bits(rr.refine(x, xq, base_D, base_I, 10, metric)[0], De)
    D, I = g.refine(xq, base_D, base_I, 10)
    info = g.last_refine_info()
    assert rr.same_bits(D, De) and np.array_equal(I, Ie), info
    assert "kernel=refine_flat16_kernel " in info and "select=1" in info and "store=f16" in info and read_path(d) in info, info
    sub = g.compute_distance_subset(xq, base_I, base_D.copy())
    assert rr.same_bits(sub, rr.compute_distance_subset(rounded(x), xq, base_I, base_D, metric))
    assert "select=0" in g.last_refine_info() and sub[3, k_base // 2] == base_D[3, k_base // 2]


def test_refine_bad_label():
    x, xq = data(64)
    base_I = np.arange(20, dtype=np.int64).reshape(2, 10)
    base_I[1, 4] = NTOTAL
    with pytest.raises(vlq.VlqError) as e:
        index(64, "l2").refine(xq[:2], np.zeros((2, 10), np.float32), base_I, 5)
    assert e.value.code == 1          # VLQ_ERR_INVALID


def test_gpu_refine_flat_f16_store():
    d, k = 64, 10
    x, xq = data(d)
    r = vlq.GpuRefineFlat(vlq.GpuFlat(d, metric="l2", device=0), storage="f16")
    r.add(x)
    r.k_factor = 3.0
    bD, bI = kr.search(xq[:5], x, 30, "l2")
    De, Ie = rr.refine(rounded(x), xq[:5], bD, bI, k, "l2")
    D, I = r.search(xq[:5].copy(), k)        # (a writable array: the search hands it to torch)
    assert rr.same_bits(D, De) and np.array_equal(I, Ie)
    assert "store=f16" in r.last_refine_info()
    r.store.close()
    r.base.close()


@pytest.mark.parametrize("d", [64, 5])
def test_write_path(d):
    x, xq = data(d)
    g = vlq.GpuFlat(d, metric="l2", device=0, storage="f16")
    g.add(x[:200])
    g.add(x[200:])
    assert g.ntotal == NTOTAL and vlq.lib().vlq_flat_storage(g._h) == 1
    assert np.array_equal(bits(g.reconstruct_n()), bits(rounded(x)))
    assert np.array_equal(bits(g.reconstruct_n(199, 3)), bits(rounded(x[199:202])))
    D, I = g.search(xq, 10)
    D1, I1 = index(d, "l2").search(xq, 10)
    De, Ie = expected(33, d, "l2", 10)
    assert np.array_equal(bits(D), bits(D1)) and np.array_equal(I, I1) and np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)
    with pytest.raises(vlq.VlqError) as e:
        g.range_search(xq, 1.0)
    assert e.value.code == 3 and "float16" in str(e.value)      # VLQ_ERR_UNSUPPORTED
    g.close()
