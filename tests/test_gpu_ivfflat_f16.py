"""GPU: float16 list storage of IVFFlat (vlq.GpuIVFFlat(storage="f16"); csrc/scan_flat16.hip, csrc/scan_range_flat16.hip).  The
whole specification is one property without a tolerance: an f16 index over x returns, bit for bit, what the fp32 index returns
over x.astype(float16).astype(float32).  So every expected value is the numpy restatement (tests/ivfflat_ref.py,
tests/range_ref.py) applied to the rounded vectors; D is compared as bits, I and lims exactly.

Six lists of 0, 1, 63, 65, 257 and 553 rows (an empty list, partial and full waves, more than two 256-row trips) around six
far-apart centroids, so that add() with these centroids rebuilds the very same lists; every list is probed by every query."""
import functools

import numpy as np
import pytest

import ivfflat_ref as fr
import range_ref as rr
import vector_line_quantization_amd as vlq
from util import bits

pytestmark = pytest.mark.gpu
LENS = np.array([63, 0, 553, 1, 257, 65])
NLIST, NQ = LENS.size, 5
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
NTOTAL = int(OFFS[-1])
LIST_OF = np.repeat(np.arange(NLIST), LENS)
IDS = (np.arange(NTOTAL, dtype=np.int64) * 7 + 1000)
TILE_D, QUAD_D, TAIL_D = [8, 64, 72, 136], [12, 4], [30, 5, 3]


def rounded(x):
    return x.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def data(d):
    """(x [NTOTAL][d] in list order, centroids, queries, keys [NQ][NLIST]: every list, in a different order per query)"""
    rng = np.random.default_rng(1600 + d)
    cent = (4 * rng.standard_normal((NLIST, d))).astype(np.float32)
    cent[LENS == 0] = 100.0                      # (no vector is ever nearest to the empty list's centroid)
    x = (cent[LIST_OF] + 0.5 * rng.standard_normal((NTOTAL, d))).astype(np.float32)
    xq = (2 * rng.standard_normal((NQ, d))).astype(np.float32)
    keys = np.stack([rng.permutation(NLIST) for _ in range(NQ)]).astype(np.int64)
    assert np.isfinite(x).all() and (rounded(x) != x).mean() > 0.95
    return x, cent, xq, keys


def lists(x):
    return dict(vecs=x, ids=IDS, list_offsets=OFFS)


@functools.lru_cache(maxsize=None)
def knn_expected(d, metric, k):
    """the restatement over the rounded vectors, with one key of -1 among the probes: (keys, D, I, visited, ndis)"""
    x, _c, xq, keys = data(d)
    keys = np.insert(keys, 2, -1, axis=1)
    De, Ie, nv, nd = fr.search_preassigned(lists(rounded(x)), xq, keys, k, metric)
    # the case discriminates: a path that keeps fp32 rows, or sums in another order, gives other bits
    Du = fr.search_preassigned(lists(x), xq, keys, k, metric)[0]
    assert not np.array_equal(bits(Du), bits(De))
    if d >= 4:        # (for d < 4 the four-accumulator order and the plain one are the same expression)
        assert fr.discriminates(lists(rounded(x)), xq, keys, k, metric, De)
    return keys, De, Ie, int(nv.sum()), int(nd.sum())


def index(d, metric, x=None, cent=None):
    g = vlq.GpuIVFFlat(d, NLIST, device=0, metric=metric, storage="f16")
    if cent is not None:
        g.set_coarse_centroids(cent)
    if x is not None:
        g.set_lists(x, IDS, OFFS)
    return g


def read_path(d):
    return "read=tile128" if d % 8 == 0 else "read=row"


@pytest.mark.parametrize("d,k,metric", [(d, k, m) for d in TILE_D + QUAD_D + TAIL_D for k in (1, 10) for m in ("l2", "ip")]
                         + [(72, 300, "l2"), (72, 1024, "ip")])       # (KPL 4 and KPL 16 once each)
def test_knn(d, k, metric):
    x, _c, xq, _k = data(d)
    keys, De, Ie, nv, nd = knn_expected(d, metric, k)
    g = index(d, metric, x)
    D, I = g.search_preassigned(xq, keys, k)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)
    assert g.stats() == (NQ, nv, nd)
    info = g.last_scan_info()
    assert "scan_flat16_kernel<%d, %s>" % (1 if k <= 64 else 4 if k <= 256 else 16, metric.upper()) in info, info
    assert "store=f16" in info and read_path(d) in info, info
    g.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", [64, 72, 12, 30])
def test_range(d, metric):
    x, _c, xq, keys = data(d)
    z = lists(rounded(x))
    everything = np.float32(-np.inf if metric == "ip" else np.inf)
    radius = np.float32(np.median(rr.range_search_preassigned(z, xq, keys, everything, metric)[1]))
    le, De, Ie = rr.range_search_preassigned(z, xq, keys, radius, metric)
    assert 0 < De.size < NQ * NTOTAL
    g = index(d, metric, x)
    lims, D, I = g.range_search_preassigned(xq, keys, float(radius))
    assert np.array_equal(lims, le) and np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)
    info = g.last_scan_info()
    assert "range_flat16_kernel" in info and "store=f16" in info and read_path(d) in info, info
    g.close()


@pytest.mark.parametrize("how", ["set_lists", "add_preassigned", "add"])
@pytest.mark.parametrize("d", [64, 30])
def test_write_path(d, how):
    x, cent, xq, _k = data(d)
    keys, De, Ie, _nv, _nd = knn_expected(d, "l2", 10)
    order = np.lexsort((LIST_OF, np.arange(NTOTAL) - OFFS[LIST_OF]))      # round-robin over the lists: a list keeps its order
    g = index(d, "l2", x if how == "set_lists" else None, cent)
    if how == "add_preassigned":         # two calls (the lists grow), one vector dropped by a negative assignment
        cut = NTOTAL // 3
        rows = np.insert(order, cut + 5, order[0])
        assign = LIST_OF[rows].astype(np.int64)
        assign[cut + 5] = -1
        for a, b in ((0, cut), (cut, rows.size)):
            g.add_preassigned(x[rows[a:b]], assign[a:b], IDS[rows[a:b]])
    elif how == "add":                   # the assignment is made on the fp32 vectors: the fp32 index's lists
        g.add(x[order], IDS[order])
        f = vlq.GpuIVFFlat(d, NLIST, device=0, metric="l2")
        f.set_coarse_centroids(cent)
        f.add(x[order], IDS[order])
        for li in range(NLIST):
            assert np.array_equal(g.get_list(li)[1], f.get_list(li)[1]), li
        f.close()
    assert g.ntotal == NTOTAL
    for li in range(NLIST):
        rows, ids = g.get_list(li)
        assert np.array_equal(bits(rows), bits(rounded(x[OFFS[li]:OFFS[li + 1]]))) and np.array_equal(ids, IDS[OFFS[li]:OFFS[li + 1]]), li
    D, I = g.search_preassigned(xq, keys, 10)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)
    g.close()


def test_encoder_edge_values():
    """-0, a half subnormal, the largest half, beyond it (-> inf), two ties to even: stored and read back, never searched;
    18 components take the encoder's 16-byte steps and its one-by-one tail"""
    row = np.array([-0.0, 1e-6, 65504, 70000, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], np.float32)
    x = np.stack([row, -row, row[::-1]])
    g = vlq.GpuIVFFlat(6, 1, device=0, storage="f16")
    g.set_lists(x, np.arange(3, dtype=np.int64), np.array([0, 3], np.int64))
    rows, _ids = g.get_list(0)
    with np.errstate(over="ignore"):
        assert np.array_equal(bits(rows), bits(rounded(x)))
    g.close()


def test_set_lists_from_host_in_pages():
    """more host rows than one 65 536-row staging page: the second page lands behind the first.  The size is the page's, not
    a choice: nothing smaller reaches the second page, and nothing else in the suite does (3 MB of rows, no search)"""
    n, d = 65536 + 70, 12
    x = np.random.default_rng(7).standard_normal((n, d)).astype(np.float32)
    g = vlq.GpuIVFFlat(d, 2, device=0, storage="f16")
    g.set_lists(x, np.arange(n, dtype=np.int64), np.array([0, 65530, n], np.int64))
    assert np.array_equal(bits(g.get_list(0)[0]), bits(rounded(x[:65530]))) and np.array_equal(bits(g.get_list(1)[0]), bits(rounded(x[65530:])))
    g.close()


def test_whole_search():
    d, nprobe, k = 64, 3, 10
    x, cent, xq, _k = data(d)
    g = index(d, "l2", x, cent)
    _cdis, keys = g.coarse_search(xq, nprobe)
    De, Ie, _nv, _nd = fr.search_preassigned(lists(rounded(x)), xq, keys, k, "l2")
    D, I = g.search(xq, nprobe, k)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)
    g.close()
