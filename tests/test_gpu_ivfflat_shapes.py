"""GPU: the row shapes of the IVFFlat scan (csrc/scan_flat.hip) against the numpy restatement tests/ivfflat_ref.py, which
tests/test_ivfflat_ref.py holds to the reference: both read paths with d below, at and above one 128-byte piece, whole and
partial last pieces, every selection width, lists loaded at once and grown by add_preassigned.  General floats over the
shared small index (tests/newscan_index.py): D as bits, I exactly equal."""
import numpy as np
import pytest

import ivfflat_ref as fr
import newscan_index as nx
import vector_line_quantization_amd as vlq
from util import bits

pytestmark = pytest.mark.gpu
TILE_D = [4, 8, 12, 28, 36, 60, 64, 68, 96, 100, 132, 260, 1028]      # d % 4 == 0: read=tile128
DWORD_D = [1, 2, 6, 7, 33, 35, 65, 129]                                 # read=dword
ALL_D = TILE_D + DWORD_D
KS = (1, 10, 64, 65, 256, 257, 1024)
PAD_BITS = {"l2": np.float32(fr.FLT_MAX).view(np.uint32), "ip": np.float32(-fr.FLT_MAX).view(np.uint32)}
WIDE_PROBES = (36, "l2")                     # the case that runs with nprobe = 1024, mostly -1 keys
LAY = nx.layout()
LAY_SHORT = nx.layout(lengths=nx.SHORT_LENGTHS)       # d = 1028: the same boundaries, 1448 vectors


def config(d, metric):
    """(k, loaded by add_preassigned) of a case: k rotates with d, the loading alternates, the metrics differ in both"""
    i = ALL_D.index(d) + (3 if metric == "ip" else 0)
    return KS[i % len(KS)], bool((ALL_D.index(d) + (metric == "ip")) % 2)


def build(lay, p, metric, grown):
    g = vlq.GpuIVFFlat(p["d"], lay["nlist"], device=0, metric=metric)
    g.set_coarse_centroids(p["coarse"])
    if not grown:
        g.set_lists(p["vecs"], lay["ids"], lay["list_offsets"])
        return g
    # two batches after a reservation smaller than the total: the lists grow with slack, list_len differs from the offsets
    rows, assign = nx.input_order(lay)
    g.reserve_memory(lay["ntotal"] // 4)
    cut = lay["ntotal"] // 3
    for a, b in ((0, cut), (cut, lay["ntotal"])):
        g.add_preassigned(p["vecs"][rows[a:b]], assign[a:b], lay["ids"][rows[a:b]])
    assert g.ntotal == lay["ntotal"]
    for li in (int(np.argmax(lay["lens"])), int(np.argmin(lay["lens"]))):
        assert g.list_length(li) == lay["lens"][li]
    return g


def test_configurations_cover_what_they_claim():
    nx.check_layout(LAY)
    nx.check_layout(LAY_SHORT)
    for ds, lo in ((TILE_D, 4), (DWORD_D, 1)):
        assert any(d < 32 for d in ds) and any(d > 32 and d % 32 for d in ds) and min(ds) == lo
    assert 32 not in ALL_D and 64 in TILE_D and 96 in TILE_D          # (d = 32 and 128: the reference-made fixtures)
    for metric in ("l2", "ip"):
        cfg = [config(d, metric) for d in ALL_D]
        assert {c[0] for c in cfg} == set(KS) and {c[1] for c in cfg} == {False, True}
        ragged = [config(d, metric) for d in TILE_D if d > 32 and d % 32]
        assert {c[1] for c in ragged} == {False, True} and {1 if c[0] <= 64 else 4 if c[0] <= 256 else 16 for c in ragged} == {1, 4, 16}
    assert config(36, "l2")[1] != config(36, "ip")[1]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", ALL_D)
def test_shape(d, metric):
    lay = LAY_SHORT if d > 1000 else LAY
    p = nx.flat_parts(lay, d)
    k, grown = config(d, metric)
    keys = lay["keys"]
    if (d, metric) == WIDE_PROBES:
        rng = np.random.default_rng(d)
        wide = np.full((lay["nq"], 1024), -1, np.int64)
        for i in range(lay["nq"]):
            wide[i, np.sort(rng.permutation(1024)[:lay["nprobe"]])] = keys[i]
        keys = wide
    z = dict(vecs=p["vecs"], ids=lay["ids"], list_offsets=lay["list_offsets"])
    De, Ie, nv, nd = fr.search_preassigned(z, p["xq"], keys, k, metric)
    if d >= 4:        # (for d < 4 the four-accumulator order and the plain one are the same expression)
        assert fr.discriminates(z, p["xq"], keys, k, metric, De), "a plain left-to-right sum reproduces the expected rows"
    g = build(lay, p, metric, grown)
    g.stats(reset=True)
    D, I = g.search_preassigned(p["xq"], keys, k)
    what = "d=%d %s k=%d grown=%d" % (d, metric, k, grown)
    assert np.array_equal(bits(D), bits(De)), what
    assert np.array_equal(I, Ie), what
    assert (bits(D)[I == -1] == PAD_BITS[metric]).all() and (I[4] == -1).all(), what
    assert (I[:, 0] != -1).any(), what
    assert g.stats() == (lay["nq"], int(nv.sum()), int(nd.sum())), what
    info = g.last_scan_info()
    kpl = 1 if k <= 64 else 4 if k <= 256 else 16
    assert "kernel=scan_flat_kernel<%d, %s>" % (kpl, metric.upper()) in info, info
    assert ("read=tile128" if d % 4 == 0 else "read=dword") in info, info
    if grown:         # dropping the slack moves the lists and changes no row
        g.reclaim_memory()
        D2, I2 = g.search_preassigned(p["xq"], keys, k)
        assert np.array_equal(bits(D2), bits(De)) and np.array_equal(I2, Ie), what
    g.close()


@pytest.mark.parametrize("metric,d", [("l2", 36), ("ip", 100)])
def test_large_batch_search_is_coarse_then_scan(metric, d):
    """2100 queries: the screened coarse path under L2; search() is coarse_search + search_preassigned, and equal queries
    give equal rows"""
    p = nx.flat_parts(LAY, d)
    g = build(LAY, p, metric, False)
    nq, n0, nprobe = 2100, LAY["nq"], LAY["nprobe"]
    xq = np.ascontiguousarray(np.tile(p["xq"], ((nq + n0 - 1) // n0, 1))[:nq])
    for k in (10, 1):
        D, I = g.search(xq, nprobe, k)
        cdis, keys = g.coarse_search(xq, nprobe)
        D2, I2 = g.search_preassigned(xq, keys, k)
        assert np.array_equal(bits(D), bits(D2)) and np.array_equal(I, I2)
        for r in range(n0, nq, n0):
            m = min(n0, nq - r)
            assert np.array_equal(bits(D[:m]), bits(D[r:r + m])) and np.array_equal(I[:m], I[r:r + m])
        assert np.array_equal(keys[:n0], keys[n0:2 * n0])
        # ... and the rows are the restatement's over those keys
        z = dict(vecs=p["vecs"], ids=LAY["ids"], list_offsets=LAY["list_offsets"])
        De, Ie, _v, _n = fr.search_preassigned(z, p["xq"], keys[:n0], k, metric)
        assert np.array_equal(bits(D[:n0]), bits(De)) and np.array_equal(I[:n0], Ie)
    g.close()
