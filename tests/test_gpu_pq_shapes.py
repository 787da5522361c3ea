"""GPU: the flat PQ scan (csrc/scan_pq.hip) on generated data against the numpy restatement (tests/pq_ref.py): every boundary
of the trip of 64 lanes and 256 rows, of the selection's k, of the query tile and of the code loads, and a search that spans
two query pages."""
import numpy as np
import pytest

import pq_ref as pr
import vector_line_quantization_amd as vlq
from util import bits

pytestmark = pytest.mark.gpu

# (ntotal, nq, k): ntotal in {0, 1, 63, 64, 65, 257, 1000}, nq in {1, 3, 5} (no multiple of the tile), k in {1, 64, 65, 256, 257, 1024}
SHAPES = [(0, 1, 1), (1, 3, 64), (63, 5, 65), (64, 1, 256), (65, 3, 257), (257, 5, 1024), (1000, 3, 64), (1000, 5, 257), (1000, 1, 1024),
          (257, 3, 1), (1000, 5, 65)]
MS = [1, 3, 4, 8, 12, 20, 64]


def generated(M, nbits=8, dsub=2, nb=1000, nq=5, seed=0):
    rng = np.random.default_rng(9000 + 17 * M + seed)
    ksub = 1 << nbits
    cent = rng.standard_normal((M, ksub, dsub)).astype(np.float32)
    codes = np.unique(rng.integers(0, ksub, (nb + 200, M), dtype=np.uint8), axis=0)
    codes = np.ascontiguousarray(codes[rng.permutation(codes.shape[0])][:nb])
    xq = rng.standard_normal((nq, M * dsub)).astype(np.float32)
    return cent, codes, xq


@pytest.mark.parametrize("M", MS)
def test_shapes_against_the_restatement(M):
    metric = "ip" if M in (3, 12) else "l2"
    cent, codes, xq = generated(M, nb=1000 if M > 1 else 256)
    g = vlq.GpuPQ(cent.shape[2] * M, M, 8, metric=metric)
    g.set_centroids(cent)
    for nt, nq, k in SHAPES:
        nt = min(nt, codes.shape[0])
        g.set_codes(codes[:nt])
        D, I = g.search(xq[:nq], k)
        Dn, In = pr.search(cent, codes[:nt], xq[:nq], k, metric)[:2]
        assert np.array_equal(bits(D), bits(Dn)) and np.array_equal(I, In), (M, nt, nq, k, g.last_scan_info())
    info = g.last_scan_info()
    assert ("group4, none, 16>" if M % 16 == 0 else "group4, none, 4>" if M % 4 == 0 and M > 4 else "M4, none, 4>" if M == 4 else "left, none, 1>") in info
    g.close()


@pytest.mark.parametrize("st,M", [(pr.ST_SDC, 3), (pr.ST_SDC, 8), (pr.ST_POLYSEMOUS, 8), (pr.ST_POLYSEMOUS, 16), (pr.ST_POLYSEMOUS_GENERALIZE, 8)])
def test_other_search_types_against_the_restatement(st, M):
    nbits = 4 if st == pr.ST_POLYSEMOUS_GENERALIZE else 8      # 16 centroids: codes share bytes with the query's often enough
    cent, codes, xq = generated(M, nbits=nbits, seed=st)
    g = vlq.GpuPQ(cent.shape[2] * M, M, nbits)
    g.set_centroids(cent)
    g.search_type = st
    hts = {pr.ST_SDC: [None], pr.ST_POLYSEMOUS: [4 * M - 6, 4 * M, 8 * M + 1], pr.ST_POLYSEMOUS_GENERALIZE: [M - 1, M, M + 1]}[st]
    for ht in hts:
        if ht is not None:
            g.polysemous_ht = ht
        for nt, nq, k in [(65, 3, 1), (257, 5, 65), (1000, 5, 64), (1000, 3, 257), (1000, 1, 1024)]:
            g.set_codes(codes[:nt])
            g.stats(reset=True)
            D, I = g.search(xq[:nq], k)
            Dn, In, npass = pr.search(cent, codes[:nt], xq[:nq], k, "l2", st, ht)[:3]
            assert np.array_equal(bits(D), bits(Dn)) and np.array_equal(I, In), (st, M, ht, nt, nq, k)
            assert g.stats() == (nq, nq * nt, npass)
    g.close()


def test_a_search_across_a_query_page():
    """n just above the page of 32 768 queries over a tiny index: the rows around the boundary against the restatement, the
    whole batch against two batches under the page"""
    M, nbits, n = 4, 4, 32768 + 3
    cent, codes, _ = generated(M, nbits=nbits, nb=70)
    xq = np.random.default_rng(77).standard_normal((n, 2 * M)).astype(np.float32)
    g = vlq.GpuPQ(2 * M, M, nbits)
    g.set_centroids(cent)
    g.set_codes(codes)
    D, I = g.search(xq, 5)
    assert g.stats() == (n, n * codes.shape[0], 0)
    for lo, hi in ((0, 4), (32764, n)):
        Dn, In = pr.search(cent, codes, xq[lo:hi], 5)[:2]
        assert np.array_equal(bits(D[lo:hi]), bits(Dn)) and np.array_equal(I[lo:hi], In)
    half = 20001
    Da, Ia = g.search(xq[:half], 5)
    Db, Ib = g.search(xq[half:], 5)
    assert np.array_equal(bits(D), bits(np.concatenate([Da, Db]))) and np.array_equal(I, np.concatenate([Ia, Ib]))
    g.close()
