"""GPU: the exhaustive Hamming scan (csrc/scan_hamming.hip under csrc/hamming_plan.h) at the smallest shapes at which it can go
wrong, on random codes added through add_codes, against the restatement (tests/lsh_ref.py) bit for bit including labels -- the
semantics are closed (integer distances, the total order (distance, position)), so no reference run is needed.

  code size  4, 8, 16, 24, 32, 40, 64, 128: loads of 4, 8 and 16 bytes, one piece and several
  ntotal     1, 63, 64, 255, 256, 257 (a trip of 256 lanes and both sides), 1000, 4097 (the shortest slice and one more)
  k          1, 10, 64 | 65, 256 | 257, 1024: one, four and sixteen keys per lane; k > ntotal among them
  nq         1, 3, 5: the tile's tail at Q = 2 and Q = 4
Random codes of few bytes collide in distance all the time: nearly every row has ties at the k-th place."""
import functools

import numpy as np
import pytest

import lsh_ref as lr
import vector_line_quantization_amd as vlq
from util import bits

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def data(ntotal, nq, cs, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * ntotal + 3 * nq + cs)
    codes = rng.integers(0, 256, (ntotal, cs), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, cs), dtype=np.uint8)
    if cs >= 32 and ntotal > 8:         # wide random codes are all about cs * 4 bits apart: plant near neighbours of each query
        for i in range(nq):
            noise = rng.integers(0, 256, (3, 8, cs), dtype=np.uint8)
            codes[rng.integers(0, ntotal, 8)] = q[i] ^ (noise[0] & noise[1] & noise[2])
    codes.setflags(write=False)
    q.setflags(write=False)
    return codes, q


@functools.lru_cache(maxsize=None)
def expected(ntotal, nq, cs, k, seed=0):
    codes, q = data(ntotal, nq, cs, seed)
    D, I = lr.search_codes(q, codes, k)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


def same(D, I, Dn, In, what):
    assert np.array_equal(bits(D), bits(Dn)), "%s: distances differ" % (what,)
    assert np.array_equal(I, In), "%s: labels differ" % (what,)


def index(cs, codes=None):
    g = vlq.GpuLSH(cs * 8, cs * 8, rotate_data=False, device=0)
    if codes is not None and codes.shape[0]:
        g.add_codes(codes)
    return g


SHAPES = []
SHAPES += [(nt, 3, 8, 10) for nt in (1, 63, 64, 255, 256, 257, 1000, 4097)]
SHAPES += [(nt, 5, 16, 65) for nt in (1, 64, 257, 4097)]
SHAPES += [(1000, nq, cs, 10) for cs in (4, 8, 16, 24, 32, 40, 64, 128) for nq in (1, 3)]
SHAPES += [(1000, nq, 8, k) for k in (1, 10, 64, 65, 256, 257, 1024) for nq in (1, 5)]
SHAPES += [(4097, 3, cs, 257) for cs in (4, 24, 128)] + [(257, 5, 40, 1024), (4097, 5, 32, 256)]
SHAPES = sorted(set(SHAPES))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "nt%d_nq%d_cs%d_k%d" % s)
def test_shape(shape):
    ntotal, nq, cs, k = shape
    codes, q = data(ntotal, nq, cs)
    g = index(cs, codes)
    try:
        D, I = g.search_codes(q, k)
        same(D, I, *expected(ntotal, nq, cs, k), g.last_scan_info())
        lr.check_labels(D, I, q, codes)
    finally:
        g.close()


@pytest.mark.parametrize("shape", [(4097, 5, 8, 10), (4097, 3, 24, 65), (1000, 5, 128, 256), (4097, 5, 16, 1024), (257, 3, 4, 10)],
                         ids=lambda s: "nt%d_nq%d_cs%d_k%d" % s)
def test_forced_splits(shape):
    """every (query_tile, slices) the plan admits gives the rows of the unforced plan"""
    ntotal, nq, cs, k = shape
    codes, q = data(ntotal, nq, cs)
    Dn, In = expected(ntotal, nq, cs, k)
    g = index(cs, codes)
    try:
        same(*g.search_codes(q, k), Dn, In, "unforced")
        seen = set()
        for qt in (1, 2, 4):
            for s in (1, 2, 3, 16, 17, 64):
                g.scan_split(qt, s)
                same(*g.search_codes(q, k), Dn, In, "Q=%d S=%d" % (qt, s))
                info = g.last_scan_info()
                assert "S=%d " % s in info and ("Q=%d " % (1 if k > 256 else qt)) in info, info
                seen.add(info.split()[0])
        assert len(seen) == (1 if k > 256 else 3), seen
    finally:
        g.close()


@pytest.mark.parametrize("cs,k", [(8, 10), (16, 100), (128, 300)])
def test_identical_codes(cs, k):
    """all codes identical: every distance is the same, the row is positions 0 .. k-1"""
    codes = np.tile(np.arange(cs, dtype=np.uint8) * 37 + 11, (3000, 1))
    g = index(cs, codes)
    try:
        for s in (0, 5):
            g.scan_split(0, s)
            D, I = g.search_codes(codes[:3], k)
            assert (D == 0).all() and np.array_equal(I, np.tile(np.arange(k), (3, 1)))
            q = codes[:3].copy()
            q[:, 0] ^= 0x81
            D, I = g.search_codes(q, k)
            assert (D == 2).all() and np.array_equal(I, np.tile(np.arange(k), (3, 1)))
    finally:
        g.close()


def test_query_equal_to_a_stored_code():
    codes, _q = data(1000, 3, 16)
    pick = np.array([999, 0, 517, 256, 255])
    g = index(16, codes)
    try:
        D, I = g.search_codes(codes[pick], 4)
        assert (D[:, 0] == 0).all() and np.array_equal(I[:, 0], pick)
        same(D, I, *lr.search_codes(codes[pick], codes, 4), "self")
    finally:
        g.close()


def test_page_seam():
    """two pages of queries (32 768 + 5): the rows do not depend on the page a query falls in"""
    nq, ntotal, k = 32768 + 5, 300, 4
    rng = np.random.default_rng(77)
    codes = rng.integers(0, 256, (ntotal, 8), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 8), dtype=np.uint8)
    g = index(8, codes)
    try:
        D, I = g.search_codes(q, k)
        same(D, I, *lr.search_codes(q, codes, k), "two pages")
        sl = np.r_[0:3, 32765:32773]
        g.scan_split(4, 3)
        D2, I2 = g.search_codes(q, k)
        same(D2[sl], I2[sl], D[sl], I[sl], "forced")
    finally:
        g.close()


def test_padding_and_growth():
    """k > ntotal pads 2^31 / -1; codes appended in many uneven pieces are the codes appended at once"""
    codes, q = data(1000, 5, 24)
    g = index(24)
    try:
        at = 0
        for n in (1, 2, 61, 64, 128, 300, 444):
            g.add_codes(codes[at:at + n])
            at += n
            assert g.ntotal == at
            if n in (1, 61, 444):
                k = 70 if at < 70 else 10
                D, I = g.search_codes(q, k)
                same(D, I, *lr.search_codes(q, codes[:at], k), "ntotal=%d" % at)
        assert at == 1000 and np.array_equal(g.get_codes(), codes)
        assert np.array_equal(g.get_codes(998, 2), codes[998:])
    finally:
        g.close()
