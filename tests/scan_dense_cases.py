"""The cases of tests/test_gpu_scan_dense.py, run in a fresh process each (python tests/scan_dense_cases.py CASE): the walking
order is a per-process switch.

The stored-sums loop of the 16-byte scan streams a query's live probes as ONE index space of sum(len) codes, 64 at a time,
across list boundaries (csrc/scan16.hip).  These cases choose, through search_preassigned, which lists meet inside one block of
64: many boundaries in one block, boundaries on and next to block edges, totals on and next to multiples of the trip size.

Index: d 128, nlist 128, M 16 x 8 bit, random coarse and PQ centroids, random code bytes.  The list lengths go by list id, so
that the list-id walk (VLQ_WALK_FIRST=1) and the coarse order (-1) both make the small lists neighbours.  Every comparison is
bit for bit on D and I: against the oracle, against the same handle on stored rows, and ncode against the oracle's count."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.pyoracle import OracleIndex  # noqa: E402
from util import bits  # noqa: E402

D_, NLIST, M_ = 128, 128, 16
KERNEL2 = "kernel=scan16_kernel<1, 2, 1, false, false, false>"
KERNEL4 = "kernel=scan16_kernel<1, 4, 1, false, false, false>"
SHAPES = ((3072, KERNEL2), (1100, KERNEL4))

LENS = [0, 1, 1, 1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 1100] + [1] * 64 + [330] * 38
ONES = list(range(26, 90))         # the 64 lists of one code
L330 = list(range(90, 128))
BIG = 25                           # 1100 codes


def by_len(n):
    return LENS.index(n)


# probe patterns of up to 64 keys (padded with -1, which is a pattern of its own: dead probes between live ones)
PATTERNS = [
    ONES,                                                          # one block with 63 boundaries
    [0, 1, 2, 3, 0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0],              # lengths 0 .. 65: boundaries at lanes 0, 1, 63; empty first, middle, last
    [by_len(63), by_len(65)],                                      # boundaries next to the block edge
    [by_len(127), by_len(129)],
    [by_len(64), by_len(64), by_len(128)],                         # ... and exactly on it
    [by_len(128)], [by_len(127)], [by_len(129)],                   # totals of 128 n, 128 n +- 1
    [by_len(256)], [by_len(255)], [by_len(257)],                   # 256 n, 256 n +- 1
    [by_len(384)], [by_len(383)], [by_len(385)],
    [by_len(255), by_len(257)], [by_len(255), by_len(256)], [by_len(256), by_len(257)],      # 512, 511, 513
    [by_len(383), by_len(385)], [by_len(383), by_len(384)], [by_len(384), by_len(385)],      # 768, 767, 769
    [26, 27, BIG, 28, 29],                                         # the long list between one-code lists
    [-1, 90, -1, by_len(31), 91, -1],                              # -1 keys
    [90, 90, by_len(32), by_len(32), 30, 30, 91],                  # a key twice in adjacent probes, equal coarse_dis: exact ties
    [-1, 0, -1, 0],                                                # all probes dead or empty: total 0
    [by_len(5), by_len(3), by_len(2)],                             # 10 codes: fewer than k = 32
    L330[:32],                                                     # the benchmark's shape: 32 lists of 330
    [BIG] + L330[:10] + [by_len(385), by_len(383)] + ONES[:20],
]


def index():
    import vector_line_quantization_amd as vlq
    rng = np.random.default_rng(29)
    lens = np.array(LENS, np.int64)
    assert len(lens) == NLIST and 24 <= lens.mean() < 1024 and round(float(lens.mean())) == 132, lens.mean()
    coarse = rng.random((NLIST, D_)).astype(np.float32)
    pq = (0.2 * rng.standard_normal((M_, 256, 8))).astype(np.float32)
    off = np.zeros(NLIST + 1, np.int64)
    off[1:] = np.cumsum(lens)
    codes = rng.integers(0, 256, (off[-1], M_), dtype=np.uint8)
    ids = rng.permutation(off[-1]).astype(np.int64)
    ox = OracleIndex(D_, NLIST, M_, 8, coarse, pq)
    ox.set_lists(codes, ids, off)
    g = vlq.GpuIVFPQ(D_, NLIST, M_, 8)
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.set_lists(codes, ids, off)
    return rng, g, ox, coarse


def batch(rng, coarse, patterns, nq, nprobe):
    """pattern j in rows j, j + len(patterns), ...: every row another random query; coarse_dis = the true distances (equal
    for equal keys)"""
    xq = rng.random((nq, D_)).astype(np.float32)
    keys = np.full((nq, nprobe), -1, np.int64)
    for j, p in enumerate(patterns):
        assert len(p) <= nprobe
        keys[j::len(patterns), :len(p)] = p
    cdis = np.empty((nq, nprobe), np.float32)
    for j in range(nprobe):
        cdis[:, j] = ((xq.astype(np.float64) - coarse[np.maximum(keys[:, j], 0)]) ** 2).sum(1)
    return xq, keys, cdis


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def check(g, ox, xq, keys, cdis, k, kernel, what, store_pairs=False):
    nq = len(xq)
    want = ox.search_preassigned(xq, keys, cdis, k, store_pairs=store_pairs, canonical=True)
    before = g.scan_sums_state()
    g.set_scan_sums(1)
    g.stats(reset=True)
    got = g.search_preassigned(xq, keys, cdis, k, store_pairs=store_pairs)
    info = g.last_scan_info()
    ncode = g.stats()[1]
    now = g.scan_sums_state()
    print(what, k, nq, "ncode", ncode, ox.last_ncode, "seen", now[1] - before[1], "und", now[2] - before[2], "fin", now[3] - before[3])
    assert info.endswith(" rows=sums") and kernel in info, (what, info)
    assert now[0] and now[1] - before[1] == nq and now[2] - before[2] == 0, (what, k, nq, now, before)
    assert same(got, want), ("oracle", what, k, nq)
    assert ncode == ox.last_ncode, (what, k, nq, ncode, ox.last_ncode)
    g.set_scan_sums(0)
    ref = g.search_preassigned(xq, keys, cdis, k, store_pairs=store_pairs)
    assert g.last_scan_info().endswith(" rows=stored"), g.last_scan_info()
    g.set_scan_sums(1)
    assert same(got, ref), ("stored rows", what, k, nq)


def case_stream():
    rng, g, ox, coarse = index()
    for nq, kernel in SHAPES:
        xq, keys, cdis = batch(rng, coarse, PATTERNS, nq, 64)
        for k in (1, 10, 32):
            check(g, ox, xq, keys, cdis, k, kernel, "stream")


def case_narrow():
    rng, g, ox, coarse = index()
    one = [[BIG], [90], [by_len(31)], [0], [-1], [26], [by_len(385)]]
    seven = [[26, 27, BIG, 28, 29, by_len(63), by_len(65)], [0, 1, 2, 3, 4, 5, 6], L330[:7], [by_len(64)] * 7]
    for nq, kernel in SHAPES:
        for nprobe, pats in ((1, one), (7, seven)):
            xq, keys, cdis = batch(rng, coarse, pats, nq, nprobe)
            for k in (1, 10, 32):
                check(g, ox, xq, keys, cdis, k, kernel, "nprobe %d" % nprobe)


def case_wide():
    # more than 64 probes: no walking-order records, the stream runs in windows of 64 probes
    rng, g, ox, coarse = index()
    p65 = [ONES + [BIG], [BIG] + ONES, list(range(65))]
    p128 = [list(range(128)), list(range(127, -1, -1)), ONES + list(range(26)) + L330]
    for nq, kernel in SHAPES:
        for nprobe, pats in ((65, p65), (128, p128)):
            xq, keys, cdis = batch(rng, coarse, pats, nq, nprobe)
            for k in (10, 32):
                check(g, ox, xq, keys, cdis, k, kernel, "nprobe %d" % nprobe)


def case_options():
    rng, g, ox, coarse = index()
    for nq, kernel in SHAPES:
        xq, keys, cdis = batch(rng, coarse, PATTERNS, nq, 64)
        g.set_search_options(True, 1, 700)         # cuts in the middle of the longer patterns
        ox.max_codes = 700
        check(g, ox, xq, keys, cdis, 10, kernel, "max_codes 700")
        g.set_search_options(True, 1, 0)
        ox.max_codes = 0
    xq, keys, cdis = batch(rng, coarse, PATTERNS, 3072, 64)
    check(g, ox, xq, keys, cdis, 10, KERNEL2, "store_pairs", store_pairs=True)


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]]()
    print("ok", sys.argv[1])
