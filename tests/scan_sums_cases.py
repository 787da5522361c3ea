"""The cases of tests/test_gpu_scan_sums.py, run in a fresh process each (python tests/scan_sums_cases.py CASE): the walking
order is a per-process switch, and a handle that dropped the stored-sums loop must not be shared with another case.

Common index: d 128, nlist 64, M 16, about 20 000 vectors of the benchmark generator's byte data (bench.py: gmm), 3 000 of them
drawn around one centre so that lists beyond 1 000 codes exist (the further-chunks path of the two-wave shape starts at 384
codes), one probed list left empty, nprobe 16.  Every comparison is bit for bit on D and I."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.pyoracle import OracleIndex  # noqa: E402
from util import bits  # noqa: E402

D_, NLIST, M_, NPROBE = 128, 64, 16, 16
KERNEL2 = "kernel=scan16_kernel<1, 2, 1, false, false, false>"
KERNEL4 = "kernel=scan16_kernel<1, 4, 1, false, false, false>"


def gmm(rng, centres, sub, n, pick=None, spread=0.4):
    """bench.py's generator G1 with its default sigma / rank / spread, on the CPU"""
    if pick is None:
        pick = rng.integers(0, centres.shape[0], n)
    x = centres[pick] + 0.005 * rng.standard_normal((n, D_)) + spread * rng.standard_normal((n, 12)) @ sub
    return np.clip(np.round(x * 255.0), 0, 255).astype(np.float32)


def nearest(x, c):
    """index of the nearest row of c for every row of x, in float64 about the data's mean (offset data: |x|^2 would drown the rest)"""
    mu = x.mean(0, dtype=np.float64)
    x, c = x.astype(np.float64) - mu, c.astype(np.float64) - mu
    return ((c * c).sum(1)[None] - 2.0 * x @ c.T).argmin(1)


def kmeans(rng, x, k, niter):
    c = x[rng.permutation(len(x))[:k]].astype(np.float64)
    for _ in range(niter):
        a = nearest(x, c)
        for j in range(k):
            s = x[a == j]
            if len(s):
                c[j] = s.mean(0, dtype=np.float64)
    return c.astype(np.float32)


def train(rng, xb):
    coarse = kmeans(rng, xb, NLIST, 8)
    res = xb - coarse[nearest(xb, coarse)]
    pq = np.stack([kmeans(rng, res[:, m * 8:(m + 1) * 8], 256, 4) for m in range(M_)])
    return coarse, pq


def oracle_from(g, coarse, pq, max_codes=0):
    """an oracle over exactly the lists the handle holds"""
    codes, ids, off = [], [], [0]
    for i in range(NLIST):
        c, ii = g.get_list(i)
        codes.append(c.reshape(-1, M_))
        ids.append(ii)
        off.append(off[-1] + len(ii))
    return OracleIndex(D_, NLIST, M_, 8, coarse, pq, codes=np.concatenate(codes), ids=np.concatenate(ids),
                       list_offsets=np.array(off, np.int64), max_codes=max_codes)


def common_world(seed=7):
    """the host side of common(): the trained oracle index with its lists, the queries and the generator's state"""
    rng = np.random.default_rng(seed)
    centres = rng.random((200, D_))
    sub = rng.standard_normal((12, D_)) / 12 ** 0.5
    xb = np.concatenate([gmm(rng, centres, sub, 17000), gmm(rng, centres, sub, 3000, pick=np.full(3000, 5), spread=0.08)])
    coarse, pq = train(rng, xb[:17000])                # (the dense cluster is not in the training set: it falls into few lists)
    ox = OracleIndex(D_, NLIST, M_, 8, coarse, pq)
    assign, _ = ox.encode(xb, canonical=True)
    lens = np.bincount(assign, minlength=NLIST)
    empty = int(np.argsort(lens)[NLIST // 2])          # a list of ordinary size, probed like its neighbours
    xb = xb[assign != empty]
    ox.add(xb, canonical=True)
    lens = np.diff(ox.list_offsets)
    assert lens[empty] == 0 and lens.max() > 1000 and 24 <= lens.mean() < 1024, (lens[empty], lens.max(), lens.mean())
    xq = gmm(rng, centres, sub, 3072)
    return rng, ox, coarse, pq, xq, (centres, sub)


def common(seed=7):
    import vector_line_quantization_amd as vlq
    rng, ox, coarse, pq, xq, (centres, sub) = common_world(seed)
    g = vlq.GpuIVFPQ(D_, NLIST, M_, 8)
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.set_lists(ox.codes, ox.ids, ox.list_offsets)
    return rng, g, ox, coarse, pq, xq, (centres, sub)


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def state_delta(g, before):
    now = g.scan_sums_state()
    return now[0], now[1] - before[1], now[2] - before[2], now[3] - before[3]


def case_shapes():
    rng, g, ox, coarse, pq, xq, _ = common()
    for nq, kernel in ((3072, KERNEL2), (1100, KERNEL4)):
        x = xq[:nq]
        for k in (1, 10, 32):
            before = g.scan_sums_state()
            g.set_scan_sums(1)
            got = g.search(x, NPROBE, k)
            info = g.last_scan_info()
            en, seen, und, fin = state_delta(g, before)
            assert info.endswith(" rows=sums") and kernel in info, info
            assert en and seen == nq and und == 0 and 0 < fin <= nq * (k + 8), (nq, k, en, seen, und, fin)
            assert same(got, ox.search(x, NPROBE, k, canonical=True)), ("oracle", nq, k)
            g.set_scan_sums(0)
            ref = g.search(x, NPROBE, k)
            assert g.last_scan_info().endswith(" rows=stored")
            assert same(got, ref), ("stored rows", nq, k)
        g.set_scan_sums(1)
        for k in (33, 64):
            got = g.search(x, NPROBE, k)
            info = g.last_scan_info()
            assert info.endswith(" rows=stored") and kernel in info, info
            assert same(got, ox.search(x, NPROBE, k, canonical=True)), ("oracle", nq, k)


def tie_index(distinct):
    """lists of `distinct` different codes each, repeated in turn to the list's length (4: the data of test_gpu_ties.py)"""
    import vector_line_quantization_amd as vlq
    rng = np.random.default_rng(3)
    coarse = rng.random((NLIST, D_)).astype(np.float32)
    pq = (0.2 * rng.standard_normal((M_, 256, 8))).astype(np.float32)
    lens = rng.integers(200, 500, NLIST)
    off = np.zeros(NLIST + 1, np.int64)
    off[1:] = np.cumsum(lens)
    codes = np.empty((off[-1], M_), np.uint8)
    for l in range(NLIST):
        few = rng.integers(0, 256, (distinct(lens[l]), M_), dtype=np.uint8)
        codes[off[l]:off[l + 1]] = few[np.arange(lens[l]) % len(few)]
    ids = rng.permutation(off[-1]).astype(np.int64)
    ox = OracleIndex(D_, NLIST, M_, 8, coarse, pq)
    ox.set_lists(codes, ids, off)
    g = vlq.GpuIVFPQ(D_, NLIST, M_, 8)
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.set_lists(codes, ids, off)
    return rng, g, ox


def case_ties():
    # Every code three times in its list: each k-th distance is tied, the finalists resolve it by position.  Three equal codes
    # are three finalists; for more than 64 of them over twenty distinct codes would have to lie within 2.25 eps (about 1e-3 of
    # distances that differ in the first digit): every query is decided.
    # Four distinct codes per list: runs of 50 to 125 equal codes, more than the 64 finalists a query may have -- those queries
    # come out right through the stored-rows loop.
    for distinct, want_undecided in ((lambda n: (n + 2) // 3, False), (lambda n: 4, True)):
        for nq in (3072, 1100):
            rng, g, ox = tie_index(distinct)          # (a fresh handle: one that dropped the loop stays on stored rows)
            xq = rng.random((nq, D_)).astype(np.float32)
            got = g.search(xq, NPROBE, 10)
            assert g.last_scan_info().endswith(" rows=sums"), g.last_scan_info()
            en, seen, und, fin = g.scan_sums_state()
            print("ties", want_undecided, nq, en, seen, und, fin)
            assert same(got, ox.search(xq, NPROBE, 10, canonical=True)), ("oracle", want_undecided, nq)
            assert seen == nq and (und > 0) == want_undecided, (want_undecided, nq, und)


def case_defeat():
    """coordinates 1000 + N(0, 0.01^2), not rounded: the distances of a query's codes differ by far less than the bound"""
    import vector_line_quantization_amd as vlq
    rng = np.random.default_rng(11)
    xb = (1000.0 + 0.01 * rng.standard_normal((20000, D_))).astype(np.float32)
    coarse, pq = train(rng, xb)
    ox = OracleIndex(D_, NLIST, M_, 8, coarse, pq)
    ox.add(xb, canonical=True)
    g = vlq.GpuIVFPQ(D_, NLIST, M_, 8)
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.set_lists(ox.codes, ox.ids, ox.list_offsets)
    xq = (1000.0 + 0.01 * rng.standard_normal((3072, D_))).astype(np.float32)
    want = ox.search(xq, NPROBE, 10, canonical=True)
    got = g.search(xq, NPROBE, 10)
    assert g.last_scan_info().endswith(" rows=sums"), g.last_scan_info()
    assert same(got, want)
    en, seen, und, fin = g.scan_sums_state()
    assert seen == 3072 and und == 3072 and not en, (en, seen, und, fin)
    got = g.search(xq, NPROBE, 10)
    assert g.last_scan_info().endswith(" rows=stored"), g.last_scan_info()
    assert same(got, want)
    g.set_lists(ox.codes, ox.ids, ox.list_offsets)        # new lists: the handle tries again
    assert g.scan_sums_state()[0]


def case_nonfinite():
    rng, g, ox, coarse, pq, xq, _ = common()
    x = xq.copy()
    odd = {17: np.nan, 400: np.inf, 1201: -np.inf, 2000: 1e30, 3000: -1e30}
    for row, v in odd.items():
        x[row, 5::7] = v
    before = g.scan_sums_state()
    got = g.search(x, NPROBE, 10)
    assert g.last_scan_info().endswith(" rows=sums")
    en, seen, und, fin = state_delta(g, before)
    assert en and seen == 3072 and und <= len(odd), (en, seen, und)
    g.set_scan_sums(0)
    ref = g.search(x, NPROBE, 10)
    assert same(got, ref)
    normal = np.setdiff1d(np.arange(3072), list(odd))
    want = ox.search(x[normal], NPROBE, 10, canonical=True)
    assert same((got[0][normal], got[1][normal]), want)


def case_stale():
    rng, g, ox, coarse, pq, xq, (centres, sub) = common()
    x = xq[:3072]

    def check(what, c=coarse, p=pq):
        o = oracle_from(g, c, p)
        got = g.search(x, NPROBE, 10)
        assert g.last_scan_info().endswith(" rows=sums"), (what, g.last_scan_info())
        assert same(got, o.search(x, NPROBE, 10, canonical=True)), what
        return o

    check("set_lists")
    g.add(gmm(rng, centres, sub, 6000))                 # regrows: the packed lists have no slack
    check("add that regrows")
    g.add(gmm(rng, centres, sub, 200))                  # fits the 25 % slack the regrown layout left
    o = check("add that fits the slack")
    g.reserve_memory(40000)
    check("reserve_memory")
    g.reclaim_memory()
    check("reclaim_memory")
    cut = [(a, max(a, b - 1)) for a, b in zip(o.list_offsets[:-1], o.list_offsets[1:])]      # every list loses its last code
    g.set_lists(np.concatenate([o.codes[a:b] for a, b in cut]), np.concatenate([o.ids[a:b] for a, b in cut]),
                np.concatenate([[0], np.cumsum([b - a for a, b in cut])]).astype(np.int64))
    check("second set_lists")
    pq2 = (pq * 1.25 + 0.5).astype(np.float32)
    g.set_pq_centroids(pq2)
    g.search(x[:8], NPROBE, 1)
    check("second set_pq_centroids", coarse, pq2)
    coarse2 = (coarse + 1.5).astype(np.float32)
    g.set_coarse_centroids(coarse2)
    check("second set_coarse_centroids", coarse2, pq2)


def case_preassigned():
    rng, g, ox, coarse, pq, xq, _ = common()
    x = xq[:3072]
    cdis, keys = ox.coarse_search(x, NPROBE, canonical=True)
    keys = keys.copy()
    keys[::5, 3] = -1
    keys[1::7, 9] = keys[1::7, 2]                       # a repeated key: the list is scanned twice
    for max_codes, store_pairs in ((0, False), (0, True), (700, False)):
        g.set_search_options(True, 1, max_codes)
        ox.max_codes = max_codes
        g.set_scan_sums(1)
        got = g.search_preassigned(x, keys, cdis, 10, store_pairs=store_pairs)
        assert g.last_scan_info().endswith(" rows=sums"), g.last_scan_info()
        g.set_scan_sums(0)
        ref = g.search_preassigned(x, keys, cdis, 10, store_pairs=store_pairs)
        assert g.last_scan_info().endswith(" rows=stored")
        assert same(got, ref), (max_codes, store_pairs)
        assert same(got, ox.search_preassigned(x, keys, cdis, 10, store_pairs=store_pairs, canonical=True)), (max_codes, store_pairs)


if __name__ == "__main__":
    globals()["case_" + sys.argv[1]]()
    print("ok", sys.argv[1])
