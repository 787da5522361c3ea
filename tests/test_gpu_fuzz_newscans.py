"""GPU: seeded random configurations of the inner-product scan, the polysemous scan and the IVFFlat scan against their
restatements (tests/ip_ref.py, tests/polysemous_ref.py over the oracle, tests/ivfflat_ref.py), bit for bit: odd M / dsub /
nbits / d, one list and many, an empty index, nprobe beyond nlist, k beyond what a query scans, max_codes cuts, thresholds
from nothing-passes to everything-passes, host and device buffers, batches on both sides of the 20-query coarse switch and
of the 1024-query ordering switch.  VLQ_FUZZ_NEWSCAN_SEEDS=240 for a soak run."""
import os

import numpy as np
import pytest

import ip_ref
import ivfflat_ref as fr
import vector_line_quantization_amd as vlq
from oracle import pyoracle
from polysemous_ref import labels_to_ids, oracle_filtered, oracle_scan
from util import bits

pytestmark = pytest.mark.gpu
KINDS = ("ip", "poly", "flat")
SAMPLE = 40            # rows compared with the restatement when the batch is larger (the rest: batch independence)


def draw(seed):
    rng = np.random.default_rng(7000 + seed)
    c = dict(kind=KINDS[seed % 3],                                         # every kind in any three consecutive seeds
             nlist=int(rng.choice([1, 2, 7, 33])), nb=int(rng.choice([0, 5, 200, 3000, 3000])),
             nq=int(rng.choice([1, 7, 19, 20, 33, 1100])), nprobe=int(rng.choice([1, 3, 16, 64, 200])),
             k=int(rng.choice([1, 5, 64, 65, 300])), max_codes=int(rng.choice([0, 0, 50, 400])),
             device=bool(rng.integers(0, 2)), store_pairs=bool(rng.integers(0, 2)))
    if c["kind"] == "flat":
        c["d"] = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 12, 16, 30, 33, 36, 64, 68, 100, 129, 132]))
        c["metric"] = str(rng.choice(["l2", "ip"]))
        c["max_codes"] = 0
        return rng, c
    if c["kind"] == "ip":
        c["M"] = int(rng.choice([1, 2, 3, 4, 5, 8, 12, 13, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64]))
        c["nbits"] = int(rng.choice([8, 8, 8, 8, 4, 5, 6, 7]))
        c["mode"] = int(rng.choice([1, 2]))                                 # 2 = not by_residual
    else:
        c["M"] = int(rng.choice(np.arange(4, 65, 4)))
        c["nbits"] = int(rng.choice([8, 8, 8, 5, 6]))
        c["mode"] = int(rng.choice([0, 1, 2]))
        c["ht_pick"] = int(rng.integers(0, 4))                              # 1, the 10 % quantile, the median, 8 M + 1
    c["dsub"] = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8]))
    c["d"] = c["M"] * c["dsub"]
    return rng, c


def lists_and_probes(rng, c):
    """list offsets and ids of nb vectors in nlist imbalanced lists; per query up to nprobe distinct keys at random places of
    a row of -1, a fifth of them knocked out; the sample's rows and the map from batch rows to sample rows"""
    nlist, nb = c["nlist"], c["nb"]
    lens = rng.multinomial(nb, rng.dirichlet(np.full(nlist, 0.7)))
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    ids = rng.permutation(max(nb, 1))[:nb].astype(np.int64) * 3 - 5
    ns = min(c["nq"], SAMPLE)
    keys = np.full((ns, c["nprobe"]), -1, np.int64)
    for i in range(ns):
        n = min(nlist, c["nprobe"])
        keys[i, np.sort(rng.permutation(c["nprobe"])[:n])] = rng.permutation(nlist)[:n]
    keys[rng.random(keys.shape) < 0.2] = -1
    src = rng.permutation(np.arange(c["nq"]) % ns)                        # batch row -> sample row
    return off, ids, keys, src


def to_device(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def run(g, c, call, sample_args, src):
    """the sample alone and, for a larger batch, the whole batch: every batch row must be its sample row"""
    def once(args):
        if c["device"]:
            D, I = call(*to_device(*args))
            g.stats()                      # synchronises the index's stream
            return D.cpu().numpy(), I.cpu().numpy()
        return call(*args)

    D, I = once(sample_args)
    if c["nq"] > D.shape[0]:
        Db, Ib = once([np.ascontiguousarray(a[src]) for a in sample_args])
        assert np.array_equal(bits(Db), bits(D[src])) and np.array_equal(Ib, I[src]), c
    return D, I


@pytest.mark.parametrize("seed", range(int(os.environ.get("VLQ_FUZZ_NEWSCAN_SEEDS", "24"))))
def test_random_configuration(seed):
    rng, c = draw(seed)
    off, ids, keys, src = lists_and_probes(rng, c)
    ns, d, k, nlist = keys.shape[0], c["d"], c["k"], c["nlist"]
    xq = rng.standard_normal((ns, d)).astype(np.float32)
    coarse = rng.standard_normal((nlist, d)).astype(np.float32)

    if c["kind"] == "flat":
        vecs = rng.standard_normal((c["nb"], d)).astype(np.float32)
        g = vlq.GpuIVFFlat(d, nlist, device=0, metric=c["metric"])
        g.set_coarse_centroids(coarse)
        g.set_lists(vecs, ids, off)
        De, Ie, nv, nd = fr.search_preassigned(dict(vecs=vecs, ids=ids, list_offsets=off), xq, keys, k, c["metric"])
        g.stats(reset=True)
        D, I = run(g, c, lambda x, kk: g.search_preassigned(x, kk, k), [xq, keys], src)
        assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie), c
        if c["nq"] == ns:
            assert g.stats() == (ns, int(nv.sum()), int(nd.sum())), c
        g.close()
        return

    M, nbits = c["M"], c["nbits"]
    ksub = 1 << nbits
    pq = (0.5 * rng.standard_normal((M, ksub, c["dsub"]))).astype(np.float32)
    codes = rng.integers(0, ksub, (c["nb"], M), dtype=np.uint8)
    cdis = (rng.random(keys.shape) * 9 + 1).astype(np.float32)
    by_res, upt = c["mode"] != 2, 1 if c["mode"] == 1 else 0
    g = vlq.GpuIVFPQ(d, nlist, M, nbits, device=0, metric="ip" if c["kind"] == "ip" else "l2")
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.set_search_options(by_res, upt, c["max_codes"])
    g.set_lists(codes, ids, off)
    sp = c["store_pairs"]
    call = lambda x, kk, cd: g.search_preassigned(x, kk, cd, k, store_pairs=sp)

    if c["kind"] == "ip":
        z = dict(coarse_centroids=coarse, pq_centroids=pq, codes=codes, ids=ids, list_offsets=off, by_residual=int(by_res),
                 max_codes=c["max_codes"])
        De, Ie, nc = ip_ref.search_preassigned(z, xq, keys, k, store_pairs=sp)
        g.stats(reset=True)
        D, I = run(g, c, call, [xq, keys, cdis], src)
        assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie), c
        assert "kernel=scan_ip_kernel<%d>" % (M // 4 if (nbits == 8 and M % 4 == 0) else 0) in g.last_scan_info()
        if c["nq"] == ns:
            assert g.stats() == (ns, int(nc.sum())), c
        g.close()
        return

    ox = pyoracle.OracleIndex(d, nlist, M, nbits, coarse, pq, codes=codes, ids=ids, list_offsets=off, by_residual=by_res,
                              use_precomputed_table=upt, max_codes=c["max_codes"])
    scan = oracle_scan(ox, xq, keys, cdis)
    assert np.array_equal(g.query_codes(xq, keys), scan["qcodes"]), c
    hd = np.sort(np.concatenate(scan["hd"])) if scan["ncode"].sum() else np.array([8, 16], np.int64)
    ht = [1, int(hd[int(0.10 * hd.size)]) + 1, int(hd[hd.size // 2]) + 1, 8 * M + 1][c["ht_pick"]]
    De, Pe, npass, ncode = oracle_filtered(scan, ht, k)
    Ie = Pe if sp else labels_to_ids(off, ids, Pe)
    g.set_polysemous_ht(ht)
    g.stats(reset=True)
    g.polysemous_stats(reset=True)
    D, I = run(g, c, call, [xq, keys, cdis], src)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie), (c, ht)
    assert "kernel=scan_poly_kernel<%d>" % (M // 4) in g.last_scan_info()
    if c["nq"] == ns:
        assert g.stats() == (ns, int(ncode.sum())) and g.polysemous_stats() == int(npass.sum()), (c, ht)
    g.close()
