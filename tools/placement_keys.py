#!/usr/bin/env python3
"""How concentrated are the lists that one XCD's chunk of queries probes, under different keys for the scan order?
(the table-row hit rate of the query-major scan is decided by which queries share an XCD.)

The scan sorts the queries by a key and gives XCD x the x-th contiguous eighth of that order; 256 workgroups (= queries)
are resident on an XCD at a time (a "round").  A term2 row can hit the XCD's L2 only if another query of the same round
asked for the same list, so   1 - distinct lists of a round / probes of a round   bounds the row hit rate from above.

Candidate keys of a query (all ranks are list_rank, the spatial order of the lists; list_part = rank * 8 / nlist):
  nearest   the rank of its nearest list                                             (the key up to round 6)
  vote      p* = the partition holding most of its probes (tie: the partition of the nearest probe among the tied);
            the rank of its nearest probe that lies in p*
  median    the median rank of its probes

   python tools/placement_keys.py                                   the bench's default data
   python tools/placement_keys.py --sigma 0.03 --rank 0 --spread 0  G1
   --host: no device -- torch's CPU generator draws other numbers than the device's (same distribution), and the coarse
           keys come from a float32 matmul instead of coarse_search."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def spatial_list_rank(cent):
    """numpy restatement of spatial_list_rank (csrc/coarse_stage.hip): recursive two-means bisection of the centroids"""
    nlist = cent.shape[0]
    order = np.arange(nlist)
    stack = [(0, nlist)]
    while stack:
        lo, hi = stack.pop()
        n = hi - lo
        if n <= 2:
            continue
        idx = order[lo:hi]
        x = cent[idx]
        fb = int(np.argmax(((x - x[0]) ** 2).sum(1)))
        cb = x[fb].copy()
        fa = int(np.argmax(((x - cb) ** 2).sum(1)))
        ca = x[fa].copy()
        na = 0
        for _ in range(4):
            toa = ((x - ca) ** 2).sum(1) < ((x - cb) ** 2).sum(1)
            na = int(toa.sum())
            if na == 0 or na == n:
                break
            ca = x[toa].astype(np.float64).mean(0).astype(np.float32)
            cb = x[~toa].astype(np.float64).mean(0).astype(np.float32)
        if na == 0 or na == n:
            continue
        order[lo:hi] = np.concatenate([idx[toa], idx[~toa]])
        stack.append((lo, lo + na))
        stack.append((lo + na, hi))
    rank = np.empty(nlist, np.int64)
    rank[order] = np.arange(nlist)
    return rank


def candidate_keys(keys, rank, nlist):
    r = rank[keys]                                  # [nq][nprobe], nearest first
    part = r * 8 // nlist
    votes = (part[:, :, None] == np.arange(8)[None, None, :]).sum(1)          # [nq][8]
    top = votes.max(1)
    tied = np.take_along_axis(votes, part, 1) == top[:, None]                  # probes whose partition holds the most
    first = tied.argmax(1)                                                     # the nearest of them
    return {
        "nearest": r[:, 0],
        "vote": r[np.arange(r.shape[0]), first],
        "median": np.sort(r, 1)[:, r.shape[1] // 2],
    }


def concentration(keys, key, nlist, round_wg=256):
    nq, nprobe = keys.shape
    order = np.argsort(key, kind="stable")
    chunk = (nq + 7) // 8
    distinct_chunk, visits, distinct_round, rounds = [], 0, 0, 0
    for x in range(8):
        qs = order[x * chunk:(x + 1) * chunk]
        if qs.size == 0:
            continue
        distinct_chunk.append(np.unique(keys[qs]).size)
        for r0 in range(0, qs.size, round_wg):
            kr = keys[qs[r0:r0 + round_wg]]
            visits += kr.size
            distinct_round += np.unique(kr).size
            rounds += 1
    # neighbours of the order: the share of a query's probes its successor probes too (walk_stat_kernel's statistic)
    a, b = keys[order[:-1]], keys[order[1:]]
    shared = (a[:, :, None] == b[:, None, :]).any(2).mean()
    return (float(np.mean(distinct_chunk)), int(np.max(distinct_chunk)), visits / distinct_round,
            1.0 - distinct_round / visits, float(shared))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--nt", type=int, default=100000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--sigma", type=float, default=0.005)
    ap.add_argument("--gmm-centres", type=int, default=2000)
    ap.add_argument("--rank", type=int, default=12)
    ap.add_argument("--spread", type=float, default=0.4)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    dev = torch.device("cpu") if args.host else torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    centres = torch.rand((args.gmm_centres, args.d), generator=gen, device=dev)
    gen.manual_seed(11)
    xt = bench.gmm(torch, gen, centres, args.nt, args.sigma, dev, args.rank, args.spread)
    gen.manual_seed(1234)
    coarse = bench.kmeans(torch, xt, args.nlist, 10, gen)
    gen.manual_seed(33)
    xq = bench.gmm(torch, gen, centres, args.nq, args.sigma, dev, args.rank, args.spread)
    if args.host:
        d2 = (coarse * coarse).sum(1)[None, :] - 2.0 * xq @ coarse.T
        keys = d2.topk(args.nprobe, dim=1, largest=False).indices.numpy()
    else:
        import vector_line_quantization_amd as vlq
        g = vlq.GpuIVFPQ(args.d, args.nlist, 16, 8, device=0)
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        g.set_coarse_centroids(coarse.contiguous())
        _cd, keys_d = g.coarse_search(xq.contiguous(), args.nprobe)
        torch.cuda.synchronize()
        keys = keys_d.cpu().numpy()
    rank = spatial_list_rank(coarse.cpu().numpy())
    print("nq %d  nlist %d  nprobe %d  sigma %g rank %d spread %g  (%s)" % (
        args.nq, args.nlist, args.nprobe, args.sigma, args.rank, args.spread, "host" if args.host else "device keys"))
    print("%-8s  %21s  %17s  %16s  %16s" % ("key", "distinct lists / chunk", "visits / list / rd", "not first in rd", "neighbours share"))
    for name, key in candidate_keys(keys, rank, args.nlist).items():
        dc, dmax, vis, bound, shared = concentration(keys, key, args.nlist)
        print("%-8s  %12.0f (max %4d)  %17.2f  %15.1f%%  %15.1f%%" % (name, dc, dmax, vis, 100 * bound, 100 * shared))


if __name__ == "__main__":
    main()
