#!/usr/bin/env python3
"""Polysemous Hamming filtering (vlq_ivfpq_set_polysemous_ht, csrc/scan_poly.hip) on the bench index, table mode 1: scan
milliseconds (HIP events around the scan kernel only), pass rate and recall@1 against the unfiltered search of the same
handle, for a sweep of thresholds.  ht = 0 is the unfiltered scan: the plan's kernel, which this mode does not touch.  The
thresholds alternate inside every repetition (ht = 0 among them), so drift of the clocks falls on all rows alike; each timed
search follows one untimed search at the same threshold.  The figure of a row is the median over the repetitions.  The bench
data's centroids are not polysemous-trained: the recall column is the cost of filtering an untrained codebook.
    python tools/time_polysemous.py [reps]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
HTS = (0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 129)
dev = torch.device("cuda", 0)
a = argparse.Namespace(nq=10000, nb=1000000, nt=100000, d=128, nlist=4096, M=16, nprobe=32, k=10, sigma=0.005,
                       gmm_centres=2000, rank=12, spread=0.4)
g, centres, coarse, pq, xb = bench.build_index(a, dev)
gen = torch.Generator(device=dev); gen.manual_seed(33)
xq = bench.gmm(torch, gen, centres, a.nq, a.sigma, dev, a.rank, a.spread)
D = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev); I = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
g.set_search_options(by_residual=True, use_precomputed_table=1)
ms = {ht: [] for ht in HTS}
rate, rec, kernel = {}, {}, {}
I0 = None
for rep in range(reps):
    for ht in HTS:
        g.set_polysemous_ht(ht)
        g.profile(False)
        g.search(xq, a.nprobe, a.k, D=D, I=I)
        torch.cuda.synchronize()
        g.stats(reset=True); g.polysemous_stats(reset=True)
        g.profile(2); g.profile_read(reset=True)
        g.search(xq, a.nprobe, a.k, D=D, I=I)
        torch.cuda.synchronize()
        ms[ht].append(g.profile_read(reset=True)["scan_ms"])
        if rep == 0:
            kernel[ht] = g.last_scan_info().split()[0]
            rate[ht] = g.polysemous_stats() / float(g.stats()[1]) if ht else 1.0
            if ht == 0: I0 = I.clone()
            rec[ht] = float((I[:, 0] == I0[:, 0]).float().mean())
g.profile(False)
g.set_polysemous_ht(0)
print("%5s %10s %10s %10s" % ("ht", "scan ms", "pass rate", "recall@1"))
for ht in HTS:
    print("%5d %10.3f %10.4f %10.4f   (min %.3f max %.3f of %d; %s)" % (ht, statistics.median(ms[ht]), rate[ht], rec[ht], min(ms[ht]),
                                                                        max(ms[ht]), reps, kernel[ht]), flush=True)
