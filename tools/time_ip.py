#!/usr/bin/env python3
"""Inner-product metric (vlq_ivfpq_set_metric, csrc/scan_ip.hip) against L2 on the bench index: the SAME index contents
(bench.py's headline shape: d 128, 4096 lists, M 16 x 8 bit, nprobe 32, k 10, 10 000 queries) searched under L2 (table mode 1,
the plan's kernel) and under inner product.  Scan milliseconds are HIP events around the scan launch only
(vlq_ivfpq_profile mode 2); the whole search is timed with events around the call, device-resident buffers.  The two metrics
alternate inside every repetition, each timed search follows untimed searches at the same metric, and the figure of a row is
the median over the repetitions.  The code-byte rate is scanned codes x code size / scan time, against the 8 TB/s HBM peak.
    python tools/time_ip.py [reps] [out_file]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
out_file = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda", 0)
a = argparse.Namespace(nq=10000, nb=1000000, nt=100000, d=128, nlist=4096, M=16, nprobe=32, k=10, sigma=0.005,
                       gmm_centres=2000, rank=12, spread=0.4)
g, centres, coarse, pq, xb = bench.build_index(a, dev)
gen = torch.Generator(device=dev); gen.manual_seed(33)
xq = bench.gmm(torch, gen, centres, a.nq, a.sigma, dev, a.rank, a.spread)
D = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev); I = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
g.set_search_options(by_residual=True, use_precomputed_table=1)
scan = {"l2": [], "ip": []}
whole = {"l2": [], "ip": []}
ncode, kernel = {}, {}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
stream = torch.cuda.current_stream()
g.set_stream(stream.cuda_stream)
for metric in ("l2", "ip"):          # warm-up: clocks up, code objects loaded, walk times measured
    g.metric = metric
    for _ in range(10):
        g.search(xq, a.nprobe, a.k, D=D, I=I)
torch.cuda.synchronize()
for rep in range(reps):
    for metric in ("l2", "ip"):
        g.metric = metric
        g.profile(False)
        for _ in range(3):
            g.search(xq, a.nprobe, a.k, D=D, I=I)
        torch.cuda.synchronize()
        e0.record(stream)
        g.search(xq, a.nprobe, a.k, D=D, I=I)
        e1.record(stream)
        torch.cuda.synchronize()
        whole[metric].append(e0.elapsed_time(e1))
        g.stats(reset=True)
        g.profile(2); g.profile_read(reset=True)
        g.search(xq, a.nprobe, a.k, D=D, I=I)
        torch.cuda.synchronize()
        scan[metric].append(g.profile_read(reset=True)["scan_ms"])
        if rep == 0:
            ncode[metric] = g.stats()[1]
            kernel[metric] = g.last_scan_info().split()[0]
g.profile(False)
g.metric = "l2"
lines = ["bench headline shape: d %d, %d lists, M %d x 8 bit, nprobe %d, k %d, %d queries, %d vectors; %d repetitions, medians"
         % (a.d, a.nlist, a.M, a.nprobe, a.k, a.nq, a.nb, reps)]
for m in ("l2", "ip"):
    s = statistics.median(scan[m])
    lines.append("%-3s scan %.3f ms (min %.3f max %.3f)  whole search %.3f ms (min %.3f max %.3f)  codes scanned %d  code bytes %.2f TB/s = %.1f %% of 8 TB/s  %s"
                 % (m, s, min(scan[m]), max(scan[m]), statistics.median(whole[m]), min(whole[m]), max(whole[m]), ncode[m],
                    ncode[m] * a.M / (s * 1e-3) / 1e12, 100.0 * ncode[m] * a.M / (s * 1e-3) / 8e12, kernel[m]))
lines.append("ratio ip / l2: scan %.3f, whole search %.3f" % (statistics.median(scan["ip"]) / statistics.median(scan["l2"]),
                                                             statistics.median(whole["ip"]) / statistics.median(whole["l2"])))
print("\n".join(lines), flush=True)
if out_file:
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")
