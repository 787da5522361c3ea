#!/usr/bin/env python3
"""Range search of IVFFlat (vlq.GpuIVFFlat.range_search, csrc/scan_range_flat.hip) beside the k-NN search of the same index, on
tools/time_ivfflat.py's index: d 128, 1 M vectors of bench.py's generator, 4096 lists (the headline's coarse k-means, same
seeds), nprobe 32, one batch of 10 000 queries, device-resident buffers.

In one process: GpuIVFFlat.search at k = 10 (existing code: the yardstick), range_search at a radius chosen for about 10 hits
per query, and at one for about 1000.  The radii come from the pooled distances of a k = 1024 search (the values at ranks
10 * nq and 1000 * nq; a query with more than 1024 vectors inside the radius makes the true count larger: the counts printed
are the ones found).  Every timed call follows untimed calls of the same shape, the three alternate inside every repetition,
and a row's figure is the median over the repetitions.  A range search synchronises the stream once inside the call (it reads
the number of hits to size the result), so its time is taken on the host clock around call + synchronize; the k-NN search is
timed the same way.  Printed: ms per batch, hits, the list bytes one pass reads (ndis x 4 d) and bytes per second -- for the
range search over BOTH passes (twice the bytes).
    python tools/time_range.py [reps] [out_file]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
out_file = sys.argv[2] if len(sys.argv) > 2 else None
if not torch.cuda.is_available():
    raise SystemExit("tools/time_range.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
a = argparse.Namespace(nq=10000, nb=1000000, nt=100000, d=128, nlist=4096, nprobe=32, k=10, sigma=0.005, gmm_centres=2000, rank=12,
                       spread=0.4)
# tools/time_ivfflat.py's data and coarse quantizer (bench.build_index's generator and seeds, without the PQ)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
centres = torch.rand((a.gmm_centres, a.d), generator=gen, device=dev)
gen.manual_seed(11)
xt = bench.gmm(torch, gen, centres, a.nt, a.sigma, dev, a.rank, a.spread)
gen.manual_seed(22)
xb = bench.gmm(torch, gen, centres, a.nb, a.sigma, dev, a.rank, a.spread)
gen.manual_seed(1234)
coarse = bench.kmeans(torch, xt, a.nlist, 10, gen)
gen.manual_seed(33)
xq = bench.gmm(torch, gen, centres, a.nq, a.sigma, dev, a.rank, a.spread)
torch.cuda.synchronize()

g = vlq.GpuIVFFlat(a.d, a.nlist, device=0, metric="l2")
stream = torch.cuda.current_stream()
g.set_stream(stream.cuda_stream)
g.set_coarse_centroids(coarse.contiguous())
for i0 in range(0, a.nb, 262144):
    g.add(xb[i0:i0 + 262144].contiguous())
g.reclaim_memory()
torch.cuda.synchronize()
assert g.ntotal == a.nb

D = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev)
I = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
Dk, _Ik = g.search(xq, a.nprobe, 1024)
torch.cuda.synchronize()
pool = torch.sort(Dk.flatten()).values
r10, r1000 = float(pool[10 * a.nq]), float(pool[1000 * a.nq])
del Dk, _Ik, pool
g.stats(reset=True)
g.search(xq, a.nprobe, a.k, D=D, I=I)
torch.cuda.synchronize()
_nq, _nlistv, ndis = g.stats(reset=True)

calls = {"knn": lambda: g.search(xq, a.nprobe, a.k, D=D, I=I),
         "range10": lambda: g.range_search(xq, a.nprobe, r10),
         "range1000": lambda: g.range_search(xq, a.nprobe, r1000)}
hits = {"range10": int(calls["range10"]()[0][-1]), "range1000": int(calls["range1000"]()[0][-1])}
info = g.last_scan_info()
for _ in range(3):          # warm-up: clocks up, code objects loaded
    for c in calls.values():
        c()
torch.cuda.synchronize()
ms = {n: [] for n in calls}
for rep in range(reps):
    for n, c in calls.items():
        for _ in range(2):
            c()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c()
        torch.cuda.synchronize()
        ms[n].append((time.perf_counter() - t0) * 1e3)

med = {n: statistics.median(v) for n, v in ms.items()}
nbytes = ndis * 4 * a.d
lines = ["IVFFlat range search beside the k-NN search, bench headline data: d %d, %d vectors, %d lists, nprobe %d, one batch of %d queries; "
         "%d repetitions, medians of call + synchronize on the host clock" % (a.d, a.nb, a.nlist, a.nprobe, a.nq, reps),
         "k-NN search k = %d              %.3f ms (min %.3f max %.3f)   %d bytes of vectors in one pass = %.2f TB/s"
         % (a.k, med["knn"], min(ms["knn"]), max(ms["knn"]), nbytes, nbytes / (med["knn"] * 1e-3) / 1e12)]
for n, radius in (("range10", r10), ("range1000", r1000)):
    lines.append("range search radius %-10.6g %.3f ms (min %.3f max %.3f)   %d hits = %.1f per query, %.2fx the k-NN search, "
                 "2 x %d bytes = %.2f TB/s" % (radius, med[n], min(ms[n]), max(ms[n]), hits[n], hits[n] / a.nq, med[n] / med["knn"], nbytes,
                                               2 * nbytes / (med[n] * 1e-3) / 1e12))
lines.append(info)
print("\n".join(lines), flush=True)
if out_file:
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")
