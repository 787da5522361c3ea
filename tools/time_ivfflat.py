#!/usr/bin/env python3
"""IVFFlat (vlq.GpuIVFFlat, csrc/scan_flat.hip) on the bench headline's data: d 128, 1 M vectors of bench.py's generator, 4096
lists (the headline's coarse k-means, same seeds), nprobe 32, k 10, one batch of 10 000 queries, device-resident buffers.

The whole search (coarse stage + list scan) and the list scan alone (search_preassigned over the keys of coarse_search) are
timed with events on the index's stream; every timed call follows untimed calls of the same shape, the two alternate inside
every repetition, and a row's figure is the median over the repetitions.  Printed: ms per batch, the bytes the scan must read
(ndis x 4 d), that figure over the scan time as a fraction of the 8 TB/s HBM peak, and recall@1 / 1-recall@10 of the first
1000 queries against exact L2 labels computed on the host (the data are integer-valued: every distance is exact in fp32).
    python tools/time_ivfflat.py [reps] [out_file]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
out_file = sys.argv[2] if len(sys.argv) > 2 else None
if not torch.cuda.is_available():
    raise SystemExit("tools/time_ivfflat.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
a = argparse.Namespace(nq=10000, nb=1000000, nt=100000, d=128, nlist=4096, nprobe=32, k=10, sigma=0.005, gmm_centres=2000, rank=12,
                       spread=0.4)
# bench.build_index's data and coarse quantizer (same generator, same seeds), without the PQ
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
cdis = torch.empty((a.nq, a.nprobe), dtype=torch.float32, device=dev)
keys = torch.empty((a.nq, a.nprobe), dtype=torch.int64, device=dev)
g.coarse_search(xq, a.nprobe, cdis=cdis, keys=keys)
for _ in range(5):          # warm-up: clocks up, code objects loaded
    g.search(xq, a.nprobe, a.k, D=D, I=I)
    g.search_preassigned(xq, keys, a.k, D=D, I=I)
torch.cuda.synchronize()
g.stats(reset=True)
g.search_preassigned(xq, keys, a.k, D=D, I=I)
_nq, nlistv, ndis = g.stats(reset=True)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
whole, scan = [], []
for rep in range(reps):
    for what, out in (("whole", whole), ("scan", scan)):
        call = (lambda: g.search(xq, a.nprobe, a.k, D=D, I=I)) if what == "whole" else (lambda: g.search_preassigned(xq, keys, a.k, D=D, I=I))
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        e0.record(stream)
        call()
        e1.record(stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
g.search(xq, a.nprobe, a.k, D=D, I=I)
torch.cuda.synchronize()
info = g.last_scan_info()
g.stats(reset=True)

# exact labels of the first 1000 queries, on the host
nr = 1000
xq_h, I_h = xq[:nr].cpu().numpy(), I.cpu().numpy()
best = np.full(nr, np.inf, np.float32)
gt = np.zeros(nr, np.int64)
qn = (xq_h * xq_h).sum(1)
for i0 in range(0, a.nb, 65536):
    xbb = xb[i0:i0 + 65536].cpu().numpy()
    d2 = qn[:, None] + (xbb * xbb).sum(1)[None, :] - 2.0 * (xq_h @ xbb.T)
    m, am = d2.min(1), d2.argmin(1)
    upd = m < best
    best[upd], gt[upd] = m[upd], am[upd] + i0
r1, r10 = float((I_h[:nr, 0] == gt).mean()), float((I_h[:nr] == gt[:, None]).any(1).mean())

s, w = statistics.median(scan), statistics.median(whole)
nbytes = ndis * 4 * a.d
lines = ["IVFFlat, bench headline data: d %d, %d vectors, %d lists, nprobe %d, k %d, one batch of %d queries; %d repetitions, medians"
         % (a.d, a.nb, a.nlist, a.nprobe, a.k, a.nq, reps),
         "whole search %.3f ms (min %.3f max %.3f)   list scan %.3f ms (min %.3f max %.3f)   %s" % (w, min(whole), max(whole), s, min(scan), max(scan), info),
         "distances computed %d, lists visited %d: %d bytes of vectors = %.2f TB/s over the scan = %.1f %% of the 8 TB/s peak"
         % (ndis, nlistv, nbytes, nbytes / (s * 1e-3) / 1e12, 100.0 * nbytes / (s * 1e-3) / 8e12),
         "recall@1 %.3f, 1-recall@10 %.3f against exact L2 labels (first %d queries; the IVFPQ headline: recall@1 0.48)" % (r1, r10, nr)]
print("\n".join(lines), flush=True)
if out_file:
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")
