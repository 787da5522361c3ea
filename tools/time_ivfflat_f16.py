#!/usr/bin/env python3
"""IVFFlat list scan with float32 and float16 list storage (vlq.GpuIVFFlat(storage=...); csrc/scan_flat.hip, csrc/scan_flat16.hip)
on the data and by the method of tools/time_ivfflat.py: d 128, 1 M vectors of bench.py's generator, 4096 lists, nprobe 32, k 10,
one batch of 10 000 queries, device-resident buffers.

Two indexes over the same vectors and centroids, one per storage.  search_preassigned over the keys of coarse_search (the list
scan alone) is timed with events on the indexes' stream; every timed call follows two untimed calls of the same shape, the two
storages alternate inside every repetition, and a figure is the median over the repetitions with min and max.  Printed per
storage: ms per batch, the bytes the scan must read (ndis x bytes per row), that figure over the scan time as a fraction of the
8 TB/s HBM peak, and recall@1 of the first 1000 queries against exact L2 labels computed on the host from the fp32 vectors.
    python tools/time_ivfflat_f16.py [reps] [out_file]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
out_file = sys.argv[2] if len(sys.argv) > 2 else None
if not torch.cuda.is_available():
    raise SystemExit("tools/time_ivfflat_f16.py needs a HIP device: nothing here is measured on a CPU")
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

stream = torch.cuda.current_stream()
STORAGES = ("f32", "f16")
index = {}
for st in STORAGES:
    g = vlq.GpuIVFFlat(a.d, a.nlist, device=0, metric="l2", storage=st)
    g.set_stream(stream.cuda_stream)
    g.set_coarse_centroids(coarse.contiguous())
    for i0 in range(0, a.nb, 262144):
        g.add(xb[i0:i0 + 262144].contiguous())
    g.reclaim_memory()
    torch.cuda.synchronize()
    assert g.ntotal == a.nb
    index[st] = g

D = {st: torch.empty((a.nq, a.k), dtype=torch.float32, device=dev) for st in STORAGES}
I = {st: torch.empty((a.nq, a.k), dtype=torch.int64, device=dev) for st in STORAGES}
cdis = torch.empty((a.nq, a.nprobe), dtype=torch.float32, device=dev)
keys = torch.empty((a.nq, a.nprobe), dtype=torch.int64, device=dev)
index["f32"].coarse_search(xq, a.nprobe, cdis=cdis, keys=keys)      # (the quantizer is the same in both)
ndis = {}
for st in STORAGES:
    for _ in range(5):          # warm-up: clocks up, code objects loaded
        index[st].search_preassigned(xq, keys, a.k, D=D[st], I=I[st])
    torch.cuda.synchronize()
    index[st].stats(reset=True)
    index[st].search_preassigned(xq, keys, a.k, D=D[st], I=I[st])
    ndis[st] = index[st].stats(reset=True)[2]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
ms = {st: [] for st in STORAGES}
for rep in range(reps):
    for st in STORAGES:
        for _ in range(2):
            index[st].search_preassigned(xq, keys, a.k, D=D[st], I=I[st])
        torch.cuda.synchronize()
        e0.record(stream)
        index[st].search_preassigned(xq, keys, a.k, D=D[st], I=I[st])
        e1.record(stream)
        torch.cuda.synchronize()
        ms[st].append(e0.elapsed_time(e1))
info = {st: index[st].last_scan_info() for st in STORAGES}

# exact labels of the first 1000 queries, on the host
nr = 1000
xq_h = xq[:nr].cpu().numpy()
best = np.full(nr, np.inf, np.float32)
gt = np.zeros(nr, np.int64)
qn = (xq_h * xq_h).sum(1)
for i0 in range(0, a.nb, 65536):
    xbb = xb[i0:i0 + 65536].cpu().numpy()
    d2 = qn[:, None] + (xbb * xbb).sum(1)[None, :] - 2.0 * (xq_h @ xbb.T)
    m, am = d2.min(1), d2.argmin(1)
    upd = m < best
    best[upd], gt[upd] = m[upd], am[upd] + i0

lines = ["IVFFlat list scan by storage, bench headline data: d %d, %d vectors, %d lists, nprobe %d, k %d, one batch of %d queries; "
         "%d repetitions, medians" % (a.d, a.nb, a.nlist, a.nprobe, a.k, a.nq, reps)]
med = {}
for st in STORAGES:
    s = med[st] = statistics.median(ms[st])
    nbytes = ndis[st] * (2 if st == "f16" else 4) * a.d
    r1 = float((I[st].cpu().numpy()[:nr, 0] == gt).mean())
    lines.append("%s: list scan %.3f ms (min %.3f max %.3f)   %s" % (st, s, min(ms[st]), max(ms[st]), info[st]))
    lines.append("     distances computed %d: %d bytes of vectors = %.2f TB/s over the scan = %.1f %% of the 8 TB/s peak; recall@1 %.3f "
                 "(first %d queries, exact L2 labels)" % (ndis[st], nbytes, nbytes / (s * 1e-3) / 1e12, 100.0 * nbytes / (s * 1e-3) / 8e12, r1, nr))
lines.append("f16 / f32 scan time %.3f; labels equal in %.4f of the %d x %d slots"
             % (med["f16"] / med["f32"], float((I["f16"] == I["f32"]).float().mean()), a.nq, a.k))
print("\n".join(lines), flush=True)
if out_file:
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")
