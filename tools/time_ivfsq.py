#!/usr/bin/env python3
"""IVF scalar quantizer (vlq.GpuIVFSQ, csrc/scan_sq.hip) on the bench headline's data, beside the IVFFlat scan as it stands
(vlq.GpuIVFFlat, csrc/scan_flat.hip) as the yardstick, in one process: d 128, 1 M vectors of bench.py's generator, 4096 lists
(the headline's coarse k-means, same seeds), nprobe 32, k 10, one batch of 10 000 queries, L2, device-resident buffers.

For IVFFlat, SQ8 (QT_8bit) and SQ4 (QT_4bit): the whole search (coarse stage + list scan) and the list scan alone
(search_preassigned over the keys of coarse_search) are timed with events on the index's stream; every timed call follows
untimed calls of the same shape, the indexes alternate inside every repetition, and a row's figure is the median over the
repetitions.  Printed per index: ms per batch, the code bytes the scan must read (codes scanned x code_size), that figure over
the scan time against the 8 TB/s HBM peak, and recall@1 / 1-recall@10 of the first 1000 queries against exact L2 labels
computed on the host.  The scalar quantizer's range is trained (RS_minmax) on the k-means training set.

Behind the timings: the resources of the instantiations that ran (resource_lines below) -- VGPRs and SGPRs as
tools/kernel_regs.sh reads them from the compiled ISA (needs hipcc; it compiles csrc/scan_sq.hip for the device only), the
dynamic LDS of the launch, and the workgroups of four waves a CU holds: min(floor(512 / VGPRs rounded up to 8) waves per SIMD,
floor(160 KB / LDS)).  If SQ8 comes out slower than IVFFlat the tool says so and asks for the instruction count per code from the
disassembly to be filed with the figures.
    python tools/time_ivfsq.py [reps] [out_file]
    python tools/time_ivfsq.py --resources        # the resource lines alone: no device needed"""
import argparse, os, re, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import vector_line_quantization_amd as vlq



def resource_lines(infos):
    """one line per scan_sq_kernel instantiation named in the last_scan_info texts `infos`"""
    here = os.path.dirname(os.path.abspath(__file__))
    try:
        regs = subprocess.run([os.path.join(here, "kernel_regs.sh"), "scan_sq"], capture_output=True, text=True, timeout=900).stdout
    except (OSError, subprocess.TimeoutExpired):
        regs = ""
    out = []
    for info in infos:
        m = re.search(r"kernel=scan_sq_kernel<(\d+), (L2|IP), (\d), (\w+), (\w+)> read=(\w+) lds=(\d+)", info)
        if not m:
            continue
        inst = "scan_sq_kernel<%s, %s, %s, %s, %s>" % (m.group(1), "true" if m.group(2) == "IP" else "false", m.group(3),
                                                      "true" if m.group(4) == "uniform" else "false", "true" if m.group(5) == "order8" else "false")
        lds = int(m.group(7))
        row = [l for l in regs.splitlines() if inst in l]
        if not row:
            out.append("%s: lds %d B; registers not read (tools/kernel_regs.sh needs hipcc)" % (inst, lds))
            continue
        vgpr, sgpr = int(row[0].split()[0]), int(row[0].split()[1])
        waves = min(8, 512 // ((vgpr + 7) // 8 * 8))
        out.append("%s: %d VGPR, %d SGPR, lds %d B -> %d workgroups of 4 waves per CU (registers allow %d waves per SIMD, LDS allows %d workgroups)"
                   % (inst, vgpr, sgpr, lds, min(waves, 160 * 1024 // lds), waves, 160 * 1024 // lds))
    return out


if len(sys.argv) > 1 and sys.argv[1] == "--resources":
    print("\n".join(resource_lines(["kernel=scan_sq_kernel<1, L2, 8, nonuniform, order8> read=tile128 lds=41760",
                                    "kernel=scan_sq_kernel<1, L2, 4, nonuniform, order8> read=tile128 lds=41760"])))
    raise SystemExit(0)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
out_file = sys.argv[2] if len(sys.argv) > 2 else None
if not torch.cuda.is_available():
    raise SystemExit("tools/time_ivfsq.py needs a HIP device: nothing here is measured on a CPU")
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


def fill(g):
    g.set_stream(stream.cuda_stream)
    g.set_coarse_centroids(coarse.contiguous())
    if isinstance(g, vlq.GpuIVFSQ):
        g.train(xt.cpu().numpy())
    for i0 in range(0, a.nb, 262144):
        g.add(xb[i0:i0 + 262144].contiguous())
    g.reclaim_memory()
    torch.cuda.synchronize()
    assert g.ntotal == a.nb
    return g


flat = fill(vlq.GpuIVFFlat(a.d, a.nlist, device=0, metric="l2"))
sq8 = fill(vlq.GpuIVFSQ(a.d, a.nlist, "8bit", device=0, metric="l2"))
sq4 = fill(vlq.GpuIVFSQ(a.d, a.nlist, "4bit", device=0, metric="l2"))
ROWS = [("IVFFlat", flat, 4 * a.d), ("SQ8", sq8, sq8.code_size), ("SQ4", sq4, sq4.code_size)]

D = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev)
I = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
cdis = torch.empty((a.nq, a.nprobe), dtype=torch.float32, device=dev)
keys = torch.empty((a.nq, a.nprobe), dtype=torch.int64, device=dev)
flat.coarse_search(xq, a.nprobe, cdis=cdis, keys=keys)


def scan(g):
    if isinstance(g, vlq.GpuIVFSQ):
        g.search_preassigned(xq, keys, None, a.k, D=D, I=I)
    else:
        g.search_preassigned(xq, keys, a.k, D=D, I=I)


for _n, g, _b in ROWS:          # warm-up: clocks up, code objects loaded
    for _ in range(5):
        g.search(xq, a.nprobe, a.k, D=D, I=I)
        scan(g)
torch.cuda.synchronize()
flat.stats(reset=True)
scan(flat)
_nq, nlistv, ndis = flat.stats(reset=True)      # the three indexes hold the same lists (one coarse stage assigned them)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
times = {(n, w): [] for n, _g, _b in ROWS for w in ("whole", "scan")}
for rep in range(reps):
    for n, g, _b in ROWS:
        for what in ("whole", "scan"):
            call = (lambda: g.search(xq, a.nprobe, a.k, D=D, I=I)) if what == "whole" else (lambda: scan(g))
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            e0.record(stream)
            call()
            e1.record(stream)
            torch.cuda.synchronize()
            times[(n, what)].append(e0.elapsed_time(e1))

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

scan_ms = {}
lines = ["IVF scalar quantizer beside IVFFlat, bench headline data: d %d, %d vectors, %d lists, nprobe %d, k %d, one batch of %d queries, L2; "
         "%d repetitions, medians" % (a.d, a.nb, a.nlist, a.nprobe, a.k, a.nq, reps),
         "codes scanned per batch %d, lists visited %d (the same lists in the three indexes)" % (ndis, nlistv)]
for n, g, row_bytes in ROWS:
    g.search(xq, a.nprobe, a.k, D=D, I=I)
    torch.cuda.synchronize()
    I_h = I.cpu().numpy()
    r1, r10 = float((I_h[:nr, 0] == gt).mean()), float((I_h[:nr] == gt[:, None]).any(1).mean())
    w, s = times[(n, "whole")], times[(n, "scan")]
    sm = scan_ms[n] = statistics.median(s)
    nbytes = ndis * row_bytes
    lines.append("%-7s whole search %.3f ms (min %.3f max %.3f)   list scan %.3f ms (min %.3f max %.3f)   %d bytes per vector: %d bytes of codes = "
                 "%.2f TB/s over the scan = %.1f %% of the 8 TB/s peak   recall@1 %.3f, 1-recall@10 %.3f   %s"
                 % (n, statistics.median(w), min(w), max(w), sm, min(s), max(s), row_bytes, nbytes, nbytes / (sm * 1e-3) / 1e12,
                    100.0 * nbytes / (sm * 1e-3) / 8e12, r1, r10, g.last_scan_info()))
lines += resource_lines([sq8.last_scan_info(), sq4.last_scan_info()])
if scan_ms["SQ8"] > scan_ms["IVFFlat"]:
    lines.append("SQ8 is SLOWER than IVFFlat on the same data: file the instruction count per code from the disassembly with these figures")
print("\n".join(lines), flush=True)
if out_file:
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")
