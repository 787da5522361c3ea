#!/usr/bin/env python3
"""Flat exact k-NN and refine with float32 and float16 vector storage (vlq.GpuFlat(storage=...); csrc/scan_knn.hip against
csrc/scan_knn16.hip, csrc/refine_flat.hip against csrc/refine_flat16.hip) by the method of tools/time_knn.py and
tools/time_ivfflat_f16.py: d 128, 1 M random Gaussian vectors, L2 and inner product, device-resident buffers.

Two handles over the same vectors, one per storage, on one stream.  Every call is timed with events on that stream; before
anything is timed the device is kept busy for about a second (clocks), both storages of a shape run untimed first, the two
storages alternate inside every repetition, and a row reports the median and [min .. max] over the repetitions for each.
  search   nq 1 / 16 (direct path), 64 / 1000 / 10 000 (fused GEMM path), k 10 / 100
  refine   10 000 queries, k 10, k_base 100 / 1000; the shortlist is uniform random labels with arbitrary incoming distances
           (no row shared on purpose: the gather's worst locality), the timed call includes the bad-label flag's read
Per row: f16 / f32 of the medians, and the algorithmic bytes -- the stored bytes a call must read once (search: ntotal x row
bytes, on the direct path once per pass of 19 queries; refine: n x k_base x row bytes) -- over the f16 and the f32 time.  The
fp32 handle's kernels are the comparison, in the same process; where the [min .. max] ranges do not overlap the row says which
storage is slower.
    python tools/time_knn_f16.py [reps] [out_file] [ntotal]"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_file = sys.argv[2] if len(sys.argv) > 2 else None
nb = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
if not torch.cuda.is_available():
    raise SystemExit("tools/time_knn_f16.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
d = 128
rng = np.random.default_rng(11)
xq_all = torch.from_numpy(rng.standard_normal((10000, d)).astype(np.float32)).to(dev)
xb = torch.from_numpy(rng.standard_normal((nb, d)).astype(np.float32)).to(dev)
torch.cuda.synchronize()
stream = torch.cuda.current_stream()
STORAGES = ("f32", "f16")
ROW_BYTES = {"f32": 4 * d, "f16": 2 * d}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fns):
    """{storage: [ms]}: both untimed twice, then alternating inside every repetition"""
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    ms = {st: [] for st in fns}
    for _ in range(reps):
        for st, fn in fns.items():
            ms[st].append(timed(fn))
    return ms


def report(what, ms, nbytes, info):
    med = {st: statistics.median(ms[st]) for st in STORAGES}
    rate = {st: nbytes[st] / (med[st] * 1e-3) / 1e12 for st in STORAGES}
    apart = "f16 slower" if min(ms["f16"]) > max(ms["f32"]) else "f16 faster" if max(ms["f16"]) < min(ms["f32"]) else "ranges overlap"
    line = ("%-28s f32 %9.3f ms [%8.3f .. %8.3f] %6.3f TB/s   f16 %9.3f ms [%8.3f .. %8.3f] %6.3f TB/s   f16/f32 %.3f (%s)   %s"
            % (what, med["f32"], min(ms["f32"]), max(ms["f32"]), rate["f32"], med["f16"], min(ms["f16"]), max(ms["f16"]), rate["f16"],
               med["f16"] / med["f32"], apart, info))
    print(line, flush=True)
    lines.append(line)
    if out_file:        # (kept current: a long run leaves what it has)
        with open(out_file, "w") as f:
            f.write("\n".join(lines) + "\n")


lines = ["flat exact k-NN and refine by storage: d %d, %d Gaussian vectors, %d repetitions, median [min .. max]; TB/s = algorithmic "
         "bytes over the median (8 TB/s HBM peak); %s" % (d, nb, reps, torch.cuda.get_device_name(0))]
for metric in ("l2", "ip"):
    flat = {}
    for st in STORAGES:
        g = vlq.GpuFlat(d, metric=metric, device=0, storage=st)
        g.set_stream(stream.cuda_stream)
        for i0 in range(0, nb, 262144):
            g.add(xb[i0:i0 + 262144])
        torch.cuda.synchronize()
        assert g.ntotal == nb
        flat[st] = g
    D0 = torch.empty((1000, 10), dtype=torch.float32, device=dev)
    I0 = torch.empty((1000, 10), dtype=torch.int64, device=dev)
    t_end = time.time() + 1.0
    while time.time() < t_end:          # clocks up before the first timed call
        flat["f32"].search(xq_all[:1000], 10, D0, I0)
        torch.cuda.synchronize()
    for nq in (1, 16, 64, 1000, 10000):
        for k in (10, 100):
            xq = xq_all[:nq].contiguous()
            D = {st: torch.empty((nq, k), dtype=torch.float32, device=dev) for st in STORAGES}
            I = {st: torch.empty((nq, k), dtype=torch.int64, device=dev) for st in STORAGES}
            ms = measure({st: (lambda st=st: flat[st].search(xq, k, D[st], I[st])) for st in STORAGES})
            same = float((I["f16"] == I["f32"]).float().mean())
            report("%s search nq %5d k %3d" % (metric, nq, k), ms, {st: nb * ROW_BYTES[st] for st in STORAGES},
                   "labels equal %.4f   %s" % (same, flat["f16"].last_scan_info()))
    n, k = 10000, 10
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    for k_base in (100, 1000):
        base_I = torch.randint(0, nb, (n, k_base), generator=gen, device=dev, dtype=torch.int64)
        base_D = torch.rand((n, k_base), generator=gen, device=dev)
        D = {st: torch.empty((n, k), dtype=torch.float32, device=dev) for st in STORAGES}
        I = {st: torch.empty((n, k), dtype=torch.int64, device=dev) for st in STORAGES}
        torch.cuda.synchronize()
        ms = measure({st: (lambda st=st: flat[st].refine(xq_all, base_D, base_I, k, D[st], I[st])) for st in STORAGES})
        same = float((I["f16"] == I["f32"]).float().mean())
        report("%s refine n %d k_base %4d" % (metric, n, k_base), ms, {st: n * k_base * ROW_BYTES[st] for st in STORAGES},
               "labels equal %.4f   %s" % (same, flat["f16"].last_refine_info()))
    for g in flat.values():
        g.close()
