#!/usr/bin/env python3
"""Cost and benefit of IndexRefineFlat on the device (vlq.GpuFlat.refine, csrc/refine_flat.hip) on the bench's own data and
shape: d 128, 1 M vectors, 4096 lists, PQ 16x8 bit, nprobe 32, k 10; 10 000 queries at k_factor 1, 4, 10, 100, and the small
batches of 1 and 16 queries at k_factor 10.

Per row, in one process, with events on the stream every index uses: the device is kept busy first (clocks), every variant of
a row runs untimed once, the variants alternate inside every repetition, a row reports the median (and minimum / maximum):
    first_k      the first stage (GpuIVFPQ.search) at k
    first_kbase  the first stage at k_base = int(k * k_factor)
    refine       GpuFlat.refine alone on the shortlist the first stage left on the device (the call reads its bad-label flag
                 behind the kernel: one stream synchronisation, inside the timed span)
    frac_hbm     gathered bytes n * k_base * 4 d per second of `refine`, as a fraction of the 8 TB/s HBM peak of DESIGN.md
    recall       recall@1 and recall@10 against GpuFlat.search (exact) on the same data, before (first stage at k) and after
                 refining
Results go to profiles/time_refine_flat.json.
    python tools/time_refine_flat.py [reps] [out.json]      env: NB=1000000 (stored vectors)"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_refine_flat.json")
if not torch.cuda.is_available():
    raise SystemExit("tools/time_refine_flat.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
HBM_PEAK = 8e12
a = argparse.Namespace(nq=10000, nb=int(os.environ.get("NB", "1000000")), nt=100000, d=128, nlist=4096, M=16, nprobe=32, k=10, sigma=0.005,
                       gmm_centres=2000, rank=12, spread=0.4)
stream = torch.cuda.current_stream()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def recalls(I, gt):
    """recall@1 (the exact nearest is the first result) and recall@10 (share of the exact 10 among the 10 results)"""
    I, gt = I.cpu().numpy(), gt.cpu().numpy()
    r1 = float((I[:, 0] == gt[:, 0]).mean())
    r10 = float(np.mean([len(set(I[q, :10].tolist()) & set(gt[q, :10].tolist())) / 10.0 for q in range(I.shape[0])]))
    return r1, r10


g, centres, coarse, pq, xb = bench.build_index(a, dev)          # the headline index; ids are positions
flat = vlq.GpuFlat(a.d, metric="l2")
flat.set_stream(stream.cuda_stream)
for i0 in range(0, xb.shape[0], 262144):
    flat.add(xb[i0:i0 + 262144].contiguous())
torch.cuda.synchronize()
gen = torch.Generator(device=dev)
gen.manual_seed(33)
xq_all = bench.gmm(torch, gen, centres, a.nq, a.sigma, dev, a.rank, a.spread)
for _ in range(50):                                              # clock pre-warm
    g.search(xq_all, a.nprobe, a.k)
torch.cuda.synchronize()
gt_all = flat.search(xq_all, a.k)[1]
torch.cuda.synchronize()

rows = []
for nq, kf in [(10000, 1.0), (10000, 4.0), (10000, 10.0), (10000, 100.0), (1, 10.0), (16, 10.0)]:
    k = a.k
    kb = int(np.float32(k) * np.float32(kf))
    xq, gt = xq_all[:nq].contiguous(), gt_all[:nq]
    Dk = torch.empty((nq, k), dtype=torch.float32, device=dev); Ik = torch.empty((nq, k), dtype=torch.int64, device=dev)
    Db = torch.empty((nq, kb), dtype=torch.float32, device=dev); Ib = torch.empty((nq, kb), dtype=torch.int64, device=dev)
    D = torch.empty((nq, k), dtype=torch.float32, device=dev); I = torch.empty((nq, k), dtype=torch.int64, device=dev)
    fns = {"first_k": lambda: g.search(xq, a.nprobe, k, D=Dk, I=Ik),
           "first_kbase": lambda: g.search(xq, a.nprobe, kb, D=Db, I=Ib),
           "refine": lambda: flat.refine(xq, Db, Ib, k, D=D, I=I)}
    for fn in fns.values():                                      # untimed first run of every variant
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            ms[n].append(timed(fn))
    torch.cuda.synchronize()
    before, after = recalls(Ik, gt), recalls(I, gt)
    row = {"nq": nq, "k": k, "k_factor": kf, "k_base": kb, "info": flat.last_refine_info(),
           "recall1_before": before[0], "recall10_before": before[1], "recall1_after": after[0], "recall10_after": after[1]}
    for n in fns:
        row[n + "_ms"] = statistics.median(ms[n])
        row[n + "_ms_min"], row[n + "_ms_max"] = min(ms[n]), max(ms[n])
    row["gathered_bytes"] = nq * kb * 4 * a.d
    row["frac_hbm"] = row["gathered_bytes"] / (row["refine_ms"] * 1e-3) / HBM_PEAK
    rows.append(row)
    print("nq=%-5d k=%d k_factor=%-4g k_base=%-4d first(k) %.3f ms | first(k_base) %.3f ms | refine %.3f ms (%.3f .. %.3f; %.2f of first(k_base), "
          "%.3f of the HBM peak) | recall@1 %.3f -> %.3f, recall@10 %.3f -> %.3f" % (
              nq, k, kf, kb, row["first_k_ms"], row["first_kbase_ms"], row["refine_ms"], row["refine_ms_min"], row["refine_ms_max"],
              row["refine_ms"] / row["first_kbase_ms"], row["frac_hbm"], before[0], after[0], before[1], after[1]), flush=True)

with open(out_file, "w") as f:
    json.dump({"shape": vars(a), "reps": reps, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, f, indent=1)
print("wrote", out_file)
