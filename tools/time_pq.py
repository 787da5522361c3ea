#!/usr/bin/env python3
"""Flat PQ search (vlq.GpuPQ, csrc/scan_pq.hip) beside the only route the library had before it: a GpuIVFPQ with one list,
by_residual off and nprobe 1 over the same codes (one workgroup per query walks the whole database), in one process.

d 128, M 16, nbits 8, 1 M random codes, random centroids and queries; nq in {1, 64, 1000, 10000}, k in {10, 100}; ST_PQ under
L2, and ST_polysemous at the threshold that passes about 1 % of the codes (set_polysemous_ht on the baseline).  Buffers are
device-resident; every call is timed with events on the stream both indexes use.  Before anything is timed the device is kept
busy for about a second (clocks), every variant of a shape runs untimed first, the variants alternate inside every repetition,
and a row reports the median and the minimum / maximum over the repetitions.  Variants of the new path: the plan's own
choice, and the query tile forced to Q = 1, 2, 4 (slices left to the plan) -- the comparison that justifies the interleaved
tables, or drops them.  Results are compared once per shape: the rows of the two paths agree as far as their summation
orders allow (labels of ST_PQ may differ where the grouped and the left-to-right sum round differently; the filtered rows
are bit-equal, both sum left to right).
    python tools/time_pq.py [reps] [out.json]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_file = sys.argv[2] if len(sys.argv) > 2 else None
if not torch.cuda.is_available():
    raise SystemExit("tools/time_pq.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
d, M, nb, HT = 128, 16, 1000000, 51
rng = np.random.default_rng(5)
cent = rng.standard_normal((M, 256, d // M)).astype(np.float32)
codes = torch.from_numpy(rng.integers(0, 256, (nb, M), dtype=np.uint8)).to(dev)
xq_all = torch.from_numpy(rng.standard_normal((10000, d)).astype(np.float32)).to(dev)
torch.cuda.synchronize()
stream = torch.cuda.current_stream()

g = vlq.GpuPQ(d, M, 8)
g.set_stream(stream.cuda_stream)
g.set_centroids(cent)
g.set_codes(codes)
b = vlq.GpuIVFPQ(d, 1, M, 8)
b.set_stream(stream.cuda_stream)
b.set_coarse_centroids(np.zeros((1, d), np.float32))
b.set_pq_centroids(cent)
b.set_search_options(by_residual=False)
b.set_lists(codes, torch.arange(nb, dtype=torch.int64, device=dev), np.array([0, nb], np.int64))
torch.cuda.synchronize()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


rows = []
t_end = time.time() + 1.0
D = torch.empty((1000, 10), dtype=torch.float32, device=dev)
I = torch.empty((1000, 10), dtype=torch.int64, device=dev)
while time.time() < t_end:          # clocks up before the first timed call
    g.search(xq_all[:1000], 10, D, I)
    torch.cuda.synchronize()

for poly in (False, True):
    g.search_type = "polysemous" if poly else "pq"
    g.polysemous_ht = HT if poly else 8 * M + 1
    b.set_polysemous_ht(HT if poly else 0)
    for nq in (1, 64, 1000, 10000):
        for k in (10, 100):
            xq = xq_all[:nq].contiguous()
            D = {n: torch.empty((nq, k), dtype=torch.float32, device=dev) for n in ("plan", "q1", "q2", "q4", "base")}
            I = {n: torch.empty((nq, k), dtype=torch.int64, device=dev) for n in D}

            def new(name, q):
                def run():
                    g.set_scan_split(q, 0)
                    g.search(xq, k, D[name], I[name])
                return run
            variants = {"plan": new("plan", 0), "q1": new("q1", 1), "q2": new("q2", 2), "q4": new("q4", 4),
                        "base": lambda: b.search(xq, 1, k, D["base"], I["base"])}
            info = {}
            for name, fn in list(variants.items()):       # untimed: code objects, workspaces
                try:
                    fn(); fn()
                except vlq.VlqError as e:       # a shape the baseline does not serve is reported, not timed
                    if name != "base":
                        raise
                    info[name] = "not served: %s" % e
                    del variants[name]
                    continue
                torch.cuda.synchronize()
                info[name] = (b if name == "base" else g).last_scan_info()
            ms = {n: [] for n in variants}
            for _ in range(reps):
                for name, fn in variants.items():
                    ms[name].append(timed(fn))
            g.set_scan_split(0, 0)
            g.stats(reset=True)
            g.search(xq, k, D["plan"], I["plan"])
            pass_rate = g.stats(reset=True)[2] / float(nq * nb) if poly else None
            Dn, Db = D["plan"].cpu().numpy(), D["base"].cpu().numpy()
            same_labels = float((I["plan"].cpu().numpy() == I["base"].cpu().numpy()).mean())
            if "base" not in variants:
                ms["base"] = [float("nan")]
            row = {"type": "ST_polysemous" if poly else "ST_PQ", "nq": nq, "k": k, "pass_rate": pass_rate,
                   "max_rel_diff_vs_baseline": float(np.max(np.abs(Dn - Db) / np.maximum(np.abs(Db), 1e-30))),
                   "bit_equal_vs_baseline": bool(np.array_equal(Dn.view(np.uint32), Db.view(np.uint32))), "same_labels": same_labels,
                   "q_variants_identical": all(torch.equal(D[n], D["plan"]) and torch.equal(I[n], I["plan"]) for n in ("q1", "q2", "q4")),
                   "scan": {n: info[n] for n in info}}
            for name in ms:
                row[name] = {"median_ms": statistics.median(ms[name]), "min_ms": min(ms[name]), "max_ms": max(ms[name])}
            row["speedup_plan_vs_base"] = row["base"]["median_ms"] / row["plan"]["median_ms"]
            rows.append(row)
            print("%-13s nq %5d k %3d  plan %9.3f ms [%8.3f .. %8.3f]  q1 %9.3f  q2 %9.3f  q4 %9.3f  base %9.3f [%8.3f .. %8.3f]  x%6.2f  %s"
                  % (row["type"], nq, k, row["plan"]["median_ms"], row["plan"]["min_ms"], row["plan"]["max_ms"], row["q1"]["median_ms"],
                     row["q2"]["median_ms"], row["q4"]["median_ms"], row["base"]["median_ms"], row["base"]["min_ms"], row["base"]["max_ms"],
                     row["speedup_plan_vs_base"], info["plan"]), flush=True)
result = {"shape": {"d": d, "M": M, "nbits": 8, "ntotal": nb, "polysemous_ht": HT}, "reps": reps, "device": torch.cuda.get_device_name(0), "rows": rows}
if out_file:
    with open(out_file, "w") as f:
        json.dump(result, f, indent=1)
g.close()
b.close()
