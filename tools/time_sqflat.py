#!/usr/bin/env python3
"""Flat scalar-quantizer search (vlq.GpuSQ, csrc/scan_sqflat.hip) beside the only route the library had before it: a GpuIVFSQ
with one list, a zero centroid and nprobe 1 over the same codes (one workgroup per query walks the whole database and decodes
every code again for every query), in one process.

d 128, 1 M random codes, a random range and random queries; SQ8 under L2, SQ8 under inner product and SQ4 under L2; nq in {1, 64,
1000, 10000}, k in {10, 100}.  Buffers are device-resident; every call is timed with events on the stream both indexes use.
Before anything is timed the device is kept busy for about a second (clocks), every variant of a shape runs untimed first, the
variants alternate inside every repetition, and a row reports the median and the minimum / maximum over the repetitions.
Variants of the new path: the plan's own choice, and the query tile forced to Q = 1, 2, 4 (slices left to the plan).  Results
are compared once per shape: D of the two paths is bit-equal (the same float operations in the same order).

Acceptance is against the baseline, never against the code under test alone: at every shape the plan's median is no higher than
the baseline's, and the plan is no slower than the best forced variant by more than that variant's own min-max spread
("accept" in every row, "all_accepted" in the result).
    python tools/time_sqflat.py [reps] [out.json]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_file = sys.argv[2] if len(sys.argv) > 2 else None
if not torch.cuda.is_available():
    raise SystemExit("tools/time_sqflat.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
d, nb = 128, 1000000
rng = np.random.default_rng(5)
trained = np.concatenate([rng.standard_normal(d), 1 + rng.random(d)]).astype(np.float32)
xq_all = torch.from_numpy(rng.standard_normal((10000, d)).astype(np.float32)).to(dev)
torch.cuda.synchronize()
stream = torch.cuda.current_stream()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


rows = []
warm = False
for qtype, metric in (("8bit", "l2"), ("8bit", "ip"), ("4bit", "l2")):
    cs = d if qtype == "8bit" else d // 2
    codes = torch.from_numpy(rng.integers(0, 256, (nb, cs), dtype=np.uint8)).to(dev)
    g = vlq.GpuSQ(d, qtype, metric=metric)
    g.set_stream(stream.cuda_stream)
    g.set_trained(trained)
    g.set_codes(codes)
    b = vlq.GpuIVFSQ(d, 1, qtype, metric=metric)
    b.set_stream(stream.cuda_stream)
    b.set_coarse_centroids(np.zeros((1, d), np.float32))
    b.set_trained(trained)
    b.set_lists(codes, torch.arange(nb, dtype=torch.int64, device=dev), np.array([0, nb], np.int64))
    torch.cuda.synchronize()
    if not warm:
        t_end = time.time() + 1.0
        D = torch.empty((1000, 10), dtype=torch.float32, device=dev)
        I = torch.empty((1000, 10), dtype=torch.int64, device=dev)
        while time.time() < t_end:          # clocks up before the first timed call
            g.search(xq_all[:1000], 10, D, I)
            torch.cuda.synchronize()
        warm = True
    for nq in (1, 64, 1000, 10000):
        keys = torch.zeros((nq, 1), dtype=torch.int64, device=dev)
        cdis = torch.zeros((nq, 1), dtype=torch.float32, device=dev)
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
                        "base": lambda: b.search_preassigned(xq, keys, cdis, k, D["base"], I["base"])}
            info = {}
            for name, fn in variants.items():       # untimed: code objects, workspaces
                fn(); fn()
                torch.cuda.synchronize()
                info[name] = (b if name == "base" else g).last_scan_info()
            ms = {n: [] for n in variants}
            for _ in range(reps):
                for name, fn in variants.items():
                    ms[name].append(timed(fn))
            g.set_scan_split(0, 0)
            Dn, Db = D["plan"].cpu().numpy(), D["base"].cpu().numpy()
            row = {"qtype": qtype, "metric": metric, "nq": nq, "k": k,
                   "bit_equal_vs_baseline": bool(np.array_equal(Dn.view(np.uint32), Db.view(np.uint32))),
                   "same_labels": float((I["plan"].cpu().numpy() == I["base"].cpu().numpy()).mean()),
                   "q_variants_identical": all(torch.equal(D[n], D["plan"]) and torch.equal(I[n], I["plan"]) for n in ("q1", "q2", "q4")),
                   "scan": info}
            for name in ms:
                row[name] = {"median_ms": statistics.median(ms[name]), "min_ms": min(ms[name]), "max_ms": max(ms[name])}
            best = min(("q1", "q2", "q4"), key=lambda n: row[n]["median_ms"])
            row["best_forced"] = best
            row["speedup_plan_vs_base"] = row["base"]["median_ms"] / row["plan"]["median_ms"]
            row["accept"] = bool(row["bit_equal_vs_baseline"] and row["plan"]["median_ms"] <= row["base"]["median_ms"] and
                                 row["plan"]["median_ms"] <= row[best]["median_ms"] + (row[best]["max_ms"] - row[best]["min_ms"]))
            rows.append(row)
            print("SQ%s %s nq %5d k %3d  plan %9.3f ms [%8.3f .. %8.3f]  q1 %9.3f  q2 %9.3f  q4 %9.3f  base %9.3f [%8.3f .. %8.3f]  x%6.2f  %s  %s"
                  % (qtype[0], metric, nq, k, row["plan"]["median_ms"], row["plan"]["min_ms"], row["plan"]["max_ms"], row["q1"]["median_ms"],
                     row["q2"]["median_ms"], row["q4"]["median_ms"], row["base"]["median_ms"], row["base"]["min_ms"], row["base"]["max_ms"],
                     row["speedup_plan_vs_base"], "ok" if row["accept"] else "MISSED", info["plan"]), flush=True)
    g.close()
    b.close()
    del codes
result = {"shape": {"d": d, "ntotal": nb}, "reps": reps, "device": torch.cuda.get_device_name(0), "all_accepted": all(r["accept"] for r in rows), "rows": rows}
print("all accepted: %s" % result["all_accepted"])
if out_file:
    with open(out_file, "w") as f:
        json.dump(result, f, indent=1)
