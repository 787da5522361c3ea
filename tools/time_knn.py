#!/usr/bin/env python3
"""Flat exact k-NN search (vlq.GpuFlat, csrc/scan_knn.hip) beside the only route the library had before it: the coarse stage of
a GpuIVFPQ whose "centroids" are the database (nlist = ntotal, M = 1, nbits = 1; coarse_search with nprobe = k), which writes the
whole [page][ntotal] distance matrix and selects from it -- the route of include/faiss_amd/IndexFlat.h -- in one process.

d 128, random Gaussian vectors, ntotal in {100 000, 1 000 000}; nq in {1, 16, 64, 1000, 10000}, k in {10, 100}; L2 and inner
product.  Buffers are device-resident; every call is timed with events on the stream both indexes use.  Before anything is
timed the device is kept busy for about a second (clocks), every variant of a shape runs untimed first, the variants alternate
inside every repetition, and a row reports the median and the minimum / maximum over the repetitions.  Variants of the new
path: the plan's own choice; the row tile forced to 32, 64, 128 (slices left to the plan); the slices forced to 1, 8, 64 (row
tile left to the plan).  Results are compared once per shape: distances bit-equal to the baseline's (except the inner product
below 20 queries, where the new path takes the reference's fvec_inner_product order and the baseline the fmaf chain), and
every forced variant bit-equal to the plan's rows.
    python tools/time_knn.py [reps] [out.json] [ntotal,ntotal,...]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_file = sys.argv[2] if len(sys.argv) > 2 else None
sizes = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [100000, 1000000]
if not torch.cuda.is_available():
    raise SystemExit("tools/time_knn.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
d = 128
rng = np.random.default_rng(11)
xq_all = torch.from_numpy(rng.standard_normal((10000, d)).astype(np.float32)).to(dev)
torch.cuda.synchronize()
stream = torch.cuda.current_stream()
FORCED = {"r32": (32, 0), "r64": (64, 0), "r128": (128, 0), "s1": (0, 1), "s8": (0, 8), "s64": (0, 64)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


rows, builds = [], {}
for nb in sizes:
    xb_host = rng.standard_normal((nb, d)).astype(np.float32)
    xb = torch.from_numpy(xb_host).to(dev)
    torch.cuda.synchronize()
    flat = {}
    for metric in ("l2", "ip"):
        t0 = time.time()
        flat[metric] = vlq.GpuFlat(d, metric=metric)
        flat[metric].set_stream(stream.cuda_stream)
        flat[metric].add(xb)
        torch.cuda.synchronize()
        builds["flat_%s_%d_s" % (metric, nb)] = time.time() - t0
    t0 = time.time()
    base = vlq.GpuIVFPQ(d, nb, 1, 1)
    base.set_stream(stream.cuda_stream)
    base.set_coarse_centroids(xb_host)          # (the handle keeps host-side state of the "centroids": a host array, as the shell passes)
    torch.cuda.synchronize()
    builds["base_%d_s" % nb] = time.time() - t0
    print("ntotal %d: built flat l2 %.2f s, flat ip %.2f s, baseline %.2f s" % (nb, builds["flat_l2_%d_s" % nb], builds["flat_ip_%d_s" % nb],
                                                                             builds["base_%d_s" % nb]), flush=True)
    t_end = time.time() + 1.0
    D0 = torch.empty((1000, 10), dtype=torch.float32, device=dev)
    I0 = torch.empty((1000, 10), dtype=torch.int64, device=dev)
    while time.time() < t_end:          # clocks up before the first timed call
        flat["l2"].search(xq_all[:1000], 10, D0, I0)
        torch.cuda.synchronize()
    for metric in ("l2", "ip"):
        g = flat[metric]
        base.metric = metric
        for nq in (1, 16, 64, 1000, 10000):
            for k in (10, 100):
                xq = xq_all[:nq].contiguous()
                names = ["plan"] + list(FORCED) + ["base"]
                D = {n: torch.empty((nq, k), dtype=torch.float32, device=dev) for n in names}
                I = {n: torch.empty((nq, k), dtype=torch.int64, device=dev) for n in names}

                def new(name, split):
                    def run():
                        g.scan_split(*split)
                        g.search(xq, k, D[name], I[name])
                    return run
                variants = {"plan": new("plan", (0, 0))}
                variants.update({n: new(n, s) for n, s in FORCED.items()})
                variants["base"] = lambda: base.coarse_search(xq, k, D["base"], I["base"])
                info = {}
                for name, fn in variants.items():       # untimed: code objects, workspaces
                    fn(); fn()
                    torch.cuda.synchronize()
                    if name != "base":
                        info[name] = g.last_scan_info()
                ms = {n: [] for n in variants}
                for _ in range(reps):
                    for name, fn in variants.items():
                        ms[name].append(timed(fn))
                g.scan_split(0, 0)
                Dp, Db = D["plan"].cpu().numpy(), D["base"].cpu().numpy()
                row = {"metric": metric, "ntotal": nb, "nq": nq, "k": k,
                       "bit_equal_vs_baseline": bool(np.array_equal(Dp.view(np.uint32), Db.view(np.uint32))),
                       "same_labels_vs_baseline": float((I["plan"].cpu().numpy() == I["base"].cpu().numpy()).mean()),
                       "forced_variants_identical": all(torch.equal(D[n], D["plan"]) and torch.equal(I[n], I["plan"]) for n in FORCED),
                       "scan": info}
                for name in ms:
                    row[name] = {"median_ms": statistics.median(ms[name]), "min_ms": min(ms[name]), "max_ms": max(ms[name])}
                row["base_over_plan"] = row["base"]["median_ms"] / row["plan"]["median_ms"]
                best = min(FORCED, key=lambda n: row[n]["median_ms"])
                row["best_forced"] = best
                row["plan_over_best_forced"] = row["plan"]["median_ms"] / row[best]["median_ms"]
                rows.append(row)
                print("%s nt %7d nq %5d k %3d  plan %9.3f ms [%8.3f .. %8.3f]  %s  base %9.3f [%8.3f .. %8.3f]  base/plan %6.2f  eq %d/%d  %s"
                      % (metric, nb, nq, k, row["plan"]["median_ms"], row["plan"]["min_ms"], row["plan"]["max_ms"],
                         " ".join("%s %.3f" % (n, row[n]["median_ms"]) for n in FORCED), row["base"]["median_ms"], row["base"]["min_ms"],
                         row["base"]["max_ms"], row["base_over_plan"], row["bit_equal_vs_baseline"], row["forced_variants_identical"],
                         info["plan"]), flush=True)
                if out_file:        # (kept current: a long run leaves what it has)
                    with open(out_file, "w") as f:
                        json.dump({"shape": {"d": d}, "reps": reps, "device": torch.cuda.get_device_name(0), "builds": builds, "rows": rows}, f, indent=1)
    for g in flat.values():
        g.close()
    base.close()
    del xb
