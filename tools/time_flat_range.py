#!/usr/bin/env python3
"""Range search of the flat index (vlq.GpuFlat.range_search, csrc/scan_range_knn.hip) beside the k-NN search of the same index
(vlq_flat_search at k = 10) in one process and at the same shape.

d 128, 1 000 000 random Gaussian vectors, nq in {16, 1000, 10000}; L2 and inner product.  Two radii per shape, taken from the
distances of a k = 1000 search of the same queries: the pooled value of rank 10 nq (10 hits per query) and the median of the
queries' 1000th distances (the order of 1000 hits per query).  Buffers are device-resident.  A range search synchronises (it
reads the total), so every call -- the k-NN search with a synchronisation behind it, the range search with its result copied out of the handle -- is timed as a whole on the host clock.
Before anything is timed the device is kept busy for about a second (clocks) and every call of a shape runs untimed; the calls
alternate inside every repetition; a row reports the median and the minimum / maximum over the repetitions.
    python tools/time_flat_range.py [reps] [out.json] [ntotal]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_file = sys.argv[2] if len(sys.argv) > 2 else None
nb = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
if not torch.cuda.is_available():
    raise SystemExit("tools/time_flat_range.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
d = 128
rng = np.random.default_rng(11)
xq_all = torch.from_numpy(rng.standard_normal((10000, d)).astype(np.float32)).to(dev)
xb = torch.from_numpy(rng.standard_normal((nb, d)).astype(np.float32)).to(dev)
torch.cuda.synchronize()
stream = torch.cuda.current_stream()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


rows = []
for metric in ("l2", "ip"):
    g = vlq.GpuFlat(d, metric=metric)
    g.set_stream(stream.cuda_stream)
    g.add(xb)
    torch.cuda.synchronize()
    t_end = time.time() + 1.0
    while time.time() < t_end:          # clocks up before the first timed call
        g.search(xq_all[:1000], 10)
        torch.cuda.synchronize()
    for nq in (16, 1000, 10000):
        xq = xq_all[:nq].contiguous()
        Dk, _ = g.search(xq, 1000)
        torch.cuda.synchronize()
        # 10 hits: the value of rank 10 nq among the pooled distances of these rows (exactly 10 nq pairs lie inside it).  1000 hits:
        # the pool holds only 1000 per query, so the median over the queries of the 1000th distance (the count is what it is)
        pool = torch.sort(Dk.flatten(), descending=metric == "ip").values
        radii = {"hits10": float(pool[10 * nq]), "hits1000": float(Dk[:, 999].median())}
        D10 = torch.empty((nq, 10), dtype=torch.float32, device=dev)
        I10 = torch.empty((nq, 10), dtype=torch.int64, device=dev)
        calls = {"knn10": lambda: g.search(xq, 10, D10, I10)}
        out = {}
        for name, r in radii.items():
            def run(name=name, r=r):
                out[name] = g.range_search(xq, r)
            calls[name] = run
        info = {}
        for name, fn in calls.items():       # untimed: code objects, workspaces
            fn(); fn()
            torch.cuda.synchronize()
            info[name] = g.last_scan_info()
        ms = {n: [] for n in calls}
        for _ in range(reps):
            for name, fn in calls.items():
                ms[name].append(timed(fn))
        row = {"metric": metric, "ntotal": nb, "nq": nq, "radii": radii, "scan": info}
        for name in calls:
            row[name] = stat(ms[name])
        for name in radii:
            lims = out[name][0].cpu().numpy()
            row[name]["hits_per_query"] = float(lims[-1]) / nq
            row[name]["over_knn10"] = row[name]["median_ms"] / row["knn10"]["median_ms"]
            assert (np.diff(lims) >= 0).all() and out[name][1].shape[0] == lims[-1]
        rows.append(row)
        print("%s nq %5d  knn10 %9.3f ms [%8.3f .. %8.3f]  %s   %s" % (
            metric, nq, row["knn10"]["median_ms"], row["knn10"]["min_ms"], row["knn10"]["max_ms"],
            "  ".join("%s %9.3f ms [%8.3f .. %8.3f] x%.2f (%.1f hits/q)" % (n, row[n]["median_ms"], row[n]["min_ms"], row[n]["max_ms"],
                                                                          row[n]["over_knn10"], row[n]["hits_per_query"]) for n in radii),
            info["hits10"]), flush=True)
        if out_file:        # (kept current: a long run leaves what it has)
            with open(out_file, "w") as f:
                json.dump({"shape": {"d": d, "ntotal": nb}, "reps": reps, "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    g.close()
