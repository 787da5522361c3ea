#!/usr/bin/env python3
"""One Lloyd iteration of vlq.GpuKMeans (csrc/kmeans.hip) split into assign / group / update, beside the same iteration by the
means the library had before it: GpuFlat.search for the assignment, the labels to the host, a numpy float32 update
(np.add.at, the same bits), the centroids back into the flat index.

Shapes: the headline's coarse training shape d 128, k 4096, n 1 048 576; a PQ sub-quantizer's d 8, k 256, n 65 536; and the
coarse shape with half the rows in one cluster (the update alone: one chain of 524 288 rows).  Rows are device-resident.  The
assignment and the whole update call (grouping, update, the status read, the splits) are timed with a host clock around calls that end in a stream synchronisation; group and
update are the step's own stream times between events (vlq_kmeans_last_info).  The device is kept busy for about a second first,
every variant runs untimed before it is timed, a row gives the median and the minimum / maximum.  The update kernel reads every
row once: its bound is 4 n d bytes at the HBM rate of 8 TB/s.
The last line trains 1024 centroids with vlq.kmeans, hands them to a GpuIVFFlat and prints its recall@1 against GpuFlat.
    python tools/time_kmeans.py [reps] [out.json] [big_n]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_file = sys.argv[2] if len(sys.argv) > 2 else None
big_n = int(sys.argv[3]) if len(sys.argv) > 3 else 1048576
if not torch.cuda.is_available():
    raise SystemExit("tools/time_kmeans.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
rng = np.random.default_rng(11)
HBM_BYTES_PER_S = 8e12
stream_ptr = torch.cuda.current_stream().cuda_stream      # every handle works on torch's stream: its copies are ordered behind them


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return (statistics.median(v), min(v), max(v))


def info(km):
    return dict(kv.split("=", 1) for kv in km.last_info().split() if "=" in kv)


def host_update(x_host, labels, k):
    """what a caller without the device update does: the reference's float32 sums on the host"""
    c = np.zeros((k, x_host.shape[1]), np.float32)
    np.add.at(c, labels, x_host)
    cnt = np.bincount(labels, minlength=k)
    full = cnt > 0
    c[full] /= cnt[full].astype(np.float32)[:, None]
    return c


def one_shape(name, d, k, n, skew):
    xh = rng.standard_normal((n, d), dtype=np.float32)
    xh += 2 * rng.standard_normal((k, d), dtype=np.float32)[rng.integers(0, k, n)]
    x = torch.from_numpy(xh).to(dev)
    km = vlq.GpuKMeans(d, k, niter=1, max_points_per_centroid=1 << 30)
    km.set_stream(stream_ptr)
    cent = km.train(x)                                    # untimed: code objects, workspaces, centroids in the handle
    D, I = km.assign(x)
    if skew:
        Ih = I.cpu().numpy()
        Ih[rng.permutation(n)[:n // 2]] = 7
        I = torch.from_numpy(Ih).to(dev)
    out = torch.empty((k, d), dtype=torch.float32, device=dev)
    km.update(x, I, out)
    t_assign, t_call, t_group, t_update = [], [], [], []
    for _ in range(reps):
        t_assign.append(clock(lambda: km.assign(x)))
        t_call.append(clock(lambda: km.update(x, I, out)))
        i = info(km)
        t_group.append(float(i["group_ms"]))
        t_update.append(float(i["update_ms"]))
    row = {"name": name, "d": d, "k": k, "n": n, "assign_ms": med(t_assign), "group_ms": med(t_group), "update_ms": med(t_update),
           "update_call_ms": med(t_call), "info": km.last_info()}
    floor_ms = 4.0 * n * d / HBM_BYTES_PER_S * 1e3
    row["update_hbm_floor_ms"] = floor_ms
    row["update_row_bytes_per_s"] = 4.0 * n * d / (row["update_ms"][0] * 1e-3)
    # the parent's means: flat search, labels to the host, numpy update, centroids back
    flat = vlq.GpuFlat(d)
    flat.set_stream(stream_ptr)
    flat.add(cent)
    h_assign, h_update, h_back = [], [], []
    same = None
    for _ in range(max(1, min(reps, 2))):
        got = {}
        def search():
            got["I"] = I.cpu().numpy() if skew else flat.search(x, 1)[1][:, 0].cpu().numpy()
        h_assign.append(clock(search))
        t0 = time.perf_counter()
        c = host_update(xh, got["I"], k)
        h_update.append((time.perf_counter() - t0) * 1e3)
        def back():
            flat.reset()
            flat.add(c)
        h_back.append(clock(back))
        if same is None and int(info(km)["nsplit"]) == 0:
            counts = np.bincount(got["I"], minlength=k)
            ours = out.cpu().numpy()
            same = bool(np.array_equal(ours[counts > 0].view(np.uint32), c[counts > 0].view(np.uint32)))
        flat.reset()
        flat.add(cent)
    row.update(host_assign_ms=med(h_assign), host_update_ms=med(h_update), host_back_ms=med(h_back), same_bits=same)
    print("%-7s d %3d k %4d n %7d: assign %.3f ms, group %.3f ms, update %.3f ms (%.1f %% of the HBM floor %.4f ms, %.3g row bytes/s), "
          "update call %.3f ms | host route: search + labels %.3f ms, numpy update %.1f ms, centroids back %.3f ms | same bits %s"
          % (name, d, k, n, row["assign_ms"][0], row["group_ms"][0], row["update_ms"][0], 100 * floor_ms / row["update_ms"][0], floor_ms,
             row["update_row_bytes_per_s"], row["update_call_ms"][0], row["host_assign_ms"][0], row["host_update_ms"][0],
             row["host_back_ms"][0], same), flush=True)
    print("        spread: assign %.3f .. %.3f, group %.3f .. %.3f, update %.3f .. %.3f; %s"
          % (*row["assign_ms"][1:], *row["group_ms"][1:], *row["update_ms"][1:], km.last_info()), flush=True)
    km.close()
    flat.close()
    return row


warm = vlq.GpuFlat(128)
warm.set_stream(stream_ptr)
xw = torch.from_numpy(rng.standard_normal((100000, 128)).astype(np.float32)).to(dev)
warm.add(xw[:4096])
t_end = time.time() + 1.0
while time.time() < t_end:          # clocks up before the first timed call
    warm.search(xw, 1)
    torch.cuda.synchronize()
warm.close()

rows = [one_shape("coarse", 128, 4096, big_n, False), one_shape("pq", 8, 256, 65536, False), one_shape("skewed", 128, 4096, big_n, True)]

# sanity: trained centroids as the coarse quantizer of an IVFFlat index
d, nlist, nb, nq, nprobe = 64, 1024, 200000, 2000, 8
xb = (rng.standard_normal((nb, d)) + 2 * rng.standard_normal((nlist, d))[rng.integers(0, nlist, nb)]).astype(np.float32)
xq = xb[rng.permutation(nb)[:nq]] + 0.1 * rng.standard_normal((nq, d)).astype(np.float32)
t0 = time.perf_counter()
cent = vlq.kmeans(xb, nlist, niter=10)
train_ms = (time.perf_counter() - t0) * 1e3
ivf = vlq.GpuIVFFlat(d, nlist)
ivf.set_coarse_centroids(cent)
ivf.add(xb)
flat = vlq.GpuFlat(d)
flat.add(xb)
recall = float((ivf.search(xq, nprobe, 1)[1][:, 0] == flat.search(xq, 1)[1][:, 0]).mean())
print("sanity: vlq.kmeans d %d k %d n %d niter 10 in %.1f ms (host rows in, centroids out); GpuIVFFlat nprobe %d recall@1 against GpuFlat %.4f"
      % (d, nlist, nb, train_ms, nprobe, recall), flush=True)
if out_file:
    with open(out_file, "w") as f:
        json.dump({"reps": reps, "shapes": rows, "sanity": {"train_ms": train_ms, "recall_at_1": recall}}, f, indent=1)
