#!/usr/bin/env python3
"""The device linear transform (vlq.GpuLinearTransform, csrc/transform.hip) beside the only device route the library had before
it: vlq.GpuLSH.apply with the same matrix (lsh_encode_kernel, one lane per output with a scalar fmaf chain).

Shapes 128->128, 128->64, 96->96, 960->256 at n = 10 000 and 1 000 000 (960->256 at 1 000 000 rows is 3.8 GB of input: it runs at
250 000 unless asked for), with a bias.  Rows are device-resident, both handles work on one stream and every call is timed with
events on it.  The device is kept busy for about a second first (clocks), every variant runs untimed before it is timed, the
variants alternate inside a repetition, a row gives the median and the minimum / maximum.  The outputs are compared once per
shape: bit-equal.  GpuLSH.apply writes its workspace and copies the rows out (one more pass over xt): that is the route as it
is, not a kernel time.  The HBM floor is 4 n (d_in + d_out) bytes at 8 TB/s.
Then the small batches at 128->128 (n = 1 .. 128: linear_rows_kernel up to the plan's small_n, the strip kernel behind it), and
the whole search of GpuPreTransform([rotation], GpuIVFPQ) beside the bare GpuIVFPQ at d 128, nlist 4096, M 16, nprobe 32, k 10,
10 000 queries over 1 000 000 vectors (random centroids and codebooks: a timing, not a recall).
    python tools/time_transform.py [reps] [out.json] [big_n] [all]        ("all": 960->256 at big_n rows too)"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_file = sys.argv[2] if len(sys.argv) > 2 else None
big_n = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
wide_n = big_n if len(sys.argv) > 4 and sys.argv[4] == "all" else min(big_n, 250000)
if not torch.cuda.is_available():
    raise SystemExit("tools/time_transform.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(3)
HBM_BYTES_PER_S = 8e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(variants):
    """{name: (median, min, max) ms}; the variants alternate inside a repetition"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            ts[name].append(timed(fn))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ts.items()}


def device_rows(n, d):
    t = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    return t


rows = []
warm = vlq.GpuLinearTransform(128, 128, vlq.random_rotation(128, 128))
warm.set_stream(stream.cuda_stream)
xw, ow = device_rows(100000, 128), torch.empty((100000, 128), dtype=torch.float32, device=dev)
t_end = time.time() + 1.0
while time.time() < t_end:          # clocks up before the first timed call
    warm.apply(xw, ow)
    torch.cuda.synchronize()

for d_in, d_out in ((128, 128), (128, 64), (96, 96), (960, 256)):
    A = (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
    b = rng.standard_normal(d_out).astype(np.float32)
    t = vlq.GpuLinearTransform(d_in, d_out, A, b)
    lsh = vlq.GpuLSH(d_in, d_out, rotate_data=True)
    lsh.set_rotation(A, b)
    t.set_stream(stream.cuda_stream)
    lsh.set_stream(stream.cuda_stream)
    for n in (10000, big_n if d_in < 512 else wide_n):
        x = device_rows(n, d_in)
        o1 = torch.empty((n, d_out), dtype=torch.float32, device=dev)
        o2 = torch.empty_like(o1)
        m = measure({"transform": lambda: t.apply(x, o1), "lsh_apply": lambda: lsh.apply(x, o2)})
        torch.cuda.synchronize()
        floor_ms = 4.0 * n * (d_in + d_out) / HBM_BYTES_PER_S * 1e3
        row = {"d_in": d_in, "d_out": d_out, "n": n, "ms": m["transform"], "lsh_ms": m["lsh_apply"], "hbm_floor_ms": floor_ms,
               "floor_share": floor_ms / m["transform"][0], "same_bits": bool(torch.equal(o1.view(torch.int32), o2.view(torch.int32))),
               "info": t.last_info()}
        rows.append(row)
        print("%4d -> %4d n %8d: transform %8.4f ms (%.4f .. %.4f), %4.1f %% of the HBM floor %.4f ms; lsh_apply %8.4f ms (%.4f .. %.4f); "
              "same bits %s" % (d_in, d_out, n, *m["transform"], 100 * row["floor_share"], floor_ms, *m["lsh_apply"], row["same_bits"]), flush=True)
        del x, o1, o2

small = []
t = vlq.GpuLinearTransform(128, 128, vlq.random_rotation(128, 128), np.zeros(128, np.float32))
t.set_stream(stream.cuda_stream)
x = device_rows(128, 128)
for n in (1, 2, 4, 8, 16, 17, 32, 64, 128):
    o = torch.empty((n, 128), dtype=torch.float32, device=dev)
    xs = x[:n]
    m = measure({"apply": lambda: t.apply(xs, o)})["apply"]
    small.append({"n": n, "ms": m, "info": t.last_info()})
    print("128 -> 128 n %3d: %.4f ms (%.4f .. %.4f)  %s" % (n, *m, t.last_info().split()[0]), flush=True)

# the whole search behind a rotation
d, nlist, M, nb, nq, nprobe, k = 128, 4096, 16, big_n, 10000, 32, 10
xb, xq = device_rows(nb, d), device_rows(nq, d)
cent = rng.standard_normal((nlist, d)).astype(np.float32)
pq = rng.standard_normal((M, 256, d // M)).astype(np.float32)
search = {}
for name in ("bare", "pretransform"):
    g = vlq.GpuIVFPQ(d, nlist, M, 8)
    g.set_coarse_centroids(cent)
    g.set_pq_centroids(pq)
    if name == "pretransform":
        g = vlq.GpuPreTransform([vlq.GpuLinearTransform(d, d, vlq.random_rotation(d, d), is_orthonormal=True)], g)
    g.set_stream(stream.cuda_stream)
    for i0 in range(0, nb, 100000):
        g.add(xb[i0:i0 + 100000])
    search[name] = g
torch.cuda.synchronize()
D = torch.empty((nq, k), dtype=torch.float32, device=dev)
I = torch.empty((nq, k), dtype=torch.int64, device=dev)
m = measure({"bare": lambda: search["bare"].search(xq, nprobe, k, D, I), "pretransform": lambda: search["pretransform"].search(xq, k, nprobe, D, I)})
print("search nq %d nb %d: bare GpuIVFPQ %.4f ms (%.4f .. %.4f), GpuPreTransform %.4f ms (%.4f .. %.4f)" % (nq, nb, *m["bare"], *m["pretransform"]), flush=True)
if out_file:
    with open(out_file, "w") as f:
        json.dump({"reps": reps, "apply": rows, "small": small, "search": m}, f, indent=1)
