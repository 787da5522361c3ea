#!/usr/bin/env python3
"""vlq.GpuMoments (csrc/moments.hip) and the whole vlq.train_pca at the shapes PCA training is run at, beside the same
covariance on the host.

Shapes (n, d): (128 000, 128) and (96 000, 96) -- one output tile, the kernel reads every row once, its floor is 4 n d bytes at
the HBM rate -- and (250 000, 960), 36 tile pairs, bound by the fp32 MFMA rate (2 n d^2 useful flops; the kernel issues
2 n 128^2 per launched pair, the upper triangle only).  Rows are device-resident.  moment_kernel's time is the stream time between
events around its launches (vlq_moments_last_info, moment_ms); the compute call (means, moment_kernel, the join) and train_pca
(the call above, the matrix to the host, numpy's eigh, prepare_Ab, the transform's handle) are timed with a host clock around work
that ends in a synchronisation.  The device is kept busy for about a second first, every variant runs untimed before it is
timed, a row gives the median and the minimum / maximum.  The plan's alternatives (strip rows kr; slices S) are timed through
GpuMoments.set_split, alternating with the default.  The host figure is numpy float32 x.T @ x on the machine's CPUs.
    python tools/time_pca_train.py [reps] [out.json]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_file = sys.argv[2] if len(sys.argv) > 2 else None
if not torch.cuda.is_available():
    raise SystemExit("tools/time_pca_train.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
rng = np.random.default_rng(24)
HBM_BYTES_PER_S, MFMA_F32_FLOPS = 8e12, 157.3e12


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return (statistics.median(v), min(v), max(v))


def info(m):
    return dict(kv.split("=", 1) for kv in m.last_info().split() if "=" in kv)


def time_split(mom, x, splits):
    """moment_ms and the whole compute call of every (kr, S) of `splits`, alternating between them within a repetition"""
    ker, call, plans = {s: [] for s in splits}, {s: [] for s in splits}, {}
    for s in splits:                       # untimed: code objects, scratch
        mom.set_split(*s)
        mom.compute(x)
        plans[s] = mom.last_info()
    for _ in range(reps):
        for s in splits:
            mom.set_split(*s)
            call[s].append(clock(lambda: (mom.compute(x), mom.last_info())))
            ker[s].append(float(info(mom)["moment_ms"]))
    mom.set_split(0, 0)
    return {s: {"moment_ms": med(ker[s]), "compute_call_ms": med(call[s]), "info": plans[s]} for s in splits}


def one_shape(n, d):
    xh = (rng.standard_normal((n, d), dtype=np.float32) * (2.0 ** (-np.arange(d) / 64)).astype(np.float32) + 3).astype(np.float32)
    x = torch.from_numpy(xh).to(dev)
    mom = vlq.GpuMoments(d)
    mom.compute(x)
    s_plan = int(info(mom)["S"])
    splits = [(0, 0), (16, 0), (64, 0), (0, max(1, s_plan // 2)), (0, s_plan * 2)]
    table = time_split(mom, x, splits)
    mom.close()
    vlq.train_pca(x, min(64, d)).close()
    t_train = [clock(lambda: vlq.train_pca(x, min(64, d)).close()) for _ in range(max(2, reps // 2))]
    t0 = time.perf_counter()
    w = np.linalg.eigh(np.eye(d) + np.ones((d, d)))[0]
    t_eigh = (time.perf_counter() - t0) * 1e3 + 0 * w[0]
    t_host = []
    for _ in range(2):
        t0 = time.perf_counter()
        c = xh.T @ xh
        t_host.append((time.perf_counter() - t0) * 1e3 + 0 * float(c[0, 0]))
    ms = table[(0, 0)]["moment_ms"][0]
    pairs = int(info_of(table[(0, 0)]["info"])["pairs"])
    row = {"n": n, "d": d, "splits": {"kr=%d S=%d" % s: v for s, v in table.items()}, "train_pca_ms": med(t_train), "eigh_ms_same_d": t_eigh,
           "host_numpy_f32_ms": med(t_host), "hbm_floor_ms": 4.0 * n * d / HBM_BYTES_PER_S * 1e3,
           "mfma_floor_ms_issued": 2.0 * n * 128 * 128 * pairs / MFMA_F32_FLOPS * 1e3, "useful_tflops": 2.0 * n * d * d / (ms * 1e-3) / 1e12}
    print("n %7d d %4d: moment_kernel %.3f ms (%.3f .. %.3f) = %.1f useful TFLOP/s; HBM floor %.4f ms (%.0f %%), MFMA floor of the issued tiles "
          "%.4f ms (%.0f %%); compute call %.3f ms; train_pca %.1f ms (%.1f .. %.1f; eigh at this d alone %.1f ms); host numpy f32 x.T @ x %.1f ms"
          % (n, d, *table[(0, 0)]["moment_ms"], row["useful_tflops"], row["hbm_floor_ms"], 100 * row["hbm_floor_ms"] / ms,
             row["mfma_floor_ms_issued"], 100 * row["mfma_floor_ms_issued"] / ms, table[(0, 0)]["compute_call_ms"][0], *row["train_pca_ms"], t_eigh,
             row["host_numpy_f32_ms"][0]), flush=True)
    for s, v in table.items():
        print("        kr=%2d S=%4d: moment_kernel %.3f ms (%.3f .. %.3f), compute call %.3f ms; %s"
              % (*s, *v["moment_ms"], v["compute_call_ms"][0], v["info"]), flush=True)
    return row


def info_of(text):
    return dict(kv.split("=", 1) for kv in text.split() if "=" in kv)


warm = vlq.GpuMoments(128)
xw = torch.from_numpy(rng.standard_normal((100000, 128)).astype(np.float32)).to(dev)
t_end = time.time() + 1.0
while time.time() < t_end:          # clocks up before the first timed call
    warm.compute(xw)
    warm.last_info()
warm.close()

rows = [one_shape(128000, 128), one_shape(96000, 96), one_shape(250000, 960)]
if out_file:
    with open(out_file, "w") as f:
        json.dump({"reps": reps, "shapes": rows}, f, indent=1)
