#!/usr/bin/env python3
"""vlq.GpuPQTrainer.train (csrc/pq_train.hip: every slice's assignment in one launch per iteration) beside what the library
offered for the same job before it: a loop of M vlq.GpuKMeans runs over contiguous slice copies -- which is also the trainer's
loop route -- timed in the same process.

Shapes (d, M, nbits; n 65 536 rows = the reference's subsample at 8 bits, 25 iterations): (128, 16, 8), (96, 48, 8), (128, 8, 8).
Rows are device-resident.  A whole train is timed with a host clock around a call that ends in a stream synchronisation; the
per-iteration assignment is the stream time between events (vlq_pqtrain_last_info: train_assign_ms / iters).  The device is kept
busy for about a second first, every variant runs untimed before it is timed, a row gives the median and the minimum / maximum.
The two routes' codebooks are compared bit for bit.
    python tools/time_pq_train.py [reps] [out.json] [n]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_file = sys.argv[2] if len(sys.argv) > 2 else None
n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
if not torch.cuda.is_available():
    raise SystemExit("tools/time_pq_train.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
rng = np.random.default_rng(23)
NITER = 25
stream_ptr = torch.cuda.current_stream().cuda_stream      # every handle works on torch's stream


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return (statistics.median(v), min(v), max(v))


def one_shape(d, M, nbits):
    ksub, dsub = 1 << nbits, d // M
    xh = rng.standard_normal((n, d), dtype=np.float32)
    xh += 2 * rng.standard_normal((ksub, d), dtype=np.float32)[rng.integers(0, ksub, n)]
    x = torch.from_numpy(xh).to(dev)
    tr = vlq.GpuPQTrainer(d, M, nbits, niter=NITER)
    tr.set_stream(stream_ptr)
    kms = [vlq.GpuKMeans(dsub, ksub, niter=NITER) for _ in range(M)]
    for km in kms:
        km.set_stream(stream_ptr)
    got = {}

    def batched():
        got["batched"] = tr.train(x)

    def loop():          # the slice copies are part of the job: nothing else reads a strided slice
        got["loop"] = torch.stack([kms[m].train(x[:, m * dsub:(m + 1) * dsub].contiguous()) for m in range(M)])

    batched()
    loop()
    same = bool(torch.equal(got["batched"].view(torch.int32), got["loop"].view(torch.int32)))
    t_b, t_l, t_a = [], [], []
    for _ in range(reps):
        t_b.append(clock(batched))
        i = dict(kv.split("=", 1) for kv in tr.last_info().split() if "=" in kv)
        t_a.append(float(i["train_assign_ms"]) / int(i["iters"]))
        t_l.append(clock(loop))
    row = {"d": d, "M": M, "nbits": nbits, "n": n, "niter": NITER, "batched_train_ms": med(t_b), "loop_train_ms": med(t_l),
           "assign_ms_per_iter": med(t_a), "same_bits": same, "info": tr.last_info()}
    print("d %3d M %2d nbits %d n %d niter %d: batched train %.2f ms (%.2f .. %.2f), loop of %d GpuKMeans %.2f ms (%.2f .. %.2f), "
          "assignment per iteration %.4f ms (%.4f .. %.4f) | same bits %s" % (d, M, nbits, n, NITER, *row["batched_train_ms"], M,
                                                                            *row["loop_train_ms"], *row["assign_ms_per_iter"], same), flush=True)
    print("        " + tr.last_info(), flush=True)
    tr.close()
    for km in kms:
        km.close()
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

rows = [one_shape(128, 16, 8), one_shape(96, 48, 8), one_shape(128, 8, 8)]
if out_file:
    with open(out_file, "w") as f:
        json.dump({"reps": reps, "shapes": rows}, f, indent=1)
