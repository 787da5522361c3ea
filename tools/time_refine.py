#!/usr/bin/env python3
"""Cost and benefit of the IVFPQR refine stage on the bench's own data and shape (d 128, 1 M vectors, 4096 lists, nprobe 32,
10 000 queries): PQ 16x8 bit + refine 16x8 bit and the demo's PQ 8x8 bit + refine 16x8 bit (tests/demo_sift1M.cpp:98,
"IVF4096,PQ8+16"); k 10 with k_factor 1, 4, 16 and k 100 with k_factor 4.

Per row, HIP-event times of three calls taken in one process and alternating step by step (clock pre-warm, warm-up of
every shape, then `steps` timed steps, as bench.py does):
    first   search_preassigned(k = k_coarse, store_pairs) -- the first stage alone, the yardstick
    refined search_refined (coarse stage + first stage + refine stage)
    refine  the refine kernel alone, on the shortlist the first stage returned
and recall@1 against exact L2 ground truth (torch, on the device) of the refined search next to the plain index's.
   python tools/time_refine.py [steps]      env: MS=16,8 (first-stage code sizes)  ROWS=10:1,10:4,10:16,100:4 (k:k_factor)"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import vector_line_quantization_amd as vlq

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
dev = torch.device("cuda", 0)
base = argparse.Namespace(nq=10000, nb=1000000, nt=100000, d=128, nlist=4096, M=16, nprobe=32, k=10, sigma=0.005,
                          gmm_centres=2000, rank=12, spread=0.4)
MR, NBITS_R = 16, 8


def train_refine(g, a, coarse, pq, xt, gen):
    """refine_pq on the second-level residuals of a training sample (IndexIVFPQ.cpp:1317-1334)"""
    xs = xt[torch.randperm(xt.shape[0], generator=gen, device=dev)[:65536]].contiguous()
    assign, codes = g.encode(xs)
    assign, codes = torch.from_numpy(assign).to(dev), torch.from_numpy(codes).to(dev).long()
    dec = torch.cat([pq[m][codes[:, m]] for m in range(a.M)], dim=1)
    r2 = xs - coarse[assign] - dec
    ds = a.d // MR
    return torch.stack([bench.kmeans(torch, r2[:, m * ds:(m + 1) * ds].contiguous(), 1 << NBITS_R, 10, gen) for m in range(MR)])


def timed(fn_list, steps):
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for _ in fn_list]
    for s in range(steps):
        for i, fn in enumerate(fn_list):
            ev[i][s][0].record()
            fn()
            ev[i][s][1].record()
    torch.cuda.synchronize()
    return [float(np.median([a.elapsed_time(b) for a, b in e])) for e in ev]


for M in [int(v) for v in os.environ.get("MS", "16,8").split(",")]:
    a = argparse.Namespace(**vars(base))
    a.M = M
    g0, centres, coarse, pq, xb = bench.build_index(a, dev)          # the plain index (trains coarse + PQ)
    gen = torch.Generator(device=dev); gen.manual_seed(11)
    xt = bench.gmm(torch, gen, centres, a.nt, a.sigma, dev, a.rank, a.spread)
    gen.manual_seed(4321)
    rpq = train_refine(g0, a, coarse, pq, xt, gen)
    g = vlq.GpuIVFPQ(a.d, a.nlist, M, 8)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.set_coarse_centroids(coarse.contiguous())
    g.set_pq_centroids(pq.contiguous())
    g.set_refine_pq(MR, NBITS_R, rpq.contiguous())
    for i0 in range(0, xb.shape[0], 262144):
        g.add(xb[i0:i0 + 262144].contiguous())                       # IndexIVFPQR::add_core on the device
    torch.cuda.synchronize()
    gen.manual_seed(33)
    xq = bench.gmm(torch, gen, centres, a.nq, a.sigma, dev, a.rank, a.spread)
    cdis, keys = g.coarse_search(xq, a.nprobe)
    for _ in range(50):                                              # clock pre-warm
        g.search(xq, a.nprobe, 10)
    torch.cuda.synchronize()
    Dp, Ip = g0.search(xq, a.nprobe, 10)
    g0.stats()
    r1_plain, _ = bench.recall(torch, xq, xb, Ip.cpu().numpy(), a.nb, dev)
    for k, kf in [(int(r.split(":")[0]), float(r.split(":")[1])) for r in os.environ.get("ROWS", "10:1,10:4,10:16,100:4").split(",")]:
        kc = int(k * kf)
        Dsl = torch.empty((a.nq, kc), dtype=torch.float32, device=dev); sl = torch.empty((a.nq, kc), dtype=torch.int64, device=dev)
        D = torch.empty((a.nq, k), dtype=torch.float32, device=dev); I = torch.empty((a.nq, k), dtype=torch.int64, device=dev)
        Dk = torch.empty((a.nq, k), dtype=torch.float32, device=dev); Ik = torch.empty((a.nq, k), dtype=torch.int64, device=dev)
        fns = [lambda: g.search_preassigned(xq, keys, cdis, kc, store_pairs=True, D=Dsl, I=sl),
               lambda: g.search_refined(xq, a.nprobe, k, kf, D=D, I=I),
               lambda: g.refine(xq, sl, k, D=Dk, I=Ik),
               lambda: g.search(xq, a.nprobe, k, D=Dk, I=Ik)]
        timed(fns, 20)                                               # warm-up of this shape
        first, refined, refine, plain = timed(fns, steps)
        fns[1]()
        torch.cuda.synchronize()
        g.stats()
        r1, _ = bench.recall(torch, xq, xb, I.cpu().numpy(), a.nb, dev)
        print("PQ%dx8+%dx%d k=%-3d k_factor=%-4g k_coarse=%-4d first stage %.3f ms | search_refined %.3f ms | refine kernel alone %.3f ms "
              "(%.2f of the first stage) | plain search(k) %.3f ms | recall@1 refined %.3f, plain %.3f" % (
                  M, MR, NBITS_R, k, kf, kc, first, refined, refine, refine / first, plain, r1, r1_plain), flush=True)
    del g, g0
