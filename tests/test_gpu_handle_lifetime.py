"""Lifetime of the handles: every kind of index is built (the database added in three batches, so the lists grow and are laid
out again), searched once into device memory and destroyed straight away, with its work still in flight and its workspaces
allocated -- three times over in one process.  The buffers of a handle free themselves when it is deleted (csrc/dev_buf.h);
the rows of every cycle must be the first cycle's, bit for bit, and the third cycle must still find memory and streams."""
import numpy as np
import pytest

import vector_line_quantization_amd as vlq

pytestmark = pytest.mark.gpu

D_, M_, NBITS, NLIST, NB, NQ, NPROBE, K = 32, 8, 8, 16, 2000, 64, 4, 10
KINDS = ("l2", "ip", "polysemous", "ivfpqr", "imi", "line", "ivfflat", "ivfsq", "pq", "flat", "sq", "lsh")
ONE_LIST = ("pq", "flat", "sq", "lsh")          # the handles without inverted lists: add(x), search(x, k)


def world():
    rng = np.random.RandomState(1234)
    w = {"xb": rng.randn(NB, D_).astype(np.float32), "xq": rng.randn(NQ, D_).astype(np.float32)}
    w["coarse"] = w["xb"][rng.permutation(NB)[:NLIST]].copy()
    w["imi"] = (0.7 * rng.randn(2, 4, D_ // 2)).astype(np.float32)                 # 2 x 2 bits: 4^2 = 16 cells
    w["pq"] = (0.5 * rng.randn(M_, 1 << NBITS, D_ // M_)).astype(np.float32)
    w["rpq"] = (0.1 * rng.randn(8, 256, D_ // 8)).astype(np.float32)
    w["lambda"] = np.linspace(0.0, 1.0, 16).astype(np.float32)
    return w


def one_cycle(kind, w):
    """build, add in three batches, search once into device memory, destroy without synchronising; the rows as host arrays"""
    import torch
    if kind == "line":
        g = vlq.GpuVLQ(D_, NLIST, M_, NBITS, 4, 16)
        g.set_coarse_centroids(w["coarse"])
        g.build_graph()
        g.set_lambda_codebook(w["lambda"])
    elif kind == "ivfflat":
        g = vlq.GpuIVFFlat(D_, NLIST)
        g.set_coarse_centroids(w["coarse"])
    elif kind == "ivfsq":
        g = vlq.GpuIVFSQ(D_, NLIST, "8bit")
        g.set_coarse_centroids(w["coarse"])
        g.train(w["xb"])
    elif kind == "pq":
        g = vlq.GpuPQ(D_, M_, NBITS)
        g.set_centroids(w["pq"])
    elif kind == "flat":
        g = vlq.GpuFlat(D_)
    elif kind == "sq":
        g = vlq.GpuSQ(D_, "8bit")
        g.train(w["xb"])
    elif kind == "lsh":
        g = vlq.GpuLSH(D_, 64, rotate_data=True, train_thresholds=True)
        g.train(w["xb"])
    else:
        g = vlq.GpuIVFPQ(D_, NLIST, M_, NBITS, metric="ip" if kind == "ip" else "l2")
        if kind == "imi":
            g.set_imi_centroids(2, w["imi"])
        else:
            g.set_coarse_centroids(w["coarse"])
    if kind not in ("ivfflat", "ivfsq") + ONE_LIST:
        g.set_pq_centroids(w["pq"])
    if kind == "polysemous":
        g.set_polysemous_ht(28)
    if kind == "ivfpqr":
        g.set_refine_pq(8, 8, w["rpq"])
    # the index works on torch's stream: the copies below are ordered behind the search without anybody waiting for it
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    for lo, hi in ((0, 300), (300, 1100), (1100, NB)):
        g.add(w["xb"][lo:hi])
    assert g.ntotal == NB
    xq = torch.from_numpy(w["xq"]).cuda()
    if kind == "line":
        D, I = g.search(xq, NPROBE, 8, K)
    elif kind == "ivfpqr":
        D, I = g.search_refined(xq, NPROBE, K, 2.0)
    elif kind in ONE_LIST:
        D, I = g.search(xq, K)
    else:
        D, I = g.search(xq, NPROBE, K)
    assert D.is_cuda and I.is_cuda
    # host copies taken before the destroy, asynchronously: the destroy itself is the first to wait for the stream
    Dh = torch.empty(D.shape, dtype=D.dtype, pin_memory=True)
    Ih = torch.empty(I.shape, dtype=I.dtype, pin_memory=True)
    Dh.copy_(D, non_blocking=True)
    Ih.copy_(I, non_blocking=True)
    g.close()
    torch.cuda.synchronize()
    return Dh.numpy().copy(), Ih.numpy().copy()


@pytest.mark.parametrize("kind", KINDS)
def test_three_lifetimes_give_the_same_rows(kind):
    w = world()
    D0, I0 = one_cycle(kind, w)
    assert (I0[:, 0] >= 0).all(), "every query finds something in its %d probes" % NPROBE
    assert np.isfinite(D0[:, 0]).all()
    for cycle in (1, 2):
        D, I = one_cycle(kind, w)          # (the third cycle's creation succeeding is part of this)
        assert np.array_equal(D.view(np.uint32), D0.view(np.uint32)), (kind, cycle)
        assert np.array_equal(I, I0), (kind, cycle)
