"""Numpy restatement of IndexRefineFlat's seam (IndexFlat.cpp:73-93, :194-213, :245-260), as include/vlq_ivfpq.h
(vlq_flat_compute_distance_subset, vlq_flat_refine) specifies it.

TEST INFRASTRUCTURE ONLY.  Every fp32 operation is one numpy float32 operation in the reference's order:

  distance   fvec_L2sqr / fvec_inner_product per (query, label) pair at every batch size (utils.cpp:974-1012: no BLAS branch):
             l2_sse / ip_sse of ivfflat_ref.py / ip_ref.py, knn_ref.py's per-pair order
  skip       a label < 0 keeps the distance it came in with (`continue`)
  rows       the k best of the k_base entries by the total order (distance, shortlist position): L2 ascending; inner product
             descending, the lower position first among equals.  Skipped entries take part with the distance and the label
             they carry.  The order is that of the distances' bit images (the device's keys): -0 sorts before +0, which no
             computed distance is.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from ivfflat_ref import F32, ip_sse, l2_sse  # noqa: E402


def is_ip(metric):
    return metric in ("ip", 0)


def compute_distance_subset(xb, xq, labels, distances, metric):
    """a copy of distances [n][k] with the live entries (label >= 0) recomputed"""
    xb = np.asarray(xb, F32).reshape(-1, xq.shape[1])
    labels = np.asarray(labels, np.int64)
    out = np.array(distances, dtype=F32, copy=True)
    live = labels >= 0
    assert (labels[live] < xb.shape[0]).all(), "a label >= ntotal"
    if live.any():
        rows, _cols = np.nonzero(live)
        fn = ip_sse if is_ip(metric) else l2_sse
        out[live] = fn(np.asarray(xq, F32)[rows], xb[labels[live]])
    return out


def ordered_image(dis):
    """the order-preserving uint32 image of float32 values (csrc/wave_topk.cuh: f32_to_ordered)"""
    b = np.ascontiguousarray(dis, F32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def reorder(sub_D, labels, k, metric):
    """reorder_2_heaps: the k best of every row by (distance, position), in the defined order"""
    img = ordered_image(sub_D).astype(np.uint64)
    if is_ip(metric):
        img = np.uint64(0xFFFFFFFF) - img
    key = (img << np.uint64(32)) | np.arange(sub_D.shape[1], dtype=np.uint64)[None, :]
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(np.asarray(sub_D, F32), order, axis=1), np.take_along_axis(np.asarray(labels, np.int64), order, axis=1)


def refine(xb, xq, base_D, base_I, k, metric):
    """(D, I) of lines 245-260 of IndexRefineFlat::search"""
    sub = compute_distance_subset(xb, xq, base_I, base_D, metric)
    return reorder(sub, base_I, k, metric)


def k_base(k, k_factor):
    """idx_t(k * k_factor), IndexFlat.cpp:224"""
    return int(F32(k) * F32(k_factor))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))
