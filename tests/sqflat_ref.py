"""Numpy restatement of IndexScalarQuantizer's search, as include/vlq_ivfpq.h (vlq_sq_*) specifies it.

TEST INFRASTRUCTURE ONLY.  The codec, the two operation orders, the encoder and RS_minmax training are those of
tests/ivfsq_ref.py (IndexScalarQuantizer.cpp); what differs from the IVF index (:727-781):

  y       the query itself: no centroid is subtracted under L2
  accu0   the constant 0: under inner product and d % 8 == 0 the result is still (0 + lo) + hi; the scalar order starts at 0
  rows    the reference leaves its heap unordered (no maxheap_reorder / minheap_reorder in this search).  The library's rows
          are sorted: L2 the k smallest (dis, position) ascending, FLT_MAX / -1 padding; inner product the k largest, the
          earlier position first among equals, descending, -FLT_MAX / -1 padding.  sorted_rows() brings a reference row into
          that order.
"""
import numpy as np

import ivfsq_ref as sr
from ivfsq_ref import FLT_MAX, F32, QTYPES  # noqa: F401


def all_distances(codes, xq, metric, qtype, trained, order8=None):
    """dis [nq][ntotal]: compute_distance_L2 / compute_distance_IP of every query against every stored code"""
    d = xq.shape[1]
    if order8 is None:
        order8 = d % 8 == 0
    rec = sr.decode(codes, d, qtype, trained, order8)
    out = np.empty((xq.shape[0], rec.shape[0]), F32)
    for i in range(xq.shape[0]):
        out[i] = sr.distances(xq[i], rec, metric == "ip", order8, F32(0))
    return out


def rows_of(dis, k, metric):
    """the library's rows from all distances of a batch: (D [nq][k], I [nq][k])"""
    ip = metric == "ip"
    nq, n = dis.shape
    D = np.full((nq, k), -FLT_MAX if ip else FLT_MAX, F32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        val = (-dis[i] if ip else dis[i]) + F32(0)      # + 0.0: -0 and +0 are one value to the heap's compare
        order = np.lexsort((np.arange(n), val))[:k]
        order = order[val[order] < FLT_MAX]
        D[i, :order.size] = dis[i][order]
        I[i, :order.size] = order
    return D, I


def search(codes, trained, xq, k, metric, qtype, order8=None):
    return rows_of(all_distances(codes, xq, metric, qtype, trained, order8), k, metric)


def sorted_rows(D, I, metric):
    """a reference row (heap order) in the library's order: distance ascending (inner product: descending), then label
    ascending; the padding (label -1) last"""
    ip = metric == "ip"
    Ds, Is = np.empty_like(D), np.empty_like(I)
    for r in range(D.shape[0]):
        val = (-D[r] if ip else D[r]) + F32(0)
        order = np.lexsort((I[r], val, I[r] == -1))
        Ds[r], Is[r] = D[r][order], I[r][order]
    return Ds, Is


def tie_across_kth(dis, k, metric):
    """rows where a group of equal distances crosses the k-th place: the (k+1)-th best equals the k-th"""
    Dk1, Ik1 = rows_of(dis, k + 1, metric)
    return (Dk1[:, k] == Dk1[:, k - 1]) & (Ik1[:, k] != -1)


def tied_rows(D, I):
    return sr.tied_rows(D, I)
