"""Restatement of the flat index's range search (faiss::IndexFlat::range_search, IndexFlat.cpp:58-70; utils.cpp:1090-1262) as
include/vlq_ivfpq.h (vlq_flat_range_search) specifies it.

TEST INFRASTRUCTURE ONLY.  Every fp32 operation is one float32 operation in the stated order:

  dispatch   nq < 20 and d % 4 == 0: range_search_sse, fvec_L2sqr / fvec_inner_product per pair (tests/ivfflat_ref.py: l2_sse,
             tests/ip_ref.py: ip_sse); otherwise range_search_blas.  The nq is the whole call's.
  blas L2    (x_norm + y_norm) - 2 * ip, left to right (utils.cpp:1148), the norms in fvec_norm_L2sqr's order (ip_sse(x, x)), ip
             the fmaf chain over k = 0 .. d-1 from 0 (tests/knn_ref.py: ip_chain).  No clamp.
  blas IP    ip alone
  hit        dis < radius (L2), ip > radius (inner product, un-negated); strict, a NaN on either side is no hit
  result     lims [nq + 1]: exclusive prefix sums of the hits per query; D, I packed behind each other, a query's hits in
             ascending position
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from ip_ref import ip_sse  # noqa: E402
from ivfflat_ref import l2_sse  # noqa: E402
from knn_ref import ip_chain, is_direct  # noqa: E402

F32 = np.float32


def norms(x):
    """fvec_norm_L2sqr per row"""
    x = np.asarray(x, F32)
    return ip_sse(x, x)


def matrix(xq, xb, metric, nq_call=None):
    """[nq][nb] distances (L2) resp. inner products of the path the call's nq takes"""
    xq = np.asarray(xq, F32)
    xb = np.asarray(xb, F32).reshape(-1, xq.shape[1])
    nq, d = xq.shape
    ip = metric in ("ip", 0)
    if is_direct(nq if nq_call is None else nq_call, d):
        return (ip_sse if ip else l2_sse)(xq[:, None, :], xb[None, :, :])
    dot = ip_chain(xq, xb)
    if ip:
        return dot
    with np.errstate(over="ignore", invalid="ignore"):
        s = (norms(xq)[:, None] + norms(xb)[None, :]).astype(F32)
        return (s - (F32(2) * dot).astype(F32)).astype(F32)


def from_matrix(dis, radius, metric):
    """(lims, D, I) of the hits of dis [nq][nb] at the radius"""
    with np.errstate(invalid="ignore"):
        hit = dis > F32(radius) if metric in ("ip", 0) else dis < F32(radius)
    lims = np.zeros(dis.shape[0] + 1, np.int64)
    np.cumsum(hit.sum(1), out=lims[1:])
    q, j = np.nonzero(hit)          # row-major: ascending position within a query
    return lims, np.ascontiguousarray(dis[q, j], F32), j.astype(np.int64)


def range_search(xq, xb, radius, metric, nq_call=None):
    xq = np.asarray(xq, F32)
    xb = np.asarray(xb, F32).reshape(-1, xq.shape[1])
    if xb.shape[0] == 0 or xq.shape[0] == 0:
        return np.zeros(xq.shape[0] + 1, np.int64), np.zeros(0, F32), np.zeros(0, np.int64)
    return from_matrix(matrix(xq, xb, metric, nq_call), radius, metric)


def same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
