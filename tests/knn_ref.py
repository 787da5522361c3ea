"""Restatement of the flat exact k-NN search (faiss::IndexFlat::search, IndexFlat.cpp:41-56; utils.cpp:726-946) as
include/vlq_ivfpq.h (vlq_flat_*) specifies it.

TEST INFRASTRUCTURE ONLY.  Every fp32 operation is one float32 operation in the stated order:

  dispatch   nq < 20 and d % 4 == 0: the per-pair SSE kernels ("direct"); otherwise the GEMM formulation ("gemm").  The nq is
             the whole call's.
  L2         direct: fvec_L2sqr per pair; gemm: (|x|^2 + |y|^2) - 2 ip, norms in fvec_norm_L2sqr's order, ip the fmaf chain over
             k = 0 .. d-1 from 0.  Both are the oracle's orc_knn_L2sqr (oracle/ivfpq_oracle.cpp), force_path 1 / 2, canonical.
  IP         direct: fvec_inner_product (tests/ip_ref.py: ip_sse); gemm: the fmaf chain, restated here in numpy (fma32).
  rows       the k best by the total order (distance, position): L2 ascending, padded FLT_MAX / -1; inner product descending,
             the lower position first among equals, padded -FLT_MAX / -1.  -0 and +0 are one value.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from ip_ref import ip_sse  # noqa: E402

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def is_direct(nq, d):
    """utils.cpp:741, :939"""
    return nq < 20 and d % 4 == 0


def _fma32_odd(p, c):
    """round32(p + c) for float64 p (an exact product of two float32) and c: the float64 sum is rounded to odd (TwoSum gives the
    error term), so that the final rounding to float32 is the single rounding of the exact p + c"""
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    si = s.view(np.int64).copy()
    fix = (e != 0) & ((si & 1) == 0)
    up = (e > 0) == (s > 0)         # towards larger magnitude
    si = np.where(fix, np.where(up, si + 1, si - 1), si)
    return si.view(np.float64).astype(F32)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays.  The product is exact in float64.  Rounding the float64 sum again to float32 is wrong only
    where that sum sits on a float32 rounding midpoint (its low 29 mantissa bits are 1 0...0) or the result is subnormal: those
    few elements are redone by _fma32_odd."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    out = s.astype(F32)
    slow = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | (np.abs(s) < 2.0 ** -125)
    slow &= s != 0
    if slow.any():
        out[slow] = _fma32_odd(p[slow], c[slow])
    return out


def ip_chain(xq, xb):
    """[nq][nb] inner products, the fmaf chain over k = 0 .. d-1 from 0"""
    xq, xb = np.asarray(xq, F32), np.asarray(xb, F32)
    acc = np.zeros((xq.shape[0], xb.shape[0]), F32)
    for c in range(xq.shape[1]):
        acc = fma32(xq[:, c][:, None], xb[:, c][None, :], acc)
    return acc


def ip_matrix(xq, xb, direct):
    if direct:
        return ip_sse(np.asarray(xq, F32)[:, None, :], np.asarray(xb, F32)[None, :, :])
    return ip_chain(xq, xb)


def rows_from_matrix(dis, k, descending):
    """the k best of every row of dis [nq][nb] by (value, position)"""
    nq, nb = dis.shape
    D = np.full((nq, k), -FLT_MAX if descending else FLT_MAX, F32)
    I = np.full((nq, k), -1, np.int64)
    v = dis + F32(0)
    key = -v if descending else v
    order = np.argsort(key, axis=1, kind="stable")[:, :k]         # stable: the lower position first among equals
    kept = np.take_along_axis(key, order, axis=1) < FLT_MAX         # the heap starts at FLT_MAX and admits only below it
    m = order.shape[1]
    D[:, :m] = np.where(kept, np.take_along_axis(dis, order, axis=1), D[:, :m])
    I[:, :m] = np.where(kept, order, -1)
    return D, I


def l2_oracle(xq, xb, k, direct):
    from oracle import pyoracle
    xq = np.ascontiguousarray(xq, F32)
    xb = np.ascontiguousarray(xb, F32)
    nq, d = xq.shape
    D = np.empty((nq, k), F32)
    I = np.empty((nq, k), np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pyoracle.lib().orc_knn_L2sqr(p(xq), p(xb), C.c_size_t(d), C.c_size_t(nq), C.c_size_t(xb.shape[0]), C.c_size_t(k), p(D), p(I),
                                 C.c_int(1), C.c_int(1 if direct else 2))
    return D, I


def search(xq, xb, k, metric, nq_call=None):
    """(D, I) of IndexFlat::search; nq_call: the queries of the whole call when xq holds some of them"""
    xq = np.asarray(xq, F32)
    xb = np.asarray(xb, F32).reshape(-1, xq.shape[1])
    nq, d = xq.shape
    direct = is_direct(nq if nq_call is None else nq_call, d)
    ip = metric in ("ip", 0)
    if xb.shape[0] == 0:
        return np.full((nq, k), -FLT_MAX if ip else FLT_MAX, F32), np.full((nq, k), -1, np.int64)
    if ip:
        return rows_from_matrix(ip_matrix(xq, xb, direct), k, True)
    D, I = l2_oracle(xq, xb, k, direct)
    D[I < 0] = FLT_MAX
    return D, I


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))
