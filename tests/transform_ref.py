"""Restatement of the vector transforms as include/vlq_ivfpq.h (vlq_transform_*) specifies them.  TEST INFRASTRUCTURE ONLY.
Every fp32 operation is one float32 operation in the stated order (knn_ref.fma32, ip_ref.ip_sse)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from ip_ref import ip_sse  # noqa: E402
from knn_ref import fma32  # noqa: E402

F32 = np.float32


def linear(x, A, b=None):
    """xt[r][j]: the fmaf chain over i ascending of A[j][i] * x[r][i], starting from b[j] (0.0f without a bias)"""
    x, A = np.asarray(x, F32), np.asarray(A, F32)
    xt = np.zeros((x.shape[0], A.shape[0]), F32) if b is None else np.broadcast_to(np.asarray(b, F32), (x.shape[0], A.shape[0])).copy()
    for i in range(A.shape[1]):
        xt = fma32(A[:, i][None, :], x[:, i][:, None], xt)
    return xt


def linear_reverse(y, A, b=None):
    """transform_transpose: the chain over j ascending from 0.0f of A[j][i] * (y[r][j] - b[j]), the difference rounded first"""
    y = np.asarray(y, F32)
    if b is not None:
        y = (y - np.asarray(b, F32)[None, :]).astype(F32)
    return linear(y, np.ascontiguousarray(np.asarray(A, F32).T))


def remap(x, m):
    x, m = np.asarray(x, F32), np.asarray(m)
    return np.where(m[None, :] < 0, F32(0), x[:, np.maximum(m, 0)]).astype(F32)


def remap_reverse(xt, m, d_in):
    x = np.zeros((xt.shape[0], d_in), F32)
    for j, i in enumerate(m):
        if i >= 0:
            x[:, i] = xt[:, j]
    return x


def l2norm(x):
    """fvec_renorm_L2: nr in the SSE order; rows with nr > 0 times (float)(1.0 / sqrtf(nr))"""
    x = np.asarray(x, F32)
    nr = ip_sse(x, x)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (1.0 / np.sqrt(nr).astype(np.float64)).astype(F32)
        return np.where((nr > 0)[:, None], (x * inv[:, None]).astype(F32), x)
