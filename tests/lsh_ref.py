"""Restatement of faiss::IndexLSH (IndexLSH.cpp, hamming.cpp:264-379, :474-506) as include/vlq_ivfpq.h (vlq_lsh_*) specifies it.

TEST INFRASTRUCTURE ONLY.  Every fp32 operation is one float32 operation in the stated order:

  apply      rotate_data: xt[j] = fmaf chain over i = 0 .. d-1 ascending of A[j][i] * x[i], starting from b[j] (0.0f without a
             bias) -- knn_ref.fma32; otherwise the first nbits components.  Thresholds: one float32 subtraction afterwards.
  bits       bit j = xt[j] >= 0 (-0.0f sets it, NaN does not); dimension 0 is the least significant bit of byte 0; pad bits zero
  train      per-bit median of the un-thresholded xt: element n/2 of the sorted column (n odd), (x[n/2-1] + x[n/2]) / 2 in
             float32 (n even)
  search     integer Hamming distances as float32; the k best by the total order (distance, position), ascending, padded
             2147483648.0 (= (float)INT_MAX) / -1
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from knn_ref import fma32  # noqa: E402

F32 = np.float32
PAD = F32(2147483648.0)
SERVED = (4,) + tuple(range(8, 129, 8))        # hammings_knn's widths (hamming.cpp:482-505), up to 128 bytes

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def served(code_size):
    return code_size in SERVED


def apply(x, nbits, A=None, b=None, thresholds=None):
    """apply_preprocess: [n][nbits] float32"""
    x = np.asarray(x, F32)
    n, d = x.shape
    if A is not None:
        A = np.asarray(A, F32).reshape(nbits, d)
        xt = np.zeros((n, nbits), F32) if b is None else np.broadcast_to(np.asarray(b, F32), (n, nbits)).copy()
        for i in range(d):
            xt = fma32(A[:, i][None, :], x[:, i][:, None], xt)
    else:
        assert d >= nbits
        xt = x[:, :nbits].copy()
    if thresholds is not None:
        xt = (xt - np.asarray(thresholds, F32)[None, :]).astype(F32)
    return xt


def bits(xt):
    """fvecs2bitvecs: [n][(nbits + 7) // 8] uint8"""
    with np.errstate(invalid="ignore"):
        on = np.asarray(xt, F32) >= 0
    return np.packbits(on, axis=1, bitorder="little")


def encode(x, nbits, A=None, b=None, thresholds=None):
    return bits(apply(x, nbits, A, b, thresholds))


def train(x, nbits, A=None, b=None):
    """IndexLSH::train's thresholds [nbits]"""
    xt = np.sort(apply(x, nbits, A, b), axis=0)
    n = xt.shape[0]
    if n % 2 == 1:
        return xt[n // 2].copy()
    return ((xt[n // 2 - 1] + xt[n // 2]) / F32(2)).astype(F32)


def hamming(qcodes, codes):
    """[nq][nb] int32"""
    qcodes, codes = np.asarray(qcodes, np.uint8), np.asarray(codes, np.uint8)
    out = np.zeros((qcodes.shape[0], codes.shape[0]), np.int32)
    for c in range(qcodes.shape[1]):
        out += _POP8[qcodes[:, c][:, None] ^ codes[:, c][None, :]]
    return out


def search_codes(qcodes, codes, k):
    """(D, I): the k best by (distance, position)"""
    codes = np.asarray(codes, np.uint8).reshape(-1, qcodes.shape[1])
    nq, nb = qcodes.shape[0], codes.shape[0]
    D = np.full((nq, k), PAD, F32)
    I = np.full((nq, k), -1, np.int64)
    if nb:
        hd = hamming(qcodes, codes)
        order = np.argsort(hd, axis=1, kind="stable")[:, :k]
        m = order.shape[1]
        D[:, :m] = np.take_along_axis(hd, order, axis=1).astype(F32)
        I[:, :m] = order
    return D, I


def check_labels(D, I, qcodes, codes):
    """every returned label's recomputed distance equals its D, labels of a row are distinct, padding is PAD / -1 at the end"""
    hd = hamming(qcodes, codes) if codes.shape[0] else np.zeros((qcodes.shape[0], 0), np.int32)
    for r in range(D.shape[0]):
        live = I[r] >= 0
        n = int(live.sum())
        assert live[:n].all(), "row %d: padding before a live entry" % r
        assert n == min(D.shape[1], codes.shape[0]), "row %d: %d live entries" % (r, n)
        assert np.unique(I[r, :n]).size == n, "row %d: a label twice" % r
        assert np.array_equal(hd[r, I[r, :n]].astype(F32), D[r, :n]), "row %d: a label's distance is not its D" % r
        assert (D[r, n:] == PAD).all(), "row %d: padding distance" % r
