"""Numpy restatement of IndexIVFFlat's search, as include/vlq_ivfpq.h (vlq_ivfflat_*) specifies it.

TEST INFRASTRUCTURE ONLY.  Every fp32 operation is one numpy float32 operation in the reference's order:

  fvec_L2sqr (utils.cpp:481-506)           four accumulators s[l] += (x[4i+l] - y[4i+l])^2 (sub, mul, add not fused); the
                                           zero-padded tail is added only when d % 4 != 0; then (s0 + s1) + (s2 + s3)
  fvec_inner_product (utils.cpp:509-533)   the same with s[l] += x[4i+l] * y[4i+l]; the tail added whatever d is
  list walk  key < 0 skipped, key >= nlist an error; every other key counts as a visited list, empty or not, and its
             vectors are scanned in stored order (IndexIVF.cpp:290-314, :340-364)
  rows       L2: the k smallest (dis, scan position), ascending, FLT_MAX / -1 padding (max-heap, dis < top)
             inner product: the k largest ip, earlier scan position first among equals, descending, -FLT_MAX / -1 padding
             (min-heap, ip > top)
  plain      l2_plain / ip_plain: one accumulator, left to right (fvec_L2sqr_ref's order, utils.cpp:441-452) -- what a
             fixture must NOT be reproduced by, or it cannot tell the right order from a wrong one
"""
import numpy as np

from ip_ref import FLT_MAX, F32, ip_sse  # noqa: F401


def l2_sse(x, y):
    """fvec_L2sqr over the last axis of x and y (broadcast against each other), float32."""
    x = np.asarray(x, dtype=F32)
    y = np.asarray(y, dtype=F32)
    d = x.shape[-1]
    shape = np.broadcast_shapes(x.shape[:-1], y.shape[:-1])
    s = [np.zeros(shape, F32) for _ in range(4)]
    d4 = d - d % 4

    def sq(j):
        a = (x[..., j] - y[..., j]).astype(F32)
        return (a * a).astype(F32)

    for i in range(0, d4, 4):
        for l in range(4):
            s[l] = (s[l] + sq(i + l)).astype(F32)
    if d4 < d:
        for l in range(4):
            s[l] = (s[l] + (sq(d4 + l) if d4 + l < d else F32(0))).astype(F32)
    return ((s[0] + s[1]).astype(F32) + (s[2] + s[3]).astype(F32)).astype(F32)


def l2_plain(x, y):
    x = np.asarray(x, dtype=F32)
    y = np.asarray(y, dtype=F32)
    s = np.zeros(np.broadcast_shapes(x.shape[:-1], y.shape[:-1]), F32)
    for j in range(x.shape[-1]):
        a = (x[..., j] - y[..., j]).astype(F32)
        s = (s + (a * a).astype(F32)).astype(F32)
    return s


def ip_plain(x, y):
    x = np.asarray(x, dtype=F32)
    y = np.asarray(y, dtype=F32)
    s = np.zeros(np.broadcast_shapes(x.shape[:-1], y.shape[:-1]), F32)
    for j in range(x.shape[-1]):
        s = (s + (x[..., j] * y[..., j]).astype(F32)).astype(F32)
    return s


def scan_query(q, keys, vecs, ids, list_offsets, k, metric, dist=None):
    """search_knn_L2sqr / search_knn_inner_product of one query: (D [k], I [k], lists visited, ndis)."""
    nlist = list_offsets.shape[0] - 1
    ip = metric == "ip"
    if dist is None:
        dist = ip_sse if ip else l2_sse
    dis_all, lab_all = [], []
    nvisit = ndis = 0
    for key in keys:
        key = int(key)
        if key < 0:
            continue
        if key >= nlist:
            raise ValueError("key %d >= nlist %d" % (key, nlist))
        nvisit += 1
        o0, o1 = int(list_offsets[key]), int(list_offsets[key + 1])
        ndis += o1 - o0
        if o1 > o0:
            dis_all.append(dist(q, vecs[o0:o1]))
            lab_all.append(ids[o0:o1])
    D = np.full(k, -FLT_MAX if ip else FLT_MAX, F32)
    I = np.full(k, -1, np.int64)
    if dis_all:
        dis = np.concatenate(dis_all)
        lab = np.concatenate(lab_all)
        val = (-dis if ip else dis) + F32(0)        # + 0.0: -0 and +0 are one value to the heap's compare
        order = np.lexsort((np.arange(dis.size), val))[:k]
        order = order[val[order] < FLT_MAX]
        D[:order.size] = dis[order]
        I[:order.size] = lab[order]
    return D, I, nvisit, ndis


def search_preassigned(z, xq, keys, k, metric, dist=None):
    """Rows of a whole batch from a fixture's arrays z: (D, I, lists visited [nq], ndis [nq])."""
    nq = xq.shape[0]
    D = np.empty((nq, k), F32)
    I = np.empty((nq, k), np.int64)
    nv = np.empty(nq, np.int64)
    nd = np.empty(nq, np.int64)
    for i in range(nq):
        D[i], I[i], nv[i], nd[i] = scan_query(xq[i], keys[i], z["vecs"], z["ids"], z["list_offsets"], k, metric, dist)
    return D, I, nv, nd


def discriminates(z, xq, keys, k, metric, Dref):
    """True if the plain left-to-right order differs in bits from Dref in at least one slot."""
    Dp, _I, _v, _n = search_preassigned(z, xq, keys, k, metric, ip_plain if metric == "ip" else l2_plain)
    return not np.array_equal(Dp.view(np.uint32), Dref.view(np.uint32))
