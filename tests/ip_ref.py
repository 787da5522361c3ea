"""Numpy restatement of the inner-product metric of IndexIVFPQ, as include/vlq_ivfpq.h (vlq_ivfpq_set_metric) specifies it.

TEST INFRASTRUCTURE ONLY.  Every fp32 operation is one numpy float32 operation in the reference's order:

  fvec_inner_product (utils.cpp:509-533)   four accumulators s[l] += x[4i+l] * y[4i+l] (multiply and add not fused), the
                                           zero-padded tail product added unconditionally, then (s0 + s1) + (s2 + s3)
  table      sim_table[m][j] = -fvec_inner_product(q_m, pq_centroid[m][j], dsub), once per query (IndexIVFPQ.cpp:548-555)
  dis0       by residual -fvec_inner_product(q, centroid[key], d) (:609-616; coarse_dis is not used), else 0 (:579-590)
  code       dis = dis0; dis += tab[m][code[m]] for m = 0 .. M-1 (:786-800); admitted by (dis, scan position)
  list walk  key < 0 skipped, key >= nlist an error, empty lists skipped, stop after the list that takes the number of
             scanned codes to max_codes (:1002-1035)
  rows       the k smallest (dis, scan position), every value negated: descending inner products, -FLT_MAX / -1 padding
  coarse     the nprobe largest inner products, descending, the lower id first among equals (IndexFlat.cpp:47-50,
             utils.cpp:726-755)
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def ip_sse(x, y):
    """fvec_inner_product over the last axis of x and y (broadcast against each other), float32."""
    x = np.asarray(x, dtype=F32)
    y = np.asarray(y, dtype=F32)
    d = x.shape[-1]
    shape = np.broadcast_shapes(x.shape[:-1], y.shape[:-1])
    s = [np.zeros(shape, F32) for _ in range(4)]
    d4 = d - d % 4
    for i in range(0, d4, 4):
        for l in range(4):
            s[l] = (s[l] + (x[..., i + l] * y[..., i + l]).astype(F32)).astype(F32)
    for l in range(4):      # the masked tail: lanes past d hold 0 * 0
        if d4 + l < d:
            s[l] = (s[l] + (x[..., d4 + l] * y[..., d4 + l]).astype(F32)).astype(F32)
        else:
            s[l] = (s[l] + F32(0)).astype(F32)
    return ((s[0] + s[1]).astype(F32) + (s[2] + s[3]).astype(F32)).astype(F32)


def query_table(q, pq_centroids):
    """-compute_inner_prod_table(q): [M][ksub]."""
    M, ksub, dsub = pq_centroids.shape
    qm = np.asarray(q, F32).reshape(M, 1, dsub)
    return -ip_sse(qm, pq_centroids)


def scan_query(q, keys, coarse_centroids, pq_centroids, codes, ids, list_offsets, k, by_residual=True, max_codes=0,
               store_pairs=False):
    """search_knn_with_key of one query: (D [k], I [k], ncode)."""
    nlist = list_offsets.shape[0] - 1
    M = pq_centroids.shape[0]
    tab = query_table(q, pq_centroids)
    dis_all, lab_all = [], []
    nscan = 0
    for key in keys:
        key = int(key)
        if key < 0:
            continue
        if key >= nlist:
            raise ValueError("key %d >= nlist %d" % (key, nlist))
        o0, o1 = int(list_offsets[key]), int(list_offsets[key + 1])
        n = o1 - o0
        nscan += n
        if n == 0:
            continue
        dis0 = -ip_sse(q, coarse_centroids[key]) if by_residual else F32(0)
        dis = np.full(n, dis0, F32)
        lc = codes[o0:o1]
        for m in range(M):
            dis = (dis + tab[m][lc[:, m]]).astype(F32)
        dis_all.append(dis)
        lab_all.append((np.int64(key) << 32 | np.arange(n, dtype=np.int64)) if store_pairs else ids[o0:o1])
        if max_codes and nscan >= max_codes:
            break
    D = np.full(k, -FLT_MAX, F32)
    I = np.full(k, -1, np.int64)
    if dis_all:
        dis = np.concatenate(dis_all)
        lab = np.concatenate(lab_all)
        # + 0.0: -0 and +0 are one value to the heap's `<`
        order = np.lexsort((np.arange(dis.size), dis + F32(0)))[:k]
        order = order[dis[order] < FLT_MAX]
        D[:order.size] = -dis[order]
        I[:order.size] = lab[order]
    return D, I, nscan


def search_preassigned(z, xq, keys, k, store_pairs=False):
    """Rows of a whole batch from a fixture's arrays z: (D, I, ncode [nq])."""
    nq = xq.shape[0]
    D = np.empty((nq, k), F32)
    I = np.empty((nq, k), np.int64)
    nc = np.empty(nq, np.int64)
    for i in range(nq):
        D[i], I[i], nc[i] = scan_query(xq[i], keys[i], z["coarse_centroids"], z["pq_centroids"], z["codes"], z["ids"],
                                       z["list_offsets"], k, bool(int(z["by_residual"])), int(z["max_codes"]), store_pairs)
    return D, I, nc


def coarse_search(centroids, xq, nprobe):
    """quantizer->search of an IndexFlatIP: (keys, coarse_dis), descending, lower id first among equals."""
    ip = ip_sse(np.asarray(xq, F32)[:, None, :], np.asarray(centroids, F32)[None, :, :])
    nq, nlist = ip.shape
    keys = np.full((nq, nprobe), -1, np.int64)
    dis = np.full((nq, nprobe), -FLT_MAX, F32)
    for i in range(nq):
        order = np.lexsort((np.arange(nlist), -(ip[i] + F32(0))))[:nprobe]
        keys[i, :order.size] = order
        dis[i, :order.size] = ip[i][order]
    return keys, dis
