"""numpy float32 restatement of the IVFPQR refine stage (the loop of IndexIVFPQR::search, IndexIVFPQ.cpp:1392-1444).

For each query and each shortlist entry (list << 32 | offset, -1 = skip), in shortlist order:

    r1 = x - coarse_centroid[list]                 Index::compute_residual
    r2 = r1 - pq.decode(codes[list][ofs])
    r3 = refine_pq.decode(refine code of the slot)
    dis = fvec_L2sqr(r3, r2, d)                    utils.cpp:481-506: four running sums, sum l % 4 takes dimensions
                                                   l, l + 4, ... ascending, t = r3 - r2, s = s + t * t with the multiply
                                                   and the add rounded separately, result (s0 + s1) + (s2 + s3)

and the k smallest (dis, shortlist position), ascending, padded with -1 / FLT_MAX; labels are ids[slot].  Every numpy
operation below is one correctly rounded float32 operation per element, so the result is the reference's bit for bit
(tests/test_refine_restatement.py holds it to the fixtures).  Vectorised over the candidates of a query; a Python loop
runs over the d / 4 chain steps.
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def pq_decode(centroids, codes):
    """centroids [M][ksub][dsub], codes [n][M] u8 -> [n][M * dsub]"""
    M = centroids.shape[0]
    return np.concatenate([centroids[m][codes[:, m]] for m in range(M)], axis=1)


def l2sqr_sse(a, b):
    """fvec_L2sqr of the rows of a and b in the reference's operation order"""
    n, d = a.shape
    t = (a - b).astype(np.float32)
    sq = (t * t).astype(np.float32)
    s = np.zeros((n, 4), np.float32)
    for i in range(d // 4):
        s = (s + sq[:, 4 * i:4 * i + 4]).astype(np.float32)
    r = d % 4
    if r:
        tail = np.zeros((n, 4), np.float32)
        tail[:, :r] = sq[:, d - r:]
        s = (s + tail).astype(np.float32)
    return ((s[:, 0] + s[:, 1]).astype(np.float32) + (s[:, 2] + s[:, 3]).astype(np.float32)).astype(np.float32)


def refine_distances(x, shortlist, coarse, pq_centroids, codes, refine_centroids, refine_codes, list_offsets):
    """[n][k_coarse] refined distances (NaN where the entry is -1) and the list slots (-1 there)"""
    x = np.ascontiguousarray(x, np.float32)
    n, kc = shortlist.shape
    dis = np.full((n, kc), np.nan, np.float32)
    slots = np.full((n, kc), -1, np.int64)
    off = np.asarray(list_offsets, np.int64)
    for q in range(n):
        sl = shortlist[q]
        js = np.nonzero(sl != -1)[0]
        if js.size == 0:
            continue
        lists = sl[js] >> 32
        ofs = sl[js] & 0xffffffff
        assert (lists >= 0).all() and (lists < off.size - 1).all() and (ofs < off[lists + 1] - off[lists]).all(), "pair outside the lists"
        slot = off[lists] + ofs
        r1 = (x[q][None, :] - coarse[lists]).astype(np.float32)
        r2 = (r1 - pq_decode(pq_centroids, codes[slot])).astype(np.float32)
        r3 = pq_decode(refine_centroids, refine_codes[slot])
        dis[q, js] = l2sqr_sse(r3, r2)
        slots[q, js] = slot
    return dis, slots


def refine_ref(x, shortlist, k, coarse, pq_centroids, codes, refine_centroids, refine_codes, ids, list_offsets):
    """D [n][k], I [n][k] of the refine stage"""
    dis, slots = refine_distances(x, shortlist, coarse, pq_centroids, codes, refine_centroids, refine_codes, list_offsets)
    n = shortlist.shape[0]
    D = np.full((n, k), FLT_MAX, np.float32)
    I = np.full((n, k), -1, np.int64)
    for q in range(n):
        js = np.nonzero((slots[q] >= 0) & (dis[q] < FLT_MAX))[0]      # `dis < heap top`, the heap starts at FLT_MAX
        order = js[np.argsort(dis[q, js], kind="stable")][:k]         # (distance, shortlist position)
        D[q, :order.size] = dis[q, order]
        I[q, :order.size] = ids[slots[q, order]]
    return D, I


def case_refine_ref(case, shortlist, k=None):
    """refine_ref on a refine_* fixture (tests/util.py Case)"""
    return refine_ref(case.xq, shortlist, case.k if k is None else k, case["coarse_centroids"], case["pq_centroids"], case["codes"],
                      case["refine_centroids"], case["refine_codes"], case["ids"], case["list_offsets"])


REFINE_CASE_NAMES = ["refine_c1_small", "refine_tail", "refine_padding", "refine_duplicates", "refine_k_wide"]
