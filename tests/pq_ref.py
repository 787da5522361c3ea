"""Numpy restatement of IndexPQ's search, as include/vlq_ivfpq.h (vlq_pq_*) specifies it.

TEST INFRASTRUCTURE ONLY.  Every fp32 operation is one numpy float32 operation in the reference's order:

  tables     compute_distance_tables / compute_inner_prod_tables (ProductQuantizer.cpp:439-493) per sub-quantizer with
             fvec_L2sqr / fvec_inner_product (l2_sse, ip_sse) -- the reference's own order while dsub < 16; for dsub >= 16 the
             reference goes through BLAS and this is the library's order, not the reference's
  ST_PQ      pq_estimators_from_tables (ProductQuantizer.cpp:46-143): M == 4: ((t0 + t1) + t2) + t3; M % 4 == 0: from 0, the
             groups ((t0 + t1) + t2) + t3 added one by one; any other M: from 0, left to right
  polysemous q_code = first argmin from 1e20 of the query's table (ProductQuantizer.cpp:363-383); a code passes if hd < ht, hd =
             popcount of the XOR or the number of differing bytes; passers are summed from 0, left to right (IndexPQ.cpp:242-247)
  ST_SDC     the query encoded with compute_codes; sdc_table[m][i + j * ksub] = sum_c (ci[c] - cj[c])^2 left to right; a code's
             distance is sum_m sdc[m][b[m] + q[m] * ksub], from 0, left to right (ProductQuantizer.cpp:595-660)
  rows       L2: the k smallest (dis, position), ascending, FLT_MAX / -1 padding (max-heap, dis < top); inner product: the k
             largest, earlier position first among equals, descending, -FLT_MAX / -1 padding (min-heap)
"""
import numpy as np

from ip_ref import F32, FLT_MAX, ip_sse
from ivfflat_ref import l2_sse

ST_PQ, ST_HE, ST_GENERALIZED_HE, ST_SDC, ST_POLYSEMOUS, ST_POLYSEMOUS_GENERALIZE = range(6)


def tables(xq, cent, metric):
    """[nq][M][ksub]; metric "l2" or "ip"."""
    M, ksub, dsub = cent.shape
    x = np.asarray(xq, F32).reshape(-1, M, 1, dsub)
    return (ip_sse if metric == "ip" else l2_sse)(x, cent[None])


def first_argmin_codes(tabs):
    """compute_code_from_distance_table: the first j whose entry is below everything before it, from 1e20; none: 255."""
    t = np.where(tabs < F32(1e20), tabs, np.inf)
    c = np.argmin(t, axis=-1)
    return np.where(np.isinf(t.min(axis=-1)), 255, c).astype(np.uint8)


def compute_codes(x, cent):
    return first_argmin_codes(tables(x, cent, "l2"))


def sdc_table(cent):
    """[M][ksub (j)][ksub (i)]: entry [m][j][i] is the reference's dis_tab[i + j * ksub]."""
    M, ksub, dsub = cent.shape
    acc = np.zeros((M, ksub, ksub), F32)
    for c in range(dsub):
        df = (cent[:, None, :, c] - cent[:, :, None, c]).astype(F32)      # [m][j][i] = ci - cj
        acc = (acc + (df * df).astype(F32)).astype(F32)
    return acc


def sdc_query_tables(qcodes, sdc):
    """[nq][M][ksub]: tab[q][m][b] = sdc[m][b + qcode[q][m] * ksub]"""
    M = sdc.shape[0]
    return np.stack([sdc[np.arange(M), qc.astype(np.int64)] for qc in qcodes])


def sums(tab, codes, order):
    """distance of every code for one query's table [M][ksub]; order "m4", "group4", "left"."""
    M = tab.shape[0]
    t = tab[np.arange(M)[None, :], codes.astype(np.int64)]       # [n][M]
    if order == "left":
        dis = np.zeros(codes.shape[0], F32)
        for m in range(M):
            dis = (dis + t[:, m]).astype(F32)
        return dis
    dis = np.zeros(codes.shape[0], F32)
    for g in range(0, M, 4):      # (a last group of fewer than four: only what the generator's "would differ" check asks for)
        dism = t[:, g]
        for m in range(g + 1, min(g + 4, M)):
            dism = (dism + t[:, m]).astype(F32)
        dis = dism if order == "m4" else (dis + dism).astype(F32)
    return dis


def order_of(M, search_type):
    if search_type != ST_PQ:
        return "left"
    return "m4" if M == 4 else "group4" if M % 4 == 0 else "left"


def hamming(codes, qcode, generalized):
    x = np.bitwise_xor(codes, qcode[None, :])
    if generalized:
        return (x != 0).sum(axis=1)
    return np.unpackbits(x, axis=1).sum(axis=1)


def topk(dis, pos, k, largest):
    """the k best (dis, position) of the candidates; padded"""
    D = np.full(k, -FLT_MAX if largest else FLT_MAX, F32)
    I = np.full(k, -1, np.int64)
    ok = (dis > -FLT_MAX) if largest else (dis < FLT_MAX)        # the heap admits nothing at its initial top
    dis, pos = dis[ok], pos[ok]
    o = np.lexsort((pos, -dis if largest else dis))[:k]
    D[:o.size] = dis[o]
    I[:o.size] = pos[o]
    return D, I


def search(cent, codes, xq, k, metric="l2", search_type=ST_PQ, ht=None, tabs=None, order=None):
    """(D, I, n_hamming_pass, tables, q_codes).  tabs: use these [nq][M][ksub] tables instead of computing them (the device's own
    tables for dsub >= 16).  order: override the summation order (the generator's discrimination checks)."""
    M, ksub, dsub = cent.shape
    nq = xq.shape[0]
    qcodes = None
    if search_type == ST_SDC:
        qcodes = compute_codes(xq, cent)
        if tabs is None:
            tabs = sdc_query_tables(qcodes, sdc_table(cent))
        largest = False
    else:
        ip = search_type == ST_PQ and metric == "ip"
        if tabs is None:
            tabs = tables(xq, cent, "ip" if ip else "l2")
        largest = ip
        if search_type in (ST_POLYSEMOUS, ST_POLYSEMOUS_GENERALIZE):
            qcodes = first_argmin_codes(tabs)
    order = order or order_of(M, search_type)
    D = np.empty((nq, k), F32)
    I = np.empty((nq, k), np.int64)
    n_pass = 0
    pos = np.arange(codes.shape[0], dtype=np.int64)
    for i in range(nq):
        if search_type in (ST_POLYSEMOUS, ST_POLYSEMOUS_GENERALIZE):
            keep = hamming(codes, qcodes[i], search_type == ST_POLYSEMOUS_GENERALIZE) < ht
            n_pass += int(keep.sum())
            D[i], I[i] = topk(sums(tabs[i], codes[keep], order), pos[keep], k, False)
        else:
            D[i], I[i] = topk(sums(tabs[i], codes, order), pos, k, largest)
    return D, I, n_pass, tabs, qcodes


def same_rows(D, I, Dr, Ir):
    """D bit-equal; I equal up to the order inside groups of exactly equal D, and free in the group across the k-th place
    (which of several equal heap tops a pop removes is the heap's business) unless that group is the padding."""
    if not np.array_equal(D.view(np.uint32), Dr.view(np.uint32)):
        return False
    k = D.shape[1]
    for r in range(D.shape[0]):
        for v in np.unique(D[r]):
            m = D[r] == v
            if v == D[r, k - 1] and abs(v) != FLT_MAX:
                continue
            if not np.array_equal(np.sort(I[r][m]), np.sort(Ir[r][m])):
                return False
    return True
