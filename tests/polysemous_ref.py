"""numpy restatement of the polysemous filter of IndexIVFPQ::search_knn_with_key (IndexIVFPQ.cpp:887-947, :1002-1034): of the
codes a query scans, those whose Hamming distance to the query's code is below the threshold, and of those the first k by
(distance, scan position).  tests/test_polysemous_restatement.py holds it to the reference's own output on the fixtures
whose mode the reference defines; the GPU tests of the other two modes lean on it."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
POLY_CASE_NAMES = ["poly_nonresidual", "poly_imi", "poly_table1", "poly_table0_m20"]
POLY_DEFINED = ["poly_nonresidual", "poly_imi"]          # q_code is the reference's own there
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(codes, qcode):
    """popcount(qcode XOR code) over the whole code, for every row of codes [n][M]"""
    return POPCOUNT[np.bitwise_xor(codes, qcode[None, :])].sum(axis=1)


def visited(keys_row, list_offsets, max_codes=0):
    """(probe, key, length) of the lists a query scans, in order: keys < 0 and empty lists skipped, stop after the list that
    reaches max_codes (IndexIVFPQ.cpp:1004-1033).  Second value: the query's ncode."""
    out, nscan = [], 0
    for p, key in enumerate(keys_row):
        key = int(key)
        if key < 0:
            continue
        n = int(list_offsets[key + 1] - list_offsets[key])
        nscan += n
        if n:
            out.append((p, key, n))
        if max_codes and nscan >= max_codes:
            break
    return out, nscan


def scan_hamming(keys_row, qcodes_row, codes, list_offsets, max_codes=0):
    """pair label (list << 32 | offset) and Hamming distance of every code the query scans, in scan order; ncode"""
    vis, nscan = visited(keys_row, list_offsets, max_codes)
    pairs, hd = [], []
    for p, key, n in vis:
        o = int(list_offsets[key])
        pairs.append((np.int64(key) << 32) | np.arange(n, dtype=np.int64))
        hd.append(hamming(codes[o:o + n], qcodes_row[p]))
    if not pairs:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), nscan
    return np.concatenate(pairs), np.concatenate(hd), nscan


def filtered_topk(all_D_row, all_pairs_row, pairs, hd, ht, k):
    """all_D_row / all_pairs_row: distance and pair label of EVERY scanned code (any order, -1 padding); pairs / hd: the scan
    order and its Hamming distances.  Returns (D[k], pair labels[k], codes that passed)."""
    dist = dict(zip(all_pairs_row[all_pairs_row >= 0].tolist(), all_D_row[all_pairs_row >= 0].tolist()))
    assert len(dist) == pairs.size, "all_D does not hold every scanned code"
    keep = np.nonzero(hd < ht)[0]
    d = np.array([dist[int(pairs[i])] for i in keep], np.float32)
    order = np.lexsort((keep, d))[:k]                    # (distance, scan position)
    D = np.full(k, FLT_MAX, np.float32)
    P = np.full(k, -1, np.int64)
    D[:order.size] = d[order]
    P[:order.size] = pairs[keep[order]]
    return D, P, int(keep.size)


def case_filtered(case, ht, rows=None):
    """the restatement over a poly_* fixture: D, pair labels [n][k], passes per query [n], ncode per query [n]"""
    rows = range(case.nq) if rows is None else rows
    D, P, npass, ncode = [], [], [], []
    for i in rows:
        pairs, hd, ns = scan_hamming(case["keys"][i], case["poly_qcodes"][i], case["codes"], case["list_offsets"], case.max_codes)
        d, p, n = filtered_topk(case["all_D"][i], case["all_pairs"][i], pairs, hd, ht, case.k)
        D.append(d); P.append(p); npass.append(n); ncode.append(ns)
    return np.array(D), np.array(P), np.array(npass, np.int64), np.array(ncode, np.int64)


def pairs_to_ids(case, P):
    """stored ids of pair labels (-1 stays)"""
    off, ids = case["list_offsets"], case["ids"]
    out = np.full(P.shape, -1, np.int64)
    ok = P >= 0
    out[ok] = ids[off[P[ok] >> 32] + (P[ok] & 0xFFFFFFFF)]
    return out


def first_argmin_codes(tables):
    """q_code of tables [..., M, ksub]: the first minimum of every sub-quantizer's row"""
    return np.argmin(tables, axis=-1).astype(np.uint8)


def oracle_qcodes(ox, xq, keys):
    """q_code [nq][nprobe][M] of every (query, probe) from the oracle's tables alone: the first argmin of the table the
    mode defines (csrc/scan_poly.hip, include/vlq_ivfpq.h).  Rows of keys outside 0 .. nlist-1 stay 0."""
    nq, nprobe = keys.shape
    out = np.zeros((nq, nprobe, ox.M), np.uint8)
    F32 = np.float32
    pt = ox.precomputed_table if ox.by_residual and ox.use_precomputed_table in (1, 2) else None
    for i in range(nq):
        live = [p for p in range(nprobe) if 0 <= keys[i, p] < ox.nlist]
        if not live:
            continue
        if not ox.by_residual:
            out[i, live] = first_argmin_codes(ox.distance_table(xq[i]))          # one code per query
            continue
        if pt is not None:
            m2ip = (F32(-2) * ox.inner_prod_table(xq[i])).astype(F32)            # fvec_madd: one multiply, one add
        for p in live:
            key = int(keys[i, p])
            if pt is None:                                                       # table type 0: the float32 residual's table
                tab = ox.distance_table((xq[i] - ox.coarse_centroids[key]).astype(F32))
            elif ox.imi_nbits:                                                   # table type 2: a row per half
                k0, k1 = key & ((1 << ox.imi_nbits) - 1), key >> ox.imi_nbits
                half = ox.M // 2
                tab = np.concatenate([pt[k0][:half], pt[k1][half:]])
                tab = (tab + m2ip).astype(F32)
            else:
                tab = (pt[key] + m2ip).astype(F32)
            out[i, p] = first_argmin_codes(tab)
    return out


def oracle_scan(ox, xq, keys, coarse_dis):
    """everything the filtered rows of a batch are made of, from the oracle alone: dict with qcodes, all_D / all_pairs (the
    unfiltered distance and pair label of every scanned code: search_preassigned at k = the largest ncode, store_pairs), and
    per query the scan order's pair labels, Hamming distances and ncode"""
    qcodes = oracle_qcodes(ox, xq, keys)
    scans = [scan_hamming(keys[i], qcodes[i], ox.codes, ox.list_offsets, ox.max_codes) for i in range(keys.shape[0])]
    k_all = max(1, max(s[2] for s in scans))
    all_D, all_pairs = ox.search_preassigned(xq, keys, coarse_dis, k_all, store_pairs=True)
    return dict(qcodes=qcodes, all_D=all_D, all_pairs=all_pairs, pairs=[s[0] for s in scans], hd=[s[1] for s in scans],
                ncode=np.array([s[2] for s in scans], np.int64))


def oracle_filtered(scan, ht, k, rows=None):
    """the restatement's rows over an oracle_scan: D, pair labels [n][k], passes per query [n], ncode per query [n]"""
    rows = range(len(scan["pairs"])) if rows is None else rows
    D, P, npass = [], [], []
    for i in rows:
        d, p, n = filtered_topk(scan["all_D"][i], scan["all_pairs"][i], scan["pairs"][i], scan["hd"][i], ht, k)
        D.append(d); P.append(p); npass.append(n)
    return np.array(D), np.array(P), np.array(npass, np.int64), scan["ncode"][list(rows)]


def labels_to_ids(list_offsets, ids, P):
    """stored ids of pair labels (-1 stays)"""
    out = np.full(P.shape, -1, np.int64)
    ok = P >= 0
    out[ok] = ids[list_offsets[P[ok] >> 32] + (P[ok] & 0xFFFFFFFF)]
    return out
