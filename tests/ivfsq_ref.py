"""Numpy restatement of IndexIVFScalarQuantizer's encode and search, as include/vlq_ivfpq.h (vlq_ivfsq_*) specifies it.

TEST INFRASTRUCTURE ONLY.  Every fp32 operation is one numpy float32 operation in the reference's order
(IndexScalarQuantizer.cpp):

  decode    f = float(c) + 0.5f;  xi = f * (1.f / den) when d % 8 == 0 (the AVX codec, :67-80, :96-115), f / den otherwise
            (:63-65, :91-93); den = 255 / 15;  rec = vmin_i + xi * vdiff_i
  L2        y = x - centroid (per probe), t_i = (y_i - rec_i)^2;  inner product: y = x, t_i = y_i * rec_i
  order8    (d % 8 == 0) eight accumulators over i mod 8; L2 ((a0+a1)+(a2+a3)) + ((a4+a5)+(a6+a7)); inner product
            (accu0 + ((a0+a1)+(a2+a3))) + ((a4+a5)+(a6+a7)), accu0 the probe's coarse inner product
  scalar    one accumulator over ascending i, from 0 (L2) or accu0 (inner product)
  walk      a key < 0 ENDS the walk (:897, :934); a key >= nlist in front of it is an error
  rows      L2: the k smallest (dis, scan position), ascending, FLT_MAX / -1 padding; inner product: the k largest, earlier scan
            position first among equals, descending, -FLT_MAX / -1 padding
  encode    xi = (r_i - vmin_i) / vdiff_i clamped to [0, 1]; 8 bits (int)(255 * xi) in float, 4 bits (int)(xi * 15.0) in double;
            component i of a 4-bit code is the low nibble of byte i / 2 for even i, the high one for odd i
  train     RS_minmax, rangestat_arg 0: per-dimension (uniform types: overall) min and max - min of the residuals
"""
import numpy as np

from ip_ref import FLT_MAX, F32  # noqa: F401

QTYPES = {"8bit": 0, "4bit": 1, "8bit_uniform": 2, "4bit_uniform": 3}


def bits_of(qtype):
    return 8 if qtype in (0, 2) else 4


def is_uniform(qtype):
    return qtype >= 2


def code_size(d, qtype):
    return d if bits_of(qtype) == 8 else (d + 1) // 2


def ranges(trained, d, qtype):
    """(vmin [d], vdiff [d]) of ScalarQuantizer::trained"""
    t = np.asarray(trained, dtype=F32).ravel()
    if is_uniform(qtype):
        assert t.size == 2
        return np.full(d, t[0], F32), np.full(d, t[1], F32)
    assert t.size == 2 * d
    return t[:d].copy(), t[d:].copy()


def components(codes, d, qtype):
    """the integer code of every component: [n][d] uint8"""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, code_size(d, qtype))
    if bits_of(qtype) == 8:
        return codes[:, :d]
    out = np.empty((codes.shape[0], 2 * codes.shape[1]), np.uint8)
    out[:, 0::2] = codes & 0xF
    out[:, 1::2] = codes >> 4
    return out[:, :d]


def decode(codes, d, qtype, trained, order8=None):
    """rec [n][d]: decode_vector in the operation order the distance code uses for this d (order8 None: d % 8 == 0)"""
    if order8 is None:
        order8 = d % 8 == 0
    vmin, vdiff = ranges(trained, d, qtype)
    den = F32(255.0 if bits_of(qtype) == 8 else 15.0)
    f = (components(codes, d, qtype).astype(F32) + F32(0.5)).astype(F32)
    xi = (f * (F32(1.0) / den).astype(F32)).astype(F32) if order8 else (f / den).astype(F32)
    return (vmin[None, :] + (xi * vdiff[None, :]).astype(F32)).astype(F32)


def decode_scalar(codes, d, qtype, trained):
    """ScalarQuantizer::decode (decode_vector, :457-462, :531-536): always the scalar codec"""
    return decode(codes, d, qtype, trained, order8=False)


def encode(res, qtype, trained):
    """encode_vector of residuals res [n][d]: codes [n][code_size]"""
    res = np.asarray(res, dtype=F32)
    n, d = res.shape
    vmin, vdiff = ranges(trained, d, qtype)
    xi = ((res - vmin[None, :]).astype(F32) / vdiff[None, :]).astype(F32)
    xi = np.where(xi < 0, F32(0), xi)
    xi = np.where(xi > 1, F32(1), xi).astype(F32)
    if bits_of(qtype) == 8:
        return (F32(255.0) * xi).astype(F32).astype(np.int32).astype(np.uint8)
    c = (xi.astype(np.float64) * 15.0).astype(np.int32).astype(np.uint8)
    if d % 2:
        c = np.concatenate([c, np.zeros((n, 1), np.uint8)], axis=1)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def train(res, qtype):
    """sq.train with RS_minmax, rangestat_arg 0 over residuals res [n][d]: ScalarQuantizer::trained"""
    res = np.asarray(res, dtype=F32)
    if is_uniform(qtype):
        vmin, vmax = res.min(), res.max()
        return np.array([vmin, F32(vmax - vmin)], F32)
    vmin, vmax = res.min(axis=0), res.max(axis=0)
    return np.concatenate([vmin, (vmax - vmin).astype(F32)]).astype(F32)


def distances(y, rec, ip, order8, accu0=F32(0)):
    """distance of the (shifted) query y [d] to every decoded row rec [n][d]"""
    y = np.asarray(y, dtype=F32)
    n, d = rec.shape

    def term(i):
        if ip:
            return (y[i] * rec[:, i]).astype(F32)
        t = (y[i] - rec[:, i]).astype(F32)
        return (t * t).astype(F32)

    if order8:
        a = [np.zeros(n, F32) for _ in range(8)]
        for i in range(d):
            a[i % 8] = (a[i % 8] + term(i)).astype(F32)
        lo = ((a[0] + a[1]).astype(F32) + (a[2] + a[3]).astype(F32)).astype(F32)
        hi = ((a[4] + a[5]).astype(F32) + (a[6] + a[7]).astype(F32)).astype(F32)
        if ip:
            return ((F32(accu0) + lo).astype(F32) + hi).astype(F32)
        return (lo + hi).astype(F32)
    acc = np.full(n, F32(accu0) if ip else F32(0), F32)
    for i in range(d):
        acc = (acc + term(i)).astype(F32)
    return acc


def scan_query(q, keys, cdis, z, k, metric, qtype, order8=None):
    """search_with_probes_L2 / search_with_probes_ip of one query: (D [k], I [k]).  order8 None: what the reference takes
    for this d; given: that order whatever d is (8 | d is needed for True) -- the wrong order, for the fixtures' checks."""
    list_offsets, cent = z["list_offsets"], z["coarse_centroids"]
    nlist, d = list_offsets.shape[0] - 1, cent.shape[1]
    ip = metric == "ip"
    if order8 is None:
        order8 = d % 8 == 0
    dis_all, lab_all = [], []
    for p, key in enumerate(keys):
        key = int(key)
        if key < 0:
            break
        if key >= nlist:
            raise ValueError("key %d >= nlist %d" % (key, nlist))
        o0, o1 = int(list_offsets[key]), int(list_offsets[key + 1])
        if o1 > o0:
            rec = decode(z["codes"][o0:o1], d, qtype, z["trained"], order8)
            y = np.asarray(q, F32) if ip else (np.asarray(q, F32) - cent[key]).astype(F32)
            dis_all.append(distances(y, rec, ip, order8, cdis[p] if ip else 0))
            lab_all.append(z["ids"][o0:o1])
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
    return D, I


def search_preassigned(z, xq, keys, cdis, k, metric, qtype, order8=None):
    """Rows of a whole batch from a fixture's arrays z (coarse_centroids, trained, codes, ids, list_offsets): (D, I)"""
    nq = xq.shape[0]
    D = np.empty((nq, k), F32)
    I = np.empty((nq, k), np.int64)
    for i in range(nq):
        D[i], I[i] = scan_query(xq[i], keys[i], None if cdis is None else cdis[i], z, k, metric, qtype, order8)
    return D, I


def other_order_differs(z, xq, keys, cdis, k, metric, qtype, Dref):
    """True if the OTHER operation order (the scalar one where d % 8 == 0 and the other way round; for d % 8 != 0 the eight
    accumulators with the multiply by 1 / den) differs in bits from Dref in at least one slot."""
    d = xq.shape[1]
    Do, _I = search_preassigned(z, xq, keys, cdis, k, metric, qtype, order8=(d % 8 != 0))
    return not np.array_equal(Do.view(np.uint32), Dref.view(np.uint32))


def tied_rows(D, I):
    """rows with two equal distances among their results"""
    out = np.zeros(D.shape[0], bool)
    for r in range(D.shape[0]):
        v = D[r][I[r] != -1]
        out[r] = np.unique(v).size != v.size
    return out


def tie_across_kth(z, xq, keys, cdis, k, metric, qtype):
    """rows where a group of equal distances crosses the k-th place: the (k+1)-th best equals the k-th"""
    Dk1, Ik1 = search_preassigned(z, xq, keys, cdis, k + 1, metric, qtype)
    return (Dk1[:, k] == Dk1[:, k - 1]) & (Ik1[:, k] != -1)


def same_pairs(D, I, Dr, Ir, rows):
    """(distance, label) multisets equal on the given rows"""
    for r in np.nonzero(rows)[0]:
        a = sorted(zip(D[r].view(np.uint32).tolist(), I[r].tolist()))
        b = sorted(zip(Dr[r].view(np.uint32).tolist(), Ir[r].tolist()))
        if a != b:
            return False
    return True
