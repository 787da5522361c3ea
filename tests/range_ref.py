"""Numpy restatement of IndexIVFFlat::range_search (IndexIVF.cpp:401-449), as include/vlq_ivfpq.h (vlq_ivfflat_range_*)
specifies it.

TEST INFRASTRUCTURE ONLY.  Distances are ivfflat_ref's l2_sse / ip_sse (one numpy float32 operation per fp32 operation of
the reference's SSE kernels).  Per query the probes are taken in the order given and the rows of a list in stored order; a
row is a hit if dis < radius (L2) or ip > radius (inner product), both strict, so a NaN on either side is no hit.  A key < 0
or >= nlist is an error (the reference aborts).  lims are the exclusive prefix sums of the hits per query.
"""
import os

import numpy as np

from ivfflat_ref import F32, ip_plain, ip_sse, l2_plain, l2_sse

HERE = os.path.dirname(os.path.abspath(__file__))
SRC_DIR = os.path.join(HERE, "golden", "ivfflat")
RANGE_DIR = os.path.join(HERE, "golden", "ivfflat_range")

# the cases of tests/golden/make_golden_range.py: fixture name -> (source fixture, prefix of its arrays, metric)
CASES = {
    "flat_l2_d32": ("flat_l2_d32", "", "l2"),
    "flat_ip_d32": ("flat_ip_d32", "", "ip"),
    "flat_l2_d128_long": ("flat_l2_d128_long", "", "l2"),
    "flat_tail_d30_l2": ("flat_tail_d30_l2", "", "l2"),
    "flat_tail_d30_ip": ("flat_tail_d30_ip", "", "ip"),
    "flat_tail_d5_l2": ("flat_tail_d5_l2", "", "l2"),
    "flat_tail_d3_ip": ("flat_tail_d3_ip", "", "ip"),
    "flat_ragged_d36_l2": ("flat_ragged_d36_l2", "", "l2"),
    "flat_ragged_d100_ip": ("flat_ragged_d100_ip", "", "ip"),
    "flat_padding_ties_l2": ("flat_padding_ties_l2", "", "l2"),
    "flat_coarse_int_l2": ("flat_coarse_int", "l2_", "l2"),
    "flat_coarse_int_ip": ("flat_coarse_int", "ip_", "ip"),
}
WIDE_CASES = ("flat_l2_d128_long", "flat_ragged_d36_l2", "flat_ragged_d100_ip")      # these also carry `wide` and `all`


def scan_query(q, keys, vecs, ids, list_offsets, radius, metric, dist=None):
    """(D, I, probe index of each hit, list position of each hit) of one query, in scan order"""
    nlist = list_offsets.shape[0] - 1
    ip = metric == "ip"
    if dist is None:
        dist = ip_sse if ip else l2_sse
    radius = F32(radius)
    D, I, P, J = [], [], [], []
    for ik, key in enumerate(keys):
        key = int(key)
        if key < 0 or key >= nlist:
            raise ValueError("Invalid key=%d at ik=%d nlist=%d" % (key, ik, nlist))
        o0, o1 = int(list_offsets[key]), int(list_offsets[key + 1])
        if o1 == o0:
            continue
        dis = dist(q, vecs[o0:o1])
        with np.errstate(invalid="ignore"):
            hit = np.nonzero(dis > radius if ip else dis < radius)[0]
        D.append(dis[hit])
        I.append(ids[o0:o1][hit])
        P.append(np.full(hit.size, ik, np.int64))
        J.append(hit.astype(np.int64))
    if not D:
        return np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(D).astype(F32), np.concatenate(I).astype(np.int64), np.concatenate(P), np.concatenate(J)


def range_search_preassigned(z, xq, keys, radius, metric, dist=None, where=False, prefix=""):
    """(lims [nq + 1], D [total], I [total]) of a batch from a fixture's arrays z; where=True: also the probe index and the
    list position of every hit"""
    nq = xq.shape[0]
    parts = [scan_query(xq[i], keys[i], z[prefix + "vecs"], z[prefix + "ids"], z[prefix + "list_offsets"], radius, metric, dist)
             for i in range(nq)]
    lims = np.zeros(nq + 1, np.int64)
    lims[1:] = np.cumsum([p[0].size for p in parts])
    cat = [np.concatenate([p[c] for p in parts]) if parts else np.zeros(0) for c in range(4)]
    out = (lims, cat[0].astype(F32), cat[1].astype(np.int64))
    return out + (cat[2].astype(np.int64), cat[3].astype(np.int64)) if where else out


def one_radius_can(z, xq, keys, metric, prefix=""):
    """Whether ANY radius leaves one query without a hit while another query has hits from two different probes: the first
    needs radius <= every query's best distance, the second radius > some query's best distance in its second-best probe
    (inner products: the same on the negated values)."""
    everything = F32(-np.inf if metric == "ip" else np.inf)
    lims, D, _I, P, _J = range_search_preassigned(z, xq, keys, everything, metric, where=True, prefix=prefix)
    val = -D if metric == "ip" else D
    best, second = [], []
    for q in range(xq.shape[0]):
        v, p = val[lims[q]:lims[q + 1]], P[lims[q]:lims[q + 1]]
        per_probe = sorted(v[p == ik].min() for ik in np.unique(p))
        best.append(per_probe[0] if per_probe else np.inf)
        second.append(per_probe[1] if len(per_probe) > 1 else np.inf)
    return bool(min(second) < max(best))


def hits_from_two_probes(z, xq, keys, radius, metric, prefix=""):
    lims, _D, _I, P, _J = range_search_preassigned(z, xq, keys, radius, metric, where=True, prefix=prefix)
    return any(np.unique(P[lims[q]:lims[q + 1]]).size >= 2 for q in range(xq.shape[0]))


def plain(metric):
    return ip_plain if metric == "ip" else l2_plain


def load_case(name):
    """(source fixture, range fixture, prefix, metric, keys): the keys are the source's, or the range fixture's own where the
    source's hold -1 (flat_padding_ties: the recorded quantizer->assign keys)"""
    src, prefix, metric = CASES[name]
    z = np.load(os.path.join(SRC_DIR, src + ".npz"))
    r = np.load(os.path.join(RANGE_DIR, name + ".npz"))
    assert str(r["src"]) == src
    keys = r["keys"] if "keys" in r.files else z[prefix + "keys"]
    return z, r, prefix, metric, keys


def radius_names(r):
    return [str(s) for s in r["radius_names"]]
