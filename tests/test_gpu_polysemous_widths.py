"""GPU: every code width of the polysemous scan (csrc/scan_poly.hip: scan_poly_kernel<W, KPL>, W = M / 4 = 1 .. 16) against
the restatement tests/polysemous_ref.py fed from the oracle alone (oracle_scan: tests/test_newscan_helpers.py holds that
to the poly_* fixtures).  Random codes over the shared small index (tests/newscan_index.py); every table mode, the
multi-index table type 2, 5- and 6-bit codes, a max_codes cut; thresholds from the restatement's own Hamming distances.  At
the median threshold the long list leaves one wave more passers than its ring of 128 slots holds: the ring wraps.
D as bits, I exactly equal, ids and pair labels."""
import numpy as np
import pytest

import newscan_index as nx
import vector_line_quantization_amd as vlq
from oracle import pyoracle
from polysemous_ref import FLT_MAX, labels_to_ids, oracle_filtered, oracle_scan
from util import bits

pytestmark = pytest.mark.gpu
DSUBS = (1, 2, 3, 4, 5, 6, 8)
KS = (10, 100, 300)                           # KPL 1, 4, 16
IMI = {16: 3, 28: 3, 40: 3, 52: 3}            # M: imi_nbits (widths whose table mode is 1: table type 2)
NBITS = {12: 5, 20: 6, 48: 5, 64: 6}          # table modes 0, 2, 0, 1
MAX_CODES = {8: 400, 28: 400, 36: 400, 56: 400}
RING = 128                                    # kPolyRing: slots of a wave's passer ring


def config(M):
    W = M // 4
    return dict(mode=W % 3, dsub=DSUBS[W % len(DSUBS)], nbits=NBITS.get(M, 8), imi_nbits=IMI.get(M, 0), max_codes=MAX_CODES.get(M, 0))


def build(M):
    c = config(M)
    imi_nbits = c["imi_nbits"]
    lay = nx.layout(nlist=(1 << (2 * imi_nbits)) if imi_nbits else 12)
    p = nx.pq_parts(lay, M, c["dsub"], c["nbits"])
    by_residual, upt = c["mode"] != 2, 1 if c["mode"] == 1 else 0
    g = vlq.GpuIVFPQ(p["d"], lay["nlist"], M, c["nbits"], device=0)
    imi = None
    if imi_nbits:
        assert c["mode"] == 1
        imi = np.random.default_rng(M).standard_normal((2, 1 << imi_nbits, p["d"] // 2)).astype(np.float32)
        g.set_imi_centroids(imi_nbits, imi)
    else:
        g.set_coarse_centroids(p["coarse"])
    g.set_pq_centroids(p["pq"])
    g.set_search_options(by_residual, upt, c["max_codes"])
    g.set_lists(p["codes"], lay["ids"], lay["list_offsets"])
    ox = pyoracle.OracleIndex(p["d"], lay["nlist"], M, c["nbits"], None if imi_nbits else p["coarse"], p["pq"], imi_centroids=imi,
                              imi_nbits=imi_nbits, codes=p["codes"], ids=lay["ids"], list_offsets=lay["list_offsets"],
                              by_residual=by_residual, use_precomputed_table=upt, max_codes=c["max_codes"])
    return c, lay, p, g, ox


def test_configurations_cover_what_they_claim():
    cfgs = {M: config(M) for M in range(4, 65, 4)}
    assert {c["mode"] for c in cfgs.values()} == {0, 1, 2}
    assert all(cfgs[M]["mode"] == 1 for M in IMI) and len(IMI) == 4 and len(NBITS) == 4
    assert {cfgs[M]["mode"] for M in NBITS} == {0, 1, 2}
    assert {cfgs[M]["mode"] for M in MAX_CODES} == {0, 1, 2}
    for kind in (lambda W: W % 4 == 0, lambda W: W % 4 == 2, lambda W: W % 2 == 1):         # uint4, uint2, dword loads
        assert {cfgs[M]["mode"] for M in cfgs if kind(M // 4)} == {0, 1, 2}


@pytest.mark.parametrize("M", range(4, 65, 4))
def test_width(M):
    c, lay, p, g, ox = build(M)
    nx.check_layout(lay)
    xq, keys, cdis = p["xq"], lay["keys"], p["coarse_dis"]
    scan = oracle_scan(ox, xq, keys, cdis)
    assert np.array_equal(g.query_codes(xq, keys), scan["qcodes"]), c
    full = np.array([lay["lens"][kq[kq >= 0]].sum() for kq in keys])
    if c["max_codes"]:
        assert (scan["ncode"] < full).any(), "the max_codes cut does not fall inside a walk"
    else:
        assert np.array_equal(scan["ncode"], full)

    hd_cat = np.sort(np.concatenate(scan["hd"]))
    t10 = int(hd_cat[int(0.10 * hd_cat.size)]) + 1             # hd < t: about 10 % / half of the scanned codes
    t50 = int(hd_cat[hd_cat.size // 2]) + 1
    hts = [1, t10, t50, 8 * M + 1]
    assert 1 < t10 < t50 < 8 * M + 1
    share = float((hd_cat < t50).mean())
    assert 0.3 <= share <= 0.7, share
    # the ring wraps: at the median threshold some query finds more than 4 x 128 passers in the long list, and one of its
    # waves (wave w takes offsets 64 w .. 64 w + 63 of every 256) more than its 128 slots
    long_list = int(np.argmax(lay["lens"]))
    assert lay["lens"][long_list] >= nx.LONG
    most, most_wave = 0, 0
    for pairs, hd in zip(scan["pairs"], scan["hd"]):
        sel = ((pairs >> 32) == long_list) & (hd < t50)
        most = max(most, int(sel.sum()))
        if sel.any():
            most_wave = max(most_wave, int(np.bincount(((pairs[sel] & 0xFFFFFFFF) % 256) // 64, minlength=4).max()))
    assert most > 4 * RING and most_wave > RING, (most, most_wave)

    kmax = max(KS)
    for ht in hts:
        De, Pe, npass, ncode = oracle_filtered(scan, ht, kmax)           # once: a smaller k is its head
        Ie = labels_to_ids(lay["list_offsets"], lay["ids"], Pe)
        g.set_polysemous_ht(ht)
        if ht == t10:
            assert (npass < kmax).any() and (npass > 0).any(), "no partly padded row"
        if ht == 8 * M + 1:
            assert np.array_equal(npass, ncode)
        for k in KS:
            for store_pairs in (False, True):
                g.stats(reset=True)
                g.polysemous_stats(reset=True)
                D, I = g.search_preassigned(xq, keys, cdis, k, store_pairs=store_pairs)
                what = "M=%d ht=%d k=%d pairs=%d %s" % (M, ht, k, store_pairs, c)
                assert np.array_equal(bits(D), bits(De[:, :k])), what
                assert np.array_equal(I, (Pe if store_pairs else Ie)[:, :k]), what
                assert (bits(D)[I == -1] == FLT_MAX.view(np.uint32)).all(), what
                assert g.polysemous_stats() == int(npass.sum()), what
                assert g.stats() == (xq.shape[0], int(ncode.sum())), what
                assert "kernel=scan_poly_kernel<%d>" % (M // 4) in g.last_scan_info(), what
    g.close()
