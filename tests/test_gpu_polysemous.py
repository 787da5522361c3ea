"""GPU: polysemous Hamming filtering in the IVFPQ list scan (vlq_ivfpq_set_polysemous_ht, csrc/scan_poly.hip) against the
reference's search_knn_with_key with polysemous_ht set (poly_nonresidual, poly_imi: the modes where the code of the query
is the reference's own) and against the numpy restatement tests/polysemous_ref.py, which tests/test_polysemous_restatement.py
holds to the reference (poly_table1, poly_table0_m20: the library's own definition of the code, include/vlq_ivfpq.h)."""
import numpy as np
import pytest

import vector_line_quantization_amd as vlq
from polysemous_ref import POLY_CASE_NAMES, POLY_DEFINED, case_filtered, first_argmin_codes, pairs_to_ids
from util import CASE_NAMES, Case, assert_same_topk, bits

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED = 1, 3


def make_index(case):
    g = vlq.GpuIVFPQ(case.d, case.nlist, case.M, case.nbits, device=0)
    if case.imi_nbits:
        g.set_imi_centroids(case.imi_nbits, case["imi_centroids"])
    else:
        g.set_coarse_centroids(case["coarse_centroids"])
    g.set_pq_centroids(case["pq_centroids"])
    g.set_search_options(bool(case.by_residual), 1 if case.mode in (1, 2) else 0, case.max_codes)
    g.set_lists(case["codes"], case["ids"], case["list_offsets"])
    return g


_expected = {}


def expected(case, t):
    """(D, ids, pairs, passes per query, ncode per query) at threshold t: the reference's where it defines the mode, the
    restatement's otherwise; computed once"""
    key = (case.name, t)
    if key not in _expected:
        if case.name in POLY_DEFINED:
            _expected[key] = (case["poly_D"][t], case["poly_I"][t], case["poly_pairs"][t], case["poly_npass"][t], case["poly_ncode"])
        else:
            D, P, npass, ncode = case_filtered(case, int(case["poly_hts"][t]))
            _expected[key] = (D, pairs_to_ids(case, P), P, npass, ncode)
    return _expected[key]


@pytest.fixture(scope="module", params=POLY_CASE_NAMES)
def setup(request):
    case = Case(request.param)
    g = make_index(case)
    yield case, g
    g.close()


def test_query_codes(setup):
    case, g = setup
    assert np.array_equal(g.query_codes(case.xq, case["keys"]), case["poly_qcodes"])
    keys = case["keys"].copy()
    keys[::3, 1] = -1
    qc = g.query_codes(case.xq, keys)
    assert not qc[::3, 1].any()
    keep = keys >= 0
    assert np.array_equal(qc[keep], case["poly_qcodes"][keep])
    if not case.by_residual:
        assert (qc[keep].reshape(-1, case.M) == np.repeat(qc[:, 0], keep.sum(axis=1), axis=0)).all()


def test_query_codes_first_index_wins_on_ties():
    case = Case("duplicates_ties")
    pq = case["pq_centroids"].copy()
    pq[:, 7] = pq[:, 3]                 # two equal centroids in every sub-quantizer: equal table entries
    pq[:, 200] = pq[:, 100]
    g = vlq.GpuIVFPQ(case.d, case.nlist, case.M, case.nbits, device=0)
    g.set_coarse_centroids(case["coarse_centroids"])
    g.set_pq_centroids(pq)
    g.set_lists(case["codes"], case["ids"], case["list_offsets"])
    # term 2 + (-2) * term 3 of the list's table, from the library's own introspection (fvec_madd, one multiply and one add)
    t2 = g.precomputed_table()
    ip = g.query_tables(case.xq, inner_product=True)
    keys = case["keys"]
    tab = t2[keys] + np.float32(-2) * ip[:, None]
    want = first_argmin_codes(tab)
    qc = g.query_codes(case.xq, keys)
    assert np.array_equal(qc, want)
    assert not np.isin(qc, (7, 200)).any() and np.isin(qc, (3, 100)).any()
    g.close()


def check_seam(case, g, t, rows, store_pairs, device):
    ht = int(case["poly_hts"][t])
    De, Ie, Pe, npass, ncode = expected(case, t)
    g.set_polysemous_ht(ht)
    g.stats(reset=True)
    g.polysemous_stats(reset=True)
    x, keys, cd = case.xq[rows], case["keys"][rows], case["coarse_dis"][rows]
    if device:
        import torch
        xt, kt, ct = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, keys, cd))
        D, I = g.search_preassigned(xt, kt, ct, case.k, store_pairs=store_pairs)
        g.stats()                      # synchronises the index's stream
        D, I = D.cpu().numpy(), I.cpu().numpy()
    else:
        D, I = g.search_preassigned(x, keys, cd, case.k, store_pairs=store_pairs)
    what = "%s ht=%d pairs=%d device=%d" % (case.name, ht, store_pairs, device)
    assert_same_topk(D, I, De[rows], (Pe if store_pairs else Ie)[rows], what)
    assert g.polysemous_stats() == int(npass[rows].sum()), what
    assert g.stats()[1] == int(ncode[rows].sum()), what
    if case.name not in POLY_DEFINED:      # every distance is one of the reference's unfiltered distances of that code
        if store_pairs:
            for r, i in enumerate(rows):
                ref = dict(zip(case["all_pairs"][i].tolist(), bits(case["all_D"][i]).tolist()))
                for p, d in zip(I[r], bits(D[r])):
                    assert p == -1 or ref[int(p)] == int(d), what


@pytest.mark.parametrize("t", range(4))
def test_seam(setup, t):
    case, g = setup
    full = list(range(case.nq))
    small = list(range(case.n_small))
    for store_pairs in (False, True):
        check_seam(case, g, t, full, store_pairs, False)
        check_seam(case, g, t, small, store_pairs, False)
    check_seam(case, g, t, full, True, True)
    check_seam(case, g, t, full, False, True)
    for i in (0, 1, case.nq - 1):
        check_seam(case, g, t, [i], True, False)
    g.set_polysemous_ht(0)


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if Case(n).M % 4 == 0])
def test_everything_passes(name):
    case = Case(name)
    g = make_index(case)
    for store_pairs in (False, True):
        g.stats(reset=True)
        D0, I0 = g.search_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k, store_pairs=store_pairs)
        ncode0 = g.stats(reset=True)[1]
        g.set_polysemous_ht(8 * case.M + 1)
        g.polysemous_stats(reset=True)
        D1, I1 = g.search_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k, store_pairs=store_pairs)
        assert "scan_poly" in g.last_scan_info()
        assert_same_topk(D1, I1, D0, I0, name)
        assert g.stats()[1] == ncode0 and g.polysemous_stats() == ncode0
        g.set_polysemous_ht(0)
    g.close()


def test_whole_search(setup):
    case, g = setup
    for t in (1, 2):
        g.set_polysemous_ht(int(case["poly_hts"][t]))
        D, I = g.search(case.xq, case.nprobe, case.k)
        cd, keys = g.coarse_search(case.xq, case.nprobe)
        D2, I2 = g.search_preassigned(case.xq, keys, cd, case.k)
        assert np.array_equal(bits(D), bits(D2)) and np.array_equal(I, I2)
    g.set_polysemous_ht(0)


def test_envelope():
    case = Case("poly_table1")
    g = make_index(case)
    args = (case.xq, case["keys"], case["coarse_dis"], case.k)
    D0, I0 = g.search_preassigned(*args)
    with pytest.raises(vlq.VlqError) as e:
        g.set_polysemous_ht(-1)
    assert e.value.code == ERR_INVALID
    g.set_polysemous_ht(40)
    g.set_scan_schedule(2)             # speed only: ignored in this mode
    D1, _ = g.search_preassigned(*args)
    assert not np.array_equal(bits(D0), bits(D1))
    g.set_scan_schedule(0)
    g.set_float16_tables(True)
    with pytest.raises(vlq.VlqError) as e:
        g.search_preassigned(*args)
    assert e.value.code == ERR_UNSUPPORTED
    g.set_float16_tables(False)
    wide = 1025                        # more than VLQ_MAX_NPROBE probes: the runs of 1024
    keys = np.full((2, wide), -1, np.int64)
    keys[:, :case.nprobe] = case["keys"][:2]
    with pytest.raises(vlq.VlqError) as e:
        g.search_preassigned(case.xq[:2], keys, np.zeros((2, wide), np.float32), case.k)
    assert e.value.code == ERR_UNSUPPORTED
    g.set_refine_pq(8, 8, np.zeros((8, 256, case.d // 8), np.float32))
    g.set_refine_codes(np.zeros((case["codes"].shape[0], 8), np.uint8))
    for call in (lambda: g.search_refined(case.xq, case.nprobe, 5, 2.0),
                 lambda: g.search_refined_preassigned(case.xq, case["keys"], case["coarse_dis"], 5, 2.0),
                 lambda: g.refine(case.xq, np.zeros((case.nq, 10), np.int64), 5)):
        with pytest.raises(vlq.VlqError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED
    g.set_polysemous_ht(0)             # back to the plain path: the results of before
    D2, I2 = g.search_preassigned(*args)
    assert np.array_equal(bits(D0), bits(D2)) and np.array_equal(I0, I2)
    g.close()
    odd = vlq.GpuIVFPQ(30, 4, 5, 8, device=0)      # M = 5: not a multiple of 4
    odd.set_coarse_centroids(np.zeros((4, 30), np.float32))
    odd.set_pq_centroids(np.zeros((5, 256, 6), np.float32))
    odd.set_polysemous_ht(3)
    with pytest.raises(vlq.VlqError) as e:
        odd.search(np.zeros((1, 30), np.float32), 2, 3)
    assert e.value.code == ERR_UNSUPPORTED
    odd.close()


def test_monotone():
    case = Case("poly_table1")
    g = make_index(case)
    args = (case.xq, case["keys"], case["coarse_dis"], case.k)
    last = -1
    for ht in (1, 20, 45, 53, 58, 62, 70, 90, 129):
        g.set_polysemous_ht(ht)
        g.polysemous_stats(reset=True)
        D, P = g.search_preassigned(*args, store_pairs=True)
        n = g.polysemous_stats()
        assert n >= last
        last = n
        # the row is the unfiltered row (every scanned code, by (distance, scan position)) restricted to the passers
        De, Pe, _n, _c = case_filtered(case, ht)
        assert_same_topk(D, P, De, Pe, "ht=%d" % ht)
    g.close()
