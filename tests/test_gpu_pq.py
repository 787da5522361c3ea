"""GPU: the flat PQ index (vlq.GpuPQ, csrc/scan_pq.hip) against fixtures made from the reference's own faiss::IndexPQ
(tests/golden/make_golden_pq.py).  Fixtures only: no reference tree, no oracle."""
import numpy as np
import pytest

import pq_ref as pr
import vector_line_quantization_amd as vlq
from test_pq_ref import CASES, METRIC, blas_bound, load, runs
from util import assert_same_topk, bits

pytestmark = pytest.mark.gpu
FLT_MAX = np.float32(np.finfo(np.float32).max)
PAD_BITS = {"l2": FLT_MAX.view(np.uint32), "ip": np.float32(-FLT_MAX).view(np.uint32)}


def make_index(z, codes=True):
    g = vlq.GpuPQ(int(z["d"]), int(z["M"]), int(z["nbits"]), metric=METRIC[int(z["metric"])], device=0)
    g.set_centroids(z["centroids"])
    if codes:
        g.set_codes(z["codes"])
    g.search_type = int(z["search_type"])
    return g


@pytest.fixture(scope="module", params=CASES)
def setup(request):
    z = load(request.param)
    g = make_index(z)
    yield request.param, z, g
    g.close()


def reference_rows(name, z, g, ht, D, I):
    """the rows a search must give: the fixture's; for the BLAS fixture the restatement over the device's own tables"""
    if not name.startswith("pq_blas"):
        return D, I
    tabs = g.query_tables(z["xq"])
    return pr.search(z["centroids"], z["codes"], z["xq"], int(z["k"]), METRIC[int(z["metric"])], int(z["search_type"]), ht, tabs=tabs)[:2]


def test_search(setup):
    """D as bits, labels exact (free only inside a tie group across the k-th place, which only pq_ties has), the padding per
    metric, IndexPQStats, what the scan read"""
    name, z, g = setup
    k, metric, st = int(z["k"]), METRIC[int(z["metric"])], int(z["search_type"])
    assert g.ntotal == z["codes"].shape[0]
    for ht, Dr, Ir, stats in runs(z):
        if ht is not None:
            g.polysemous_ht = ht
        g.stats(reset=True)
        D, I = g.search(z["xq"], k)
        got = g.stats(reset=True)
        Dr, Ir = reference_rows(name, z, g, ht, Dr, Ir)
        g.stats(reset=True)
        loose = assert_same_topk(D, I, Dr, Ir, "%s ht %s" % (name, ht))
        assert loose == 0 or name == "pq_ties"
        if name == "pq_ties":
            assert loose < D.shape[0] * 2 // 3 + 1
        assert (bits(D)[I == -1] == PAD_BITS["l2" if st != pr.ST_PQ else metric]).all()
        assert list(got) == [int(v) for v in stats], (name, ht)
    info = g.last_scan_info()
    kpl = 1 if k <= 64 else 4 if k <= 256 else 16
    order = pr.order_of(int(z["M"]), st).replace("m4", "M4")
    assert "kernel=scan_pq_kernel<" in info and ", %d, %s, " % (kpl, order) in info


def test_what_the_scan_reads(setup):
    name, z, g = setup
    st, nt = int(z["search_type"]), 4
    tabs = g.query_tables(z["xq"][:nt])
    if name.startswith("pq_blas"):
        # the reference's tables are BLAS's: entry by entry to the rounding bound of both evaluation orders
        assert (np.abs(tabs.astype(np.float64) - z["tables"][:nt]) <= blas_bound(z)[:nt]).all()
        return
    if st == pr.ST_SDC:
        want = pr.sdc_query_tables(z["q_codes"][:nt], pr.sdc_table(z["centroids"]))
    else:
        want = z["tables"][:nt]
    assert np.array_equal(bits(tabs), bits(want))
    if st != pr.ST_PQ:
        assert np.array_equal(g.query_codes(z["xq"]), z["q_codes"])
    else:
        with pytest.raises(vlq.VlqError):
            g.query_codes(z["xq"])


@pytest.mark.parametrize("name", ["pq_m16_d64_l2", "pq_m16_d64_ip", "pq_m6_d30", "pq_ties", "pq_poly_m16", "pq_polygen_m16", "pq_sdc_m8", "pq_kwide"])
def test_rows_do_not_depend_on_the_split(name):
    """Q in {1, 2, 4} x S in {1, 2, 7}: rows identical to the (1, 1) run, labels included; slice ends fall off multiples of 64"""
    z = load(name)
    g = make_index(z)
    k = int(z["k"])
    if "hts" in z:
        g.polysemous_ht = int(z["hts"][0])
    g.set_scan_split(1, 1)
    D0, I0 = g.search(z["xq"], k)
    assert "Q=1 S=1" in g.last_scan_info()
    n = z["codes"].shape[0]
    assert all(-(-n // s) % 64 for s in (2, 7))
    for q in (1, 2, 4):
        for s in (1, 2, 7):
            g.set_scan_split(q, s)
            g.stats(reset=True)
            D, I = g.search(z["xq"], k)
            info = g.last_scan_info()
            assert "Q=%d S=%d " % (1 if k > 256 else q, s) in info and ("join=%d" % (s > 1)) in info
            assert np.array_equal(bits(D), bits(D0)) and np.array_equal(I, I0), (name, q, s)
            if "hts" in z:
                assert g.stats()[2] == int(z["stats0"][2])
    g.close()


def test_k_beyond_ntotal():
    z = load("pq_kwide")
    g = make_index(z, codes=False)
    nb = int(z["small_nb"])
    g.set_codes(z["codes"][:nb])
    D, I = g.search(z["xq"], int(z["k"]))
    assert assert_same_topk(D, I, z["D_small"], z["I_small"], "k > ntotal") == 0
    # a k between: the first rows of the k = 1024 answer (no ties in this fixture), through the KPL = 4 instantiation
    g.set_codes(z["codes"])
    D, I = g.search(z["xq"], 200)
    assert np.array_equal(bits(D), bits(z["D0"][:, :200])) and np.array_equal(I, z["I0"][:, :200])
    assert ", 4, group4, none, " in g.last_scan_info()
    g.close()


@pytest.mark.parametrize("name", ["pq_m4_d16", "pq_m6_d30"])
def test_add_on_the_device(name):
    """add gives the reference's codes; add twice equals add once; reset empties the index"""
    z = load(name)
    g = make_index(z, codes=False)
    assert g.ntotal == 0
    g.add(z["xb"])
    assert g.ntotal == z["codes"].shape[0] and np.array_equal(g.codes(), z["codes"])
    assert np.array_equal(g.encode(z["xb"][:100]), z["codes"][:100])
    D, I = g.search(z["xq"], int(z["k"]))
    assert assert_same_topk(D, I, z["D0"], z["I0"], name) == 0
    g.reset()
    assert g.ntotal == 0
    D, I = g.search(z["xq"], 3)
    assert (I == -1).all() and (bits(D) == PAD_BITS["l2"]).all()
    half = z["xb"].shape[0] // 2 + 7
    g.reserve_memory(100)
    g.add(z["xb"][:half])
    g.add(z["xb"][half:])
    assert np.array_equal(g.codes(), z["codes"]) and np.array_equal(g.codes(half - 3, 9), z["codes"][half - 3: half + 6])
    D, I = g.search(z["xq"], int(z["k"]))
    assert assert_same_topk(D, I, z["D0"], z["I0"], name + " added twice") == 0
    g.close()


def test_torch_device_buffers_and_batch_independence():
    import torch
    z = load("pq_m16_d64_l2")
    g = make_index(z, codes=False)
    dev = torch.device("cuda:0")
    g.set_codes(torch.from_numpy(z["codes"]).to(dev))
    xq = torch.from_numpy(z["xq"]).to(dev)
    torch.cuda.synchronize()
    k = int(z["k"])
    D, I = g.search(xq, k)
    assert D.is_cuda and I.is_cuda
    g.last_scan_info()          # synchronises the index's stream
    assert assert_same_topk(D.cpu().numpy(), I.cpu().numpy(), z["D0"], z["I0"], "device buffers") == 0
    # every query alone, and odd batches, give the rows of the whole batch
    for lo, hi in ((0, 1), (1, 4), (4, 9), (9, 32)):
        Db, Ib = g.search(z["xq"][lo:hi], k)
        assert np.array_equal(bits(Db), bits(z["D0"][lo:hi])) and np.array_equal(Ib, z["I0"][lo:hi])
    g.close()


def test_refusals():
    z = load("pq_m6_d30")
    g = make_index(z)
    for k in (0, 1025):
        with pytest.raises(vlq.VlqError):
            g.search(z["xq"][:2], k)
    for st in ("he", "generalized_he"):
        with pytest.raises(vlq.VlqError) as e:
            g.search_type = st
        assert e.value.code == 3 and ("ST_HE" in str(e.value) or "ST_generalized_HE" in str(e.value))
    assert g.search_type == 0
    g.close()
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuPQ(32, 4, 9)
    assert e.value.code == 3
    g = vlq.GpuPQ(48, 12)                                   # code_size % 8 != 0
    g.set_centroids(np.zeros((12, 256, 4), np.float32))
    g.search_type = "polysemous"
    with pytest.raises(vlq.VlqError) as e:
        g.search(np.zeros((1, 48), np.float32), 1)
    assert "code_size" in str(e.value)
    g.close()
    g = vlq.GpuPQ(32, 8, metric="ip")
    g.set_centroids(np.zeros((8, 256, 4), np.float32))
    g.search_type = "polysemous"
    with pytest.raises(vlq.VlqError) as e:
        g.search(np.zeros((1, 32), np.float32), 1)
    assert "METRIC_L2" in str(e.value)
    g.close()
