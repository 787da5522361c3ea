"""GPU (run with -m gpu on an MI355X): the IVFPQR refine stage on the device against the reference's IndexIVFPQR
(refine_* fixtures) and against the numpy restatement tests/refine_ref.py, which tests/test_refine_restatement.py holds
to the same fixtures bit for bit."""
import numpy as np
import pytest

import vector_line_quantization_amd as vlq
from refine_ref import FLT_MAX, REFINE_CASE_NAMES, case_refine_ref, refine_ref
from util import Case, assert_same_topk, bits

pytestmark = pytest.mark.gpu


def gpu_index(case, with_lists=True, with_refine=True):
    g = vlq.GpuIVFPQ(case.d, case.nlist, case.M, case.nbits)
    g.set_coarse_centroids(case["coarse_centroids"])
    g.set_pq_centroids(case["pq_centroids"])
    g.set_search_options(by_residual=True, use_precomputed_table=min(case.mode, 1), max_codes=0)
    if with_refine:
        g.set_refine_pq(int(case["refine_cfg"][0]), int(case["refine_cfg"][1]), case["refine_centroids"])
    if with_lists:
        g.set_lists(case["codes"], case["ids"], case["list_offsets"])
        if with_refine:
            g.set_refine_codes(case["refine_codes"])
    return g


@pytest.fixture(scope="module", params=REFINE_CASE_NAMES)
def case(request):
    return Case(request.param)


def test_seam_vs_reference(case):
    """refine() on the reference's own shortlist == IndexIVFPQR::search's D bit for bit; no query left out"""
    g = gpu_index(case)
    D, I = g.refine(case.xq, case["shortlist"], case.k)
    assert_same_topk(D, I, case["refine_D"], case["refine_I"], case.name)


def test_whole_search_vs_reference(case):
    """from the fixture's probes, on the queries whose shortlist does not depend on the reference's heap history"""
    g = gpu_index(case)
    D, I = g.search_refined_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k, float(case["k_factor"][0]))
    clear = ~case["boundary_tie"].astype(bool)
    assert clear.sum() * 4 >= clear.size
    assert_same_topk(D[clear], I[clear], case["refine_D"][clear], case["refine_I"][clear], case.name)


def test_whole_search_every_query_vs_oracle(case):
    """the library's shortlist order is defined ((distance, scan position)): oracle first stage at k_coarse fed to the
    restatement must equal the device on ALL queries, labels included"""
    g = gpu_index(case)
    kf = float(case["k_factor"][0])
    kc = int(case["refine_cfg"][2])
    ox = case.oracle_index()
    _Ds, sl = ox.search_preassigned(case.xq, case["keys"], case["coarse_dis"], kc, store_pairs=True, canonical=True)
    De, Ie = case_refine_ref(case, sl)
    D, I = g.search_refined_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k, kf)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)
    # search_refined = its own coarse stage + the same: through the oracle's coarse stage
    cd, keys = g.coarse_search(case.xq, case.nprobe)
    _Ds, sl = ox.search_preassigned(case.xq, keys, cd, kc, store_pairs=True, canonical=True)
    De, Ie = case_refine_ref(case, sl)
    D, I = g.search_refined(case.xq, case.nprobe, case.k, kf)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)


def test_add_on_device(case):
    """add() with a refine quantizer set = IndexIVFPQR::add_core: refine codes per list slot, then the same search"""
    g = gpu_index(case, with_lists=False)
    nb = len(case.xb)
    cuts = sorted({0, 1, min(17, nb), nb // 2, nb})
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.add(case.xb[a:b])
    assert g.ntotal == len(case.xb)
    Mr = int(case["refine_cfg"][0])
    by_id = np.zeros((len(case.xb), Mr), np.uint8)
    by_id[case["ids"]] = case["refine_codes"]
    assign, _codes = g.encode(case.xb)
    agree = assign == case["xb_assign"]
    assert agree.mean() >= 0.999
    off = case["list_offsets"]
    for i in range(case.nlist):
        c, ids = g.get_list(i)
        rc = g.get_list_refine_codes(i)
        assert rc.shape == (len(ids), Mr)
        ok = agree[ids]
        assert np.array_equal(rc[ok], by_id[ids[ok]]), "refine codes of list %d" % i
        if agree.all():
            assert np.array_equal(ids, case["ids"][off[i]:off[i + 1]]) and np.array_equal(c, case["codes"][off[i]:off[i + 1]])
            assert np.array_equal(rc, case["refine_codes"][off[i]:off[i + 1]])
    # reserve / reclaim move the refine codes with the lists
    g.reserve_memory(4 * len(case.xb))
    g.reclaim_memory()
    kf = float(case["k_factor"][0])
    D, I = g.search_refined_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k, kf)
    g2 = vlq.GpuIVFPQ(case.d, case.nlist, case.M, case.nbits)
    g2.set_coarse_centroids(case["coarse_centroids"])
    g2.set_pq_centroids(case["pq_centroids"])
    g2.set_refine_pq(Mr, int(case["refine_cfg"][1]), case["refine_centroids"])
    lists = [g.get_list(i) + (g.get_list_refine_codes(i),) for i in range(case.nlist)]
    lens = np.array([len(l[1]) for l in lists])
    g2.set_lists(np.concatenate([l[0] for l in lists]), np.concatenate([l[1] for l in lists]), np.concatenate([[0], np.cumsum(lens)]))
    with pytest.raises(vlq.VlqError) as e:          # lists loaded, refine codes not yet
        g2.search_refined(case.xq, case.nprobe, case.k, kf)
    assert e.value.code == 4
    g2.set_refine_codes(np.concatenate([l[2] for l in lists]))
    D2, I2 = g2.search_refined_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k, kf)
    assert np.array_equal(bits(D), bits(D2)) and np.array_equal(I, I2)
    if agree.all():
        clear = ~case["boundary_tie"].astype(bool)
        assert_same_topk(D[clear], I[clear], case["refine_D"][clear], case["refine_I"][clear], case.name + " after add")


def random_index(rng, d, nlist, M, Mr, nbits_r, ntotal, ids_random=True):
    ksub_r = 1 << nbits_r
    coarse = rng.standard_normal((nlist, d)).astype(np.float32) * 3
    pq = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    rpq = (rng.standard_normal((Mr, ksub_r, d // Mr)) * 0.3).astype(np.float32)
    lens = rng.multinomial(ntotal, rng.dirichlet(np.full(nlist, 0.8)))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = rng.integers(0, 256, (ntotal, M), dtype=np.uint8)
    rcodes = rng.integers(0, ksub_r, (ntotal, Mr), dtype=np.uint8)
    ids = (rng.permutation(ntotal).astype(np.int64) * 5 - 7) if ids_random else np.arange(ntotal, dtype=np.int64)
    g = vlq.GpuIVFPQ(d, nlist, M, 8)
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.set_refine_pq(Mr, nbits_r, rpq)
    g.set_lists(codes, ids, off)
    g.set_refine_codes(rcodes)
    return g, dict(coarse=coarse, pq=pq, rpq=rpq, off=off, codes=codes, rcodes=rcodes, ids=ids)


def random_shortlist(rng, n, kc, off, holes):
    nlist = off.size - 1
    nonempty = np.nonzero(np.diff(off) > 0)[0]
    lists = nonempty[rng.integers(0, nonempty.size, (n, kc))]
    # runs of one list, as a first stage returns them
    lists = np.where(rng.random((n, kc)) < 0.5, np.roll(lists, 1, axis=1), lists)
    ofs = (rng.random((n, kc)) * (off[lists + 1] - off[lists])).astype(np.int64)
    sl = (lists.astype(np.int64) << 32) | ofs
    if holes:
        sl[rng.random((n, kc)) < holes] = -1
    assert nlist > 0
    return sl


FUZZ = [  # d, M, Mr, nbits_r, n, kc, k, holes, buffers
    (16, 4, 4, 8, 1, 1, 1, 0.0, "host"),
    (16, 8, 16, 4, 7, 64, 64, 0.3, "device"),
    (30, 5, 10, 6, 300, 97, 13, 0.1, "pinned"),
    (30, 6, 30, 5, 7, 1024, 256, 0.0, "host"),
    (64, 8, 4, 8, 300, 40, 10, 0.0, "device"),
    (64, 16, 32, 7, 1, 1000, 255, 0.5, "host"),
    (96, 16, 24, 8, 5000, 40, 10, 0.05, "device"),
    (96, 12, 32, 8, 300, 512, 100, 0.0, "host"),
    (128, 16, 16, 8, 5000, 40, 10, 0.0, "pinned"),
    (128, 8, 32, 6, 300, 1024, 65, 0.2, "device"),
    (128, 16, 8, 8, 7, 640, 257, 0.9, "host"),
]


@pytest.mark.parametrize("seed,shape", list(enumerate(FUZZ)))
def test_fuzz_vs_restatement(seed, shape):
    import torch
    d, M, Mr, nbits_r, n, kc, k, holes, buffers = shape
    rng = np.random.default_rng(1000 + seed)
    g, ix = random_index(rng, d, 19, M, Mr, nbits_r, 3000)
    x = (ix["coarse"][rng.integers(0, 19, n)] + rng.standard_normal((n, d))).astype(np.float32)
    sl = random_shortlist(rng, n, kc, ix["off"], holes)
    De, Ie = refine_ref(x, sl, k, ix["coarse"], ix["pq"], ix["codes"], ix["rpq"], ix["rcodes"], ix["ids"], ix["off"])
    if buffers == "host":
        D, I = g.refine(x, sl, k)
    elif buffers == "device":
        xd, sd = torch.from_numpy(x).cuda(), torch.from_numpy(sl).cuda()
        torch.cuda.synchronize()
        Dd, Id = g.refine(xd, sd, k)
        g.stats()                                   # synchronises the index's stream
        D, I = Dd.cpu().numpy(), Id.cpu().numpy()
    else:
        xp, sp = torch.from_numpy(x).pin_memory(), torch.from_numpy(sl).pin_memory()
        Dp, Ip = torch.empty((n, k), dtype=torch.float32).pin_memory(), torch.empty((n, k), dtype=torch.int64).pin_memory()
        g.refine(xp, sp, k, D=Dp, I=Ip)
        D, I = Dp.numpy(), Ip.numpy()
    assert np.array_equal(bits(D), bits(De)), "distances differ"
    assert np.array_equal(I, Ie), "labels differ"
    assert ((I == -1) == (D == FLT_MAX)).all()


def test_batch_composition_does_not_matter():
    rng = np.random.default_rng(77)
    g, ix = random_index(rng, 64, 19, 8, 16, 8, 3000)
    x = (ix["coarse"][rng.integers(0, 19, 300)] + rng.standard_normal((300, 64))).astype(np.float32)
    sl = random_shortlist(rng, 300, 200, ix["off"], 0.1)
    D, I = g.refine(x, sl, 50)
    for q in (0, 1, 63, 64, 150, 299):
        D1, I1 = g.refine(x[q:q + 1], sl[q:q + 1], 50)
        assert np.array_equal(bits(D1[0]), bits(D[q])) and np.array_equal(I1[0], I[q])
    cd, keys = g.coarse_search(x, 5)
    Ds, Is = g.search_refined_preassigned(x, keys, cd, 10, 4.0)
    for q in (0, 17, 299):
        D1, I1 = g.search_refined_preassigned(x[q:q + 1], keys[q:q + 1], cd[q:q + 1], 10, 4.0)
        assert np.array_equal(bits(D1[0]), bits(Ds[q])) and np.array_equal(I1[0], Is[q])


def test_errors():
    case = Case("refine_c1_small")
    kf = float(case["k_factor"][0])
    g = gpu_index(case, with_refine=False)
    for call in (lambda: g.search_refined(case.xq, case.nprobe, case.k, kf),
                 lambda: g.search_refined_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k, kf),
                 lambda: g.refine(case.xq, case["shortlist"], case.k),
                 lambda: g.set_refine_codes(case["refine_codes"])):
        with pytest.raises(vlq.VlqError) as e:
            call()
        assert e.value.code == 4, "no refine quantizer: VLQ_ERR_STATE"
    # plain searches are what they were
    D, I = g.search_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k)
    assert_same_topk(D, I, case["D"], case["I"], "plain search")
    g.set_refine_pq(int(case["refine_cfg"][0]), int(case["refine_cfg"][1]), case["refine_centroids"])
    with pytest.raises(vlq.VlqError) as e:
        g.refine(case.xq, case["shortlist"], case.k)
    assert e.value.code == 4, "codes missing: VLQ_ERR_STATE"
    g.set_refine_codes(case["refine_codes"])
    g.refine(case.xq, case["shortlist"], case.k)
    g.set_lists(case["codes"], case["ids"], case["list_offsets"])        # drops the refine codes
    with pytest.raises(vlq.VlqError) as e:
        g.search_refined(case.xq, case.nprobe, case.k, kf)
    assert e.value.code == 4
    g.set_refine_codes(case["refine_codes"])
    with pytest.raises(vlq.VlqError) as e:
        g.search_refined(case.xq, case.nprobe, 300, 4.0)                 # k_coarse 1200 > 1024
    assert e.value.code == 1
    with pytest.raises(vlq.VlqError) as e:
        g.refine(case.xq, np.zeros((case.nq, 1025), np.int64), 10)
    assert e.value.code == 1
    # a pair past the end of its list
    off = case["list_offsets"]
    lst = int(np.argmax(np.diff(off) > 0))
    bad = case["shortlist"].copy()
    bad[3, 2] = (lst << 32) | int(off[lst + 1] - off[lst])
    with pytest.raises(vlq.VlqError) as e:
        g.refine(case.xq, bad, case.k)
    assert e.value.code == 1 and "pair" in str(e.value)
    bad[3, 2] = case.nlist << 32
    with pytest.raises(vlq.VlqError) as e:
        g.refine(case.xq, bad, case.k)
    assert e.value.code == 1
    D, I = g.refine(case.xq, case["shortlist"], case.k)                  # the flag was consumed
    assert_same_topk(D, I, case["refine_D"], case["refine_I"], "after the error")
    # multi-index handle, by_residual off, BLAS-sized refine sub-vectors
    imi = Case("imi_sse_tables")
    gi = vlq.GpuIVFPQ(imi.d, imi.nlist, imi.M, imi.nbits)
    gi.set_imi_centroids(imi.imi_nbits, imi["imi_centroids"])
    with pytest.raises(vlq.VlqError) as e:
        gi.set_refine_pq(4, 8, np.zeros((4, 256, imi.d // 4), np.float32))
    assert e.value.code == 3
    g.set_search_options(by_residual=False)
    with pytest.raises(vlq.VlqError) as e:
        g.search_refined(case.xq, case.nprobe, case.k, kf)
    assert e.value.code == 3
    g.set_search_options(by_residual=True)
    g.set_refine_pq(8, 8, np.zeros((8, 256, 16), np.float32))            # d / M_refine = 16: search and load only
    with pytest.raises(vlq.VlqError) as e:
        g.add(case.xb[:10])
    assert e.value.code == 3
