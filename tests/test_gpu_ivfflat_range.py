"""GPU: range search of IVFFlat (vlq.GpuIVFFlat.range_search*, csrc/scan_range_flat.hip) against fixtures made from the
reference's own IndexIVFFlat::range_search (tests/golden/make_golden_range.py).  Fixtures only: no reference tree, no oracle.
Every comparison is exact -- lims, D as bits, I, order included: a range search selects nothing, so nothing is free."""
import numpy as np
import pytest

import range_ref as rr
import vector_line_quantization_amd as vlq
from util import bits
from vector_line_quantization_amd._lib import check

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED = 1, 3
CASES = list(rr.CASES)


def make_index(z, prefix="", metric=None):
    d, nlist = z[prefix + "coarse_centroids"].shape[1], z[prefix + "coarse_centroids"].shape[0]
    g = vlq.GpuIVFFlat(d, nlist, device=0, metric=metric)
    g.set_coarse_centroids(z[prefix + "coarse_centroids"])
    g.set_lists(z[prefix + "vecs"], z[prefix + "ids"], z[prefix + "list_offsets"])
    return g


def same(got, lims, D, I):
    l, d, i = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in got)
    assert l.dtype == np.int64 and d.dtype == np.float32 and i.dtype == np.int64
    assert np.array_equal(l, lims), "lims differ"
    assert np.array_equal(bits(d), bits(D)), "D differs"
    assert np.array_equal(i, I), "I differs"


@pytest.fixture(scope="module", params=CASES)
def setup(request):
    z, r, prefix, metric, keys = rr.load_case(request.param)
    g = make_index(z, prefix, metric)
    yield request.param, z, r, prefix, metric, keys, g
    g.close()


@pytest.fixture(scope="module")
def d32():
    z, r, prefix, metric, keys = rr.load_case("flat_l2_d32")
    g = make_index(z, prefix, metric)
    yield z, r, keys, g
    g.close()


def test_seam(setup):
    """range_search_preassigned at every stored radius against the reference's range_search; the kernel that ran"""
    name, z, r, prefix, metric, keys, g = setup
    xq = z[prefix + "xq"]
    for i, rn in enumerate(rr.radius_names(r)):
        same(g.range_search_preassigned(xq, keys, float(r["radii"][i])), r["lims_" + rn], r["D_" + rn], r["I_" + rn])
        info = g.last_scan_info()
        assert "kernel=range_flat_kernel<%s>" % metric.upper() in info
        assert ("read=tile128" if xq.shape[1] % 4 == 0 else "read=dword") in info


@pytest.mark.parametrize("name", ["flat_l2_d32", "flat_ip_d32", "flat_tail_d30_l2", "flat_l2_d128_long"])
def test_range_search_is_coarse_then_preassigned(name):
    z, r, prefix, metric, _keys = rr.load_case(name)
    g = make_index(z, prefix, metric)
    xq, nprobe = z["xq"], int(z["nprobe"])
    assert xq.shape[0] in (20, 40)
    for n in (xq.shape[0], 3):          # the coarse stage's matrix path and its small-batch path
        for radius in r["radii"][[0, 2]]:
            _c, keys = g.coarse_search(xq[:n], nprobe)
            want = g.range_search_preassigned(xq[:n], keys, float(radius))
            same(g.range_search(xq[:n], nprobe, float(radius)), *want)
            assert want[0][-1] > 0
    g.close()


def test_forty_queries_and_three():
    """the issue's sizes: range_search = coarse_search + range_search_preassigned at 40 queries and at 3"""
    z, r, prefix, metric, _keys = rr.load_case("flat_ip_d32")
    g = make_index(z, prefix, metric)
    xq, nprobe = z["xq"], int(z["nprobe"])
    assert xq.shape[0] == 40
    for n in (40, 3):
        _c, keys = g.coarse_search(xq[:n], nprobe)
        same(g.range_search(xq[:n], nprobe, float(r["radii"][0])), *g.range_search_preassigned(xq[:n], keys, float(r["radii"][0])))
    g.close()


@pytest.mark.parametrize("name", ["flat_coarse_int_l2", "flat_coarse_int_ip"])
def test_whole_range_search_against_the_reference(name):
    """integer-valued data: every distance is exact, so the keys do not depend on how the coarse stage sums"""
    z, r, prefix, metric, keys = rr.load_case(name)
    g = make_index(z, prefix, metric)
    xq, nprobe, ns = z[prefix + "xq"], int(z["nprobe"]), int(r["n_small"])
    assert (xq.shape[0], ns) == (24, 7)
    _c, k = g.coarse_search(xq, nprobe)
    assert np.array_equal(k, keys)
    for i, rn in enumerate(rr.radius_names(r)):
        radius = float(r["radii"][i])
        same(g.range_search(xq, nprobe, radius), r["lims_" + rn], r["D_" + rn], r["I_" + rn])                      # 24 queries
        same(g.range_search(xq[:ns], nprobe, radius), r["lims_small_" + rn], r["D_small_" + rn], r["I_small_" + rn])   # 7 queries
    g.close()


@pytest.mark.parametrize("device_outputs", [False, True])
def test_bad_keys(d32, device_outputs):
    z, r, keys, g = d32
    xq, radius = z["xq"], float(r["radii"][0])
    if device_outputs:
        torch = pytest.importorskip("torch")
        to = lambda a: torch.from_numpy(a).cuda()
    else:
        to = lambda a: a
    for badval in (-1, int(z["nlist"])):
        bad = keys.copy()
        bad[3, 1] = badval
        with pytest.raises(vlq.VlqError) as e:
            g.range_search_preassigned(to(xq), to(bad), radius)
        assert e.value.code == ERR_INVALID and "nlist" in str(e.value)
        # the failed call leaves an empty result ...
        D, I = g.range_result()
        assert D.shape == (0,) and I.shape == (0,)
        # ... and the index goes on working
        same(g.range_search_preassigned(to(xq), to(keys), radius), r["lims_tight"], r["D_tight"], r["I_tight"])
    # nothing is left pending for the k-NN search's own flag
    g.stats(reset=True)


def test_stats_are_untouched_and_knn_search_goes_on(d32):
    z, r, keys, g = d32
    k = int(z["k"])
    g.stats(reset=True)
    D0, I0 = g.search_preassigned(z["xq"], z["keys"], k)
    before = g.stats()
    assert before[0] == z["xq"].shape[0] and before[2] > 0
    g.range_search_preassigned(z["xq"], keys, float(r["radii"][2]))
    g.range_search(z["xq"], int(z["nprobe"]), float(r["radii"][0]))
    assert g.stats() == before
    D, I = g.search_preassigned(z["xq"], z["keys"], k)
    assert np.array_equal(bits(D), bits(z["D"])) and np.array_equal(I, z["I"])
    assert np.array_equal(bits(D), bits(D0)) and np.array_equal(I, I0)
    assert "scan_flat_kernel" in g.last_scan_info()


def test_held_result():
    z, r, prefix, metric, keys = rr.load_case("flat_l2_d32")
    g = make_index(z, prefix, metric)
    lims, D, I = g.range_search_preassigned(z["xq"], keys, float(r["radii"][2]))
    same((lims, D, I), r["lims_wide"], r["D_wide"], r["I_wide"])
    D1, I1 = g.range_result()
    g.add(z["xb"][:100])                    # the lists grow (and may move): the held hits are a copy of their own
    assert g.ntotal == z["ids"].shape[0] + 100
    D2, I2 = g.range_result()
    for d, i in ((D1, I1), (D2, I2)):
        assert np.array_equal(bits(d), bits(D)) and np.array_equal(i, I)
    g.reset()                               # ... until reset
    assert g.range_result()[0].shape == (0,)
    g.close()


def test_edge_values(d32):
    z, r, keys, g = d32
    xq = z["xq"]
    lims, D, I = g.range_search_preassigned(xq[:0], keys[:0], 1.0)
    assert lims.tolist() == [0] and D.shape == (0,) and I.shape == (0,)
    lims, D, I = g.range_search(xq[:0], 5, 1.0)
    assert lims.tolist() == [0] and D.shape == (0,)
    lims, D, I = g.range_search_preassigned(xq, keys, float("nan"))
    assert np.array_equal(lims, np.zeros(xq.shape[0] + 1, np.int64)) and D.shape == (0,)
    # nprobe = nlist: every list, so every stored vector once per query, list by list in the coarse order
    nlist, n = int(z["nlist"]), int(z["ids"].shape[0])
    _c, kall = g.coarse_search(xq, nlist)
    lims, D, I = g.range_search(xq, nlist, float("inf"))
    assert np.array_equal(lims, np.arange(xq.shape[0] + 1) * n)
    _l4, D4, I4 = rr.range_search_preassigned(z, xq[:4], kall[:4], np.inf, "l2")
    assert np.array_equal(bits(D[:4 * n]), bits(D4)) and np.array_equal(I[:4 * n], I4)
    with pytest.raises(vlq.VlqError) as e:
        g.range_search(xq, 1025, 1.0)
    assert e.value.code == ERR_UNSUPPORTED


def test_refused_call_leaves_an_empty_result():
    """a successful search with hits, then a call refused before any scan: the previous hits are gone from the handle, so
    range_result is empty (and writes nothing) -- through Python and through the C ABI itself"""
    import ctypes as C
    z, r, prefix, metric, keys = rr.load_case("flat_l2_d32")
    g = make_index(z, prefix, metric)
    xq, radius, nprobe = z["xq"], float(r["radii"][2]), int(z["nprobe"])
    L = vlq.lib()
    total = int(r["lims_wide"][-1])
    px, pk = xq.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p)
    lims = np.zeros(xq.shape[0] + 1, np.int64)
    pl = lims.ctypes.data_as(C.c_void_p)
    refusals = [
        ("nprobe beyond the limit", ERR_UNSUPPORTED, lambda: g.range_search(xq, 1025, radius)),
        ("nprobe 0", ERR_INVALID, lambda: g.range_search(xq, 0, radius)),
        ("preassigned, 1025 probes", ERR_UNSUPPORTED, lambda: g.range_search_preassigned(xq, np.zeros((xq.shape[0], 1025), np.int64), radius)),
        ("C: n < 0", ERR_INVALID, lambda: check(L.vlq_ivfflat_range_search(g._h, C.c_int64(-1), px, C.c_int(nprobe), C.c_float(radius), pl, None))),
        # more queries than one launch takes (2^31 - 1): refused from the number alone, x is not read
        ("C: n = 2^31", ERR_UNSUPPORTED, lambda: check(L.vlq_ivfflat_range_search(g._h, C.c_int64(1 << 31), px, C.c_int(nprobe), C.c_float(radius), pl, None))),
        ("C: n = 2^31, preassigned", ERR_UNSUPPORTED,
         lambda: check(L.vlq_ivfflat_range_search_preassigned(g._h, C.c_int64(1 << 31), px, pk, C.c_int(nprobe), C.c_float(radius), pl, None))),
        ("C: null lims", ERR_INVALID, lambda: check(L.vlq_ivfflat_range_search(g._h, C.c_int64(xq.shape[0]), px, C.c_int(nprobe), C.c_float(radius), None, None))),
        ("C: null keys", ERR_INVALID,
         lambda: check(L.vlq_ivfflat_range_search_preassigned(g._h, C.c_int64(xq.shape[0]), px, None, C.c_int(nprobe), C.c_float(radius), pl, None))),
    ]
    for what, code, call in refusals:
        same(g.range_search_preassigned(xq, keys, radius), r["lims_wide"], r["D_wide"], r["I_wide"])
        assert total > 0
        with pytest.raises(vlq.VlqError) as e:
            call()
        assert e.value.code == code, what
        # the C ABI: buffers of the previous total with a sentinel stay untouched, whatever Python's mirror says
        D = np.full(total, -7.0, np.float32)
        I = np.full(total, -7, np.int64)
        check(L.vlq_ivfflat_range_result(g._h, D.ctypes.data_as(C.c_void_p), I.ctypes.data_as(C.c_void_p)))
        assert (D == -7.0).all() and (I == -7).all(), what
        if not what.startswith("C:"):           # (the calls made through Python: its mirror of the total agrees)
            D0, I0 = g.range_result()
            assert D0.shape == (0,) and I0.shape == (0,), what
    # an untrained index: refused by readiness, same rule
    g2 = vlq.GpuIVFFlat(xq.shape[1], int(z["nlist"]), metric="l2")
    with pytest.raises(vlq.VlqError):
        g2.range_search(xq, nprobe, radius)
    assert g2.range_result()[0].shape == (0,)
    g2.close()
    g.close()


def test_many_query_pages(d32):
    """33 000 queries: more than the coarse stage's 32 768-query page.  The range scan itself stores no per-probe counts and
    so has no page of its own (csrc/range_plan.h): one launch per pass serves them all."""
    z, r, keys, g = d32
    reps = 33000 // 40
    assert reps * 40 == 33000
    xq, kk = np.tile(z["xq"], (reps, 1)), np.tile(keys, (reps, 1))
    cnt = np.diff(r["lims_tight"])
    want_lims = np.concatenate([[0], np.cumsum(np.tile(cnt, reps))])
    want = (want_lims, np.tile(r["D_tight"], reps), np.tile(r["I_tight"], reps))
    radius = float(r["radii"][0])
    same(g.range_search_preassigned(xq, kk, radius), *want)
    _c, k1 = g.coarse_search(z["xq"], int(z["nprobe"]))
    if np.array_equal(k1, keys):        # (the coarse stage's keys of general floats are its own: compared only where equal)
        same(g.range_search(xq, int(z["nprobe"]), radius), *want)
    else:
        _c, kbig = g.coarse_search(xq, int(z["nprobe"]))
        same(g.range_search(xq, int(z["nprobe"]), radius), *g.range_search_preassigned(xq, kbig, radius))


def test_torch_device_tensors():
    torch = pytest.importorskip("torch")
    z, r, prefix, metric, keys = rr.load_case("flat_ip_d32")
    g = make_index(z, prefix, metric)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    xq, kk = torch.from_numpy(z["xq"]).cuda(), torch.from_numpy(keys).cuda()
    for i, rn in enumerate(rr.radius_names(r)):
        out = g.range_search_preassigned(xq, kk, float(r["radii"][i]))
        assert all(t.is_cuda for t in out)
        torch.cuda.synchronize()
        same(out, r["lims_" + rn], r["D_" + rn], r["I_" + rn])
    out = g.range_search(xq, int(z["nprobe"]), float(r["radii"][0]))
    torch.cuda.synchronize()
    same(out, *g.range_search(z["xq"], int(z["nprobe"]), float(r["radii"][0])))
    g.close()
