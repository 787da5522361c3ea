"""GPU: the IVF scalar-quantizer index (vlq.GpuIVFSQ, csrc/scan_sq.hip, csrc/sq_api.hip) against fixtures made from the
reference's own IndexFlatL2 / IndexFlatIP + IndexIVFScalarQuantizer (tests/golden/make_golden_ivfsq.py), through the C ABI.
Fixtures and the numpy restatement (tests/ivfsq_ref.py) only: no reference tree, no oracle."""
import numpy as np
import pytest

import ivfsq_ref as sr
import vector_line_quantization_amd as vlq
from ivfsq_cases import AVX, COARSE_INT, KWIDE, LONG, METRIC, NAMES, PAD_BITS, TIES, WITH_XB, bits, load

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = 1, 3, 4


def make_index(z, lists=True, trained=True):
    g = vlq.GpuIVFSQ(int(z["d"]), int(z["nlist"]), int(z["qtype"]), device=0, metric=METRIC[int(z["metric"])])
    g.set_coarse_centroids(z["coarse_centroids"])
    if trained:
        g.set_trained(z["trained"])
    if lists:
        g.set_lists(z["codes"], z["ids"], z["list_offsets"])
    return g


def assert_rows(name, z, D, I, Dref, Iref, k):
    """D as bits in every row; labels identical, or on the tie fixtures the (distance, label) multisets of the rows where no
    group of equal distances crosses the k-th place -- at least half of the rows"""
    metric, qtype = METRIC[int(z["metric"])], int(z["qtype"])
    assert np.array_equal(bits(D), bits(Dref)), "%s: D differs in %d of %d slots" % (name, (bits(D) != bits(Dref)).sum(), D.size)
    if name in TIES:
        rows = ~sr.tie_across_kth(z, z["xq"], z["keys"], z["cdis"], k, metric, qtype)
        assert (~rows).sum() * 2 <= rows.size
        assert sr.same_pairs(D, I, Dref, Iref, rows)
    else:
        assert np.array_equal(I, Iref), name
    assert (bits(D)[I == -1] == PAD_BITS[metric]).all()


@pytest.mark.parametrize("name", NAMES)
def test_seam(name):
    """search_preassigned with the reference's keys and coarse distances gives the reference's rows"""
    z = load(name)
    g = make_index(z)
    k, d, qtype, metric = int(z["k"]), int(z["d"]), int(z["qtype"]), METRIC[int(z["metric"])]
    assert g.ntotal == z["ids"].shape[0] and g.code_size == z["codes"].shape[1]
    assert np.array_equal(bits(g.trained), bits(z["trained"]))
    D, I = g.search_preassigned(z["xq"], z["keys"], z["cdis"], k)
    assert_rows(name, z, D, I, z["D"], z["I"], k)
    info = g.last_scan_info()
    kpl = 1 if k <= 64 else 4 if k <= 256 else 16
    assert "kernel=scan_sq_kernel<%d, %s, %d, %s, %s>" % (kpl, metric.upper(), sr.bits_of(qtype), "uniform" if sr.is_uniform(qtype) else "nonuniform",
                                                         "order8" if d % 8 == 0 else "scalar") in info
    assert ("read=tile128" if d % 8 == 0 and g.code_size % 16 == 0 else "read=lane") in info
    if metric == "l2":          # coarse_dis is not read under L2
        D2, I2 = g.search_preassigned(z["xq"], z["keys"], None, k)
        assert np.array_equal(bits(D2), bits(D)) and np.array_equal(I2, I)
    g.close()


def test_extra_k_on_the_same_data():
    z = load(KWIDE[0])
    g = make_index(z)
    D, I = g.search_preassigned(z["xq"], z["keys"], z["cdis"], 100)
    assert_rows(KWIDE[0], z, D, I, z["D_k100"], z["I_k100"], 100)
    assert "scan_sq_kernel<4, L2" in g.last_scan_info()
    g.close()


@pytest.mark.parametrize("name", COARSE_INT)
def test_whole_search_against_the_reference(name):
    """exact coarse distances: search() is the coarse stage, then the walk of its probes, and equals the reference's search"""
    z = load(name)
    g = make_index(z)
    nprobe, k = int(z["nprobe"]), int(z["k"])
    cdis, keys = g.coarse_search(z["xq"], nprobe)             # 24 queries: the matrix path of the coarse stage
    assert np.array_equal(keys, z["keys"]) and np.array_equal(bits(cdis), bits(z["cdis"]))
    D0, I0 = g.search_preassigned(z["xq"], keys, cdis, k)
    D, I = g.search(z["xq"], nprobe, k)
    assert np.array_equal(bits(D), bits(D0)) and np.array_equal(I, I0)
    assert_rows(name, z, D, I, z["D"], z["I"], k)
    D, I = g.search(z["xq"][:7], nprobe, k)                   # 7 queries: its direct path
    assert np.array_equal(bits(D), bits(z["D"][:7])) and np.array_equal(I, z["I"][:7])
    g.close()


@pytest.mark.parametrize("name", ["sq_8bit_l2_d32", "sq_4bit_ip_d32", "sq_8bit_uniform_ip_d128", "sq_4bit_l2_d33", LONG[0]])
def test_search_is_coarse_then_preassigned(name):
    z = load(name)
    g = make_index(z)
    nprobe, k = int(z["nprobe"]), int(z["k"])
    cdis, keys = g.coarse_search(z["xq"], nprobe)
    D0, I0 = g.search_preassigned(z["xq"], keys, cdis, k)
    D, I = g.search(z["xq"], nprobe, k)
    assert np.array_equal(bits(D), bits(D0)) and np.array_equal(I, I0)
    Dn, In = sr.search_preassigned(z, z["xq"], keys, cdis, k, METRIC[int(z["metric"])], int(z["qtype"]))
    assert np.array_equal(bits(D), bits(Dn)) and np.array_equal(I, In)
    g.close()


@pytest.mark.parametrize("name", WITH_XB)
def test_add_and_encode_give_the_reference_codes(name):
    z = load(name)
    g = make_index(z, lists=False)
    xb, nlist = z["xb"], int(z["nlist"])
    lens = np.diff(z["list_offsets"])
    assign = np.empty(xb.shape[0], np.int64)
    assign[z["ids"]] = np.repeat(np.arange(nlist), lens)
    codes, a = g.encode(xb)
    assert g.ntotal == 0
    assert np.array_equal(a, assign)
    assert np.array_equal(codes[z["ids"]], z["codes"])
    half = xb.shape[0] // 2
    g.reserve_memory(xb.shape[0] // 4)
    g.add(xb[:half])                                     # two batches, default ids, then given ones
    g.add(xb[half:], np.arange(half, xb.shape[0], dtype=np.int64))
    assert g.ntotal == xb.shape[0]
    for li in range(nlist):
        o0, o1 = z["list_offsets"][li], z["list_offsets"][li + 1]
        assert g.list_length(li) == o1 - o0
        c, ids = g.get_list(li)
        assert np.array_equal(ids, z["ids"][o0:o1]) and np.array_equal(c, z["codes"][o0:o1])
    k = int(z["k"])
    D, I = g.search_preassigned(z["xq"], z["keys"], z["cdis"], k)
    assert_rows(name, z, D, I, z["D"], z["I"], k)
    g.reclaim_memory()
    D, I = g.search_preassigned(z["xq"], z["keys"], z["cdis"], k)
    assert_rows(name, z, D, I, z["D"], z["I"], k)
    g.reset()
    assert g.ntotal == 0 and g.list_length(0) == 0
    g.close()


def test_train_gives_the_reference_range():
    for name in ("sq_8bit_l2_d32", "sq_4bit_uniform_ip_d32", "sq_4bit_l2_d33"):
        z = load(name)
        g = make_index(z, lists=False, trained=False)
        g.train(z["xb"][:int(z["nt"])])
        assert np.array_equal(bits(g.trained), bits(z["trained"])), name
        g.close()


def test_add_preassigned_drops_negative_lists():
    z = load("sq_8bit_l2_d32")
    g = make_index(z, lists=False)
    xb, nlist = z["xb"], int(z["nlist"])
    n = xb.shape[0]
    rng = np.random.default_rng(5)
    a = rng.integers(0, nlist, n).astype(np.int64)       # any assignment, not the nearest centroid
    a[::3] = -1
    kept = np.nonzero(a >= 0)[0]
    g.add_preassigned(xb, a)
    assert g.ntotal == kept.size
    want = sr.encode((xb[kept] - z["coarse_centroids"][a[kept]]).astype(np.float32), int(z["qtype"]), z["trained"])
    for li in range(nlist):
        c, ids = g.get_list(li)
        rows = kept[a[kept] == li]
        assert np.array_equal(ids, rows) and np.array_equal(c, want[a[kept] == li])
    g.add_preassigned(xb, a)                             # the ids stay ntotal + i
    _c, ids = g.get_list(int(a[kept[0]]))
    rows = kept[a[kept] == a[kept[0]]]
    assert np.array_equal(ids, np.concatenate([rows, kept.size + rows]))
    g.close()


@pytest.mark.parametrize("name", ["sq_8bit_l2_d32", "sq_4bit_ip_d30"])
def test_negative_key_ends_the_walk(name):
    """the reference cannot be asked (its search takes no keys): the restatement's rule, break at the first key < 0"""
    z = load(name)
    g = make_index(z)
    k, metric, qtype = int(z["k"]), METRIC[int(z["metric"])], int(z["qtype"])
    keys = z["keys"][:, :3].copy()
    cdis = np.ascontiguousarray(z["cdis"][:, :3])
    keys[:, 1] = -1
    D, I = g.search_preassigned(z["xq"], keys, cdis, k)
    D1, I1 = g.search_preassigned(z["xq"], np.ascontiguousarray(keys[:, :1]), np.ascontiguousarray(cdis[:, :1]), k)
    assert np.array_equal(bits(D), bits(D1)) and np.array_equal(I, I1)
    Dn, In = sr.search_preassigned(z, z["xq"], keys, cdis, k, metric, qtype)
    assert np.array_equal(bits(D), bits(Dn)) and np.array_equal(I, In)
    # a key >= nlist BEHIND the end of the walk is never looked at
    keys[:, 2] = int(z["nlist"]) + 5
    D2, I2 = g.search_preassigned(z["xq"], keys, cdis, k)
    assert np.array_equal(bits(D2), bits(D1)) and np.array_equal(I2, I1)
    keys[:, 0] = -1                                      # nothing walked: padding only
    D3, I3 = g.search_preassigned(z["xq"], keys, cdis, k)
    assert (I3 == -1).all() and (bits(D3) == PAD_BITS[metric]).all()
    g.close()


def test_batch_independence():
    z = load("sq_4bit_l2_d128")
    g = make_index(z)
    k = int(z["k"])
    D0, I0 = g.search_preassigned(z["xq"], z["keys"], z["cdis"], k)
    xq, keys, cdis = np.tile(z["xq"], (7, 1)), np.tile(z["keys"], (7, 1)), np.tile(z["cdis"], (7, 1))
    D, I = g.search_preassigned(xq, keys, cdis, k)
    assert np.array_equal(bits(D), np.tile(bits(D0), (7, 1))) and np.array_equal(I, np.tile(I0, (7, 1)))
    perm = np.random.default_rng(2).permutation(z["xq"].shape[0])
    Dp, Ip = g.search_preassigned(z["xq"][perm], z["keys"][perm], z["cdis"][perm], k)
    assert np.array_equal(bits(Dp), bits(D0[perm])) and np.array_equal(Ip, I0[perm])
    g.close()


def test_torch_device_buffers():
    torch = pytest.importorskip("torch")
    z = load("sq_8bit_ip_d32")
    g = make_index(z)
    k = int(z["k"])
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    xq, keys, cdis = torch.from_numpy(z["xq"]).cuda(), torch.from_numpy(z["keys"]).cuda(), torch.from_numpy(z["cdis"]).cuda()
    D = torch.empty((xq.shape[0], k), dtype=torch.float32, device="cuda")
    I = torch.empty((xq.shape[0], k), dtype=torch.int64, device="cuda")
    g.search_preassigned(xq, keys, cdis, k, D=D, I=I)
    torch.cuda.synchronize()
    assert_rows("sq_8bit_ip_d32", z, D.cpu().numpy(), I.cpu().numpy(), z["D"], z["I"], k)
    Ds, Is = g.search(xq, int(z["nprobe"]), k)
    torch.cuda.synchronize()
    assert Ds.is_cuda and (Is.cpu().numpy() >= -1).all()
    g.close()


def test_page_boundary():
    """32 768 + 5 queries at d 8: the coarse stage's query pages are crossed; every row is the row of its query alone"""
    z = load("sq_8bit_l2_d8")
    g = make_index(z)
    nprobe, k, n0 = int(z["nprobe"]), int(z["k"]), z["xq"].shape[0]
    n = 32768 + 5
    xq = np.ascontiguousarray(np.tile(z["xq"], ((n + n0 - 1) // n0, 1))[:n])
    D0, I0 = g.search(z["xq"], nprobe, k)
    D, I = g.search(xq, nprobe, k)
    reps = (n + n0 - 1) // n0
    assert np.array_equal(bits(D), np.tile(bits(D0), (reps, 1))[:n]) and np.array_equal(I, np.tile(I0, (reps, 1))[:n])
    g.close()


def test_refusals():
    z = load("sq_8bit_l2_d32")
    g = make_index(z)
    nq, k = z["xq"].shape[0], int(z["k"])
    with pytest.raises(vlq.VlqError) as e:
        g.search_preassigned(z["xq"], z["keys"], None, 1025)
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(vlq.VlqError) as e:
        g.search(z["xq"], 1025, 10)
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(vlq.VlqError) as e:
        g.search_preassigned(z["xq"], np.zeros((nq, 1025), np.int64), None, 10)
    assert e.value.code == ERR_UNSUPPORTED
    bad = z["keys"].copy()
    bad[3, 1] = int(z["nlist"])
    with pytest.raises(vlq.VlqError) as e:
        g.search_preassigned(z["xq"], bad, None, 10)
    assert e.value.code == ERR_INVALID and "nlist" in str(e.value)
    # the flag was consumed: the index goes on working
    D, I = g.search_preassigned(z["xq"], z["keys"], None, k)
    assert_rows("sq_8bit_l2_d32", z, D, I, z["D"], z["I"], k)
    g.close()
    # untrained: no range, then no centroids
    g = make_index(z, lists=False, trained=False)
    for call in (lambda: g.search(z["xq"], 3, 10), lambda: g.add(z["xb"]), lambda: g.encode(z["xb"]), lambda: g.trained):
        with pytest.raises(vlq.VlqError) as e:
            call()
        assert e.value.code == ERR_STATE
    # a constant dimension: vdiff == 0 is refused, and so is a wrong count
    t = z["trained"].copy()
    t[int(z["d"]) + 3] = 0
    with pytest.raises(vlq.VlqError) as e:
        g.set_trained(t)
    assert e.value.code == ERR_INVALID and "vdiff" in str(e.value)
    with pytest.raises(vlq.VlqError) as e:
        g.set_trained(z["trained"][:2])
    assert e.value.code == ERR_INVALID
    g.close()
    g = vlq.GpuIVFSQ(8, 4, "8bit_uniform")
    with pytest.raises(vlq.VlqError) as e:
        g.set_trained(np.array([0.5, 0.0], np.float32))
    assert e.value.code == ERR_INVALID
    with pytest.raises(vlq.VlqError) as e:
        g.search(np.zeros((1, 8), np.float32), 1, 1)
    assert e.value.code == ERR_STATE
    g.close()
    ip = vlq.GpuIVFSQ(8, 4, "8bit", metric="ip")
    ip.set_coarse_centroids(np.eye(4, 8, dtype=np.float32))
    ip.set_trained(np.concatenate([np.zeros(8), np.ones(8)]).astype(np.float32))
    with pytest.raises(vlq.VlqError) as e:              # accu0 is needed under inner product
        ip.search_preassigned(np.zeros((1, 8), np.float32), np.zeros((1, 1), np.int64), None, 1)
    assert e.value.code == ERR_INVALID
    ip.close()
    with pytest.raises(ValueError):
        vlq.GpuIVFSQ(8, 4, "8bit", metric="cosine")
    with pytest.raises(ValueError):
        vlq.GpuIVFSQ(8, 4, "6bit")
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuIVFSQ(9000, 4, "8bit")
    assert e.value.code == ERR_UNSUPPORTED
