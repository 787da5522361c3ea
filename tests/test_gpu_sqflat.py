"""GPU: vlq.GpuSQ (faiss::IndexScalarQuantizer on the device, csrc/scan_sqflat.hip) against the reference fixtures of
tests/golden/sqflat/ and the numpy restatement (tests/sqflat_ref.py).  The reference leaves its rows in heap order; parity is
stated on its rows sorted by (distance, label), descending distances under inner product."""
import numpy as np
import pytest

import ivfsq_ref as sr
import sqflat_ref as fr
import vector_line_quantization_amd as vlq
from sqflat_cases import FLT_MAX, KWIDE, METRIC, NAMES, PAD_BITS, TIES, WITH_XB, bits, check_rows, distances, ks_of, load

pytestmark = pytest.mark.gpu


def index_of(z, loaded=True):
    g = vlq.GpuSQ(int(z["d"]), int(z["qtype"]), metric=METRIC[int(z["metric"])])
    if loaded:
        g.set_trained(z["trained"])
        g.set_codes(z["codes"])
    return g


# --- seam ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_the_reference_fixture(name):
    z = load(name)
    metric = METRIC[int(z["metric"])]
    g = index_of(z)
    assert g.ntotal == z["codes"].shape[0] and g.code_size == z["codes"].shape[1]
    ties = 0
    for k, dn, inn in ks_of(z):
        D, I = g.search(z["xq"], k)
        ties += check_rows(D, I, z[dn], z[inn], distances(name), metric, (name, k, g.last_scan_info())).sum()
    assert (ties > 0) == (name in TIES)
    g.close()


@pytest.mark.parametrize("name", TIES + KWIDE + ["sqf_4bit_uniform_ip_d32"])
def test_row_order(name):
    """distances sorted, equal distances in ascending position, the padding last as +-FLT_MAX / -1"""
    z = load(name)
    metric = METRIC[int(z["metric"])]
    g = index_of(z)
    D, I = g.search(z["xq"], int(z["k"]))
    g.close()
    sign = np.float32(-1 if metric == "ip" else 1)
    for r in range(D.shape[0]):
        n = int((I[r] != -1).sum())
        assert (I[r, :n] != -1).all() and (I[r, n:] == -1).all() and (bits(D[r, n:]) == PAD_BITS[metric]).all()
        v = sign * D[r, :n]
        assert (np.diff(v) >= 0).all()
        same = np.diff(v) == 0
        assert (np.diff(I[r, :n])[same] > 0).all()
    if name in KWIDE:
        assert (I == -1).any(axis=1).all()


# --- codes and range -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WITH_XB)
def test_train_encode_add_reconstruct(name):
    z = load(name)
    nb, nt = z["xb"].shape[0], int(z["nt"])
    g = index_of(z, loaded=False)
    g.train(z["xb"][:nt])
    assert np.array_equal(bits(g.trained), bits(z["trained"]))
    assert np.array_equal(g.encode(z["xb"]), z["codes"])
    g.add(z["xb"][:nb // 2])
    g.add(z["xb"][nb // 2:])
    assert g.ntotal == nb and np.array_equal(g.codes(), z["codes"])
    assert np.array_equal(g.codes(3, 5), z["codes"][3:8])
    assert np.array_equal(bits(g.reconstruct_n()), bits(z["decoded"]))
    assert np.array_equal(bits(g.reconstruct_n(7, 9)), bits(z["decoded"][7:16]))
    h = index_of(z)
    k = int(z["k"])
    Da, Ia = g.search(z["xq"], k)
    Db, Ib = h.search(z["xq"], k)
    assert np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib)
    g.reset()
    assert g.ntotal == 0
    g.add(z["xb"][:10])
    assert np.array_equal(g.codes(), z["codes"][:10])
    g.close()
    h.close()


# --- edge cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sqf_8bit_l2_d32", "sqf_4bit_ip_d33"])
def test_empty_small_and_single(name):
    z = load(name)
    metric = METRIC[int(z["metric"])]
    dis = distances(name)
    g = index_of(z, loaded=False)
    g.set_trained(z["trained"])
    D, I = g.search(z["xq"], 7)                             # an empty index: all padding
    assert (I == -1).all() and (bits(D) == PAD_BITS[metric]).all()
    g.set_codes(z["codes"][:5])                             # k > ntotal
    D, I = g.search(z["xq"], 9)
    Dn, In = fr.rows_of(dis[:, :5], 9, metric)
    assert np.array_equal(bits(D), bits(Dn)) and np.array_equal(I, In) and (I[:, 5:] == -1).all()
    g.set_codes(z["codes"])
    D1, I1 = g.search(z["xq"], 1)                           # k = 1
    Dn, In = fr.rows_of(dis, 1, metric)
    assert np.array_equal(bits(D1), bits(Dn)) and np.array_equal(I1, In)
    D, I = g.search(z["xq"], 10)                            # a query alone and inside a batch
    for r in (0, 3, z["xq"].shape[0] - 1):
        Dr, Ir = g.search(z["xq"][r:r + 1], 10)
        assert np.array_equal(bits(Dr[0]), bits(D[r])) and np.array_equal(Ir[0], I[r])
    g.close()


def test_torch_device_buffers():
    import torch
    z = load("sqf_8bit_l2_d32")
    g = vlq.GpuSQ(int(z["d"]), "8bit")
    g.set_trained(z["trained"])
    dev = torch.device("cuda", 0)
    g.set_codes(torch.as_tensor(z["codes"]).to(dev))
    Dh, Ih = g.search(z["xq"], 10)
    xq = torch.as_tensor(z["xq"]).to(dev)
    D = torch.empty((xq.shape[0], 10), dtype=torch.float32, device=dev)
    I = torch.empty((xq.shape[0], 10), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    D2, I2 = g.search(xq, 10, D, I)
    g.last_scan_info()                                      # synchronises the index's stream
    assert D2 is D and I2 is I
    assert np.array_equal(bits(D.cpu().numpy()), bits(Dh)) and np.array_equal(I.cpu().numpy(), Ih)
    g.reset()
    g.add(torch.as_tensor(z["xb"]).to(dev))
    assert np.array_equal(g.codes(), z["codes"])
    out = torch.empty((4, int(z["d"])), dtype=torch.float32, device=dev)
    g.reconstruct_n(2, 4, out)
    assert np.array_equal(bits(out.cpu().numpy()), bits(z["decoded"][2:6]))
    g.close()


def test_a_search_across_a_query_page():
    """32 768 + 5 queries over d 8, 300 stored, k 3: the last five rows equal those searched alone"""
    z = load("sqf_8bit_l2_d8")
    n = 32768 + 5
    xq = np.random.default_rng(81).standard_normal((n, 8)).astype(np.float32)
    g = vlq.GpuSQ(8, "8bit")
    g.set_trained(z["trained"])
    g.set_codes(z["codes"][:300])
    D, I = g.search(xq, 3)
    Dt, It = g.search(xq[-5:], 3)
    assert np.array_equal(bits(D[-5:]), bits(Dt)) and np.array_equal(I[-5:], It)
    Dh, Ih = g.search(xq[32766:32770], 3)                   # the rows on both sides of the boundary
    assert np.array_equal(bits(D[32766:32770]), bits(Dh)) and np.array_equal(I[32766:32770], Ih)
    dis = fr.all_distances(z["codes"][:300], xq[-5:], "l2", 0, z["trained"])
    Dn, In = fr.rows_of(dis, 3, "l2")
    assert np.array_equal(bits(Dt), bits(Dn)) and np.array_equal(It, In)
    g.close()


# --- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    z = load("sqf_8bit_l2_d32")
    xq = z["xq"]
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuSQ(32, 7)
    assert e.value.code == 1
    g = vlq.GpuSQ(32, "8bit")
    for call in (lambda: g.search(xq, 5), lambda: g.add(z["xb"]), lambda: g.encode(z["xb"])):
        with pytest.raises(vlq.VlqError) as e:               # before set_trained
            call()
        assert e.value.code == 1
    g.set_trained(z["trained"])
    g.set_codes(z["codes"])
    want = g.search(xq, 5)
    for k, code in ((0, 1), (1025, 3)):
        with pytest.raises(vlq.VlqError) as e:
            g.search(xq, k)
        assert e.value.code == code
        got = g.search(xq, 5)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    with pytest.raises(vlq.VlqError) as e:
        g.reconstruct_n(990, 20)
    assert e.value.code == 1
    with pytest.raises(vlq.VlqError) as e:
        g.set_trained(np.zeros(64, np.float32))              # vdiff == 0
    assert e.value.code == 1
    got = g.search(xq, 5)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    g.close()
    # a d the plan refuses: the query, vmin and vdiff beside the turn tiles are beyond 160 KB of LDS
    d = 20000
    g = vlq.GpuSQ(d, "8bit")
    g.set_trained(np.concatenate([np.zeros(d), np.ones(d)]).astype(np.float32))
    x = np.random.default_rng(5).random((3, d)).astype(np.float32)
    g.add(x)
    with pytest.raises(vlq.VlqError) as e:
        g.search(x, 1)
    assert e.value.code == 3
    assert "kernel=none why=" in g.last_scan_info() and "LDS" in g.last_scan_info()
    assert g.ntotal == 3 and np.array_equal(g.codes(), g.encode(x))
    g.close()


# --- cross-check against the existing route --------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_equals_the_one_list_ivfsq(metric):
    """d 64, 20 000 stored, 64 queries, k 10: a GpuIVFSQ with one list, a zero centroid and nprobe 1, ids = positions"""
    d, nb, nq, k = 64, 20000, 64, 10
    rng = np.random.default_rng(640)
    codes = rng.integers(0, 256, (nb, d), dtype=np.uint8)
    trained = np.concatenate([rng.standard_normal(d), 1 + rng.random(d)]).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    g = vlq.GpuSQ(d, "8bit", metric=metric)
    g.set_trained(trained)
    g.set_codes(codes)
    D, I = g.search(xq, k)
    assert "S=" in g.last_scan_info() and "S=1 " not in g.last_scan_info()        # a small batch is sliced
    v = vlq.GpuIVFSQ(d, 1, "8bit", metric=metric)
    v.set_coarse_centroids(np.zeros((1, d), np.float32))
    v.set_trained(trained)
    v.set_lists(codes, np.arange(nb, dtype=np.int64), np.array([0, nb], np.int64))
    Dv, Iv = v.search_preassigned(xq, np.zeros((nq, 1), np.int64), np.zeros((nq, 1), np.float32), k)
    assert np.array_equal(bits(D), bits(Dv))
    clean = np.array([np.unique(D[r]).size == k for r in range(nq)])
    assert clean.any() and np.array_equal(I[clean], Iv[clean])
    g.close()
    v.close()


# --- refine ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sqf_8bit_l2_d32", "sqf_4bit_ip_d32"])
def test_refine_flat_over_sq(name):
    """"SQ8,RFlat": GpuRefineFlat(GpuSQ) equals GpuFlat.refine applied to GpuSQ.search at k * k_factor"""
    z = load(name)
    metric, k = METRIC[int(z["metric"])], 10
    base = index_of(z, loaded=False)
    base.set_trained(z["trained"])
    r = vlq.GpuRefineFlat(base)
    r.add(z["xb"])
    r.k_factor = 4
    D, I = r.search(z["xq"], k)
    g = index_of(z)
    bD, bI = g.search(z["xq"], 4 * k)
    store = vlq.GpuFlat(int(z["d"]), metric=metric)
    store.add(z["xb"])
    De, Ie = store.refine(z["xq"], bD, bI, k)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)
    assert not np.array_equal(I, bI[:, :k])                  # the exact re-ranking moved something
    g.close()
    store.close()
