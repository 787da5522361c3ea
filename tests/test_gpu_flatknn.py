"""GPU: the flat exact k-NN index (vlq.GpuFlat, csrc/scan_knn.hip) against fixtures made from the reference's own
faiss::IndexFlatL2 / IndexFlatIP (tests/golden/make_golden_flatknn.py) and against the restatement (tests/knn_ref.py).  The rule
of every fixture kind is test_knn_ref.check_rows'; against the restatement the device rows are bit-equal, labels included,
because both select by the total order (distance, position)."""
import functools

import numpy as np
import pytest

import knn_ref as kr
import vector_line_quantization_amd as vlq
from test_knn_ref import METRICS, NAMES, check_rows, load
from util import bits

pytestmark = pytest.mark.gpu
FLT_MAX = np.float32(np.finfo(np.float32).max)
PAD = {"l2": FLT_MAX, "ip": np.float32(-FLT_MAX)}


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load(name)


@functools.lru_cache(maxsize=None)
def restated(name, metric):
    z = fixture(name)
    D, I = kr.search(z["xq"], z["xb"], int(z["k"]), metric)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


def uneven(n):
    """three uneven pieces of range(n)"""
    a = max(1, n // 7)
    b = max(a + 1, n // 2 + 3) if n > 2 else a
    return [(0, a), (a, min(b, n)), (min(b, n), n)]


def filled(z, metric, pieces):
    g = vlq.GpuFlat(int(z["d"]), metric=metric, device=0)
    xb = z["xb"]
    for lo, hi in ([(0, xb.shape[0])] if pieces == 1 else uneven(xb.shape[0])):
        if hi > lo:
            g.add(xb[lo:hi])
    return g


@pytest.mark.parametrize("pieces", [1, 3])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_fixture(name, metric, pieces):
    """vectors added in one call and in three uneven ones (growth, the norms of appended rows)"""
    z = fixture(name)
    g = filled(z, metric, pieces)
    try:
        assert g.ntotal == z["xb"].shape[0]
        D, I = g.search(z["xq"], int(z["k"]))
        what = "%s %s %d" % (name, metric, pieces)
        check_rows(z, D, I, metric, what)
        Dn, In = restated(name, metric)
        assert np.array_equal(bits(D), bits(Dn)), what + ": distances differ from the restatement"
        assert np.array_equal(I, In), what + ": labels differ from the restatement"
        assert (bits(D)[I == -1] == PAD[metric].view(np.uint32)).all()
        info = g.last_scan_info()
        assert ("path=direct" in info) == kr.is_direct(z["xq"].shape[0], int(z["d"])), info
    finally:
        g.close()


@pytest.mark.parametrize("metric", METRICS)
def test_reconstruct_reset_and_empty(metric):
    z = fixture("blas_d30_nq20")
    xb, xq, k = z["xb"], z["xq"], int(z["k"])
    g = filled(z, metric, 3)
    try:
        assert np.array_equal(bits(g.reconstruct_n()), bits(xb))
        assert np.array_equal(bits(g.reconstruct_n(7, 100)), bits(xb[7:107]))
        with pytest.raises(vlq.VlqError):
            g.reconstruct_n(xb.shape[0] - 1, 2)
        g.reset()
        assert g.ntotal == 0
        for q in (xq, xq[:5]):                     # both paths' padded rows
            D, I = g.search(q, k)
            assert (I == -1).all() and (bits(D) == PAD[metric].view(np.uint32)).all()
        # add again, other vectors first: labels are the new positions
        g.reserve_memory(xb.shape[0])
        g.add(xb[500:])
        g.add(xb[:500])
        perm = np.concatenate([xb[500:], xb[:500]])
        assert np.array_equal(bits(g.reconstruct_n()), bits(perm))
        D, I = g.search(xq, k)
        Dn, In = kr.search(xq, perm, k, metric)
        assert np.array_equal(bits(D), bits(Dn)) and np.array_equal(I, In)
        with pytest.raises(vlq.VlqError) as e:
            g.search(xq, 1025)
        assert "1025" in str(e.value)
        with pytest.raises(vlq.VlqError):
            g.search(xq, 0)
    finally:
        g.close()


@pytest.mark.parametrize("metric", METRICS)
def test_device_tensors(metric):
    import torch
    dev = torch.device("cuda:0")
    for name in ("small_d32_nq19", "blas_d128_nq150"):
        z = fixture(name)
        k = int(z["k"])
        g = vlq.GpuFlat(int(z["d"]), metric=metric, device=0)
        try:
            xb = torch.from_numpy(z["xb"]).to(dev)
            xq = torch.from_numpy(z["xq"]).to(dev)
            torch.cuda.synchronize()
            g.add(xb[:300])
            g.add(xb[300:])
            D, I = g.search(xq, k)
            assert D.is_cuda and I.is_cuda and D.dtype == torch.float32 and I.dtype == torch.int64
            D2 = torch.empty((xq.shape[0], k), dtype=torch.float32, device=dev)
            I2 = torch.empty((xq.shape[0], k), dtype=torch.int64, device=dev)
            g.search(xq, k, D=D2, I=I2)
            back = torch.empty_like(xb)
            g.reconstruct_n(0, xb.shape[0], out=back)
            g.last_scan_info()                   # synchronises the index's stream
            Dn, In = restated(name, metric)
            for d_, i_ in ((D, I), (D2, I2)):
                assert np.array_equal(bits(d_.cpu().numpy()), bits(Dn)) and np.array_equal(i_.cpu().numpy(), In)
            assert torch.equal(back, xb)
        finally:
            g.close()


def test_create_errors():
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuFlat(0)
    assert "d=0" in str(e.value)
    with pytest.raises(ValueError):
        vlq.GpuFlat(8, metric="cosine")
    g = vlq.GpuFlat(8)
    try:
        with pytest.raises(vlq.VlqError) as e:
            g.scan_split(48, 0)
        assert "48" in str(e.value)
        with pytest.raises(vlq.VlqError) as e:
            g.scan_split(0, 65)
        assert "65" in str(e.value)
    finally:
        g.close()
