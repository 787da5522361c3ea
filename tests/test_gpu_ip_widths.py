"""GPU: every code width of the inner-product scan (csrc/scan_ip.hip: scan_ip_kernel<W, KPL>, W = M / 4 = 1 .. 16 and the
generic W = 0) against the numpy restatement tests/ip_ref.py, which tests/test_ip_restatement.py holds to the reference.
Random codes over the shared small index (tests/newscan_index.py): D as bits, I exactly equal -- the kernel and the
restatement share the (distance, scan position) order, so there is no tie allowance."""
import numpy as np
import pytest

import ip_ref
import newscan_index as nx
import vector_line_quantization_amd as vlq
from util import bits

pytestmark = pytest.mark.gpu
NEG_FLT_MAX_BITS = np.float32(-ip_ref.FLT_MAX).view(np.uint32)
DSUBS = (1, 2, 3, 4, 5, 6, 8)                 # every tail length of ip_sse_order, and two whole steps
KS = (10, 100, 300)                           # KPL 1, 4, 16
K1024 = {32: "uint4 x 2", 24: "uint2 x 3", 20: "dword x 5"}      # widths that also run at k = 1024, one per kind of load
DEVICE_BUFFERS = (12, 24, 32)                 # W 3 (dwords), 6 (uint2), 8 (uint4)
GENERIC = [(7, 5), (6, 8), (13, 8), (16, 6), (64, 4)]
LAY = nx.layout()


def config(M, nbits):
    """what a width runs with: (dsub, by_residual, max_codes), rotated / alternated with M"""
    W = (M + 3) // 4
    return DSUBS[W % len(DSUBS)], bool(W % 2), 400 if (W // 2) % 2 else 0


def build(M, nbits):
    dsub, by_residual, max_codes = config(M, nbits)
    p = nx.pq_parts(LAY, M, dsub, nbits)
    z = dict(coarse_centroids=p["coarse"], pq_centroids=p["pq"], codes=p["codes"], ids=LAY["ids"], list_offsets=LAY["list_offsets"],
             by_residual=int(by_residual), max_codes=max_codes)
    g = vlq.GpuIVFPQ(p["d"], LAY["nlist"], M, nbits, device=0, metric="ip")
    g.set_coarse_centroids(p["coarse"])
    g.set_pq_centroids(p["pq"])
    g.set_search_options(by_residual, 1, max_codes)
    g.set_lists(p["codes"], LAY["ids"], LAY["list_offsets"])
    return g, z, p


def check(M, nbits, ks, device=False):
    g, z, p = build(M, nbits)
    xq, keys, cdis = p["xq"], LAY["keys"], p["coarse_dis"]
    kmax = max(ks)
    want = "kernel=scan_ip_kernel<%d>" % (M // 4 if (nbits == 8 and M % 4 == 0) else 0)
    for store_pairs in (False, True):
        De, Ie, nc = ip_ref.search_preassigned(z, xq, keys, kmax, store_pairs=store_pairs)    # once: a smaller k is its head
        for k in ks:
            g.stats(reset=True)
            if device:
                import torch
                xt, kt, ct = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (xq, keys, cdis))
                D, I = g.search_preassigned(xt, kt, ct, k, store_pairs=store_pairs)
                g.stats()                  # synchronises the index's stream
                D, I = D.cpu().numpy(), I.cpu().numpy()
            else:
                D, I = g.search_preassigned(xq, keys, cdis, k, store_pairs=store_pairs)
            what = "M=%d nbits=%d k=%d pairs=%d %s" % (M, nbits, k, store_pairs, config(M, nbits))
            assert np.array_equal(bits(D), bits(De[:, :k])), what
            assert np.array_equal(I, Ie[:, :k]), what
            assert (bits(D)[I == -1] == NEG_FLT_MAX_BITS).all(), what
            assert g.stats() == (xq.shape[0], int(nc.sum())), what
            assert want in g.last_scan_info(), what
    full = np.array([LAY["lens"][kq[kq >= 0]].sum() for kq in keys])
    if z["max_codes"]:
        assert (nc < full).any() and (nc > z["max_codes"]).any(), "the max_codes cut does not fall inside a walk"
    else:
        assert np.array_equal(nc, full)
    assert (Ie[:, :10] != -1).any() and (Ie[:, KS[-1] - 1] == -1).any(), "no full row / no padded row"
    g.close()


def test_shared_index_conditions():
    nx.check_layout(LAY)
    cfgs = [config(M, 8) for M in range(4, 65, 4)]
    assert {c[0] for c in cfgs} == set(DSUBS)
    assert {(c[1], bool(c[2])) for c in cfgs} == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("M", range(4, 65, 4))
def test_width(M):
    check(M, 8, KS + ((1024,) if M in K1024 else ()))


@pytest.mark.parametrize("M,nbits", GENERIC)
def test_generic_kernel(M, nbits):
    check(M, nbits, KS)


@pytest.mark.parametrize("M", DEVICE_BUFFERS)
def test_device_buffers(M):
    check(M, 8, (10, 300), device=True)
