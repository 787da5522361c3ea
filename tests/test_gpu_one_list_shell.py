"""GPU: what the four one-list indexes (GpuPQ, GpuSQ, GpuFlat, GpuLSH) have in common, and where they differ on purpose.  The
shell under their handles (csrc/one_list.h) owns the device context, the one list, the paged search and the readers of the
stored rows; this file pins what a caller can see of that, kind by kind, on the smallest shapes: d = 32, 300 vectors added as
100 + 200 (the one list grows once), 5 queries, k = 4.

reserve_memory(2^32): GpuFlat and GpuLSH refuse it (VLQ_ERR_UNSUPPORTED).  GpuPQ and GpuSQ have no such check: they hand the
request to the allocator -- 48 GiB and 160 GiB at these shapes, granted (0) or refused with VLQ_ERR_HIP by whatever the card has
free; what the library itself decides, and what is asserted, is that the answer is not VLQ_ERR_UNSUPPORTED.  That call is the
last before close(), on the emptied index, so that a granted block goes back at once.  It is the one slow step of this file:
measured on an MI355X the pq case took 1.8 s and the sq case 3.2 to 3.6 s, the request granted; every other step of a case takes milliseconds."""
import numpy as np
import pytest

import vector_line_quantization_amd as vlq
from vector_line_quantization_amd._lib import VlqError

pytestmark = pytest.mark.gpu

D_, NB, NQ, K = 32, 300, 5, 4
KINDS = ("pq", "sq", "flat", "lsh")
INVALID, HIP, UNSUPPORTED = 1, 2, 3          # VLQ_ERR_* of include/vlq_ivfpq.h
FLT_MAX_BITS, LSH_PAD_BITS = 0x7F7FFFFF, 0x4F000000      # FLT_MAX; 2147483648.0f, the Hamming scan's padding
# reserve_memory(2^32): beyond the key's 32-bit position field for flat and lsh; the allocator's answer for pq and sq (see above)
RESERVE_2_32 = {"pq": (0, HIP), "sq": (0, HIP), "flat": (UNSUPPORTED,), "lsh": (UNSUPPORTED,)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def world():
    rng = np.random.RandomState(77)
    return {"xb": rng.randn(NB, D_).astype(np.float32), "xq": rng.randn(NQ, D_).astype(np.float32),
            "pq": (0.5 * rng.randn(4, 256, D_ // 4)).astype(np.float32)}


def make(kind, w):
    if kind == "pq":
        g = vlq.GpuPQ(D_, 4, 8)
        g.set_centroids(w["pq"])
    elif kind == "sq":
        g = vlq.GpuSQ(D_, "8bit")
        g.train(w["xb"])
    elif kind == "flat":
        g = vlq.GpuFlat(D_)
    else:
        g = vlq.GpuLSH(D_, 64, rotate_data=True)
    return g


def rows(g, kind, *args):
    """stored rows i0 .. i0 + n - 1 as the kind hands them out"""
    return getattr(g, {"pq": "codes", "sq": "codes", "flat": "reconstruct_n", "lsh": "get_codes"}[kind])(*args)


def code_of(call, *args):
    try:
        call(*args)
    except VlqError as e:
        return e.code
    return 0


@pytest.mark.parametrize("kind", KINDS)
def test_shell_contract(kind, world):
    import torch
    xb, xq = world["xb"], world["xq"]
    g = make(kind, world)
    try:
        assert g.last_scan_info() == "kernel=none"
        assert g.ntotal == 0
        g.add(xb[:100])
        assert g.ntotal == 100
        g.add(xb[100:])
        assert g.ntotal == NB

        # the same bits on the private stream, on another non-blocking stream and back on the first one
        D0, I0 = g.search(xq, K)
        assert D0.shape == (NQ, K) and I0.shape == (NQ, K) and (I0 >= 0).all() and (I0 < NB).all()
        assert g.last_scan_info() != "kernel=none"
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for s in (s1, s2, s1):
            g.set_stream(s.cuda_stream)
            D, I = g.search(xq, K)
            assert np.array_equal(bits(D), bits(D0)) and np.array_equal(I, I0)

        # stored rows: two halves are the whole; a range past ntotal is refused
        whole = rows(g, kind)
        assert whole.shape[0] == NB
        assert np.array_equal(np.concatenate([rows(g, kind, 0, 150), rows(g, kind, 150, 150)]), whole)
        assert rows(g, kind, 7, 0).shape[0] == 0
        assert code_of(rows, g, kind, 200, 200) == INVALID
        assert code_of(rows, g, kind, -1, 2) == INVALID

        # reserve_memory
        assert code_of(g.reserve_memory, -1) == INVALID
        g.reserve_memory(NB + 200)                # (past the grown list: the rows move)
        assert g.ntotal == NB and np.array_equal(rows(g, kind), whole)
        if RESERVE_2_32[kind] == (UNSUPPORTED,):
            assert code_of(g.reserve_memory, 1 << 32) == UNSUPPORTED
            assert g.ntotal == NB

        # search arguments
        info = g.last_scan_info()
        assert code_of(g.search, xq, 0) == INVALID
        assert code_of(g.search, xq, 1025) == UNSUPPORTED
        De, Ie = g.search(xq[:0], K)
        assert De.shape == (0, K) and Ie.shape == (0, K)
        assert g.last_scan_info() == info                      # (none of the three launched anything)
        D, I = g.search(xq, K)
        assert np.array_equal(bits(D), bits(D0)) and np.array_equal(I, I0)

        # reset: an empty index answers with its padding in every slot
        g.reset()
        assert g.ntotal == 0
        D, I = g.search(xq, K)
        assert (I == -1).all() and (bits(D) == (LSH_PAD_BITS if kind == "lsh" else FLT_MAX_BITS)).all()
        assert rows(g, kind).shape[0] == 0

        # the kinds without the 2^32 refusal: last, on the empty index, so that a granted request is given back by close()
        if RESERVE_2_32[kind] != (UNSUPPORTED,):
            assert code_of(g.reserve_memory, 1 << 32) in RESERVE_2_32[kind]
            assert g.ntotal == 0
    finally:
        g.close()
        g.close()
    assert g._h.value is None
