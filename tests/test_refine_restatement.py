"""CPU: the numpy restatement of the IVFPQR refine stage (tests/refine_ref.py) is held to the reference's own
IndexIVFPQR on every refine_* fixture -- fed the reference's shortlist it must return the reference's distances bit for
bit -- which is what makes it usable as the oracle of tests/test_gpu_refine.py on machines without the reference.
Also: the fixtures meet the conditions they were generated under, and the new C-ABI entry points exist."""
import ctypes as C
import os

import numpy as np
import pytest

import vector_line_quantization_amd as vlq
from vector_line_quantization_amd import _lib
from refine_ref import REFINE_CASE_NAMES, case_refine_ref, refine_distances
from util import GOLDEN, Case, assert_same_topk

NEW_SYMBOLS = ["vlq_ivfpq_set_refine_pq", "vlq_ivfpq_set_refine_codes", "vlq_ivfpq_get_list_refine_codes", "vlq_ivfpq_refine",
               "vlq_ivfpq_search_refined", "vlq_ivfpq_search_refined_preassigned"]


@pytest.fixture(scope="module", params=REFINE_CASE_NAMES)
def case(request):
    return Case(request.param)


def test_restatement_equals_reference_at_the_seam(case):
    D, I = case_refine_ref(case, case["shortlist"])
    assert_same_topk(D, I, case["refine_D"], case["refine_I"], case.name)


def test_fixture_shapes_and_conditions(case):
    Mr, nbits_r, kc = (int(v) for v in case["refine_cfg"])
    assert kc == int(np.float32(case.k) * case["k_factor"][0])              # long(k * k_factor), IndexIVFPQ.cpp:1375
    assert case["shortlist"].shape == (case.nq, kc) and case["refine_D"].shape == (case.nq, case.k)
    assert case["refine_centroids"].shape == (Mr, 1 << nbits_r, case.d // Mr)
    assert case["refine_codes"].shape == (case["codes"].shape[0], Mr) and case["refine_codes"].max() < (1 << nbits_r)
    assert np.array_equal(np.sort(case["ids"]), np.arange(case["ids"].size))   # sequential ids: the reference looks codes up by id
    tie = case["boundary_tie"].astype(bool)
    if case.name == "refine_duplicates":
        assert (~tie).sum() * 4 >= tie.size
    else:
        assert tie.sum() * 10 <= tie.size
    assert os.path.getsize(os.path.join(GOLDEN, case.name + ".npz")) < (1 << 20)


def test_fixtures_pin_what_they_are_named_for():
    c = Case("refine_tail")
    assert c.d % 4 == 2 and float(c["k_factor"][0]) == 3.5 and int(c["refine_cfg"][1]) < 8
    c = Case("refine_padding")
    assert (c["shortlist"] == -1).any() and (c["refine_I"] == -1).any() and (np.diff(c["list_offsets"]) == 0).any()
    c = Case("refine_duplicates")
    dis, _ = refine_distances(c.xq, c["shortlist"], c["coarse_centroids"], c["pq_centroids"], c["codes"], c["refine_centroids"],
                              c["refine_codes"], c["list_offsets"])
    assert all(np.unique(row).size < row.size for row in dis)                   # ties in the second stage
    assert all(np.unique(row).size < row.size for row in c["shortlist_D"])      # ... and in the first
    c = Case("refine_k_wide")
    assert c["shortlist"].shape[1] == 800 and c.k == 100


def test_refine_entry_points_exported():
    L = vlq.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(L, s), s


def test_refine_entry_points_reject_a_null_handle_and_need_a_device():
    L = vlq.lib()
    null = C.c_void_p()
    buf = (C.c_uint8 * 64)()
    calls = [lambda: L.vlq_ivfpq_set_refine_pq(null, C.c_int(2), C.c_int(8), buf),
             lambda: L.vlq_ivfpq_set_refine_codes(null, buf),
             lambda: L.vlq_ivfpq_get_list_refine_codes(null, C.c_int(0), buf),
             lambda: L.vlq_ivfpq_refine(null, C.c_int64(1), buf, buf, C.c_int(4), C.c_int(1), buf, buf),
             lambda: L.vlq_ivfpq_search_refined(null, C.c_int64(1), buf, C.c_int(1), C.c_int(1), C.c_float(4), buf, buf),
             lambda: L.vlq_ivfpq_search_refined_preassigned(null, C.c_int64(1), buf, buf, buf, C.c_int(1), C.c_int(1), C.c_float(4), buf, buf)]
    for call in calls:
        assert call() == 1 and b"null" in L.vlq_last_error()                   # VLQ_ERR_INVALID
    if vlq.device_count() == 0:      # no CPU path: no handle, no refine stage
        with pytest.raises(vlq.VlqError) as e:
            vlq.GpuIVFPQ(16, 4, 4, 8).set_refine_pq(8, 8, np.zeros((8, 256, 2), np.float32))
        assert "no HIP device" in str(e.value)
