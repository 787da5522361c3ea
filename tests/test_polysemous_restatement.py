"""CPU: the numpy restatement of the polysemous filter (tests/polysemous_ref.py) is held to the reference's own
search_knn_with_key with polysemous_ht set, on the two fixtures whose mode the reference defines: from the fixture's lists,
the codes of the queries and the distance of every scanned code it must return the reference's distances bit for bit, its
labels, its pass counts and its ncode, at every threshold.  The GPU tests of table type 0 / 1 lean on this restatement."""
import ctypes as C

import numpy as np
import pytest

from polysemous_ref import POLY_CASE_NAMES, POLY_DEFINED, case_filtered, pairs_to_ids
from util import Case, assert_same_topk

NEW_SYMBOLS = ["vlq_ivfpq_set_polysemous_ht", "vlq_ivfpq_query_codes", "vlq_ivfpq_polysemous_stats"]


@pytest.mark.parametrize("name", POLY_DEFINED)
def test_restatement_reproduces_the_reference(name):
    case = Case(name)
    for t, ht in enumerate(int(v) for v in case["poly_hts"]):
        D, P, npass, ncode = case_filtered(case, ht)
        assert_same_topk(D, P, case["poly_D"][t], case["poly_pairs"][t], "%s ht=%d pairs" % (name, ht))
        assert_same_topk(D, pairs_to_ids(case, P), case["poly_D"][t], case["poly_I"][t], "%s ht=%d ids" % (name, ht))
        assert np.array_equal(npass, case["poly_npass"][t]), "n_hamming_pass at ht=%d" % ht
        assert np.array_equal(ncode, case["poly_ncode"])


@pytest.mark.parametrize("name", POLY_CASE_NAMES)
def test_fixture_conditions(name):
    case = Case(name)
    lens = np.diff(case["list_offsets"])
    assert (lens > 256).any() and (lens % 64 != 0).any() and (lens == 0).any()
    hts = [int(v) for v in case["poly_hts"]]
    assert hts[0] == 1 and hts[3] == 8 * case.M + 1 and hts[0] < hts[1] < hts[2] < hts[3]
    assert case["poly_qcodes"].shape == (case.nq, case.nprobe, case.M)
    assert case["all_D"].shape[1] <= 1024
    _D, P, npass, ncode = case_filtered(case, hts[1])
    assert (npass < case.k).any() and (npass >= case.k).any() and (P == -1).any()
    frac = npass.sum() / float(ncode.sum())
    assert 0.005 < frac < 0.06, frac
    assert 0.2 < case_filtered(case, hts[2])[2].sum() / float(ncode.sum()) < 0.4
    assert case_filtered(case, 1)[2].sum() >= 1


def test_fixture_shapes():
    assert Case("poly_nonresidual").by_residual == 0
    c = Case("poly_imi")
    assert c.imi_nbits == 4 and c.mode == 2 and c.nprobe == 24
    c = Case("poly_table1")
    assert c.M == 16 and c.nbits == 8 and c.mode == 1
    c = Case("poly_table0_m20")
    assert c.M == 20 and c.nbits == 6 and c.mode == 0


def test_polysemous_entry_points_exported():
    from vector_line_quantization_amd import _lib
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(L, s), s


def test_polysemous_entry_points_reject_a_null_handle():
    from vector_line_quantization_amd import _lib
    L = _lib.lib()
    null, n = C.c_void_p(), C.c_uint64()
    assert L.vlq_ivfpq_set_polysemous_ht(null, C.c_int(3)) == 1
    assert L.vlq_ivfpq_polysemous_stats(null, C.byref(n), C.c_int(0)) == 1
    assert L.vlq_ivfpq_query_codes(null, C.c_int64(1), null, null, C.c_int(1), null) == 1
