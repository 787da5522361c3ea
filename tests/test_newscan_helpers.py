"""CPU: the helpers the width / shape tests of the inner-product, polysemous and IVFFlat scans stand on.

  * polysemous_ref.oracle_qcodes / oracle_scan / oracle_filtered build the expected rows of a random index from the oracle
    alone.  On the four poly_* fixtures they must give the fixture's own poly_qcodes (the reference's, or the library's
    definition as the fixture recorded it) and the rows case_filtered gives from the fixture's arrays.
  * newscan_index.layout is deterministic and meets the length conditions the GPU tests assert again."""
import numpy as np
import pytest

import newscan_index as nx
from polysemous_ref import POLY_CASE_NAMES, case_filtered, oracle_filtered, oracle_qcodes, oracle_scan
from util import Case, bits


@pytest.fixture(scope="module", params=POLY_CASE_NAMES)
def poly(request):
    case = Case(request.param)
    return case, oracle_scan(case.oracle_index(), case.xq, case["keys"], case["coarse_dis"])


def test_oracle_qcodes_are_the_fixtures(poly):
    case, scan = poly
    live = (case["keys"] >= 0) & (case["keys"] < case.nlist)
    assert live.mean() > 0.5
    assert np.array_equal(scan["qcodes"][live], case["poly_qcodes"][live])
    assert not scan["qcodes"][~live].any()
    # a hole changes nothing else
    keys = case["keys"].copy()
    keys[::3, 1] = -1
    qc = oracle_qcodes(case.oracle_index(), case.xq, keys)
    keep = live & (keys >= 0)
    assert np.array_equal(qc[keep], case["poly_qcodes"][keep]) and not qc[::3, 1].any()


def test_oracle_rows_are_the_restatements(poly):
    case, scan = poly
    assert scan["all_D"].shape[1] == max(1, int(scan["ncode"].max()))
    for ht in (int(v) for v in case["poly_hts"]):
        D, P, npass, ncode = oracle_filtered(scan, ht, case.k)
        De, Pe, npe, nce = case_filtered(case, ht)
        assert np.array_equal(bits(D), bits(De)) and np.array_equal(P, Pe), "%s ht=%d" % (case.name, ht)
        assert np.array_equal(npass, npe) and np.array_equal(ncode, nce)
    rows = [0, 3, case.nq - 1]
    D, P, npass, ncode = oracle_filtered(scan, int(case["poly_hts"][2]), case.k, rows)
    De, Pe, npe, nce = case_filtered(case, int(case["poly_hts"][2]), rows)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(P, Pe) and np.array_equal(npass, npe) and np.array_equal(ncode, nce)


@pytest.mark.parametrize("kw", [dict(), dict(seed=3), dict(nlist=64), dict(lengths=nx.SHORT_LENGTHS), dict(nq=40, seed=5)])
def test_layout_is_deterministic_and_meets_its_conditions(kw):
    a, b = nx.layout(**kw), nx.layout(**kw)
    for nm in ("lens", "list_offsets", "ids", "keys"):
        assert np.array_equal(a[nm], b[nm]), nm
    nx.check_layout(a)
    lens = a["lens"]
    assert sorted(lens[lens > 0].tolist()) == sorted(n for n in kw.get("lengths", nx.LENGTHS) if n)
    assert a["ntotal"] == lens.sum() == a["ids"].shape[0] and np.array_equal(np.diff(a["list_offsets"]), lens)
    assert a["keys"].shape == (kw.get("nq", 24), 7) and a["keys"].max() < a["nlist"]
    assert 0.05 < (a["keys"] < 0).mean() < 0.3
    assert np.unique(a["ids"]).size == a["ntotal"]
    long_list = int(np.argmax(lens))
    assert a["keys"][0, 0] == long_list and a["keys"][1, 0] == -1 and a["keys"][1, 1] == long_list
    assert [int(lens[k]) for k in a["keys"][2]] == list(nx.REQUIRED)
    assert lens[a["keys"][3][a["keys"][3] >= 0]].sum() == 64 and (a["keys"][4] == -1).all()


def test_layout_seeds_differ():
    assert not np.array_equal(nx.layout(seed=0)["keys"], nx.layout(seed=1)["keys"])
    assert nx.layout()["ntotal"] == 2600 and nx.layout()["nlist"] == 12


def test_parts_are_general_floats_and_deterministic():
    lay = nx.layout()
    a, b = nx.pq_parts(lay, 12, 3, 8), nx.pq_parts(lay, 12, 3, 8)
    for nm in ("coarse", "pq", "codes", "xq", "coarse_dis"):
        assert np.array_equal(a[nm], b[nm]), nm
    assert a["codes"].shape == (2600, 12) and a["pq"].shape == (12, 256, 3) and a["d"] == 36
    assert (a["xq"] != np.round(a["xq"])).all() and (a["coarse"] != np.round(a["coarse"])).all()
    assert nx.pq_parts(lay, 8, 2, 5)["codes"].max() == 31
    f = nx.flat_parts(lay, 36)
    assert f["vecs"].shape == (2600, 36) and (f["vecs"] != np.round(f["vecs"])).all()


def test_input_order_rebuilds_the_lists():
    lay = nx.layout()
    rows, assign = nx.input_order(lay)
    assert np.array_equal(np.sort(rows), np.arange(lay["ntotal"]))
    assert not np.array_equal(rows, np.arange(lay["ntotal"]))
    back = np.argsort(assign, kind="stable")                  # what appending in input order leaves: stable by list
    assert np.array_equal(rows[back], np.arange(lay["ntotal"]))
    assert np.array_equal(np.bincount(assign, minlength=lay["nlist"]), lay["lens"])
