"""CPU: the numpy restatement of IndexIVFFlat::range_search (tests/range_ref.py) reproduces every reference fixture of
tests/golden/ivfflat_range/ (tests/golden/make_golden_range.py) exactly -- lims, D as bits, I, order included -- and the
fixtures still hold the conditions their generator checked before it wrote them (its docstring lists them)."""
import glob
import os
import sys

import numpy as np
import pytest

import range_ref as rr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_range as gen  # noqa: E402

NAMES = list(rr.CASES)


def bits(a):
    return a.view(np.uint32)


def test_every_fixture_is_listed():
    on_disk = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(rr.RANGE_DIR, "*.npz")))
    assert on_disk == sorted(NAMES)
    for n in on_disk:
        assert os.path.getsize(os.path.join(rr.RANGE_DIR, n + ".npz")) <= 1000000


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_fixture(name):
    z, r, prefix, metric, keys = rr.load_case(name)
    names = rr.radius_names(r)
    want = ["tight", "tight_next"] + (["wide"] if "wide" in names else []) + (["all"] if name in rr.WIDE_CASES else []) + ["none"]
    assert names == want
    for i, rn in enumerate(names):
        lims, D, I = rr.range_search_preassigned(z, z[prefix + "xq"], keys, r["radii"][i], metric, prefix=prefix)
        assert np.array_equal(lims, r["lims_" + rn]), rn
        assert np.array_equal(bits(D), bits(r["D_" + rn])), rn
        assert np.array_equal(I, r["I_" + rn]), rn
        assert r["D_" + rn].dtype == np.float32 and r["I_" + rn].dtype == np.int64 and lims[-1] == D.size == I.size


@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """the generator's own conditions, from the committed arrays"""
    z, r, prefix, metric, keys = rr.load_case(name)
    res = gen.results_of(r)
    missed = []
    assert gen.conditions(name, metric, z, prefix, z[prefix + "xq"], keys, res, missed.append) is True, missed
    nq = keys.shape[0]
    inf = np.float32(np.inf)
    assert res["none"][0] == (inf if metric == "ip" else 0)
    if name in rr.WIDE_CASES:
        assert res["all"][0] == (-inf if metric == "ip" else inf)
        assert res["all"][1][-1] == sum(int(np.diff(z["list_offsets"])[k]) for k in keys.ravel())
        assert "wide" in res
    else:
        # `wide` outside the long and ragged cases: only where no single radius can show both halves of the `tight` condition
        assert ("wide" in res) == (not rr.one_radius_can(z, z[prefix + "xq"], keys, metric, prefix))
    assert (keys >= 0).all() and keys.shape == z[prefix + "keys"].shape
    live = z[prefix + "keys"] >= 0
    assert np.array_equal(keys[live], z[prefix + "keys"][live])
    assert ("keys" in r.files) == (not live.all())
    assert res["tight_next"][0] == np.nextafter(res["tight"][0], -inf if metric == "ip" else inf)
    assert res["tight"][1].size == nq + 1


def test_tight_condition_is_met_by_one_radius_where_the_data_allow():
    """the cases whose `tight` shows an empty query and a query with hits from two probes at once"""
    both = [n for n in NAMES if rr.one_radius_can(*_args(n))]
    assert sorted(both) == ["flat_coarse_int_ip", "flat_l2_d128_long", "flat_tail_d3_ip", "flat_tail_d5_l2"]
    for n in both:
        z, xq, keys, metric, prefix = _args(n)
        r = np.load(os.path.join(rr.RANGE_DIR, n + ".npz"))
        assert rr.hits_from_two_probes(z, xq, keys, r["radii"][0], metric, prefix) and (np.diff(r["lims_tight"]) == 0).any()


def _args(name):
    z, _r, prefix, metric, keys = rr.load_case(name)
    return z, z[prefix + "xq"], keys, metric, prefix


def test_duplicates_come_back_twice_in_scan_order():
    """flat_padding_ties: every vector is stored twice, both copies are hits, the earlier list position first"""
    z, r, prefix, metric, keys = rr.load_case("flat_padding_ties_l2")
    for rn in ("tight", "wide"):
        lims, D, I = r["lims_" + rn], r["D_" + rn], r["I_" + rn]
        assert lims[-1] > 0
        half = z["ids"].size // 2
        for q in range(lims.size - 1):
            d, i = D[lims[q]:lims[q + 1]], I[lims[q]:lims[q + 1]]
            assert sorted(i[i < half] + half) == sorted(i[i >= half])
            for a in i[i < half]:
                pa, pb = np.nonzero(i == a)[0][0], np.nonzero(i == a + half)[0][0]
                assert pa < pb and bits(d)[pa] == bits(d)[pb]


def test_small_batches_of_coarse_int_are_the_first_rows():
    for name in ("flat_coarse_int_l2", "flat_coarse_int_ip"):
        _z, r, _p, _m, _k = rr.load_case(name)
        ns = int(r["n_small"])
        assert 0 < ns < 20 <= r["lims_tight"].size - 1
        for rn in rr.radius_names(r):
            t = r["lims_" + rn][ns]
            assert np.array_equal(r["lims_small_" + rn], r["lims_" + rn][:ns + 1])
            assert np.array_equal(bits(r["D_small_" + rn]), bits(r["D_" + rn][:t])) and np.array_equal(r["I_small_" + rn], r["I_" + rn][:t])


def test_plain_sum_is_told_apart():
    """a plain left-to-right sum gives a different lims or different D bits for at least one case with d >= 4"""
    told = []
    for name in NAMES:
        z, r, prefix, metric, keys = rr.load_case(name)
        if z[prefix + "xq"].shape[1] >= 4 and gen.discriminates(metric, z, prefix, z[prefix + "xq"], keys, gen.results_of(r)):
            told.append(name)
            break
    assert told


def test_strict_comparison_and_nan():
    z, r, prefix, metric, keys = rr.load_case("flat_l2_d32")
    xq = z["xq"]
    tight = r["radii"][0]
    lims, D, _I = rr.range_search_preassigned(z, xq, keys, tight, "l2")
    assert not (D == tight).any() and (D < tight).all()
    assert rr.range_search_preassigned(z, xq, keys, np.float32(np.nan), "l2")[0][-1] == 0
    bad = keys.copy()
    bad[3, 1] = int(z["nlist"])
    with pytest.raises(ValueError):
        rr.range_search_preassigned(z, xq, bad, tight, "l2")
    bad[3, 1] = -1
    with pytest.raises(ValueError):
        rr.range_search_preassigned(z, xq, bad, tight, "l2")
