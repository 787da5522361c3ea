"""CPU: the numpy restatement of IndexPQ::search (tests/pq_ref.py) against every flat PQ fixture (tests/golden/pq/, made from
the reference's own faiss::IndexPQ by tests/golden/make_golden_pq.py), and the conditions the generator promises."""
import os

import numpy as np
import pytest

import pq_ref as pr
from util import GOLDEN, bits

CASES = ["pq_m4_d16", "pq_m16_d64_l2", "pq_m16_d64_ip", "pq_m6_d30", "pq_m8_nbits6", "pq_kwide", "pq_ties", "pq_poly_m8",
         "pq_poly_m16", "pq_poly_m24", "pq_poly_m32", "pq_polygen_m16", "pq_sdc_m8", "pq_blas_d128_m4"]
METRIC = {0: "ip", 1: "l2"}


def load(name):
    z = np.load(os.path.join(GOLDEN, "pq", name + ".npz"))
    return {k: z[k] for k in z.files}


def runs(z):
    """(ht or None, D, I, stats) of every recorded search"""
    hts = [int(h) for h in z["hts"]] if "hts" in z else [None]
    return [(ht, z["D%d" % i], z["I%d" % i], z["stats%d" % i]) for i, ht in enumerate(hts)]


def blas_bound(z):
    """2 (dsub + 3) 2^-24 (|x_m|^2 + |c_mj|^2): the rounding bound of both evaluation orders of one table entry"""
    M, dsub = int(z["M"]), int(z["d"]) // int(z["M"])
    xn = (z["xq"].reshape(-1, M, 1, dsub).astype(np.float64) ** 2).sum(-1)
    cn = (z["centroids"].astype(np.float64) ** 2).sum(-1)[None]
    return 2 * (dsub + 3) * 2.0 ** -24 * (xn + cn)


def test_every_fixture_is_listed():
    have = sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN, "pq")) if f.endswith(".npz"))
    assert have == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    z = load(name)
    metric, st, k = METRIC[int(z["metric"])], int(z["search_type"]), int(z["k"])
    blas = name.startswith("pq_blas")
    for ht, D, I, stats in runs(z):
        Dn, In, npass, tabs, qc = pr.search(z["centroids"], z["codes"], z["xq"], k, metric, st, ht, tabs=z["tables"] if blas else None)
        assert pr.same_rows(Dn, In, D, I), (name, ht)
        assert list(stats) == [z["xq"].shape[0], z["xq"].shape[0] * z["codes"].shape[0], npass]
        if st != pr.ST_SDC and not blas:
            assert np.array_equal(bits(tabs[: z["tables"].shape[0]]), bits(z["tables"]))
        if qc is not None:
            assert np.array_equal(qc, z["q_codes"])
    if blas:
        mine = pr.tables(z["xq"], z["centroids"], metric)
        assert (np.abs(mine.astype(np.float64) - z["tables"]) <= blas_bound(z)).all()
    if "xb" in z:
        assert np.array_equal(pr.compute_codes(z["xb"], z["centroids"]), z["codes"])
    if "D_small" in z:
        nb = int(z["small_nb"])
        Dn, In = pr.search(z["centroids"], z["codes"][:nb], z["xq"], k, metric, st)[:2]
        assert pr.same_rows(Dn, In, z["D_small"], z["I_small"])
        assert (z["I_small"][:, nb:] == -1).all() and (bits(z["D_small"][:, nb:]) == bits(np.float32(pr.FLT_MAX))).all()


@pytest.mark.parametrize("name", ["pq_m16_d64_l2", "pq_m16_d64_ip", "pq_m8_nbits6"])
def test_grouped_fixtures_tell_the_orders_apart(name):
    z = load(name)
    Dl = pr.search(z["centroids"], z["codes"], z["xq"], int(z["k"]), METRIC[int(z["metric"])], order="left")[0]
    assert not np.array_equal(bits(Dl), bits(z["D0"]))


def test_default_order_fixture_tells_the_orders_apart():
    z = load("pq_m6_d30")
    Dg = pr.search(z["centroids"], z["codes"], z["xq"], int(z["k"]), "l2", order="group4")[0]
    assert not np.array_equal(bits(Dg), bits(z["D0"]))


@pytest.mark.parametrize("name", CASES)
def test_ties_only_where_they_are_meant(name):
    z = load(name)
    tied = 0
    for _ht, D, I, _s in runs(z):
        for r in range(D.shape[0]):
            v = D[r][I[r] != -1]
            tied += np.unique(v).size != v.size
    assert (tied > 0) == (name == "pq_ties")
    if name == "pq_ties":
        k = int(z["k"])
        Dk1, Ik1 = pr.search(z["centroids"], z["codes"], z["xq"], k + 1)[:2]
        across = (Dk1[:, k] == Dk1[:, k - 1]) & (Ik1[:, k] != -1)
        assert across.any() and (~across).sum() * 3 >= across.size


@pytest.mark.parametrize("name", ["pq_poly_m8", "pq_poly_m16", "pq_poly_m24", "pq_poly_m32", "pq_polygen_m16"])
def test_polysemous_thresholds(name):
    z = load(name)
    n = z["xq"].shape[0] * z["codes"].shape[0]
    assert 0.005 <= z["stats0"][2] / n <= 0.20
    assert (z["I0"] == -1).any()                                # some query is left with fewer than k passers
    last = len(z["hts"]) - 1
    assert z["stats%d" % last][2] == n and int(z["hts"][last]) == (int(z["M"]) + 1 if name.startswith("pq_polygen") else 8 * int(z["M"]) + 1)
