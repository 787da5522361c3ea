"""CPU: the restatement of the flat index's range search (tests/knn_range_ref.py) against the reference's own
IndexFlat::range_search (tests/golden/flatrange/*.npz, written by tests/golden/make_golden_flatrange.py over the data of the
flat k-NN fixtures), by the rule of each fixture kind:

  small, kwide, ties, int   lims, the bits of D, and I element for element
  blas                      lims and I element for element (the radii sit in gaps wider than twice the rounding bound, so the hit
                            set is the same under any summation order); every D within 2 (d + 3) 2^-24 (|x|^2 + |y|^2) (L2)
                            resp. (d + 1) 2^-23 |x| |y| (inner product) of the reference's: the bound of tests/test_knn_ref.py
  all, none                 lims only
"""
import functools
import glob
import os

import numpy as np
import pytest

import knn_range_ref as rr
from test_knn_ref import load as load_knn

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "flatrange", "*.npz")))
NAMES = [os.path.basename(f)[:-4] for f in FIXTURES]
METRICS = ("l2", "ip")
LIMS_ONLY = ("all", "none")


@functools.lru_cache(maxsize=None)
def load(name):
    """the range fixture with its source's vectors: xb, xq, d beside the radii and the reference's results"""
    z = dict(np.load(os.path.join(HERE, "golden", "flatrange", name + ".npz")))
    src = load_knn(str(z["src"]))
    z.update(xb=src["xb"], xq=src["xq"], d=int(src["d"]), kind=str(z["kind"]), names=[str(n) for n in z["names"]])
    for a in z.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return z


def radius(z, metric, nm):
    return z["radii_" + metric][z["names"].index(nm)]


def pair_bound(z, lims, I, metric):
    d = z["d"]
    q = np.repeat(np.arange(z["xq"].shape[0]), np.diff(lims))
    xn = (z["xq"].astype(np.float64) ** 2).sum(1)[q]
    yn = (z["xb"].astype(np.float64) ** 2).sum(1)[I]
    return 2 * (d + 3) * 2.0 ** -24 * (xn + yn) if metric == "l2" else (d + 1) * 2.0 ** -23 * np.sqrt(xn) * np.sqrt(yn)


def check_result(z, metric, nm, lims, D, I, what):
    """(lims, D, I) of some implementation of the stated semantics against fixture z at the radius named nm"""
    lr = z["lims_%s_%s" % (metric, nm)]
    assert np.array_equal(lims, lr), "%s: lims differ" % what
    assert D.shape == I.shape == (int(lr[-1]),), "%s: %s / %s results for %d hits" % (what, D.shape, I.shape, lr[-1])
    if nm in LIMS_ONLY:
        return
    Dr, Ir = z["D_%s_%s" % (metric, nm)], z["I_%s_%s" % (metric, nm)]
    assert np.array_equal(I, Ir), "%s: labels differ" % what
    if z["kind"] != "blas":
        assert rr.same_bits(D, Dr), "%s: distances differ bitwise" % what
    else:
        assert (np.abs(D.astype(np.float64) - Dr.astype(np.float64)) <= pair_bound(z, lr, Ir, metric)).all(), "%s: outside the rounding bound" % what


def test_every_source_has_its_fixture():
    from test_knn_ref import NAMES as KNN_NAMES
    assert NAMES == KNN_NAMES and len(NAMES) >= 17
    for n in NAMES:
        z = load(n)
        assert str(z["src"]) == n
        assert z["names"] == (["tight", "wide", "all", "none"] if z["kind"] == "blas" else ["tight", "tight_next", "wide", "all", "none"])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name, metric):
    z = load(name)
    mat = rr.matrix(z["xq"], z["xb"], metric)
    for nm in z["names"]:
        lims, D, I = rr.from_matrix(mat, radius(z, metric, nm), metric)
        check_result(z, metric, nm, lims, D, I, "%s %s %s" % (name, metric, nm))
        for a, b in zip(lims[:-1], lims[1:]):
            assert (np.diff(I[a:b]) > 0).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("blas")])
def test_fixture_radii_discriminate(name, metric):
    """tight_next admits exactly the pairs at `tight` (the strict test), wide more, all everything, none nothing"""
    z = load(name)
    mat = rr.matrix(z["xq"], z["xb"], metric)
    n = {nm: int(z["lims_%s_%s" % (metric, nm)][-1]) for nm in z["names"]}
    assert n["tight_next"] - n["tight"] == (mat == radius(z, metric, "tight")).sum() > 0
    assert n["none"] == 0 < n["tight"] < n["tight_next"] <= n["wide"] <= n["all"] == mat.size


def test_duplicates_come_back_twice_in_position_order():
    z = load("small_ties")
    lims, D, I = rr.range_search(z["xq"], np.concatenate([z["xb"], z["xb"]]), radius(z, "l2", "tight"), "l2")
    nb = z["xb"].shape[0]
    for a, b in zip(lims[:-1], lims[1:]):
        h = (b - a) // 2
        assert (b - a) % 2 == 0 and np.array_equal(I[a:a + h] + nb, I[a + h:b]) and rr.same_bits(D[a:a + h], D[a + h:b])


def test_nan_and_infinite_radii():
    z = load("small_d32_nq19")
    for metric in METRICS:
        mat = rr.matrix(z["xq"], z["xb"], metric)
        assert rr.from_matrix(mat, np.nan, metric)[0][-1] == 0
        inf_all = -np.inf if metric == "ip" else np.inf
        assert rr.from_matrix(mat, inf_all, metric)[0][-1] == mat.size
        assert rr.from_matrix(mat, -inf_all, metric)[0][-1] == 0
