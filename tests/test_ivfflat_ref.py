"""CPU: the numpy restatement of IndexIVFFlat's search (tests/ivfflat_ref.py) reproduces every reference fixture of
tests/golden/ivfflat/ (tests/golden/make_golden_ivfflat.py), the fixtures still hold the conditions the GPU tests rely on,
and the scan's launch decision (csrc/flat_plan.h) is what the header documents."""
import glob
import os
import re

import numpy as np
import pytest

import ivfflat_ref as fr
from util import GOLDEN, assert_same_topk

DIR = os.path.join(GOLDEN, "ivfflat")
NAMES = ["flat_l2_d32", "flat_ip_d32", "flat_l2_d128_long", "flat_tail_d30_l2", "flat_tail_d30_ip", "flat_tail_d5_l2",
         "flat_tail_d5_ip", "flat_tail_d3_l2", "flat_tail_d3_ip", "flat_padding_ties_l2", "flat_padding_ties_ip", "flat_kwide",
         "flat_ragged_d36_l2", "flat_ragged_d100_ip"]
METRIC = {0: "ip", 1: "l2"}


def load(name):
    z = np.load(os.path.join(DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def test_every_fixture_is_listed():
    on_disk = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))
    assert on_disk == sorted(NAMES + ["flat_coarse_int"])
    for n in on_disk:
        assert os.path.getsize(os.path.join(DIR, n + ".npz")) <= 1000000


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_fixture(name):
    z = load(name)
    metric = METRIC[int(z["metric"])]
    ks = [(int(z["k"]), "D", "I")] + [(int(m.group(1)), m.group(0), "I_k" + m.group(1)) for m in (re.match(r"D_k(\d+)$", f) for f in z) if m]
    for k, dn, inn in ks:
        D, I, nv, nd = fr.search_preassigned(z, z["xq"], z["keys"], k, metric)
        loose = assert_same_topk(D, I, z[dn], z[inn], "%s k=%d" % (name, k))
        assert loose == 0 or "ties" in name
    assert np.array_equal(nd, z["ndis"]) and np.array_equal(nv, z["nlistv"])


@pytest.mark.parametrize("name", [n for n in NAMES if "ties" not in n])
def test_fixture_discriminates_and_has_no_ties(name):
    z = load(name)
    metric = METRIC[int(z["metric"])]
    if int(z["d"]) >= 4:        # (for d < 4 the two orders are one expression: (x0 + x1) + (x2 + 0))
        assert fr.discriminates(z, z["xq"], z["keys"], int(z["k"]), metric, z["D"]), "a plain left-to-right sum reproduces D"
    for r in range(z["D"].shape[0]):
        v = z["D"][r][z["I"][r] != -1]
        assert np.unique(v).size == v.size, "row %d holds a tie" % r


@pytest.mark.parametrize("name", ["flat_padding_ties_l2", "flat_padding_ties_ip"])
def test_tie_fixture_stays_checkable(name):
    z = load(name)
    k = int(z["k"])
    Dk1, Ik1, _v, _n = fr.search_preassigned(z, z["xq"], z["keys"], k + 1, METRIC[int(z["metric"])])
    across = (Dk1[:, k] == Dk1[:, k - 1]) & (Ik1[:, k] != -1)
    assert across.any() and (~across).sum() * 3 >= across.size
    assert ((z["I"] == -1).any(axis=1) & (z["I"] != -1).any(axis=1)).any() and (z["I"] == -1).all(axis=1).any()
    assert (z["keys"] == -1).any()


def test_long_list_fixture_shape():
    z = load("flat_l2_d128_long")
    lens = np.diff(z["list_offsets"])
    kk = z["keys"][z["keys"] >= 0]
    assert lens.max() >= 520 and (lens == 0).sum() >= 2
    assert (lens[kk] == 0).any() and (lens[kk] >= 520).any()


@pytest.mark.parametrize("name", ["flat_ragged_d36_l2", "flat_ragged_d100_ip"])
def test_ragged_fixture_shape(name):
    z = load(name)
    d, lens = int(z["d"]), np.diff(z["list_offsets"])
    assert d > 32 and d % 32 != 0 and d % 4 == 0          # the tile path with a partial last piece
    assert (lens[z["keys"][z["keys"] >= 0]] > 520).any()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_coarse_int_is_exact(metric):
    z = load("flat_coarse_int")
    p = metric + "_"
    zz = {nm[len(p):]: v for nm, v in z.items() if nm.startswith(p)}
    k, ns = int(z["k"]), int(z["n_small"])
    assert zz["xq"].shape[0] >= 20 > ns > 0
    for a in (zz["coarse_centroids"], zz["vecs"], zz["xq"]):
        assert np.array_equal(a, np.rint(a))
    D, I, _v, _n = fr.search_preassigned(zz, zz["xq"], zz["keys"], k, metric)
    assert assert_same_topk(D, I, zz["D"], zz["I"], metric) == 0
    # the reference's whole search, from a batch on its BLAS path and from one below it, is the preassigned search of these keys
    assert assert_same_topk(zz["Ds"], zz["Is"], zz["D"], zz["I"], metric) == 0
    assert assert_same_topk(zz["Ds_small"], zz["Is_small"], zz["D"][:ns], zz["I"][:ns], metric) == 0


def test_plain_order_differs_from_sse_order():
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((64, 32)).astype(np.float32), rng.standard_normal((64, 32)).astype(np.float32)
    assert not np.array_equal(fr.l2_sse(x, y), fr.l2_plain(x, y))
    assert not np.array_equal(fr.ip_sse(x, y), fr.ip_plain(x, y))
    x3, y3 = x[:, :3], y[:, :3]
    assert np.array_equal(fr.l2_sse(x3, y3), fr.l2_plain(x3, y3))
