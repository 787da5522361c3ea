"""CPU: the numpy restatement of the inner-product rules (tests/ip_ref.py, the text of include/vlq_ivfpq.h under
vlq_ivfpq_set_metric) reproduces every reference fixture -- D bit for bit, I up to the order inside groups of exactly equal
distance -- so the fixtures are held to the written specification without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ip_ref  # noqa: E402
from util import GOLDEN, assert_same_topk  # noqa: E402

CASES = ["ip_residual", "ip_nonresidual", "ip_m16_d128", "ip_padding_ties", "ip_kwide", "ip_m20_d40", "ip_d30_m6",
         "ip_m24_d48"]


def load(name):
    z = np.load(os.path.join(GOLDEN, "ip", name + ".npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", CASES)
def test_scan_restatement(name):
    z = load(name)
    k = int(z["k"])
    D, I, nc = ip_ref.search_preassigned(z, z["xq"], z["keys"], k)
    assert_same_topk(D, I, z["D"], z["I"], name)
    Dp, Ip, _ = ip_ref.search_preassigned(z, z["xq"], z["keys"], k, store_pairs=True)
    assert_same_topk(Dp, Ip, z["D"], z["I_pairs"], name + " pairs")
    assert np.array_equal(nc, z["ncode"])
    # descending inner products, -FLT_MAX / -1 padding with the sign bit set
    assert (z["D"][:, :-1] >= z["D"][:, 1:]).all()
    pad = z["I"] == -1
    assert (z["D"][pad].view(np.uint32) == np.float32(-ip_ref.FLT_MAX).view(np.uint32)).all()


def test_padding_case_has_what_it_is_for():
    z = load("ip_padding_ties")
    assert (z["keys"] == -1).any() and (z["I"] == -1).any() and int(z["max_codes"]) > 0
    lens = np.diff(z["list_offsets"])
    full = np.array([lens[kq[kq >= 0]].sum() for kq in z["keys"]])
    assert (z["ncode"] < full).any(), "no max_codes cut inside a probe list"


@pytest.mark.parametrize("name", ["ip_residual", "ip_nonresidual", "ip_m16_d128", "ip_d30_m6"])
def test_quantizer_search_restatement(name):
    """The index's own quantizer->search (float centroids: the reference's BLAS order is not restated): the keys are the
    largest inner products in float64 wherever the decision is not within rounding."""
    z = load(name)
    keys = z["keys"]
    ip = z["xq"].astype(np.float64) @ z["coarse_centroids"].astype(np.float64).T
    got = np.where(keys >= 0, np.take_along_axis(ip, np.maximum(keys, 0), axis=1), np.nan)
    assert np.allclose(got[keys >= 0], z["coarse_dis"][keys >= 0], rtol=1e-5, atol=1e-2)
    assert (np.diff(z["coarse_dis"], axis=1) <= 0).all()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_coarse_restatement(tag):
    z = load("ip_coarse_int")
    nprobe = int(z[tag + "_nprobe"])
    keys, dis = ip_ref.coarse_search(z[tag + "_cent"], z[tag + "_xq"], nprobe)
    assert np.array_equal(keys, z[tag + "_keys"])
    assert np.array_equal(dis.view(np.uint32), z[tag + "_dis"].view(np.uint32))
    exact = z[tag + "_xq"].astype(np.int64) @ z[tag + "_cent"].astype(np.int64).T
    srt = -np.sort(-exact, axis=1)
    tie = srt[:, nprobe - 1] == srt[:, nprobe]
    assert tie.sum() >= 2, "no boundary tie in the fixture"
    for r in np.nonzero(tie)[0]:          # the lower id stays
        v = srt[r, nprobe - 1]
        assert keys[r, nprobe - 1] == np.nonzero(exact[r] == v)[0][0]


@pytest.mark.parametrize("name", CASES)
def test_assignment_is_first_maximum(name):
    z = load(name)
    ip = z["enc_x"].astype(np.float64) @ z["coarse_centroids"].astype(np.float64).T
    assert np.array_equal(np.argmax(ip, axis=1), z["enc_assign"])
