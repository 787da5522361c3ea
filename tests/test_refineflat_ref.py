"""CPU: the numpy restatement of IndexRefineFlat's seam (tests/refineflat_ref.py) against every fixture of
tests/golden/refineflat (the reference's IndexRefineFlat over its own base index, tests/golden/make_golden_refineflat.py):
sub_D bit for bit, D / I by assert_same_topk -- and the fixtures against the conditions the GPU tests rely on."""
import glob
import os

import numpy as np
import pytest

import refineflat_ref as rr
from util import GOLDEN, assert_same_topk

DIR = os.path.join(GOLDEN, "refineflat")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))
CASES = {"l2_ivfpq_d32", "ip_ivfflat_d32", "tail_d3_l2", "tail_d3_ip", "tail_d5_l2", "tail_d5_ip", "tail_d30_l2", "tail_d30_ip",
         "wide_d200_l2", "kbase_1024", "kfactor_1", "padded", "padded_ip", "ties"}
LARGEST_FIXTURE = 989774      # tests/golden/c1_small.npz


def load(name):
    z = np.load(os.path.join(DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def test_every_case_has_its_fixture():
    assert set(FIXTURES) == CASES
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(DIR, name + ".npz")) < LARGEST_FIXTURE


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_reference(name):
    z = load(name)
    k, metric = int(z["k"]), int(z["metric"])
    kb = rr.k_base(k, float(z["k_factor"]))
    assert z["base_I"].shape == (z["xq"].shape[0], kb) and z["D"].shape == (z["xq"].shape[0], k)
    sub = rr.compute_distance_subset(z["xb"], z["xq"], z["base_I"], z["base_D"], metric)
    assert rr.same_bits(sub, z["sub_D"])
    skipped = z["base_I"] < 0
    assert rr.same_bits(z["sub_D"][skipped], z["base_D"][skipped])          # the reference's `continue`
    D, I = rr.reorder(sub, z["base_I"], k, metric)
    loose = assert_same_topk(D, I, z["D"], z["I"], name)
    assert loose == 0 or name == "ties"


def test_fixture_conditions():
    for name in sorted(CASES):
        z = load(name)
        k, metric, kb = int(z["k"]), int(z["metric"]), z["base_I"].shape[1]
        m = min(k + 1, kb)
        Dm, Im = rr.reorder(z["sub_D"], z["base_I"], m, metric)
        equal = (Dm[:, 1:] == Dm[:, :-1]) & (Im[:, 1:] >= 0) & (Im[:, :-1] >= 0)
        nq = Dm.shape[0]
        if name == "ties":
            across = equal[:, k - 1]
            assert 1 <= across.sum() <= nq // 2
        else:
            assert not equal.any(), name
            assert (z["boundary_tie"] == 0).sum() * 4 >= 3 * nq
    assert rr.k_base(10, 4.0) == 40 and rr.k_base(5, 4.5) == 22 and rr.k_base(10, 1.0) == 10
    assert (load("padded")["base_I"] < 0).any() and (load("padded_ip")["base_D"] == -np.finfo(np.float32).max).any()
    assert not rr.same_bits(load("l2_ivfpq_d32")["sub_D"], load("l2_ivfpq_d32")["base_D"])       # re-scoring changes the L2 cases


def test_selection_order_is_distance_then_position():
    sub = np.array([[2.0, 1.0, 2.0, 1.0, 3.0]], np.float32)
    lab = np.array([[10, 11, -1, 13, 14]], np.int64)
    D, I = rr.reorder(sub, lab, 4, "l2")
    assert D.tolist() == [[1.0, 1.0, 2.0, 2.0]] and I.tolist() == [[11, 13, 10, -1]]
    D, I = rr.reorder(sub, lab, 3, "ip")
    assert D.tolist() == [[3.0, 2.0, 2.0]] and I.tolist() == [[14, 10, -1]]
