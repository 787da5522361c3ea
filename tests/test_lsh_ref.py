"""CPU: the restatement of faiss::IndexLSH (tests/lsh_ref.py) reproduces every fixture of tests/golden/lsh/ by its kind's rule
(tests/golden/make_golden_lsh.py), and the fixture set is complete."""
import glob
import os

import numpy as np
import pytest

import lsh_ref as lr
from util import assert_same_topk

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "lsh")
NAMES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(DIR, "*.npz")))
KINDS = {"plain", "prefix", "thresh", "rot_int", "rot", "rot_thresh", "ties", "kwide", "width", "unserved"}
WIDTHS = {32: 4, 60: 8, 64: 8, 128: 16, 192: 24, 256: 32, 320: 40, 512: 64, 1024: 128}


def load(name):
    z = dict(np.load(os.path.join(DIR, name + ".npz")))
    for nm in ("d", "nbits", "k", "rotate", "thresh", "threw"):
        z[nm] = int(z[nm])
    z["kind"] = str(z["kind"])
    z.setdefault("A", None)
    z.setdefault("thresholds", None)
    return z


def test_every_kind_and_width_is_present():
    zs = {n: load(n) for n in NAMES}
    assert {z["kind"] for z in zs.values()} == KINDS
    for nbits, nbytes in WIDTHS.items():
        z = zs["width_%d" % nbits]
        assert z["nbits"] == nbits and z["codes"].shape[1] == nbytes and z["kind"] == "width"
    assert {z["xt"].shape[0] % 2 for z in zs.values() if z["kind"] == "thresh"} == {0, 1}
    rot = [z for z in zs.values() if z["kind"] == "rot"]
    assert any(z["nbits"] <= z["d"] for z in rot) and any(z["nbits"] > z["d"] for z in rot)
    assert any(z["kind"] == "rot_thresh" for z in zs.values())
    assert sum(os.path.getsize(p) for p in glob.glob(os.path.join(DIR, "*.npz"))) < 2.1 * 2 ** 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_fixture(name):
    z = load(name)
    assert (z["A"] is not None) == bool(z["rotate"]) and (z["thresholds"] is not None) == bool(z["thresh"])
    codes = lr.encode(z["xb"], z["nbits"], z["A"], None, z["thresholds"])
    qcodes = lr.encode(z["xq"], z["nbits"], z["A"], None, z["thresholds"])
    assert np.array_equal(codes, z["codes"]) and np.array_equal(qcodes, z["qcodes"])
    assert codes.shape[1] == (z["nbits"] + 7) // 8
    if z["nbits"] % 8:
        assert (codes[:, -1] >> (z["nbits"] % 8) == 0).all(), "pad bits"
    if z["kind"] == "unserved":
        assert z["threw"] == 1 and not lr.served(codes.shape[1]) and "D" not in z
        return
    assert z["threw"] == 0 and lr.served(codes.shape[1])
    D, I = lr.search_codes(qcodes, codes, z["k"])
    assert_same_topk(D, I, z["D"], z["I"], name)
    lr.check_labels(z["D"], z["I"], z["qcodes"], z["codes"])
    lr.check_labels(D, I, qcodes, codes)


@pytest.mark.parametrize("name", [n for n in NAMES if load(n)["thresh"]])
def test_restatement_trains_fixture_thresholds(name):
    z = load(name)
    t = lr.train(z["xt"], z["nbits"], z["A"])
    if z["kind"] in ("thresh", "rot_int"):
        assert np.array_equal(t.view(np.uint32), z["thresholds"].view(np.uint32))
    else:       # make_golden_lsh.py: the median moves by at most the largest perturbation of a value
        d = z["d"]
        bound = (d + 2) * 2.0 ** -23 * np.sqrt((z["A"].astype(np.float64) ** 2).sum(1)) * np.abs(z["xt"]).max()
        assert (np.abs(t.astype(np.float64) - z["thresholds"].astype(np.float64)) <= bound).all()


def test_planted_zeros_set_their_bits():
    z = load("plain")
    for x, c in ((z["xb"], z["codes"]), (z["xq"], z["qcodes"])):
        planted = [(5, 3), (6, 4), (7, 0), (8, 31)]
        assert [float(x[r, j]) for r, j in planted] == [0.0] * 4
        assert np.signbit(x[6, 4]) and np.signbit(x[7, 0]) and not np.signbit(x[5, 3])
        for r, j in planted:
            assert (c[r, j // 8] >> (j % 8)) & 1
    nan = np.full((1, 8), np.nan, np.float32)
    assert lr.bits(nan)[0, 0] == 0


def test_ties_and_kwide_conditions():
    z = load("ties")
    D1, I1 = lr.search_codes(z["qcodes"], z["codes"], z["k"] + 1)
    assert ((D1[:, z["k"]] == D1[:, z["k"] - 1]) & (I1[:, z["k"]] != -1)).any()
    z = load("kwide")
    nb = z["xb"].shape[0]
    assert z["k"] > nb and (z["I"][:, nb:] == -1).all() and (z["D"][:, nb:].view(np.uint32) == 0x4F000000).all()
