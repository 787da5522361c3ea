"""CPU: the numpy restatement of IndexIVFScalarQuantizer (tests/ivfsq_ref.py) reproduces every reference fixture of
tests/golden/ivfsq/ (tests/golden/make_golden_ivfsq.py) -- D bit for bit, the stored codes byte for byte, the trained range --
and the fixtures still hold the conditions the GPU tests rely on."""
import glob
import os
import re

import numpy as np
import pytest

import ivfsq_ref as sr
from ivfsq_cases import COARSE_INT, DIR, KWIDE, LONG, METRIC, NAMES, PAD_BITS, RAGGED, TIES, WITH_XB, bits, load


def test_every_fixture_is_listed():
    on_disk = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))
    assert on_disk == sorted(NAMES)
    for n in on_disk:
        assert os.path.getsize(os.path.join(DIR, n + ".npz")) <= 600000


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_fixture(name):
    z = load(name)
    metric, qtype, d = METRIC[int(z["metric"])], int(z["qtype"]), int(z["d"])
    assert z["codes"].shape == (z["ids"].shape[0], sr.code_size(d, qtype)) and z["codes"].dtype == np.uint8
    assert z["trained"].size == (2 if sr.is_uniform(qtype) else 2 * d) and (z["trained"][z["trained"].size // 2:] > 0).all()
    assert (z["keys"] >= 0).all()
    ks = [(int(z["k"]), "D", "I")] + [(int(m.group(1)), m.group(0), "I_k" + m.group(1)) for m in (re.match(r"D_k(\d+)$", f) for f in z) if m]
    for k, dn, inn in ks:
        D, I = sr.search_preassigned(z, z["xq"], z["keys"], z["cdis"], k, metric, qtype)
        assert np.array_equal(bits(D), bits(z[dn])), "%s k=%d" % (name, k)
        rows = np.ones(D.shape[0], bool)
        if name in TIES:
            rows = ~sr.tie_across_kth(z, z["xq"], z["keys"], z["cdis"], k, metric, qtype)
            assert (~rows).sum() * 2 <= rows.size
            assert sr.same_pairs(D, I, z[dn], z[inn], rows)
        else:
            assert np.array_equal(I, z[inn])
        assert (bits(z[dn])[z[inn] == -1] == PAD_BITS[metric]).all()


@pytest.mark.parametrize("name", WITH_XB)
def test_restatement_reproduces_codes_and_range(name):
    z = load(name)
    qtype, nlist, nt = int(z["qtype"]), int(z["nlist"]), int(z["nt"])
    lens = np.diff(z["list_offsets"])
    assign = np.empty(z["xb"].shape[0], np.int64)
    assign[z["ids"]] = np.repeat(np.arange(nlist), lens)
    res = (z["xb"] - z["coarse_centroids"][assign]).astype(np.float32)
    assert np.array_equal(sr.encode(res[z["ids"]], qtype, z["trained"]), z["codes"])
    assert np.array_equal(bits(sr.train(res[:nt], qtype)), bits(z["trained"]))
    comp = sr.components(z["codes"], int(z["d"]), qtype)
    assert (comp == 0).any() and (comp == (255 if sr.bits_of(qtype) == 8 else 15)).any()       # both clamps are met


@pytest.mark.parametrize("name", [n for n in NAMES if n not in TIES])
def test_fixture_discriminates_and_has_no_ties(name):
    z = load(name)
    metric, qtype = METRIC[int(z["metric"])], int(z["qtype"])
    assert sr.other_order_differs(z, z["xq"], z["keys"], z["cdis"], int(z["k"]), metric, qtype, z["D"]), "the other operation order reproduces D"
    assert not sr.tied_rows(z["D"], z["I"]).any()


@pytest.mark.parametrize("name", TIES)
def test_tie_fixture_has_ties(name):
    z = load(name)
    assert sr.tied_rows(z["D"], z["I"]).any()


def test_group_shapes():
    z = load(LONG[0])
    lens = np.diff(z["list_offsets"])
    kk = z["keys"][z["keys"] >= 0]
    assert lens.max() > 512 + 8 and (lens == 0).sum() >= 2 and (lens[kk] == 0).any() and (lens[kk] > 520).any()
    z = load(KWIDE[0])
    assert int(z["k"]) == 1024 and (z["I"] == -1).any(axis=1).all()
    assert (z["I_k100"] == -1).any(axis=1).any() and (z["I_k100"] != -1).all(axis=1).any()
    for n in RAGGED:
        z = load(n)
        assert int(z["d"]) % 8 == 0 and z["codes"].shape[1] % 16 != 0


@pytest.mark.parametrize("name", COARSE_INT)
def test_coarse_int_is_exact(name):
    """integer centroids and queries: the fixture's keys and coarse distances are the exact ones, whatever order sums them"""
    z = load(name)
    cent, xq, nprobe = z["coarse_centroids"], z["xq"], int(z["nprobe"])
    assert xq.shape[0] >= 20 and np.array_equal(cent, np.rint(cent)) and np.array_equal(xq, np.rint(xq))
    c64, q64 = cent.astype(np.int64), xq.astype(np.int64)
    ip = METRIC[int(z["metric"])] == "ip"
    score = q64 @ c64.T if ip else -((q64[:, None, :] - c64[None]) ** 2).sum(-1)
    srt = -np.sort(-score, axis=1)
    assert (np.diff(srt[:, :nprobe + 1], axis=1) != 0).all()
    exact = np.argsort(-score, axis=1, kind="stable")[:, :nprobe]
    assert np.array_equal(exact, z["keys"])
    want = np.take_along_axis(score, exact, axis=1)
    assert np.array_equal(z["cdis"].astype(np.int64), want if ip else -want)


def test_the_two_decodes_differ():
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 256, (64, 32)).astype(np.uint8)
    tr = np.concatenate([rng.standard_normal(32), 1 + rng.random(32)]).astype(np.float32)
    assert not np.array_equal(sr.decode(codes, 32, 0, tr, True), sr.decode(codes, 32, 0, tr, False))
    # 4 bits: component i is the low nibble of byte i / 2 for even i
    assert np.array_equal(sr.components(np.array([[0x21, 0x43]], np.uint8), 3, 1), [[1, 2, 3]])
