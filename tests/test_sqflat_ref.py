"""CPU: the numpy restatement of IndexScalarQuantizer (tests/sqflat_ref.py) reproduces every reference fixture of
tests/golden/sqflat/ (tests/golden/make_golden_sqflat.py) -- the sorted D bit for bit, the stored codes byte for byte, the trained
range and the decoded vectors bit for bit -- and the fixtures still hold the conditions the GPU tests rely on."""
import glob
import os

import numpy as np
import pytest

import ivfsq_ref as sr
import sqflat_ref as fr
from sqflat_cases import DIR, KWIDE, LONG, METRIC, NAMES, PAD_BITS, RAGGED, TIES, WITH_BYTES, WITH_XB, bits, distances, ks_of, load


def test_every_fixture_is_listed():
    on_disk = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))
    assert on_disk == sorted(NAMES)
    for n in on_disk:
        assert os.path.getsize(os.path.join(DIR, n + ".npz")) <= 600000


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_fixture(name):
    z = load(name)
    metric, qtype, d = METRIC[int(z["metric"])], int(z["qtype"]), int(z["d"])
    assert z["codes"].shape[1] == sr.code_size(d, qtype) and z["codes"].dtype == np.uint8
    assert z["trained"].size == (2 if sr.is_uniform(qtype) else 2 * d) and (z["trained"][z["trained"].size // 2:] > 0).all()
    dis = distances(name)
    for k, dn, inn in ks_of(z):
        D, I = fr.rows_of(dis, k, metric)
        Ds, Is = fr.sorted_rows(z[dn], z[inn], metric)
        assert np.array_equal(bits(D), bits(Ds)), "%s k=%d" % (name, k)
        rows = ~fr.tie_across_kth(dis, k, metric)
        if name in TIES:
            assert (~rows).any() and (~rows).sum() * 2 <= rows.size
        else:
            assert rows.all()
        assert np.array_equal(I[rows], Is[rows])
        assert (bits(z[dn])[z[inn] == -1] == PAD_BITS[metric]).all()


def test_the_reference_rows_are_in_heap_order():
    """what sorted_rows is for: the reference never reorders its heap in this search"""
    z = load("sqf_8bit_l2_d32")
    assert not np.array_equal(z["D"], np.sort(z["D"], axis=1))
    assert (z["D"][:, 0] == z["D"].max(axis=1)).all()        # a max-heap: the worst of the k on top


@pytest.mark.parametrize("name", WITH_XB)
def test_restatement_reproduces_codes_range_and_decode(name):
    z = load(name)
    qtype, nt, d = int(z["qtype"]), int(z["nt"]), int(z["d"])
    assert np.array_equal(sr.encode(z["xb"], qtype, z["trained"]), z["codes"])
    assert np.array_equal(bits(sr.train(z["xb"][:nt], qtype)), bits(z["trained"]))
    assert np.array_equal(bits(sr.decode_scalar(z["codes"], d, qtype, z["trained"])), bits(z["decoded"]))
    comp = sr.components(z["codes"], d, qtype)
    assert (comp == 0).any() and (comp == (255 if sr.bits_of(qtype) == 8 else 15)).any()       # both clamps are met


@pytest.mark.parametrize("name", [n for n in NAMES if n not in TIES])
def test_fixture_discriminates(name):
    z = load(name)
    metric, qtype, d, k = METRIC[int(z["metric"])], int(z["qtype"]), int(z["d"]), int(z["k"])
    other = fr.all_distances(z["codes"], z["xq"], metric, qtype, z["trained"], order8=(d % 8 != 0))
    assert not np.array_equal(bits(fr.rows_of(other, k, metric)[0]), bits(fr.sorted_rows(z["D"], z["I"], metric)[0])), "the other operation order reproduces D"
    if name not in KWIDE:
        assert not sr.tied_rows(z["D"], z["I"]).any()


@pytest.mark.parametrize("name", TIES)
def test_tie_fixture_has_ties(name):
    z = load(name)
    assert sr.tied_rows(z["D"], z["I"]).any()


def test_group_shapes():
    z = load(KWIDE[0])
    assert int(z["k"]) == 1024 and z["codes"].shape[0] == 800 and (z["I"] == -1).any(axis=1).all() and (z["I_k100"] != -1).all()
    assert load(LONG[0])["codes"].shape[0] > 2 * 1024
    for n in RAGGED:
        z = load(n)
        assert int(z["d"]) % 8 == 0 and z["codes"].shape[1] % 16 != 0
    for n in WITH_BYTES:
        assert load(n)["index_bytes"][:4].tobytes() == b"IxSQ"

