"""GPU: vlq.GpuLSH (faiss::IndexLSH on the device: csrc/scan_hamming.hip, csrc/lsh_api.hip) on the fixtures of tests/golden/lsh/
(the reference's own codes, distances and labels) and against the restatement tests/lsh_ref.py.

Against a fixture: stored and query codes bit-equal, D bit-equal, I by tests/util.py's assert_same_topk; every returned label's
Hamming distance, recomputed from the fixture's codes, equals its D and the labels of a row are distinct -- which closes the
boundary group assert_same_topk leaves loose.  Against the restatement: D and I equal in every slot."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import lsh_ref as lr
import refineflat_ref as rr
import vector_line_quantization_amd as vlq
from util import assert_same_topk, bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "lsh")
NAMES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(DIR, "*.npz")))
_CACHE = {}


def load(name):
    if name not in _CACHE:
        z = dict(np.load(os.path.join(DIR, name + ".npz")))
        for nm in ("d", "nbits", "k", "rotate", "thresh", "threw"):
            z[nm] = int(z[nm])
        z["kind"] = str(z["kind"])
        z.setdefault("A", None)
        z.setdefault("thresholds", None)
        if not z["threw"]:
            z["Dn"], z["In"] = lr.search_codes(z["qcodes"], z["codes"], z["k"])
        for v in z.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = z
    return _CACHE[name]


def index_of(z, thresholds=True):
    g = vlq.GpuLSH(z["d"], z["nbits"], rotate_data=bool(z["rotate"]), train_thresholds=bool(z["thresh"]), device=0)
    if z["rotate"]:
        g.set_rotation(z["A"])
    if z["thresh"] and thresholds:
        g.set_thresholds(z["thresholds"])
    return g


def same(D, I, Dn, In, what):
    assert np.array_equal(bits(D), bits(Dn)), "%s: distances differ" % (what,)
    assert np.array_equal(I, In), "%s: labels differ" % (what,)


def test_fixtures_present():
    assert len(NAMES) >= 21 and "unserved" in NAMES and "kwide" in NAMES


@pytest.mark.parametrize("pieces", (1, 3))
@pytest.mark.parametrize("name", NAMES)
def test_fixture(name, pieces):
    z = load(name)
    g = index_of(z)
    try:
        nb = z["xb"].shape[0]
        cuts = [0, nb] if pieces == 1 else [0, nb // 7, nb // 7 + (2 * nb) // 5, nb]
        for a, b in zip(cuts[:-1], cuts[1:]):
            g.add(z["xb"][a:b])
        assert g.ntotal == nb
        assert np.array_equal(g.get_codes(), z["codes"]), "stored codes"
        assert np.array_equal(g.encode(z["xq"]), z["qcodes"]), "query codes"
        if z["threw"]:
            with pytest.raises(vlq.VlqError) as e:
                g.search(z["xq"], z["k"])
            assert e.value.code == 1 and "%d bytes" % z["codes"].shape[1] in str(e.value)
            return
        D, I = g.search(z["xq"], z["k"])
        assert_same_topk(D, I, z["D"], z["I"], name)
        lr.check_labels(D, I, z["qcodes"], z["codes"])
        same(D, I, z["Dn"], z["In"], name + " vs restatement")
    finally:
        g.close()


@pytest.mark.parametrize("name", [n for n in NAMES if "thresh" in n or n == "rot_int"])
def test_train(name):
    z = load(name)
    g = index_of(z, thresholds=False)
    try:
        with pytest.raises(vlq.VlqError) as e:
            g.add(z["xb"])
        assert e.value.code == 1 and "not trained" in str(e.value)
        xt = g.apply(z["xt"])
        assert np.array_equal(bits(xt), bits(lr.apply(z["xt"], z["nbits"], z["A"])))
        t = g.train(z["xt"])
        assert g.is_trained
        assert np.array_equal(bits(t), bits(lr.train(z["xt"], z["nbits"], z["A"])))
        if z["kind"] in ("thresh", "rot_int"):
            assert np.array_equal(bits(t), bits(z["thresholds"]))
        else:       # tests/golden/make_golden_lsh.py: the median moves by at most the largest perturbation of a value
            bound = (z["d"] + 2) * 2.0 ** -23 * np.sqrt((z["A"].astype(np.float64) ** 2).sum(1)) * np.abs(z["xt"]).max()
            assert (np.abs(t.astype(np.float64) - z["thresholds"].astype(np.float64)) <= bound).all()
        # with thresholds set, apply subtracts them
        xs = g.apply(z["xq"])
        assert np.array_equal(bits(xs), bits(lr.apply(z["xq"], z["nbits"], z["A"], None, t)))
    finally:
        g.close()


@pytest.mark.parametrize("name", ["rot_64_32", "rot_16_64", "plain", "prefix"])
def test_apply(name):
    z = load(name)
    g = index_of(z)
    try:
        assert np.array_equal(bits(g.apply(z["xb"])), bits(lr.apply(z["xb"], z["nbits"], z["A"])))
    finally:
        g.close()


def test_rotation_bias():
    z = load("rot_16_64")
    b = np.linspace(-0.5, 0.5, z["nbits"]).astype(np.float32)
    g = index_of(z)
    try:
        g.set_rotation(z["A"], b)
        assert np.array_equal(bits(g.apply(z["xq"])), bits(lr.apply(z["xq"], z["nbits"], z["A"], b)))
        assert np.array_equal(g.encode(z["xq"]), lr.encode(z["xq"], z["nbits"], z["A"], b))
    finally:
        g.close()


@pytest.mark.parametrize("name", ["rot_int", "width_192", "ties"])
def test_search_codes_and_add_codes(name):
    import torch
    z = load(name)
    g, g2 = index_of(z), index_of(z)
    try:
        g.add(z["xb"])
        D, I = g.search(z["xq"], z["k"])
        Dc, Ic = g.search_codes(z["qcodes"], z["k"])
        same(Dc, Ic, D, I, "search_codes")
        g2.add_codes(z["codes"][:100])
        g2.add_codes(z["codes"][100:])
        assert np.array_equal(g2.get_codes(), z["codes"])
        D2, I2 = g2.search(z["xq"], z["k"])
        same(D2, I2, D, I, "add_codes")
        # device tensors in and out
        xq = torch.as_tensor(np.array(z["xq"])).cuda()
        torch.cuda.synchronize()
        Dt, It = g.search(xq, z["k"])
        assert Dt.is_cuda and It.is_cuda
        g.last_scan_info()          # synchronises the index's stream
        same(Dt.cpu().numpy(), It.cpu().numpy(), D, I, "torch")
        qc = torch.as_tensor(np.array(z["qcodes"])).cuda()
        torch.cuda.synchronize()
        Dt, It = g.search_codes(qc, z["k"])
        g.last_scan_info()
        same(Dt.cpu().numpy(), It.cpu().numpy(), D, I, "torch codes")
    finally:
        g.close()
        g2.close()


def test_default_rotation_is_a_rotation():
    A = vlq.random_rotation(24, 16, seed=5)
    assert A.shape == (16, 24) and A.dtype == np.float32
    assert np.allclose(A @ A.T, np.eye(16), atol=1e-5)
    A2 = vlq.random_rotation(8, 16, seed=5)
    assert np.allclose(A2.T @ A2, np.eye(8), atol=1e-5)
    assert np.array_equal(A, vlq.random_rotation(24, 16, seed=5))
    x = np.random.default_rng(3).standard_normal((50, 24)).astype(np.float32)
    g = vlq.GpuLSH(24, 16)
    try:
        assert np.array_equal(g.encode(x), lr.encode(x, 16, A))
    finally:
        g.close()


def test_empty_reset_and_readd():
    z = load("width_64")
    g = index_of(z)
    try:
        D, I = g.search(z["xq"], 7)
        assert (I == -1).all() and (bits(D) == 0x4F000000).all()
        g.add(z["xb"])
        g.reserve_memory(5000)
        assert np.array_equal(g.get_codes(), z["codes"])
        g.reset()
        assert g.ntotal == 0
        D, I = g.search(z["xq"], 7)
        assert (I == -1).all() and (bits(D) == 0x4F000000).all()
        perm = np.random.default_rng(5).permutation(z["xb"].shape[0])
        g.add(z["xb"][perm])
        assert np.array_equal(g.get_codes(), z["codes"][perm])
        D, I = g.search(z["xq"], z["k"])
        same(D, I, *lr.search_codes(z["qcodes"], z["codes"][perm], z["k"]), "re-added")
    finally:
        g.close()


def test_errors():
    z = load("width_64")
    g = index_of(z)
    try:
        g.add(z["xb"])
        with pytest.raises(vlq.VlqError) as e:
            g.search(z["xq"], 0)
        assert e.value.code == 1 and "k=0" in str(e.value)
        with pytest.raises(vlq.VlqError) as e:
            g.search(z["xq"], 1025)
        assert "1025" in str(e.value)
        with pytest.raises(vlq.VlqError) as e:
            g.search_codes(z["qcodes"], 1025)
        assert "1025" in str(e.value)
        with pytest.raises(vlq.VlqError):
            g.scan_split(3, 0)
        with pytest.raises(vlq.VlqError):
            g.scan_split(0, 65)
        with pytest.raises(vlq.VlqError):
            g.get_codes(0, g.ntotal + 1)
        with pytest.raises(vlq.VlqError):
            g.set_rotation(np.zeros((64, 64), np.float32))      # created without rotate_data
        with pytest.raises(vlq.VlqError):
            g.set_thresholds(np.zeros(64, np.float32))          # created without train_thresholds
    finally:
        g.close()
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuLSH(16, 32, rotate_data=False)
    assert e.value.code == 1 and "d=16 < nbits=32" in str(e.value)
    # nbits = 100: 13 bytes are stored, not searched
    u = load("unserved")
    g = index_of(u)
    try:
        g.add(u["xb"])
        assert np.array_equal(g.get_codes(), u["codes"])
        with pytest.raises(vlq.VlqError) as e:
            g.search_codes(u["qcodes"], 3)
        assert e.value.code == 1 and "13 bytes" in str(e.value)
    finally:
        g.close()
    # thresholds not set yet
    g = vlq.GpuLSH(32, 32, rotate_data=False, train_thresholds=True)
    try:
        assert not g.is_trained
        for call in (lambda: g.add(z["xb"][:, :32]), lambda: g.search(z["xq"][:, :32], 3), lambda: g.encode(z["xq"][:, :32])):
            with pytest.raises(vlq.VlqError) as e:
                call()
            assert e.value.code == 1 and "not trained" in str(e.value)
    finally:
        g.close()
    # a rotate_data handle of the C ABI has no matrix until vlq_lsh_set_rotation (vlq.GpuLSH sets one in its constructor)
    L = vlq.lib()
    h = C.c_void_p()
    assert L.vlq_lsh_create(C.byref(h), 0, 32, 32, 1, 0) == 0
    try:
        x = np.zeros((2, 32), np.float32)
        D, I = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int64)
        px, pD, pI = (a.ctypes.data_as(C.c_void_p) for a in (x, D, I))
        assert L.vlq_lsh_search(h, C.c_int64(2), px, 3, pD, pI) == 1 and b"not trained" in L.vlq_last_error()
        assert L.vlq_lsh_add(h, C.c_int64(2), px) == 1 and b"not trained" in L.vlq_last_error()
    finally:
        L.vlq_lsh_destroy(h)


@pytest.mark.parametrize("name", ["rot_64_32"])
def test_refine_flat_over_lsh(name):
    z = load(name)
    k, kf = 5, 4.0
    base = index_of(z)
    r = vlq.GpuRefineFlat(base)
    try:
        r.k_factor = kf
        r.add(z["xb"][:150])
        r.add(z["xb"][150:])
        assert r.ntotal == base.ntotal == z["xb"].shape[0]
        D, I = r.search(np.array(z["xq"]), k)
        kb = rr.k_base(k, kf)
        bD, bI = lr.search_codes(z["qcodes"], z["codes"], kb)
        Dn, In = rr.refine(z["xb"], z["xq"], bD, bI, k, "l2")
        same(D, I, Dn, In, "refined")
    finally:
        base.close()
        r.store.close()
