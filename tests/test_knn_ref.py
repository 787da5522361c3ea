"""CPU: the restatement of the flat exact k-NN search (tests/knn_ref.py) against the reference's own IndexFlatL2 / IndexFlatIP
rows (tests/golden/flatknn/*.npz, written by tests/golden/make_golden_flatknn.py), by the rule of each fixture kind:

  small, kwide  the reference's SSE paths: D and I bit for bit
  ties, int     D bit for bit, labels by tests/util.py's assert_same_topk rule (groups of exactly equal distance)
  blas          labels equal in every slot; every distance within 2 (d + 3) 2^-24 (|x|^2 + |y|^2) (L2) resp.
                (d + 1) 2^-23 |x| |y| (inner product) of the reference's, norms in float64: two summation orders of d products
                differ by at most 2 gamma_d sum |x_k y_k| <= 2 gamma_d |x| |y| <= gamma_d (|x|^2 + |y|^2), the two final roundings
                add at most 4u (|x|^2 + |y|^2), and the norms are the same bits on both sides
"""
import glob
import os

import numpy as np
import pytest

import knn_ref as kr
from util import assert_same_topk

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "flatknn", "*.npz")))
NAMES = [os.path.basename(f)[:-4] for f in FIXTURES]
METRICS = ("l2", "ip")


def load(name):
    z = dict(np.load(os.path.join(HERE, "golden", "flatknn", name + ".npz")))
    z["kind"] = str(z["kind"])
    return z


def bound(z, I, metric):
    d = int(z["d"])
    xn = (z["xq"].astype(np.float64) ** 2).sum(1)[:, None]
    yn = (z["xb"].astype(np.float64) ** 2).sum(1)[np.maximum(I, 0)]
    return 2 * (d + 3) * 2.0 ** -24 * (xn + yn) if metric == "l2" else (d + 1) * 2.0 ** -23 * np.sqrt(xn) * np.sqrt(yn)


def check_rows(z, D, I, metric, what):
    """rows D / I of some implementation of the stated semantics against fixture z"""
    Dr, Ir = z["D_" + metric], z["I_" + metric]
    if z["kind"] in ("small", "kwide"):
        assert kr.same_bits(D, Dr), "%s: distances differ bitwise" % what
        assert np.array_equal(I, Ir), "%s: labels differ" % what
    elif z["kind"] in ("ties", "int"):
        assert_same_topk(D, I, Dr, Ir, what)
    else:
        assert np.array_equal(I, Ir), "%s: labels differ" % what
        assert (np.abs(D.astype(np.float64) - Dr.astype(np.float64)) <= bound(z, Ir, metric)).all(), "%s: outside the rounding bound" % what


def test_every_kind_is_there():
    kinds = {load(n)["kind"] for n in NAMES}
    assert kinds == {"small", "kwide", "ties", "int", "blas"}
    assert len(NAMES) >= 17


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name, metric):
    z = load(name)
    D, I = kr.search(z["xq"], z["xb"], int(z["k"]), metric)
    check_rows(z, D, I, metric, "%s %s" % (name, metric))


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("small_d")])
def test_small_batch_inner_product_is_not_the_chain(name):
    """the fixtures tell the small-batch order (fvec_inner_product) from the GEMM path's fmaf chain"""
    z = load(name)
    Dc = kr.rows_from_matrix(kr.ip_chain(z["xq"], z["xb"]), int(z["k"]), True)[0]
    assert not kr.same_bits(Dc, z["D_ip"])


def test_fixture_paths_match_their_kind():
    for n in NAMES:
        z = load(n)
        assert kr.is_direct(z["xq"].shape[0], int(z["d"])) == (z["kind"] in ("small", "kwide", "ties")), n


def test_fma32_is_fmaf():
    import ctypes
    m = ctypes.CDLL("libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(7)
    n = 20000
    a = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 3, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 3, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 3, n)).astype(np.float32)
    c[::2] = (-a * b * (1 + 1e-4 * rng.standard_normal(n)).astype(np.float32))[::2]      # cancellation
    ref = np.array([m.fmaf(float(x), float(y), float(w)) for x, y, w in zip(a, b, c)], np.float32)
    assert kr.same_bits(kr.fma32(a, b, c), ref)
