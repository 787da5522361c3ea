"""The fixtures of tests/golden/sqflat/ (tests/golden/make_golden_sqflat.py) by group, their loader and the row comparison the
GPU tests share.  TEST INFRASTRUCTURE ONLY."""
import functools
import os
import re

import numpy as np

import sqflat_ref as fr
from util import GOLDEN

DIR = os.path.join(GOLDEN, "sqflat")
QT = ("8bit", "4bit", "8bit_uniform", "4bit_uniform")
METRIC = {0: "ip", 1: "l2"}
D32 = ["sqf_%s_%s_d32" % (qt, m) for qt in QT for m in ("ip", "l2")]
D128 = ["sqf_%s_%s_d128" % (qt, m) for qt in ("8bit", "4bit") for m in ("ip", "l2")]
SCALAR = ["sqf_%s_%s_d%d" % (qt, m, d) for qt in ("8bit", "4bit") for m in ("ip", "l2") for d in (30, 33)]
RAGGED = ["sqf_8bit_l2_d40", "sqf_4bit_ip_d48"]
TINY = ["sqf_8bit_l2_d8", "sqf_8bit_l2_d5"]
KWIDE = ["sqf_8bit_l2_d32_kwide"]
TIES = ["sqf_ties_8bit_l2", "sqf_ties_4bit_ip"]
LONG = ["sqf_8bit_l2_d32_long"]
NAMES = D32 + D128 + SCALAR + RAGGED + TINY + KWIDE + TIES + LONG
WITH_XB = D32 + SCALAR + TINY                              # fixtures that hold the added vectors and their decode
WITH_BYTES = ["sqf_8bit_l2_d32", "sqf_4bit_ip_d33"]        # ... and the bytes write_index wrote
FLT_MAX = np.float32(np.finfo(np.float32).max)
PAD_BITS = {"l2": FLT_MAX.view(np.uint32), "ip": np.float32(-FLT_MAX).view(np.uint32)}


def load(name):
    z = np.load(os.path.join(DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ks_of(z):
    """[(k, name of D, name of I)] of a fixture: its own k and every D_k<n> / I_k<n> beside it"""
    return [(int(z["k"]), "D", "I")] + [(int(m.group(1)), m.group(0), "I_k" + m.group(1)) for m in (re.match(r"D_k(\d+)$", f) for f in z) if m]


@functools.lru_cache(maxsize=None)
def distances(name):
    """the restatement's distances [nq][ntotal] of a fixture, computed once and shared (read only)"""
    z = load(name)
    dis = fr.all_distances(z["codes"], z["xq"], METRIC[int(z["metric"])], int(z["qtype"]), z["trained"])
    dis.setflags(write=False)
    return dis


def check_rows(D, I, Dref, Iref, dis, metric, what=""):
    """The library's rows D / I against a reference's rows Dref / Iref (heap order) and the restatement's distances dis
    [nq][ntotal] of the same queries: D bit-equal to the sorted reference rows; I equal in every row with no tie across the k-th
    place; in a row with such a tie the labels are distinct and below ntotal, each carries its slot's distance under the
    restatement, and the labels of the groups that lie wholly inside the row equal the reference's sets."""
    k, ntotal = D.shape[1], dis.shape[1]
    Ds, Is = fr.sorted_rows(Dref, Iref, metric)
    assert np.array_equal(bits(D), bits(Ds)), what
    across = fr.tie_across_kth(dis, k, metric)
    assert np.array_equal(I[~across], Is[~across]), what
    for r in np.nonzero(across)[0]:
        lab = I[r]
        assert (lab >= 0).all() and (lab < ntotal).all() and np.unique(lab).size == k, (what, r)
        assert np.array_equal(bits(dis[r][lab]), bits(D[r])), (what, r)
        inside = D[r] != D[r, k - 1]
        assert np.array_equal(lab[inside], Is[r][inside]), (what, r)
    return across
