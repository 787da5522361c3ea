"""The fixtures of tests/golden/ivfsq/ (tests/golden/make_golden_ivfsq.py) by group, and their loader.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

from util import GOLDEN

DIR = os.path.join(GOLDEN, "ivfsq")
QT = ("8bit", "4bit", "8bit_uniform", "4bit_uniform")
METRIC = {0: "ip", 1: "l2"}
AVX = ["sq_%s_%s_d%d" % (qt, m, d) for qt in QT for m in ("ip", "l2") for d in (32, 128)]
SCALAR = ["sq_%s_%s_d%d" % (qt, m, d) for qt in ("8bit", "4bit") for m in ("ip", "l2") for d in (30, 33)]
RAGGED = ["sq_8bit_l2_d40", "sq_4bit_ip_d48"]
TINY = ["sq_8bit_l2_d8", "sq_8bit_l2_d5"]
LONG = ["sq_8bit_l2_d128_long"]
KWIDE = ["sq_8bit_l2_d32_kwide"]
TIES = ["sq_ties_%s_%s" % (qt, m) for qt in ("8bit", "4bit") for m in ("ip", "l2")]
COARSE_INT = ["sq_coarse_int_l2", "sq_coarse_int_ip"]      # integer centroids and queries: exact coarse distances
NAMES = AVX + SCALAR + RAGGED + TINY + LONG + KWIDE + TIES + COARSE_INT
WITH_XB = [n for n in AVX if n.endswith("d32")] + SCALAR + TINY + COARSE_INT      # fixtures that hold the added vectors
FLT_MAX = np.float32(np.finfo(np.float32).max)
PAD_BITS = {"l2": FLT_MAX.view(np.uint32), "ip": np.float32(-FLT_MAX).view(np.uint32)}


def load(name):
    z = np.load(os.path.join(DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
