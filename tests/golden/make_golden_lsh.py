#!/usr/bin/env python3
"""Generate the LSH fixtures tests/golden/lsh/*.npz (a directory of their own: tests/util.py takes every .npz directly under
tests/golden/ for an IVFPQ fixture of make_golden.py).

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/lsh_driver.cpp (our driver
over the reference's public API, compiled here into oracle/_ref/) builds a faiss::IndexLSH, optionally overwrites rrot.A,
trains, adds and searches all queries in ONE call.  Fixtures are data only: xb, xq, xt (the training set), A, thresholds, codes,
qcodes, D, I, d, nbits, k, rotate, thresh, kind, threw, index_bytes (the file the reference's write_index wrote for the index).

The reference runs twice; a result that is not reproducible is refused.  Every fixture is checked against the restatement
(tests/lsh_ref.py) and for its kind's condition; a fixture that misses it is not written (the next seed is tried where the
condition is a matter of chance).  For every kind: the restatement's stored and query codes equal the reference's in every bit, D
is bit-equal, I by tests/util.py's assert_same_topk rule.

  plain       no rotation, d == nbits; general floats, some exact 0.0f and -0.0f planted (their bits must be set)
  prefix      no rotation, d > nbits
  thresh      train_thresholds, no rotation, odd and even training n: thresholds bit-equal
  rot_int     A overwritten by integers in [-3, 3], integer data in [-8, 8], thresholds on: every sum is exact, all bit-equal
  rot         the reference's own rrot.init(5) matrix (saved as data), general floats.  The vendor sgemm_'s order may flip a sign
              near zero against the fmaf chain: next seed then
  rot_thresh  the same with trained thresholds: each within (d + 2) 2^-23 |A_j| max_i |x_i| of the restatement's -- the median
              of values perturbed by at most e moves by at most e; two summation orders of d products differ by at most
              (d + 1) 2^-23 |A_j| |x_i| (tests/test_knn_ref.py's blas bound), and the mean of two adds half an ulp
  ties        half of the vectors stored twice, k = 47: some row has a tie group across the k-th place
  kwide       k = 64 > nb = 40: padding is 2^31 / -1 exactly
  width_*     nbits in 32, 60, 64, 128, 192, 256, 320, 512, 1024: HammingComputer4, hammings_knn_1, 16, 32 and M8
  unserved    nbits = 100 (13 bytes): the driver records that search threw; the codes are still saved

    python tests/golden/make_golden_lsh.py             # all cases
    python tests/golden/make_golden_lsh.py rot_64_32   # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]
import lsh_ref as lr  # noqa: E402
from make_golden_flatknn import MAX_BYTES  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402
from util import assert_same_topk  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
DEST = os.path.join(HERE, "lsh")

CASES = {}


def spec(kind, d, nbits, nb, nq, k, seed, rotate=False, thresh=False, nt=0):
    return dict(kind=kind, d=d, nbits=nbits, nb=nb, nq=nq, k=k, seed=seed, rotate=rotate, thresh=thresh, nt=nt)


CASES["plain"] = spec("plain", 32, 32, 600, 20, 10, 7100)
CASES["prefix"] = spec("prefix", 48, 32, 500, 20, 10, 7110)
CASES["thresh_odd"] = spec("thresh", 32, 32, 400, 20, 10, 7120, thresh=True, nt=301)
CASES["thresh_even"] = spec("thresh", 32, 32, 400, 20, 10, 7130, thresh=True, nt=300)
CASES["rot_int"] = spec("rot_int", 32, 64, 1000, 40, 10, 7140, rotate=True, thresh=True, nt=301)
CASES["rot_64_32"] = spec("rot", 64, 32, 400, 20, 10, 7150, rotate=True)
CASES["rot_16_64"] = spec("rot", 16, 64, 1000, 20, 10, 7160, rotate=True)
CASES["rot_thresh_64_32"] = spec("rot_thresh", 64, 32, 300, 20, 10, 7170, rotate=True, thresh=True, nt=200)
CASES["rot_thresh_16_64"] = spec("rot_thresh", 16, 64, 800, 20, 10, 7180, rotate=True, thresh=True, nt=301)
CASES["ties"] = spec("ties", 32, 32, 600, 19, 47, 7190)
CASES["kwide"] = spec("kwide", 32, 32, 40, 19, 64, 7200)
for _nbits in (32, 60, 64, 128, 192, 256, 320, 512, 1024):
    CASES["width_%d" % _nbits] = spec("width", _nbits, _nbits, max(150, min(1000, 65536 // _nbits)), 10, 10, 7300 + _nbits)
CASES["unserved"] = spec("unserved", 100, 100, 200, 10, 10, 7400)


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "lsh_driver")
    src = os.path.join(HERE, "lsh_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + REF, "-o", exe, src, os.path.join(OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def drive(exe, s, xb, xq, xt, A):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(OUT, "mkl") + ":" + env.get("LD_LIBRARY_PATH", "")
    env["OMP_NUM_THREADS"] = "4"
    arrays = {"cfg": np.array([s["d"], xb.shape[0], xq.shape[0], s["k"], s["nbits"], int(s["rotate"]), int(s["thresh"])], np.int64),
              "xb": xb, "xq": xq}
    if xt is not None:
        arrays["xt"] = xt
    if A is not None:
        arrays["A"] = A
    outs = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as td:
            fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
            write_tagged(fin, arrays)
            subprocess.check_call([exe, fin, fout], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            outs.append(read_tagged(fout))
    if sorted(outs[0]) != sorted(outs[1]):
        raise SystemExit("not reproducible: different outputs")
    for nm in outs[0]:
        if not np.array_equal(outs[0][nm].view(np.uint8), outs[1][nm].view(np.uint8)):
            raise SystemExit("not reproducible in %s" % nm)
    return outs[0]


class NextSeed(Exception):
    pass


def refuse(name, why):
    path = os.path.join(DEST, name + ".npz")
    if os.path.exists(path):
        os.remove(path)
    raise SystemExit("%s: %s -- fixture not written" % (name, why))


def data(s, seed):
    """xb, xq, xt (training set or None), A (the matrix to force, or None)"""
    rng = np.random.default_rng(seed)
    d, nb, nq, nt, kind = s["d"], s["nb"], s["nq"], s["nt"], s["kind"]
    A = None
    if kind == "rot_int":
        A = rng.integers(-3, 4, (s["nbits"], d)).astype(np.float32)
        draw = lambda n: rng.integers(-8, 9, (n, d)).astype(np.float32)  # noqa: E731
    elif kind in ("width", "unserved", "ties", "kwide"):
        # few distinct values: the sign is all these kinds are about, and the file stays small
        draw = lambda n: rng.choice(np.array([-1.0, -0.5, 0.5, 1.0], np.float32), (n, d))  # noqa: E731
    else:
        nc = 16
        centres = rng.standard_normal((nc, d))
        shift = 0.6 if s["thresh"] else 0.0       # medians away from zero, so that the thresholds matter
        draw = lambda n: (shift + centres[rng.integers(0, nc, n)] + 0.7 * rng.standard_normal((n, d))).astype(np.float32)  # noqa: E731
    xb, xq = draw(nb), draw(nq)
    xt = draw(nt) if nt else None
    if kind == "ties":
        xb = np.concatenate([xb, xb[: nb // 2]])[rng.permutation(nb + nb // 2)]
    if kind == "plain":
        for x in (xb, xq):
            x[5, 3], x[6, 4], x[7, 0], x[8, 31] = 0.0, -0.0, -0.0, 0.0
    return np.ascontiguousarray(xb), np.ascontiguousarray(xq), xt, A


def bit_of(codes, row, j):
    return (codes[row, j // 8] >> (j % 8)) & 1


def run_seed(name, s, seed):
    exe = build_driver()
    xb, xq, xt, A_in = data(s, seed)
    kind, d, nbits, k = s["kind"], s["d"], s["nbits"], s["k"]
    o = drive(exe, s, xb, xq, xt, A_in)
    A = o["A"].reshape(nbits, d) if s["rotate"] else None
    thr = o["thresholds"] if s["thresh"] else None
    if A_in is not None and not np.array_equal(A, A_in):
        refuse(name, "rrot.A is not what was written into it")
    z = {"xb": xb, "xq": xq, "d": np.array(d, np.int64), "nbits": np.array(nbits, np.int64), "k": np.array(k, np.int64),
         "rotate": np.array(int(s["rotate"]), np.int64), "thresh": np.array(int(s["thresh"]), np.int64), "kind": np.array(kind),
         "codes": o["codes"], "qcodes": o["qcodes"], "threw": np.array(int(o["threw"][0]), np.int64),
         "index_bytes": o["index_bytes"]}
    if xt is not None:
        z["xt"] = xt
    if A is not None:
        z["A"] = A
    if thr is not None:
        z["thresholds"] = thr
        tn = lr.train(xt, nbits, A)
        if kind in ("thresh", "rot_int"):
            if not np.array_equal(tn.view(np.uint32), thr.view(np.uint32)):
                refuse(name, "the restatement's thresholds are not the reference's bit for bit")
        else:
            bound = (d + 2) * 2.0 ** -23 * np.sqrt((A.astype(np.float64) ** 2).sum(1)) * np.abs(xt).max()
            if (np.abs(tn.astype(np.float64) - thr.astype(np.float64)) > bound).any():
                refuse(name, "a threshold of the reference is outside the rounding bound of the restatement's")
    cn, qn = lr.encode(xb, nbits, A, None, thr), lr.encode(xq, nbits, A, None, thr)
    if not (np.array_equal(cn, o["codes"]) and np.array_equal(qn, o["qcodes"])):
        if kind in ("rot", "rot_thresh"):
            raise NextSeed()            # a component near zero fell the other way under the vendor's summation order
        refuse(name, "the restatement's codes are not the reference's")
    if kind == "plain":
        for c in (o["codes"], o["qcodes"]):
            if not (bit_of(c, 5, 3) and bit_of(c, 6, 4) and bit_of(c, 7, 0) and bit_of(c, 8, 31)):
                refuse(name, "a planted 0.0f / -0.0f did not set its bit")
    if kind == "unserved":
        if not o["threw"][0] or lr.served(o["codes"].shape[1]):
            refuse(name, "the reference's search did not throw")
    else:
        if o["threw"][0]:
            refuse(name, "the reference's search threw")
        D, I = o["D"], o["I"].astype(np.int64)
        z["D"], z["I"] = D, I
        Dn, In = lr.search_codes(qn, cn, k)
        try:
            assert_same_topk(Dn, In, D, I, name)
            lr.check_labels(D, I, o["qcodes"], o["codes"])
        except AssertionError as e:
            refuse(name, str(e))
        if kind == "ties":
            Dk1, Ik1 = lr.search_codes(qn, cn, k + 1)
            if not ((Dk1[:, k] == Dk1[:, k - 1]) & (Ik1[:, k] != -1)).any():
                raise NextSeed()
        if kind == "kwide":
            nb = xb.shape[0]
            if not ((I[:, nb:] == -1).all() and (I[:, :nb] != -1).all() and (D[:, nb:].view(np.uint32) == 0x4F000000).all()):
                refuse(name, "padding is not 2^31 / -1 where it should be")
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    if os.path.getsize(path) > MAX_BYTES:
        refuse(name, "larger than the largest IVFFlat fixture")
    print("%-18s seed %d %8.1f KB  nb %d nq %d bytes %d" % (name, seed, os.path.getsize(path) / 1024.0, xb.shape[0], xq.shape[0], o["codes"].shape[1]))


def run_case(name):
    s = CASES[name]
    for attempt in range(40):
        try:
            return run_seed(name, s, s["seed"] + 1000 * attempt)
        except NextSeed:
            continue
    refuse(name, "the conditions failed at every seed tried")


if __name__ == "__main__":
    os.makedirs(DEST, exist_ok=True)
    for n in sys.argv[1:] or list(CASES):
        run_case(n)
    total = sum(os.path.getsize(os.path.join(DEST, f)) for f in os.listdir(DEST))
    print("tests/golden/lsh: %.1f KB" % (total / 1024.0))
    if total > 2 * 1024 * 1024:
        raise SystemExit("the directory is beyond 2 MB")
