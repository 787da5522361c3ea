#!/usr/bin/env python3
"""Generate the flat exact k-NN fixtures tests/golden/flatknn/*.npz (a directory of their own: tests/util.py takes every .npz
directly under tests/golden/ for an IVFPQ fixture of make_golden.py).

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/flatknn_driver.cpp (our
driver over the reference's public API, compiled here into oracle/_ref/) builds a faiss::IndexFlat per metric, adds xb and
searches all queries in ONE call.  Fixtures are data only: xb, xq, D_l2 / I_l2, D_ip / I_ip, d, k, kind (one fixture carries
both metrics of one data set).

Every fixture is checked against the restatement (tests/knn_ref.py) and for the conditions the tests rely on; a fixture that
misses one is not written (the next seed is tried where the condition is a matter of chance).

  small   nq < 20, d % 4 == 0: the reference's SSE paths, general floats.  The restatement reproduces D and I bit for bit; no
          row holds two equal distances; the fmaf-chain inner product differs in bits from the reference's D_ip in at least one
          slot (the small-batch order is the reference's, not the GEMM path's).
  kwide   the same with k > nb: padding
  ties    half of the vectors stored twice; rows by tests/util.py's assert_same_topk rule; at least half of the rows have no
          tie group across the k-th place, some row has one
  int     nq >= 20, small integer components: every partial sum is exact in fp32, so the reference's BLAS distances are the
          restatement's bit for bit; labels by the tie rule, under the same half-the-rows condition
  blas    nq >= 20 or d % 4 != 0, general floats: the reference's sgemm_ order is the vendor's.  Written only if the reference's
          labels equal the restatement's in every slot; every distance of the reference lies within
              2 (d + 3) 2^-24 (|x|^2 + |y|^2)   (L2)        (d + 1) 2^-23 |x| |y|   (inner product)
          of the restatement's (norms in float64).  Two summation orders of d products differ by at most 2 gamma_d sum |x_k y_k|,
          sum |x_k y_k| <= |x| |y| <= (|x|^2 + |y|^2) / 2; the two final roundings add at most 4u (|x|^2 + |y|^2); the norms are
          the same bits on both sides.

    python tests/golden/make_golden_flatknn.py                  # all cases
    python tests/golden/make_golden_flatknn.py small_d32_nq19   # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]
import knn_ref as kr  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402
from util import assert_same_topk  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
DEST = os.path.join(HERE, "flatknn")
MAX_BYTES = 595653      # the largest file under tests/golden/ivfflat/

CASES = {}


def spec(kind, d, nq, nb, k, seed):
    return dict(kind=kind, d=d, nq=nq, nb=nb, k=k, seed=seed)


for _d, _nb in ((4, 1000), (32, 1000), (128, 700)):
    for _nq in (1, 19):
        CASES["small_d%d_nq%d" % (_d, _nq)] = spec("small", _d, _nq, _nb, 10, 6100 + _d + _nq)
CASES["small_kwide"] = spec("kwide", 32, 19, 40, 64, 6200)
CASES["small_ties"] = spec("ties", 32, 19, 600, 47, 6210)
for _d in (30, 64):
    CASES["int_d%d_nq40" % _d] = spec("int", _d, 40, 1500, 20, 6300 + _d)
CASES["blas_d30_nq5"] = spec("blas", 30, 5, 1500, 10, 6400)
for _d, _nb in ((30, 1500), (128, 500), (200, 300)):
    for _nq in (20, 150):
        CASES["blas_d%d_nq%d" % (_d, _nq)] = spec("blas", _d, _nq, _nb, 10, 6500 + _d + _nq)


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "flatknn_driver")
    src = os.path.join(HERE, "flatknn_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + REF, "-o", exe, src, os.path.join(OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def drive(exe, xb, xq, k, metric):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(OUT, "mkl") + ":" + env.get("LD_LIBRARY_PATH", "")
    env["OMP_NUM_THREADS"] = "4"
    arrays = {"cfg": np.array([xb.shape[1], xb.shape[0], xq.shape[0], k, 0 if metric == "ip" else 1], np.int64), "xb": xb, "xq": xq}
    outs = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as td:
            fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
            write_tagged(fin, arrays)
            subprocess.check_call([exe, fin, fout], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            outs.append(read_tagged(fout))
    for nm in outs[0]:
        if not np.array_equal(outs[0][nm].view(np.uint8), outs[1][nm].view(np.uint8)):
            raise SystemExit("not reproducible in %s" % nm)
    if not np.array_equal(outs[0]["xb_back"].view(np.uint32), xb.view(np.uint32)):
        raise SystemExit("index.xb is not what was added")
    return outs[0]["D"], outs[0]["I"]


class NextSeed(Exception):
    pass


def refuse(name, why):
    path = os.path.join(DEST, name + ".npz")
    if os.path.exists(path):
        os.remove(path)
    raise SystemExit("%s: %s -- fixture not written" % (name, why))


def data(s, seed):
    rng = np.random.default_rng(seed)
    d, nb, nq = s["d"], s["nb"], s["nq"]
    if s["kind"] == "int":
        return rng.integers(-8, 9, (nb, d)).astype(np.float32), rng.integers(-8, 9, (nq, d)).astype(np.float32)
    nc = 16
    centres = rng.standard_normal((nc, d))
    xb = (centres[rng.integers(0, nc, nb)] + 0.7 * rng.standard_normal((nb, d))).astype(np.float32)
    xq = (centres[rng.integers(0, nc, nq)] + 0.7 * rng.standard_normal((nq, d))).astype(np.float32)
    if s["kind"] == "ties":
        xb = np.concatenate([xb, xb[: nb // 2]])[rng.permutation(nb + nb // 2)]
    return np.ascontiguousarray(xb), np.ascontiguousarray(xq)


def tied_rows(D, I):
    out = np.zeros(D.shape[0], bool)
    for r in range(D.shape[0]):
        v = D[r][I[r] != -1]
        out[r] = np.unique(v).size != v.size
    return out


def cut_rows(xq, xb, k, metric):
    """rows with a tie group across the k-th place"""
    Dk1, Ik1 = kr.search(xq, xb, k + 1, metric)
    return (Dk1[:, k] == Dk1[:, k - 1]) & (Ik1[:, k] != -1)


def bounds(xq, xb, I, metric, d):
    xn = (xq.astype(np.float64) ** 2).sum(1)[:, None]
    yn = (xb.astype(np.float64) ** 2).sum(1)[np.maximum(I, 0)]
    if metric == "l2":
        return 2 * (d + 3) * 2.0 ** -24 * (xn + yn)
    return (d + 1) * 2.0 ** -23 * np.sqrt(xn) * np.sqrt(yn)


def run_seed(name, s, seed):
    exe = build_driver()
    xb, xq = data(s, seed)
    kind, d, k = s["kind"], s["d"], s["k"]
    direct = kr.is_direct(xq.shape[0], d)
    if (kind in ("small", "kwide", "ties")) != direct:
        refuse(name, "the case does not take the path its kind names")
    z = {"xb": xb, "xq": xq, "d": np.array(d, np.int64), "k": np.array(k, np.int64), "kind": np.array(kind)}
    for metric in ("l2", "ip"):
        D, I = drive(exe, xb, xq, k, metric)
        I = I.astype(np.int64)
        Dn, In = kr.search(xq, xb, k, metric)
        z["D_" + metric], z["I_" + metric] = D, I
        what = "%s %s" % (name, metric)
        if kind in ("small", "kwide"):
            if tied_rows(D, I).any():
                raise NextSeed()
            if not (kr.same_bits(D, Dn) and np.array_equal(I, In)):
                refuse(name, "the restatement does not reproduce %s D / I bit for bit" % metric)
            if kind == "kwide" and not ((I[:, xb.shape[0]:] == -1).all() and (I[:, :xb.shape[0]] != -1).all()):
                refuse(name, "padding is not where it should be")
            if metric == "ip":
                Dc = kr.rows_from_matrix(kr.ip_chain(xq, xb), k, True)[0]
                if kr.same_bits(Dc, D):
                    raise NextSeed()        # not discriminating: the fmaf chain gives the same bits
        elif kind in ("ties", "int"):
            try:
                assert_same_topk(Dn, In, D, I, what)
            except AssertionError as e:
                refuse(name, str(e))
            cut = cut_rows(xq, xb, k, metric)
            if cut.sum() * 2 > cut.size:
                raise NextSeed()
            if kind == "ties" and not cut.any():
                raise NextSeed()
            if not tied_rows(D, I).any():
                raise NextSeed()
        else:
            if not np.array_equal(I, In):
                raise NextSeed()            # a near tie fell the other way under the vendor's summation order
            if (np.abs(D.astype(np.float64) - Dn.astype(np.float64)) > bounds(xq, xb, I, metric, d)).any():
                refuse(name, "a %s distance of the reference is outside the rounding bound of the restatement's" % metric)
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    if os.path.getsize(path) > MAX_BYTES:
        refuse(name, "larger than the largest IVFFlat fixture")
    print("%-18s seed %d %8.1f KB  nb %d nq %d" % (name, seed, os.path.getsize(path) / 1024.0, xb.shape[0], xq.shape[0]))


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
