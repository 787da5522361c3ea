#!/usr/bin/env python3
"""Generate the flat index's range-search fixtures tests/golden/flatrange/*.npz, one per fixture of tests/golden/flatknn/ (whose
xb and xq are the data: a range fixture stores its source's name, not the vectors).

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/flatrange_driver.cpp (our
driver over the reference's public API, compiled here into oracle/_ref/) builds a faiss::IndexFlat per metric, adds xb and runs
IndexFlat::range_search over all queries in ONE call per radius.  Fixtures are data only: src, kind, names (of the radii),
radii_l2 / radii_ip, and per metric and radius lims_<metric>_<name>, D_..., I_... (`all` and `none`: lims only).

Every fixture is checked against the restatement (tests/knn_range_ref.py); one that misses a condition is not written.

  small, kwide, ties, int  (the SSE path, or integer-valued data on the BLAS path: the reference's distances are the
          restatement's bit for bit).  Radii are observed distances of the restatement's matrix, so the strict test decides a pair:
            tight       the pooled distance of rank 12 nq (L2: ascending; inner product: descending)
            tight_next  one ulp towards more hits: exactly the pairs at `tight` join
            wide        rank 100 nq, capped below nq nb
          Condition: the reference's lims, bits of D and I equal the restatement's element for element.
  blas    general floats on the GEMM formulation: the reference's sgemm_ order is the vendor's.  tight and wide are the midpoint of
          the widest gap between adjacent pooled distances near that rank (within an eighth of the rank around it, else a
          quarter, a half, three quarters: the windows of tight and wide never meet); the case is written only if that gap
          exceeds twice the largest rounding bound of make_golden_flatknn.py over the case's pairs,
              2 (d + 3) 2^-24 (|x|^2 + |y|^2)   (L2)        (d + 1) 2^-23 |x| |y|   (inner product)
          so that the reference's hit set equals the restatement's under any summation order.  There is no tight_next.
          Conditions: lims and I equal, every D within that bound.
  all / none   +-FLT_MAX on the side that admits every / no pair

    python tests/golden/make_golden_flatrange.py                  # all cases
    python tests/golden/make_golden_flatrange.py small_d32_nq19   # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]
import knn_range_ref as rr  # noqa: E402
from make_golden_flatknn import MAX_BYTES, OUT, REF  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402

SRC = os.path.join(HERE, "flatknn")
DEST = os.path.join(HERE, "flatrange")
FLT_MAX = np.finfo(np.float32).max
LIMS_ONLY = ("all", "none")


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "flatrange_driver")
    src = os.path.join(HERE, "flatrange_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + REF, "-o", exe, src, os.path.join(OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def drive(exe, xb, xq, radii, metric):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(OUT, "mkl") + ":" + env.get("LD_LIBRARY_PATH", "")
    env["OMP_NUM_THREADS"] = "4"
    arrays = {"cfg": np.array([xb.shape[1], xb.shape[0], xq.shape[0], 0 if metric == "ip" else 1], np.int64), "xb": xb, "xq": xq,
              "radii": np.asarray(radii, np.float32)}
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
    return outs[0]


def refuse(name, why):
    path = os.path.join(DEST, name + ".npz")
    if os.path.exists(path):
        os.remove(path)
    raise SystemExit("%s: %s -- fixture not written" % (name, why))


def pair_bound(xq, xb, metric, d):
    """[nq][nb] rounding bounds of make_golden_flatknn.py"""
    xn = (xq.astype(np.float64) ** 2).sum(1)[:, None]
    yn = (xb.astype(np.float64) ** 2).sum(1)[None, :]
    if metric == "l2":
        return 2 * (d + 3) * 2.0 ** -24 * (xn + yn)
    return (d + 1) * 2.0 ** -23 * np.sqrt(xn) * np.sqrt(yn)


def pooled(mat, metric):
    """the matrix's values from the nearest on"""
    s = np.sort(mat.ravel())
    return s[::-1] if metric == "ip" else s


def radii_of(name, kind, mat, metric, bound):
    nq, nb = mat.shape
    s = pooled(mat, metric)
    more = -np.inf if metric == "ip" else np.inf
    r_tight, r_wide = min(12 * nq, nq * nb - 1), min(100 * nq, nq * nb - 1)
    out = {}
    if kind != "blas":
        tight = s[r_tight]
        out["tight"] = tight
        out["tight_next"] = np.nextafter(tight, np.float32(more), dtype=np.float32)
        out["wide"] = s[r_wide]
        n0, n1 = (rr.from_matrix(mat, out[nm], metric)[0][-1] for nm in ("tight", "tight_next"))
        if n1 - n0 != (mat == tight).sum() or n1 == n0:
            refuse(name, "tight_next does not admit exactly the pairs at tight (%s)" % metric)
    else:
        need = 2 * bound.max()
        for nm, r in (("tight", r_tight), ("wide", r_wide)):
            for frac in (8, 4, 2, 1.34):        # the narrowest of the windows r -+ r / frac that holds such a gap
                w = int(r / frac)
                lo, hi = max(r - w, 1), min(r + w + 1, s.size)
                gaps = np.abs(np.diff(s[lo - 1:hi].astype(np.float64)))
                g = int(np.argmax(gaps))
                if gaps[g] > need:
                    break
            else:
                refuse(name, "no gap of more than %g near rank %d (%s): the widest is %g" % (need, r, metric, gaps[g]))
            mid = np.float32((float(s[lo - 1 + g]) + float(s[lo + g])) / 2)
            if not (min(s[lo - 1 + g], s[lo + g]) < mid < max(s[lo - 1 + g], s[lo + g])):
                refuse(name, "the midpoint is not inside the gap")
            out[nm] = mid
    out["all"] = np.float32(-FLT_MAX if metric == "ip" else FLT_MAX)
    out["none"] = np.float32(FLT_MAX if metric == "ip" else -FLT_MAX)
    return out


def run_case(name):
    exe = build_driver()
    src = np.load(os.path.join(SRC, name + ".npz"))
    xb, xq, d, kind = np.ascontiguousarray(src["xb"]), np.ascontiguousarray(src["xq"]), int(src["d"]), str(src["kind"])
    z = {"src": np.array(name), "kind": np.array(kind)}
    names = None
    for metric in ("l2", "ip"):
        mat = rr.matrix(xq, xb, metric)
        bound = pair_bound(xq, xb, metric, d)
        radii = radii_of(name, kind, mat, metric, bound)
        if names is None:
            names = list(radii)
            z["names"] = np.array(names)
        z["radii_" + metric] = np.array([radii[nm] for nm in names], np.float32)
        out = drive(exe, xb, xq, z["radii_" + metric], metric)
        for r, nm in enumerate(names):
            lims, D, I = out["lims_%d" % r], out["D_%d" % r], out["I_%d" % r].astype(np.int64)
            D, I = D[:lims[-1]], I[:lims[-1]]
            ln, Dn, In = rr.from_matrix(mat, radii[nm], metric)
            what = "%s %s" % (metric, nm)
            if not (np.array_equal(lims, ln) and np.array_equal(I, In)):
                refuse(name, "the restatement's lims / I are not the reference's (%s)" % what)
            if kind != "blas":
                if not rr.same_bits(D, Dn):
                    refuse(name, "the restatement does not reproduce the bits of D (%s)" % what)
            else:
                q = np.repeat(np.arange(xq.shape[0]), np.diff(lims))
                if (np.abs(D.astype(np.float64) - Dn.astype(np.float64)) > bound[q, I]).any():
                    refuse(name, "a distance of the reference is outside the rounding bound of the restatement's (%s)" % what)
            for a, b in zip(lims[:-1], lims[1:]):
                if (np.diff(I[a:b]) <= 0).any():
                    refuse(name, "a query's labels do not ascend (%s)" % what)
            if nm == "all" and lims[-1] != mat.size or nm == "none" and lims[-1] != 0:
                refuse(name, "%s does not admit what its name says" % what)
            z["lims_%s_%s" % (metric, nm)] = lims
            if nm not in LIMS_ONLY:
                z["D_%s_%s" % (metric, nm)], z["I_%s_%s" % (metric, nm)] = D, I
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    if os.path.getsize(path) > MAX_BYTES:
        refuse(name, "larger than make_golden_flatknn.py's MAX_BYTES")
    print("%-18s %8.1f KB  %s" % (name, os.path.getsize(path) / 1024.0,
                                   " ".join("%s:%d/%d" % (nm, z["lims_l2_" + nm][-1], z["lims_ip_" + nm][-1]) for nm in names)))


if __name__ == "__main__":
    os.makedirs(DEST, exist_ok=True)
    for n in sys.argv[1:] or sorted(os.path.splitext(f)[0] for f in os.listdir(SRC) if f.endswith(".npz")):
        run_case(n)
