#!/usr/bin/env python3
"""Generate the polysemous fixtures tests/golden/poly_*.npz.

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  Every case is first an ordinary
fixture of make_golden.py (oracle/_ref/ref_driver), then tests/golden/poly_driver.cpp (our driver over the reference's
public API, compiled here into oracle/_ref/) loads that index and adds:

    poly_hts [4] = {1, t_low, t_mid, 8 M + 1}, poly_qcodes [nq][nprobe][M] (the code of the query for every probe, from the
    reference's public functions), all_D / all_pairs [nq][k_all] (the unfiltered search_knn_with_key with store_pairs at a k
    no query's scan exceeds: every scanned code's distance); where the reference defines the mode (not by_residual, table
    type 2), per threshold: poly_D, poly_I, poly_pairs [4][nq][k], poly_npass [4][nq], poly_ncode [nq] (indexIVFPQ_stats of
    one-query calls).

poly_nonresidual is trained with do_polysemous_training (the driver runs the reference's optimize_pq_for_hamming on the
quantizer ref_driver trained and encodes the vectors again): its pq_centroids, codes and table heads are the driver's.
t_low / t_mid are chosen per case so that about 2 % and 30 % of the scanned codes pass.  The script checks what the tests
rely on and refuses to write a fixture that misses a condition.  Fixtures are data only.

    python tests/golden/make_golden_poly.py                  # all cases
    python tests/golden/make_golden_poly.py poly_table1      # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden as mg  # noqa: E402
from polysemous_ref import scan_hamming  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
MAX_K = 1024          # VLQ_MAX_K (include/vlq_ivfpq.h)

POLY_CASES = {}


def pcase(fn):
    POLY_CASES[fn.__name__] = fn
    return fn


def poly_data(seed, d, nc, nt, nb, nq, heavy, absent, sigma=0.08, twice=6, heavy_sigma=0.5):
    """Gaussian mixture like make_golden.gmm_case with one centre that holds `heavy` of the stored vectors (a long list), the
    last `absent` centres in the training set and the queries only (sparse lists), the first `twice` queries equal to stored
    vectors (a Hamming distance of 0) and those vectors stored twice."""
    rng = np.random.default_rng(seed)
    centres = rng.random((nc, d))
    xt = mg.sift_like(rng, nt, d, centres, sigma)
    xb = np.concatenate([mg.sift_like(rng, nb - heavy - twice, d, centres[1:nc - absent], sigma),
                         mg.sift_like(rng, heavy, d, centres[:1], sigma * heavy_sigma)])
    xb = xb[rng.permutation(xb.shape[0])]
    xb = np.concatenate([xb, xb[:twice]])
    xq = mg.sift_like(rng, nq, d, centres, sigma)
    xq[:twice] = xb[:twice]
    return xt, xb, xq


@pcase
def poly_nonresidual():
    """by_residual = false, d 32, M 8 x 8 bit, 16 lists; PQ centroids permuted by the reference's polysemous training."""
    xt, xb, xq = poly_data(1201, 32, 16, 3000, 1500, 40, 300, 2)
    return (mg.cfg(32, 16, 8, 8, 3000, 1500, 40, 5, 10, n_small=6, pq_niter=6, by_residual=0), xt, xb, xq, None), 20000


@pcase
def poly_imi():
    """2 x 4-bit multi-index (256 lists), M 8, table type 2, nprobe 24."""
    xt, xb, xq = poly_data(1302, 16, 40, 4000, 2500, 40, 420, 3, sigma=0.1, heavy_sigma=0.1)
    return (mg.cfg(16, 256, 8, 8, 4000, 2500, 40, 24, 10, n_small=6, km_niter=8, pq_niter=6, imi_nbits=4), xt, xb, xq, None), 0


@pcase
def poly_table1():
    """d 64, M 16 x 8 bit (the headline's code size), 32 lists, nprobe 8, table type 1."""
    xt, xb, xq = poly_data(1403, 64, 32, 4000, 2000, 40, 280, 3)
    return (mg.cfg(64, 32, 16, 8, 4000, 2000, 40, 8, 10, n_small=6, pq_niter=6), xt, xb, xq, None), 0


@pcase
def poly_table0_m20():
    """M 20 (5 code words, not a multiple of 8 bytes), ksub 64 (6 bits), table type 0."""
    xt, xb, xq = poly_data(1504, 40, 24, 3000, 2000, 40, 300, 3)
    return (mg.cfg(40, 24, 20, 6, 3000, 2000, 40, 6, 10, n_small=6, pq_niter=6, upt=0), xt, xb, xq, None), 0


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "poly_driver")
    src = os.path.join(HERE, "poly_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + REF, "-o", exe, src, os.path.join(OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def refuse(name, why):
    path = os.path.join(HERE, name + ".npz")
    if os.path.exists(path):
        os.remove(path)
    raise SystemExit("%s: %s -- fixture not written" % (name, why))


def run_case(name):
    base, poly_niter = POLY_CASES[name]()
    c, xt, xb, xq, xids = base
    exe = build_driver()
    path = os.path.join(HERE, name + ".npz")
    mg.CASES[name] = lambda: base
    mg.run_case(name)                                    # 1. the ordinary fixture
    z = np.load(path)
    if not (np.diff(z["list_offsets"]) == 0).any():
        # no empty list: store the vectors again without those of the shortest list (the training set decides the lists)
        lens = np.diff(z["list_offsets"])
        xb = xb[z["xb_assign"] != int(np.argmin(lens))]
        c = c.copy()
        c[5] = xb.shape[0]
        base = (c, xt, xb, xq, xids)
        mg.run_case(name)
        z = np.load(path)
    keep = {k: z[k] for k in z.files}
    nq, nprobe, k, M, max_codes = int(c[6]), int(c[7]), int(c[8]), int(c[2]), int(c[9])
    off = keep["list_offsets"]
    lens = np.diff(off)
    if not (lens > 256).any() or not (lens % 64 != 0).any() or not (lens == 0).any():
        refuse(name, "needs a list longer than 256 codes, one whose length is no multiple of 64 and an empty one (longest %d, %d empty)"
               % (lens.max(), (lens == 0).sum()))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(OUT, "mkl") + ":" + env.get("LD_LIBRARY_PATH", "")
    env["OMP_NUM_THREADS"] = "4"

    def drive(hts, k_all):
        with tempfile.TemporaryDirectory() as td:
            fin, fout, fidx, fpout = (os.path.join(td, n) for n in ("in.bin", "out.bin", "index.faissindex", "pout.bin"))
            write_tagged(fin, {"cfg": c, "xt": xt, "xb": xb, "xq": xq, "pcfg": np.array([poly_niter, k_all], np.int64),
                               "hts": np.array(hts, np.int64)})
            subprocess.check_call([os.path.join(OUT, "ref_driver"), fin, fout, fidx], env=env)
            subprocess.check_call([exe, fin, fidx, fpout], env=env)
            return read_tagged(fout), read_tagged(fpout)

    # 2. a first pass for the codes of the queries: the thresholds come from the Hamming distances of the scanned codes
    again, out = drive([1], 0)
    for nm in ("ids", "keys", "coarse_dis", "list_offsets"):
        assert np.array_equal(again[nm], keep[nm]) and np.array_equal(out[nm], keep[nm]), "not reproducible in %s" % nm
    if poly_niter == 0:
        for nm in ("codes", "pq_centroids"):
            assert np.array_equal(out[nm], keep[nm]), "the loaded index differs in %s" % nm
    for nm in ("D", "I", "D_pairs", "I_pairs"):          # (a permutation of the centroids changes no distance)
        assert np.array_equal(out[nm].view(np.uint8), keep[nm].view(np.uint8)), "the loaded index searches differently: %s" % nm
    hd_all, nscan = [], []
    for i in range(nq):
        _p, hd, ns = scan_hamming(keep["keys"][i], out["poly_qcodes"][i], out["codes"], off, max_codes)
        hd_all.append(hd)
        nscan.append(ns)
    k_all = max(nscan)
    if k_all > MAX_K:
        refuse(name, "a query scans %d codes, more than VLQ_MAX_K" % k_all)
    hd_cat = np.sort(np.concatenate(hd_all))
    t_low = int(hd_cat[int(0.02 * hd_cat.size)]) + 1       # hd < t: about 2 % / 30 % of the scanned codes
    t_mid = int(hd_cat[int(0.30 * hd_cat.size)]) + 1
    hts = [1, t_low, t_mid, 8 * M + 1]
    if not 1 < t_low < t_mid < 8 * M + 1:
        refuse(name, "thresholds %s are not distinct" % hts)
    npass_low = np.array([(h < t_low).sum() for h in hd_all])
    if not (npass_low < k).any() or not (npass_low >= k).any():
        refuse(name, "at t_low some query must get fewer than k results and some a full row (passes per query %s)" % npass_low)
    if not (hd_cat < 1).any():
        refuse(name, "no code passes at ht = 1")

    # 3. the fixture
    _again, out = drive(hts, k_all)
    keep["poly_hts"] = np.array(hts, np.int64)
    keep["poly_qcodes"] = out["poly_qcodes"]
    keep["all_D"], keep["all_pairs"] = out["all_D"], out["all_pairs"]
    assert all((out["all_pairs"][i] >= 0).sum() == nscan[i] for i in range(nq)), "all_pairs does not hold every scanned code"
    if poly_niter > 0:
        assert not np.array_equal(out["pq_centroids"], keep["pq_centroids"]), "the polysemous training changed nothing"
        assert np.array_equal(np.sort(out["pq_centroids"].reshape(M, -1), axis=1), np.sort(keep["pq_centroids"].reshape(M, -1), axis=1))
        keep["pq_centroids"], keep["codes"] = out["pq_centroids"], out["codes"]
        for nm in ("ip_table", "dis_table"):
            keep[nm + "_head"] = out[nm][:2]
            keep[nm + "_sha256"] = mg.sha(out[nm])
    defined = int(out["poly_defined"][0]) == 1
    assert defined == (name in ("poly_nonresidual", "poly_imi"))
    if defined:
        for nm in ("poly_D", "poly_I", "poly_pairs", "poly_npass", "poly_ncode"):
            keep[nm] = out[nm]
        assert np.array_equal(out["poly_ncode"], np.array(nscan)), "ncode differs from the list sizes"
        for t, ht in enumerate(hts):
            mine = np.array([(h < ht).sum() for h in hd_all])
            assert np.array_equal(mine, out["poly_npass"][t]), "ht=%d: the reference's pass counts differ from popcount(q_code ^ code) < ht" % ht
        assert (out["poly_I"][1] == -1).any() and (out["poly_I"][1][:, -1] != -1).any()
        assert np.array_equal(out["poly_D"][3].view(np.uint32), keep["D_pairs"].view(np.uint32)), "ht = 8 M + 1 must pass everything"
    np.savez_compressed(path, **keep)
    frac = [float((hd_cat < t).mean()) for t in hts]
    print("%-18s %8.1f KB  hts=%s pass fractions %s k_all=%d longest list %d" % (
        name, os.path.getsize(path) / 1024.0, hts, ["%.3f" % f for f in frac], k_all, lens.max()))


if __name__ == "__main__":
    for n in sys.argv[1:] or list(POLY_CASES):
        run_case(n)
