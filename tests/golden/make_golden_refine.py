#!/usr/bin/env python3
"""Generate the IVFPQR fixtures tests/golden/refine_*.npz.

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  Every case is first an ordinary
fixture of make_golden.py (the reference's IndexIVFPQ through oracle/_ref/ref_driver: trained centroids, lists, coarse
stage, first-stage results -- the tests that walk over every fixture read these), then tests/golden/refine_driver.cpp
(our driver over the reference's public API, compiled here into oracle/_ref/) puts the reference's IndexIVFPQR on top of
that first stage and adds:

    refine_cfg [M_refine, nbits_refine, k_coarse], k_factor, refine_centroids, refine_codes (BY LIST SLOT: row i belongs
    to codes row i), shortlist / shortlist_D (search_knn_with_key, store_pairs, at k_coarse), boundary_tie (per query: the
    k_coarse-th and (k_coarse+1)-th first-stage distances are equal, so the reference's shortlist depends on its heap's
    history), refine_D / refine_I (IndexIVFPQR::search).

Ids are sequential in every case (the reference finds a refine code by id).  Fixtures are data only.

    python tests/golden/make_golden_refine.py                  # all cases
    python tests/golden/make_golden_refine.py refine_tail      # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")

# name -> (make_golden case tuple, M_refine, nbits_refine, refine_pq_niter, k_factor)
REFINE_CASES = {}


def rcase(fn):
    REFINE_CASES[fn.__name__] = fn
    return fn


@rcase
def refine_c1_small():
    """The demo's index ("IVF4096,PQ8+16", tests/demo_sift1M.cpp:98) scaled down: d=128, 64 lists, PQ 8x8 bit + refine
    16x8 bit, nprobe 8, k 10, k_factor 4."""
    xt, xb, xq = mg.gmm_case(111, 128, 80, 5000, 3000, 64)
    return (mg.cfg(128, 64, 8, 8, 5000, 3000, 64, 8, 10, n_small=12, pq_niter=8), xt, xb, xq, None), 16, 8, 6, 4.0


@rcase
def refine_tail():
    """d=30: PQ 5x8 bit (dsub 6) + refine 10x6 bit (dsub 3) -- the d % 4 = 2 tail of fvec_L2sqr, a non-integer k_factor
    (k_coarse = long(7 * 3.5) = 24), ksub < 256."""
    xt, xb, xq = mg.gmm_case(222, 30, 40, 4000, 3000, 40)
    return (mg.cfg(30, 24, 5, 8, 4000, 3000, 40, 6, 7, n_small=5, pq_niter=6), xt, xb, xq, None), 10, 6, 6, 3.5


@rcase
def refine_padding():
    """Fewer stored vectors (30) than k (40) and k_coarse (80), some empty lists: -1 shortlist entries, padded output."""
    xt, xb, xq = mg.gmm_case(333, 16, 10, 2000, 30, 25)
    return (mg.cfg(16, 20, 4, 8, 2000, 30, 25, 20, 40, n_small=3, pq_niter=4), xt, xb, xq, None), 8, 8, 4, 2.0


@rcase
def refine_duplicates():
    """Every vector stored 4x: exact ties in both stages."""
    xt, xb, xq = mg.gmm_case(444, 32, 20, 3000, 2000, 50, dup=4)
    return (mg.cfg(32, 16, 8, 8, 3000, 2000, 50, 6, 10, n_small=4, pq_niter=6), xt, xb, xq, None), 8, 8, 6, 4.0


@rcase
def refine_k_wide():
    """k 100, k_factor 8 (k_coarse 800): wide shortlist and wide top-k."""
    xt, xb, xq = mg.gmm_case(555, 64, 40, 4000, 4000, 32)
    return (mg.cfg(64, 32, 8, 8, 4000, 4000, 32, 16, 100, n_small=4, pq_niter=6), xt, xb, xq, None), 16, 8, 5, 8.0


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "refine_driver")
    src = os.path.join(HERE, "refine_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + REF, "-o", exe, src, os.path.join(OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def run_case(name):
    base, Mr, nbits_r, r_niter, k_factor = REFINE_CASES[name]()
    c, xt, xb, xq, xids = base
    assert xids is None, "IVFPQR fixtures use sequential ids"
    exe = build_driver()
    # 1. the ordinary fixture (writes tests/golden/<name>.npz)
    mg.CASES[name] = lambda: base
    mg.run_case(name)
    path = os.path.join(HERE, name + ".npz")
    z = np.load(path)
    keep = {k: z[k] for k in z.files}
    # 2. the same first stage again for its index file, then the IVFPQR driver on top of it
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(OUT, "mkl") + ":" + env.get("LD_LIBRARY_PATH", "")
    env["OMP_NUM_THREADS"] = "4"
    with tempfile.TemporaryDirectory() as td:
        fin, fout, fidx, frout = (os.path.join(td, n) for n in ("in.bin", "out.bin", "index.faissindex", "rout.bin"))
        write_tagged(fin, {"cfg": c, "xt": xt, "xb": xb, "xq": xq, "rcfg": np.array([Mr, nbits_r, r_niter], np.int64),
                           "k_factor": np.array([k_factor], np.float32)})
        subprocess.check_call([os.path.join(OUT, "ref_driver"), fin, fout, fidx], env=env)
        subprocess.check_call([exe, fin, fidx, frout], env=env)
        again, out = read_tagged(fout), read_tagged(frout)
    for nm in ("codes", "ids", "keys", "coarse_dis", "pq_centroids", "coarse_centroids"):
        assert np.array_equal(again[nm], keep[nm]), "ref_driver is not reproducible in %s" % nm
    assert int(out["codes_match"][0]) == 1, "the IVFPQR index's first stage differs from the IndexIVFPQ fixture"
    assert np.array_equal(out["keys"], keep["keys"]) and np.array_equal(out["coarse_dis"].view(np.uint32), keep["coarse_dis"].view(np.uint32))
    ids = keep["ids"]
    assert np.array_equal(np.sort(ids), np.arange(ids.size)), "sequential ids expected"
    k = int(c[8])
    kc = int(np.float32(k) * np.float32(k_factor))
    assert out["shortlist"].shape == (xq.shape[0], kc)
    tie = out["boundary_tie"].astype(bool)
    nq = tie.size
    # conditions of the tests, checked against the reference alone
    if name == "refine_duplicates":
        if (~tie).sum() * 4 < nq:
            raise SystemExit("%s: only %d of %d queries without a boundary tie (need a quarter): lower dup or raise nb" % (name, (~tie).sum(), nq))
    elif tie.sum() * 10 > nq:
        raise SystemExit("%s: %d of %d queries have a boundary tie (cap 10 %%): choose another seed" % (name, tie.sum(), nq))
    keep["refine_cfg"] = np.array([Mr, nbits_r, kc], np.int64)
    keep["k_factor"] = np.array([k_factor], np.float32)
    keep["refine_centroids"] = out["refine_centroids"]
    keep["refine_codes"] = out["refine_codes_by_id"][ids]          # by list slot
    for nm in ("shortlist", "shortlist_D", "boundary_tie", "refine_D", "refine_I"):
        keep[nm] = out[nm]
    np.savez_compressed(path, **keep)
    print("%-18s %8.1f KB  k_coarse=%d boundary ties %d/%d, -1 on the shortlist: %d" % (
        name, os.path.getsize(path) / 1024.0, kc, tie.sum(), nq, int((out["shortlist"] == -1).sum())))


if __name__ == "__main__":
    for n in sys.argv[1:] or list(REFINE_CASES):
        run_case(n)
