#!/usr/bin/env python3
"""Generate the IndexRefineFlat fixtures tests/golden/refineflat/*.npz.

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/refineflat_driver.cpp (our
driver over the reference's public API, compiled here into oracle/_ref/) builds the reference's IndexRefineFlat over an
IndexIVFPQ (L2 cases: the shortlist's distances are approximate, so re-scoring changes them) or an IndexIVFFlat (inner-product
cases: the reference's IndexIVFPQ has no inner-product metric) on given centroids, adds with sequential ids and records:

    xb, xq, k, k_factor, metric (0 inner product, 1 L2), nprobe, base_kind (0 IndexIVFPQ, 1 IndexIVFFlat), nlist, M, nbits
    base_D / base_I    the base's own search at k_base = idx_t(k * k_factor)
    sub_D              what IndexFlat::compute_distance_subset left in a copy of base_D
    D / I              IndexRefineFlat::search
    boundary_tie [nq]  1 where the base's k_base-th place lies inside a group of equal base distances (its shortlist then
                       depends on its heap's history)
    whole-search cases (WHOLE): coarse_centroids, list_offsets, ids and codes + pq_centroids + table_mode, or vecs -- the arrays
                       of the IVFPQ / IVFFlat fixtures

Every fixture is checked against the numpy restatement (tests/refineflat_ref.py: sub_D bit for bit, D / I by assert_same_topk)
and for the conditions the tests rely on; a fixture that misses one is not written, the next seed is tried (20 at most):

  general floats   no row has two equal refined distances among the live entries of its top k + 1, and at least 3 / 4 of the
                   rows have boundary_tie == 0  (reached with the first seed of every case, with a share of 1.0: no row of any
                   general-float fixture has a boundary tie)
  ties             at least half of the rows have no tie group across the k-th place and at least one row has one (first seed;
                   10 of its 33 rows have a boundary tie in the base, which the seam tests do not depend on)

Fixtures are data only.

    python tests/golden/make_golden_refineflat.py                  # all cases
    python tests/golden/make_golden_refineflat.py tail_d3_l2       # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]
import refineflat_ref as rr  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402
from util import assert_same_topk  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
DEST = os.path.join(HERE, "refineflat")
LARGEST_FIXTURE = 989774      # bytes of tests/golden/c1_small.npz: every fixture here stays below it
WHOLE = ("l2_ivfpq_d32", "ip_ivfflat_d32", "padded", "padded_ip", "kfactor_1")
SEEDS = 20


def mixture(seed, d, nc, nb, nq, nt=0, sigma=0.35, dup=False):
    """General floats: a Gaussian mixture around nc centres; the centres (slightly moved) are the quantizer's vectors.
    dup: half of the distinct vectors are stored twice."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((nc, d))
    cent = (centres + 0.05 * rng.standard_normal((nc, d))).astype(np.float32)
    draw = lambda n: (centres[rng.integers(0, nc, n)] + sigma * rng.standard_normal((n, d))).astype(np.float32)  # noqa: E731
    if dup:
        distinct = draw(nb * 2 // 3)
        xb = np.concatenate([distinct, distinct[:nb - distinct.shape[0]]])[rng.permutation(nb)]
    else:
        xb = draw(nb)
    return cent, xb, draw(nq), draw(nt)


# name -> dict(kind, metric, d, nlist, M, nbits, nb, nq, nprobe, k, k_factor, seed0[, dup])
CASES = {
    "l2_ivfpq_d32":   dict(kind=0, metric=1, d=32, nlist=16, M=4, nbits=8, nb=2000, nq=33, nprobe=4, k=10, k_factor=4.0, seed0=100),
    "ip_ivfflat_d32": dict(kind=1, metric=0, d=32, nlist=16, M=0, nbits=0, nb=2000, nq=33, nprobe=4, k=10, k_factor=4.0, seed0=120),
    "tail_d3_l2":     dict(kind=0, metric=1, d=3, nlist=8, M=3, nbits=4, nb=600, nq=33, nprobe=3, k=5, k_factor=4.0, seed0=140),
    "tail_d3_ip":     dict(kind=1, metric=0, d=3, nlist=8, M=0, nbits=0, nb=600, nq=33, nprobe=3, k=5, k_factor=4.0, seed0=160),
    "tail_d5_l2":     dict(kind=0, metric=1, d=5, nlist=8, M=5, nbits=4, nb=600, nq=33, nprobe=3, k=5, k_factor=4.0, seed0=180),
    "tail_d5_ip":     dict(kind=1, metric=0, d=5, nlist=8, M=0, nbits=0, nb=600, nq=33, nprobe=3, k=5, k_factor=4.0, seed0=200),
    "tail_d30_l2":    dict(kind=0, metric=1, d=30, nlist=8, M=5, nbits=6, nb=600, nq=33, nprobe=3, k=5, k_factor=4.5, seed0=220),
    "tail_d30_ip":    dict(kind=1, metric=0, d=30, nlist=8, M=0, nbits=0, nb=600, nq=33, nprobe=3, k=5, k_factor=4.5, seed0=240),
    # 200 floats: six whole 128-byte pieces and a ragged seventh of 32 bytes
    "wide_d200_l2":   dict(kind=0, metric=1, d=200, nlist=8, M=8, nbits=6, nb=400, nq=20, nprobe=3, k=5, k_factor=4.0, seed0=260),
    # sixteen trips of 64 candidates, four waves, the 1024-key sort
    "kbase_1024":     dict(kind=0, metric=1, d=16, nlist=4, M=4, nbits=6, nb=1500, nq=12, nprobe=4, k=256, k_factor=4.0, seed0=280),
    "kfactor_1":      dict(kind=0, metric=1, d=32, nlist=16, M=4, nbits=8, nb=2000, nq=33, nprobe=4, k=10, k_factor=1.0, seed0=300),
    # one probe of lists of about 5 vectors at k_base 40: rows end in -1 / FLT_MAX (-FLT_MAX) entries
    "padded":         dict(kind=0, metric=1, d=16, nlist=64, M=4, nbits=6, nb=320, nq=33, nprobe=1, k=10, k_factor=4.0, seed0=320),
    "padded_ip":      dict(kind=1, metric=0, d=16, nlist=64, M=0, nbits=0, nb=320, nq=33, nprobe=1, k=10, k_factor=4.0, seed0=340),
    "ties":           dict(kind=0, metric=1, d=16, nlist=8, M=4, nbits=6, nb=1000, nq=33, nprobe=3, k=7, k_factor=4.0, seed0=360, dup=True),
}


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "refineflat_driver")
    src = os.path.join(HERE, "refineflat_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + REF, "-o", exe, src, os.path.join(OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def run_driver(exe, c, seed):
    cent, xb, xq, xt = mixture(seed, c["d"], c["nlist"], c["nb"], c["nq"], nt=3000 if c["kind"] == 0 else 0, dup=c.get("dup", False))
    cfg = np.array([c["d"], c["nlist"], c["M"], c["nbits"], xt.shape[0], xb.shape[0], c["nq"], c["nprobe"], c["k"], c["kind"], c["metric"], 6],
                   np.int64)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(OUT, "mkl") + ":" + env.get("LD_LIBRARY_PATH", "")
    env["OMP_NUM_THREADS"] = "4"
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        arrays = {"cfg": cfg, "k_factor": np.array([c["k_factor"]], np.float32), "cent": cent, "xb": xb, "xq": xq}
        if c["kind"] == 0:
            arrays["xt"] = xt
        write_tagged(fin, arrays)
        subprocess.check_call([exe, fin, fout], env=env)
        out = read_tagged(fout)
    return cent, xb, xq, out


def check(name, c, xb, xq, out):
    """None when the fixture holds every condition, else what it misses"""
    k, metric = c["k"], c["metric"]
    kb = rr.k_base(k, c["k_factor"])
    assert out["base_I"].shape == (c["nq"], kb), (out["base_I"].shape, kb)
    live = out["base_I"] >= 0
    assert (out["base_I"][live] < xb.shape[0]).all()
    sub = rr.compute_distance_subset(xb, xq, out["base_I"], out["base_D"], metric)
    assert rr.same_bits(sub, out["sub_D"]), "%s: the restatement's distances differ from the reference's" % name
    Dw, Iw = rr.reorder(sub, out["base_I"], k, metric)
    assert_same_topk(Dw, Iw, out["D"], out["I"], name + ": restatement against the reference")
    m = min(k + 1, kb)
    Dm, Im = rr.reorder(sub, out["base_I"], m, metric)
    equal = (Dm[:, 1:] == Dm[:, :-1]) & (Im[:, 1:] >= 0) & (Im[:, :-1] >= 0)
    tie = out["boundary_tie"].astype(bool)
    if name == "ties":
        across = equal[:, k - 1] if m > k else np.zeros(c["nq"], bool)
        if across.sum() * 2 > c["nq"] or across.sum() == 0:
            return "%d of %d rows have a tie group across the k-th place" % (across.sum(), c["nq"])
        if not equal.any():
            return "no refined ties"
        return None
    if equal.any():
        return "%d rows hold two equal refined distances in their top k + 1" % equal.any(axis=1).sum()
    if (~tie).sum() * 4 < 3 * c["nq"]:
        return "only %d of %d rows without a boundary tie" % ((~tie).sum(), c["nq"])
    if name.startswith("padded") and live.all():
        return "no padded row"
    return None


def run_case(name):
    c = CASES[name]
    exe = build_driver()
    for seed in range(c["seed0"], c["seed0"] + SEEDS):
        cent, xb, xq, out = run_driver(exe, c, seed)
        miss = check(name, c, xb, xq, out)
        if miss is None:
            break
        print("%s: seed %d: %s" % (name, seed, miss))
    else:
        raise SystemExit("%s: no seed of %d meets the conditions" % (name, SEEDS))
    keep = {"xb": xb, "xq": xq, "k": np.int64(c["k"]), "k_factor": np.float32(c["k_factor"]), "metric": np.int64(c["metric"]),
            "nprobe": np.int64(c["nprobe"]), "base_kind": np.int64(c["kind"]), "nlist": np.int64(c["nlist"]), "M": np.int64(c["M"]),
            "nbits": np.int64(c["nbits"]), "seed": np.int64(seed)}
    for nm in ("base_D", "base_I", "sub_D", "D", "I", "boundary_tie"):
        keep[nm] = out[nm]
    if name in WHOLE:
        ids = out["ids"]
        assert np.array_equal(np.sort(ids), np.arange(xb.shape[0])), "sequential ids expected"
        keep["coarse_centroids"] = cent
        for nm in ("list_offsets", "ids") + (("codes", "pq_centroids", "table_mode") if c["kind"] == 0 else ("vecs",)):
            keep[nm] = out[nm]
    os.makedirs(DEST, exist_ok=True)
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **keep)
    size = os.path.getsize(path)
    if size >= LARGEST_FIXTURE:
        os.remove(path)
        raise SystemExit("%s: %d bytes, not below the largest fixture (%d)" % (name, size, LARGEST_FIXTURE))
    tie = out["boundary_tie"].astype(bool)
    print("%-16s %7.1f KB  seed %d  k_base=%d  boundary ties %d/%d  skipped entries %d" % (
        name, size / 1024.0, seed, out["base_I"].shape[1], tie.sum(), tie.size, int((out["base_I"] < 0).sum())))


if __name__ == "__main__":
    for n in sys.argv[1:] or list(CASES):
        run_case(n)
