#!/usr/bin/env python3
"""Generate the IVFFlat fixtures tests/golden/ivfflat/*.npz (a directory of their own: tests/util.py takes every .npz
directly under tests/golden/ for an IVFPQ fixture of make_golden.py).

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/ivfflat_driver.cpp (our
driver over the reference's public API, compiled here into oracle/_ref/) builds IndexFlatL2 / IndexFlatIP + IndexIVFFlat over
given centroids, adds and records: the lists, quantizer->assign keys, D / I of search_preassigned and of search, ndis and
visited lists per query (one-query calls) and, for one fixture, the bytes write_index wrote.

Every fixture is checked against the numpy restatement (tests/ivfflat_ref.py) and for the conditions the tests rely on; a
fixture that misses one is not written.  Fixtures are data only.

  discriminating data   a plain left-to-right sum must differ in bits from the reference's D in at least one slot (general
                        floats, d >= 4; for d < 4 the four-accumulator order and the plain one are the same expression:
                        (x0 + x1) + (x2 + 0))
  no accidental ties    without deliberate duplicates no returned row holds two equal distances
  checkable tie rows    flat_padding_ties: at least a third of the rows have no tie group across the k-th place

    python tests/golden/make_golden_ivfflat.py                  # all cases
    python tests/golden/make_golden_ivfflat.py flat_l2_d32      # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import ivfflat_ref as fr  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
DEST = os.path.join(HERE, "ivfflat")
MET = {"ip": 0, "l2": 1}

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def mixture(seed, d, nc, nb, nq, sigma=0.35, heavy=0):
    """General floats: a Gaussian mixture around nc centres; the centres (slightly moved) are the quantizer's vectors."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((nc, d))
    cent = (centres + 0.05 * rng.standard_normal((nc, d))).astype(np.float32)
    xb = (centres[rng.integers(0, nc, nb - heavy)] + sigma * rng.standard_normal((nb - heavy, d))).astype(np.float32)
    if heavy:
        xb = np.concatenate([xb, (centres[:1] + 0.5 * sigma * rng.standard_normal((heavy, d))).astype(np.float32)])
        xb = xb[rng.permutation(nb)]
    xq = (centres[rng.integers(0, nc, nq)] + sigma * rng.standard_normal((nq, d))).astype(np.float32)
    return cent, xb, xq


def spec(metric, nprobe, k, n_small=0, kill=None, keep_xb=False, dup=False, general=True, want_bytes=False, assign=None, extra_k=()):
    return dict(metric=metric, nprobe=nprobe, k=k, n_small=n_small, kill=kill, keep_xb=keep_xb, dup=dup, general=general,
                want_bytes=want_bytes, assign=assign, extra_k=extra_k)


@case
def flat_l2_d32():
    """d 32, 16 lists, 1500 general floats, nprobe 5, k 10, 40 queries; the stored vectors are kept (add on the device)."""
    return spec("l2", 5, 10, keep_xb=True), mixture(4101, 32, 16, 1500, 40)


@case
def flat_ip_d32():
    return spec("ip", 5, 10, keep_xb=True), mixture(4101, 32, 16, 1500, 40)


@case
def flat_l2_d128_long():
    """d 128, 16 lists, 1200 vectors; add_core with a given assignment: the vectors of two probed lists go to list 0, so that
    one list is longer than two trips of the kernel's 256 lanes and two lists are empty."""
    cent, xb, xq = mixture(4202, 128, 16, 1200, 20, heavy=420)
    a = np.argmin(((xb[:, None, :].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(-1), axis=1).astype(np.int64)
    aq = np.argsort(((xq[:, None, :].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(-1), axis=1)[:, :6]
    probed = [c for c in np.unique(aq) if c != 0]
    a[np.isin(a, probed[:2])] = 0
    return spec("l2", 6, 10, assign=a), (cent, xb, xq)


def _tail(metric, d, seed):
    return spec(metric, 3, 10, want_bytes=(d == 5 and metric == "l2")), mixture(seed, d, 8, 400, 20)


@case
def flat_tail_d30_l2():
    """d % 4 = 2"""
    return _tail("l2", 30, 4301)


@case
def flat_tail_d30_ip():
    return _tail("ip", 30, 4301)


@case
def flat_tail_d5_l2():
    """d % 4 = 1; carries the bytes of the index as write_index wrote them"""
    return _tail("l2", 5, 4302)


@case
def flat_tail_d5_ip():
    return _tail("ip", 5, 4302)


@case
def flat_tail_d3_l2():
    """d < 4: the tail alone"""
    return _tail("l2", 3, 4303)


@case
def flat_tail_d3_ip():
    return _tail("ip", 3, 4303)


def _padding(metric):
    cent, xb, xq = mixture(4404, 16, 8, 70, 24)
    xb = np.concatenate([xb, xb])                   # every vector stored twice: exact ties
    rng = np.random.default_rng(6)
    kill = (rng.random((24, 4)) < 0.45).astype(np.int64)
    kill[0] = [0, 1, 0, 0]
    kill[1] = [1, 1, 1, 1]
    return spec(metric, 4, 47, kill=kill, keep_xb=True, dup=True), (cent, xb, xq)     # odd k: a pair can lie across the k-th place


@case
def flat_padding_ties_l2():
    """8 lists, every vector stored twice, k larger than what some queries scan, -1 keys"""
    return _padding("l2")


@case
def flat_padding_ties_ip():
    return _padding("ip")


@case
def flat_kwide():
    """nprobe = nlist, k 1024 and k 1 on the same data"""
    return spec("l2", 8, 1024, extra_k=(1,)), mixture(4506, 24, 8, 1500, 6)


def _ragged(metric, d, seed):
    """d > 32 with d % 32 != 0: the last 128-byte piece of a row is partial.  add_core with a given assignment (the nearest
    centroid in L2, whatever the metric), so that the heavy centre's list is longer than two trips of the kernel's 256 lanes."""
    cent, xb, xq = mixture(seed, d, 16, 1200, 20, heavy=560)
    a = np.argmin(((xb[:, None, :].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(-1), axis=1).astype(np.int64)
    return spec(metric, 6, 10, assign=a), (cent, xb, xq)


@case
def flat_ragged_d36_l2():
    """d 36: one whole piece and one of 16 bytes"""
    return _ragged("l2", 36, 4707)


@case
def flat_ragged_d100_ip():
    """d 100: three whole pieces and one of 16 bytes"""
    return _ragged("ip", 100, 4708)


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "ivfflat_driver")
    src = os.path.join(HERE, "ivfflat_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + REF, "-o", exe, src, os.path.join(OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def drive(exe, arrays):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(OUT, "mkl") + ":" + env.get("LD_LIBRARY_PATH", "")
    env["OMP_NUM_THREADS"] = "4"
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        write_tagged(fin, arrays)
        subprocess.check_call([exe, fin, fout], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return read_tagged(fout)


def refuse(name, why):
    path = os.path.join(DEST, name + ".npz")
    if os.path.exists(path):
        os.remove(path)
    raise SystemExit("%s: %s -- fixture not written" % (name, why))


def same_rows(D, I, Dr, Ir):
    """D bit-equal; I equal up to the order inside groups of exactly equal D, and free in the group across the k-th place
    (which of several equal heap tops a pop removes is the heap's business) unless that group is the padding."""
    if not np.array_equal(D.view(np.uint32), Dr.view(np.uint32)):
        return False
    k = D.shape[1]
    for r in range(D.shape[0]):
        for v in np.unique(D[r]):
            m = D[r] == v
            if v == D[r, k - 1] and abs(v) != fr.FLT_MAX:
                continue
            if not np.array_equal(np.sort(I[r][m]), np.sort(Ir[r][m])):
                return False
    return True


def tied_rows(D, I):
    """rows with two equal distances among their results"""
    out = np.zeros(D.shape[0], bool)
    for r in range(D.shape[0]):
        v = D[r][I[r] != -1]
        out[r] = np.unique(v).size != v.size
    return out


def run(exe, s, cent, xb, xq, k, nprobe=None):
    nq = xq.shape[0]
    nprobe = nprobe or s["nprobe"]
    kill = s["kill"] if s["kill"] is not None else np.zeros((nq, nprobe), np.int64)
    arrays = {"cfg": np.array([cent.shape[1], cent.shape[0], xb.shape[0], nq, nprobe, k, MET[s["metric"]], s["n_small"]], np.int64),
              "cent": cent, "xb": xb, "xq": xq, "kill": kill}
    if s["assign"] is not None:
        arrays["assign"] = s["assign"]
    if s["want_bytes"]:
        arrays["bytes"] = np.zeros(1, np.uint8)
    out = drive(exe, arrays)
    again = drive(exe, arrays)
    for nm in out:
        if not np.array_equal(out[nm].view(np.uint8), again[nm].view(np.uint8)):
            raise SystemExit("not reproducible in %s" % nm)
    return out


def check_rows(name, s, z, xq, keys, k, D, I):
    Dn, In, nv, nd = fr.search_preassigned(z, xq, keys, k, s["metric"])
    if not same_rows(Dn, In, D, I):
        refuse(name, "the restatement (tests/ivfflat_ref.py) does not reproduce D / I at k = %d" % k)
    return nv, nd


def run_case(name):
    s, (cent, xb, xq) = CASES[name]()
    exe = build_driver()
    d, nlist = cent.shape[1], cent.shape[0]
    out = run(exe, s, cent, xb, xq, s["k"])
    z = {nm: out[nm] for nm in ("list_offsets", "vecs", "ids", "keys", "D", "I", "Ds", "Is", "ndis", "nlistv")}
    z["coarse_centroids"] = cent
    z["xq"] = xq
    for nm, v in (("d", d), ("nlist", nlist), ("nprobe", s["nprobe"]), ("k", s["k"]), ("metric", MET[s["metric"]])):
        z[nm] = np.array(v, np.int64)
    if s["keep_xb"]:
        z["xb"] = xb
    if s["assign"] is not None:
        z["assign"] = s["assign"]
    if s["want_bytes"]:
        z["index_bytes"] = out["index_bytes"]
    for ek in s["extra_k"]:
        o2 = run(exe, s, cent, xb, xq, ek)
        if not np.array_equal(o2["keys"], z["keys"]):
            refuse(name, "keys differ between the runs")
        z["D_k%d" % ek], z["I_k%d" % ek] = o2["D"], o2["I"]
        check_rows(name, s, z, xq, z["keys"], ek, o2["D"], o2["I"])
    lens = np.diff(z["list_offsets"])

    # --- what the tests rely on
    nv, nd = check_rows(name, s, z, xq, z["keys"], s["k"], z["D"], z["I"])
    if not (np.array_equal(nd, z["ndis"]) and np.array_equal(nv, z["nlistv"])):
        refuse(name, "ndis / visited lists differ from the restatement")
    if (z["I"] == -1).all():
        refuse(name, "no result at all")
    if s["general"] and d >= 4 and not fr.discriminates(z, xq, z["keys"], s["k"], s["metric"], z["D"]):
        refuse(name, "a plain left-to-right sum reproduces D: the data cannot tell the summation orders apart")
    if not s["dup"] and tied_rows(z["D"], z["I"]).any():
        refuse(name, "an accidental tie among the results")
    if s["keep_xb"] and s["assign"] is None:
        # the lists are the stored vectors in input order, by the quantizer's 1-NN; and every assignment is decided by a margin
        # no summation order can turn
        x64, c64 = xb.astype(np.float64), cent.astype(np.float64)
        score = x64 @ c64.T if s["metric"] == "ip" else -((x64[:, None, :] - c64[None]) ** 2).sum(-1)
        a = np.argmax(score, axis=1)
        top = np.sort(score, axis=1)
        if ((top[:, -1] - top[:, -2]) <= 1e-4 * np.abs(top).max(axis=1)).any():
            refuse(name, "an assignment is decided by less than 1e-4 of the scores' magnitude")
        for li in range(nlist):
            rows = np.nonzero(a == li)[0]
            o0, o1 = z["list_offsets"][li], z["list_offsets"][li + 1]
            if not (np.array_equal(z["ids"][o0:o1], rows) and np.array_equal(z["vecs"][o0:o1].view(np.uint32), xb[rows].view(np.uint32))):
                refuse(name, "list %d is not the stored vectors in input order" % li)
    if name == "flat_l2_d128_long":
        if lens.max() < 520 or (lens == 0).sum() < 2:
            refuse(name, "needs a list of 520 vectors and two empty lists (longest %d, %d empty)" % (lens.max(), (lens == 0).sum()))
        kk = z["keys"][z["keys"] >= 0]
        if not (lens[kk] == 0).any() or not (lens[kk] >= 520).any():
            refuse(name, "no query probes an empty list / the long list")
    if name.startswith("flat_ragged"):
        kk = z["keys"][z["keys"] >= 0]
        if d <= 32 or d % 32 == 0 or d % 4 != 0 or not (lens[kk] > 520).any():
            refuse(name, "needs d > 32 with a partial last piece and a probed list longer than 520 vectors (longest %d)" % lens.max())
    if name.startswith("flat_padding_ties"):
        I, D, k = z["I"], z["D"], s["k"]
        if not ((I == -1).any(axis=1) & (I != -1).any(axis=1)).any():
            refuse(name, "no partly filled row")
        if not (I == -1).all(axis=1).any():
            refuse(name, "no empty row (all keys -1)")
        pad = np.float32(-fr.FLT_MAX if s["metric"] == "ip" else fr.FLT_MAX)
        if not (D[I == -1].view(np.uint32) == pad.view(np.uint32)).all():
            refuse(name, "padding is not %r" % pad)
        # a tie group across the k-th place: the (k+1)-th best equals the k-th
        Dk1, _I, _v, _n = fr.search_preassigned(z, xq, z["keys"], k + 1, s["metric"])
        across = (Dk1[:, k] == Dk1[:, k - 1]) & (_I[:, k] != -1)
        if not across.any():
            refuse(name, "no tie across the k-th place")
        if (~across).sum() * 3 < across.size:
            refuse(name, "fewer than a third of the rows are free of a tie across the k-th place")
        if not tied_rows(D, I).any():
            refuse(name, "no exact tie among the results")
    if name == "flat_kwide" and ((z["I"][:, -1] == -1).any() or (z["keys"] < 0).any()):
        refuse(name, "a k = 1024 row is not full")
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    if os.path.getsize(path) > 1000000:
        refuse(name, "larger than 1 MB")
    print("%-22s %8.1f KB  ntotal %d longest list %d, %d empty" % (name, os.path.getsize(path) / 1024.0, lens.sum(), lens.max(), (lens == 0).sum()))


def run_coarse_int():
    """Integer-valued centroids, stored vectors and queries: every distance is exact in fp32 in any summation order, so the
    reference's BLAS coarse path (20 queries and more) and its SSE path (fewer) give the keys any exact method gives, and
    the whole search() can be compared.  Rows whose coarse stage has a tie among its nprobe + 1 best are not used."""
    name = "flat_coarse_int"
    exe = build_driver()
    z = {}
    d, nlist, nb, nq, nprobe, k, n_small = 16, 16, 600, 24, 4, 10, 7
    for metric, seed in (("l2", 4601), ("ip", 4602)):
        rng = np.random.default_rng(seed)
        cent = rng.integers(-100, 101, size=(nlist, d)).astype(np.float32)
        xb = (cent[rng.integers(0, nlist, nb)] + rng.integers(-40, 41, size=(nb, d))).astype(np.float32)
        pool = (cent[rng.integers(0, nlist, 4 * nq)] + rng.integers(-40, 41, size=(4 * nq, d))).astype(np.float32)
        score = pool.astype(np.int64) @ cent.astype(np.int64).T if metric == "ip" else \
            -((pool.astype(np.int64)[:, None, :] - cent.astype(np.int64)[None]) ** 2).sum(-1)
        srt = -np.sort(-score, axis=1)
        xq = pool[(np.diff(srt[:, :nprobe + 1], axis=1) != 0).all(axis=1)][:nq]
        if xq.shape[0] != nq:
            refuse(name, "%s: not enough queries without a coarse tie" % metric)
        s = spec(metric, nprobe, k, n_small=n_small, general=False)
        out = run(exe, s, cent, xb, xq, k)
        zz = {nm: out[nm] for nm in ("list_offsets", "vecs", "ids", "keys", "D", "I", "Ds", "Is", "Ds_small", "Is_small")}
        exact = np.argsort(-score[(np.diff(srt[:, :nprobe + 1], axis=1) != 0).all(axis=1)][:nq], axis=1, kind="stable")[:, :nprobe]
        if not np.array_equal(exact, zz["keys"]):
            refuse(name, "%s: the reference's keys are not the exact ones" % metric)
        check_rows(name, s, zz, xq, zz["keys"], k, zz["D"], zz["I"])
        if not (same_rows(zz["Ds"], zz["Is"], zz["D"], zz["I"]) and same_rows(zz["Ds_small"], zz["Is_small"], zz["D"][:n_small], zz["I"][:n_small])):
            refuse(name, "%s: search differs from search_preassigned over the same keys" % metric)
        if tied_rows(zz["D"], zz["I"]).any():
            refuse(name, "%s: an accidental tie among the results" % metric)
        zz["coarse_centroids"], zz["xq"], zz["xb"] = cent, xq, xb
        for nm, v in zz.items():
            z[metric + "_" + nm] = v
    for nm, v in (("d", d), ("nlist", nlist), ("nprobe", nprobe), ("k", k), ("n_small", n_small)):
        z[nm] = np.array(v, np.int64)
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    print("%-22s %8.1f KB" % (name, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    os.makedirs(DEST, exist_ok=True)
    for n in sys.argv[1:] or list(CASES) + ["flat_coarse_int"]:
        run_coarse_int() if n == "flat_coarse_int" else run_case(n)
