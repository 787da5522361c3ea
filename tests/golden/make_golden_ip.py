#!/usr/bin/env python3
"""Generate the inner-product fixtures tests/golden/ip/ip_*.npz (a directory of their own: tests/util.py takes every
.npz directly under tests/golden/ for an L2 fixture of make_golden.py).

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/ip_driver.cpp (our
driver over the reference's public API, compiled here into oracle/_ref/) builds IndexFlatIP + IndexIVFPQ with metric_type =
METRIC_INNER_PRODUCT, trains, adds and records: coarse and PQ centroids, the lists, the queries, quantizer->search keys and
distances, search_knn_with_key D / I / pairs, ncode per query (one-query calls), encode_multiple assignments and codes.

ip_coarse_int holds the coarse-only arrays: centroids and queries are small integers, so every inner product is exact in
fp32 in any summation order and the reference's BLAS path (20 queries and more), its SSE path (one-query calls) and an int64
dot product agree bit for bit -- checked here.  Every fixture is checked against the numpy restatement (tests/ip_ref.py)
and for the conditions the tests rely on; a fixture that misses one is not written.  Fixtures are data only.

    python tests/golden/make_golden_ip.py                  # all cases
    python tests/golden/make_golden_ip.py ip_residual      # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import ip_ref  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
DEST = os.path.join(HERE, "ip")

IP_CASES = {}


def icase(fn):
    IP_CASES[fn.__name__] = fn
    return fn


def signed_like(rng, n, d, centres, sigma):
    """Gaussian mixture rounded to integers in -128 .. 127 (exactly representable, keeps fixtures small)."""
    pick = rng.integers(0, centres.shape[0], size=n)
    x = centres[pick] + sigma * rng.standard_normal((n, d))
    return np.clip(np.rint(x * 255.0) - 128.0, -128, 127).astype(np.float32)


def mixture(seed, d, nc, nt, nb, nq, heavy=0, sigma=0.08):
    rng = np.random.default_rng(seed)
    centres = rng.random((nc, d))
    xt = signed_like(rng, nt, d, centres, sigma)
    xb = signed_like(rng, nb - heavy, d, centres, sigma)
    if heavy:
        xb = np.concatenate([xb, signed_like(rng, heavy, d, centres[:1], sigma * 0.5)])
        xb = xb[rng.permutation(xb.shape[0])]
    xq = signed_like(rng, nq, d, centres, sigma)
    return xt, xb, xq


def spec(d, nlist, M, nbits, nprobe, k, by_residual=1, max_codes=0, km_niter=8, pq_niter=6, n_enc=200, keep_xb=False, empty=0,
         kill=None):
    return dict(d=d, nlist=nlist, M=M, nbits=nbits, nprobe=nprobe, k=k, by_residual=by_residual, max_codes=max_codes,
                km_niter=km_niter, pq_niter=pq_niter, n_enc=n_enc, keep_xb=keep_xb, empty=empty, kill=kill)


@icase
def ip_residual():
    """d 32, 16 lists, M 8 x 8 bit, nprobe 5, k 10, 40 queries; the stored vectors are kept (add on the device)."""
    return spec(32, 16, 8, 8, 5, 10, keep_xb=True), mixture(2101, 32, 16, 3000, 1500, 40)


@icase
def ip_nonresidual():
    """The same with by_residual = 0."""
    return spec(32, 16, 8, 8, 5, 10, by_residual=0, keep_xb=True), mixture(2101, 32, 16, 3000, 1500, 40)


@icase
def ip_m16_d128():
    """d 128, 64 lists, M 16 (the headline's code size), nprobe 8, k 10; one list longer than two trips of the kernel (512
    codes), several empty lists."""
    return spec(128, 64, 16, 8, 8, 10, empty=3), mixture(2202, 128, 64, 5000, 3000, 40, heavy=700)


@icase
def ip_padding_ties():
    """8 lists; vectors stored twice and lists of identical codes; k larger than the codes a query scans (-FLT_MAX / -1 rows);
    keys with -1 entries; a max_codes cut that falls inside the probe list."""
    xt, xb, xq = mixture(2303, 16, 8, 1500, 60, 24)
    xb = np.concatenate([xb, xb[:30], np.repeat(xb[40:42], 12, axis=0)])
    rng = np.random.default_rng(5)
    kill = (rng.random((24, 4)) < 0.2).astype(np.int64)
    kill[0] = [0, 1, 0, 0]
    kill[1] = [1, 1, 1, 1]
    return spec(16, 8, 4, 8, 4, 96, max_codes=40, n_enc=xb.shape[0], keep_xb=True, kill=kill), (xt, xb, xq)


@icase
def ip_kwide():
    """k 1024 on about 3000 vectors."""
    return spec(32, 8, 8, 8, 8, 1024, n_enc=100), mixture(2404, 32, 8, 3000, 3000, 6)


@icase
def ip_m20_d40():
    """M 20 and d 40: a code size outside the powers of two."""
    return spec(40, 24, 20, 8, 6, 10), mixture(2505, 40, 24, 3000, 2000, 40, heavy=300)


@icase
def ip_d30_m6():
    """d 30 (d % 4 != 0: the tail rule of dis0), M 6 x 6 bit (dsub 5): a shape outside the engineered kernel."""
    return spec(30, 12, 6, 6, 4, 10), mixture(2606, 30, 12, 2000, 1200, 40)


@icase
def ip_m24_d48():
    """M 24 and d 48: a code of six words, read by three 8-byte loads; one list longer than two trips of the kernel."""
    return spec(48, 24, 24, 8, 6, 10), mixture(2707, 48, 24, 3000, 2000, 40, heavy=600)


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "ip_driver")
    src = os.path.join(HERE, "ip_driver.cpp")
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
    """D bit-equal, I equal up to the order inside groups of exactly equal D; in the group that touches the k-th place the
    choice among equal candidates is free (which of several equal heap tops a pop removes is the heap's business)."""
    if not np.array_equal(D.view(np.uint32), Dr.view(np.uint32)):
        return False
    k = D.shape[1]
    for r in range(D.shape[0]):
        last = int(np.argmax(D[r] == D[r, k - 1]))        # first slot of the last group
        a, b = I[r][np.lexsort((I[r], -D[r]))], Ir[r][np.lexsort((Ir[r], -Dr[r]))]
        if not np.array_equal(a[:last], b[:last]):
            return False
        if not np.array_equal(a[last:], b[last:]) and D[r, k - 1] == -ip_ref.FLT_MAX:
            return False
    return True


def run_case(name):
    s, (xt, xb, xq) = IP_CASES[name]()
    exe = build_driver()
    nq = xq.shape[0]
    kill = s["kill"] if s["kill"] is not None else np.zeros((nq, s["nprobe"]), np.int64)

    def go(xb_):
        cfg = np.array([s["d"], s["nlist"], s["M"], s["nbits"], xt.shape[0], xb_.shape[0], nq, s["nprobe"], s["k"], s["max_codes"],
                        s["km_niter"], s["pq_niter"], s["by_residual"], xb_.shape[0] if s["keep_xb"] else min(s["n_enc"], xb_.shape[0])], np.int64)
        return drive(exe, {"cfg": cfg, "xt": xt, "xb": xb_, "xq": xq, "kill": kill})

    out = go(xb)
    if s["empty"]:
        # empty lists: store the vectors again without those of the shortest lists (the training set decides the lists)
        full = dict(s, n_enc=xb.shape[0])
        cfg_all = np.array([s["d"], s["nlist"], s["M"], s["nbits"], xt.shape[0], xb.shape[0], nq, s["nprobe"], s["k"], s["max_codes"],
                            s["km_niter"], s["pq_niter"], s["by_residual"], full["n_enc"]], np.int64)
        assign = drive(exe, {"cfg": cfg_all, "xt": xt, "xb": xb, "xq": xq, "kill": kill})["enc_assign"]
        lens = np.diff(out["list_offsets"])
        # among the lists the queries probe, so that the scan meets them
        probed = np.unique(out["keys"][out["keys"] >= 0])
        drop = probed[np.argsort(lens[probed], kind="stable")[:s["empty"]]]
        xb = xb[~np.isin(assign, drop)]
        out = go(xb)
    again = go(xb)
    for nm in out:
        if not np.array_equal(out[nm].view(np.uint8), again[nm].view(np.uint8)):
            refuse(name, "not reproducible in %s" % nm)

    z = {nm: out[nm] for nm in ("coarse_centroids", "pq_centroids", "list_offsets", "codes", "ids", "keys", "coarse_dis", "D", "I",
                                "I_pairs", "ncode", "enc_assign", "enc_codes")}
    for nm in ("d", "nlist", "M", "nbits", "nprobe", "k", "by_residual", "max_codes"):
        z[nm] = np.array(s[nm], np.int64)
    z["xq"] = xq
    n_enc = z["enc_assign"].shape[0]
    z["enc_x"] = xb[:n_enc]
    if s["keep_xb"]:
        z["xb"] = xb
    lens = np.diff(z["list_offsets"])

    # --- what the tests rely on
    D, I, nc = ip_ref.search_preassigned(z, xq, z["keys"], s["k"])
    if not same_rows(D, I, z["D"], z["I"]):
        refuse(name, "the restatement (tests/ip_ref.py) does not reproduce D / I")
    Dp, Ip, _ = ip_ref.search_preassigned(z, xq, z["keys"], s["k"], store_pairs=True)
    if not same_rows(Dp, Ip, z["D"], z["I_pairs"]):
        refuse(name, "the restatement does not reproduce the pairs")
    if not np.array_equal(nc, z["ncode"]):
        refuse(name, "ncode differs from the list sizes")
    # the assignment of add / encode: first maximum, and decided by a margin no summation order can turn
    ipd = z["enc_x"].astype(np.float64) @ z["coarse_centroids"].astype(np.float64).T
    top = np.sort(ipd, axis=1)
    scale = np.abs(z["enc_x"].astype(np.float64)) @ np.abs(z["coarse_centroids"].astype(np.float64)).T
    if not np.array_equal(np.argmax(ipd, axis=1), z["enc_assign"]):
        refuse(name, "encode_multiple does not assign to the largest inner product")
    if ((top[:, -1] - top[:, -2]) <= 1e-5 * scale.max(axis=1)).any():
        refuse(name, "an assignment is decided by less than 1e-5 of the products' magnitude")
    if s["keep_xb"]:
        if n_enc != xb.shape[0]:
            refuse(name, "keep_xb needs every stored vector encoded")
        # the lists are the encoded vectors in input order
        for li in range(s["nlist"]):
            rows = np.nonzero(z["enc_assign"] == li)[0]
            o0, o1 = z["list_offsets"][li], z["list_offsets"][li + 1]
            if not (np.array_equal(z["ids"][o0:o1], rows) and np.array_equal(z["codes"][o0:o1], z["enc_codes"][rows])):
                refuse(name, "list %d is not the encoded vectors in input order" % li)
    if (z["I"] == -1).all(axis=1).all():
        refuse(name, "no result at all")
    if name == "ip_m16_d128":
        if not (lens > 512).any() or (lens == 0).sum() < 3:
            refuse(name, "needs a list longer than 512 codes and three empty lists (longest %d, %d empty)" % (lens.max(), (lens == 0).sum()))
        if not (lens[z["keys"][z["keys"] >= 0]] == 0).any():
            refuse(name, "no query probes an empty list")
    if name == "ip_m24_d48":
        kk = z["keys"][z["keys"] >= 0]
        if not (lens[kk] > 512).any():
            refuse(name, "no query probes a list longer than 512 codes (longest %d)" % lens.max())
    if name == "ip_padding_ties":
        cut = [(np.cumsum(lens[kq[kq >= 0]]) >= s["max_codes"]).argmax() + 1 < (kq >= 0).sum() if (np.cumsum(lens[kq[kq >= 0]]) >= s["max_codes"]).any() else False
               for kq in z["keys"]]
        if not any(cut):
            refuse(name, "no max_codes cut inside a probe list")
        if not ((z["I"] == -1).any(axis=1) & (z["I"] != -1).any(axis=1)).any():
            refuse(name, "no partly filled row")
        if not (z["I"] == -1).all(axis=1).any():
            refuse(name, "no empty row (all keys -1)")
        if not (z["D"][:, :-1] == z["D"][:, 1:])[z["I"][:, 1:] != -1].any():
            refuse(name, "no exact tie among the results")
        if not (z["D"][z["I"] == -1].view(np.uint32) == np.float32(-ip_ref.FLT_MAX).view(np.uint32)).all():
            refuse(name, "padding is not -FLT_MAX")
    if name == "ip_kwide" and (z["I"][:, -1] == -1).any():
        refuse(name, "a k = 1024 row is not full")
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    if os.path.getsize(path) >= 1 << 20:
        refuse(name, "larger than 1 MiB")
    print("%-18s %8.1f KB  ntotal %d longest list %d, %d empty" % (name, os.path.getsize(path) / 1024.0, lens.sum(), lens.max(), (lens == 0).sum()))


def coarse_int_set(exe, seed, d, nlist, nq, nprobe, amp, ndup):
    """Integer centroids / queries.  The reference leaves equal values among the KEPT columns in its heap's pop order, which is
    no rule to test against; so the rows are chosen from a pool: those whose nprobe largest products are distinct, the ones
    with a tie on the boundary (nprobe-th = (nprobe+1)-th largest) first.  On the chosen rows the reference's two paths and
    the (largest ip, lowest id) rule of tests/ip_ref.py must agree bit for bit."""
    rng = np.random.default_rng(seed)
    cent = rng.integers(-amp, amp + 1, size=(nlist, d)).astype(np.float32)
    for j in range(ndup):                      # equal centroids: exact ties
        cent[nlist - 1 - j] = cent[j]
    pool = rng.integers(-amp, amp + 1, size=(20 * nq, d)).astype(np.float32)

    def check(xq):
        out = drive(exe, {"ci_cfg": np.array([d, nlist, xq.shape[0], nprobe], np.int64), "ci_cent": cent, "ci_xq": xq})
        exact = xq.astype(np.int64) @ cent.astype(np.int64).T
        keys, dis = ip_ref.coarse_search(cent, xq, nprobe)
        assert np.array_equal(dis.astype(np.int64), np.take_along_axis(exact, keys, axis=1)), "fp32 products are not exact"
        ok = np.ones(xq.shape[0], bool)
        for a, b in (("ci_keys", keys), ("ci_keys1", keys), ("ci_dis", dis), ("ci_dis1", dis)):
            ok &= (out[a].view(np.uint8).reshape(xq.shape[0], -1) == b.view(np.uint8).reshape(xq.shape[0], -1)).all(axis=1)
        srt = -np.sort(-exact, axis=1)
        distinct = (np.diff(srt[:, :nprobe], axis=1) != 0).all(axis=1)
        boundary = srt[:, nprobe - 1] == srt[:, nprobe]
        return ok, distinct, boundary, keys, dis

    ok, distinct, boundary, _k, _d = check(pool)
    good = ok & distinct
    rows = np.concatenate([np.nonzero(good & boundary)[0][:nq // 4], np.nonzero(good & ~boundary)[0]])[:nq]
    rows.sort()
    xq = pool[rows]
    ok, distinct, boundary, keys, dis = check(xq)
    if xq.shape[0] != nq or not (ok & distinct).all() or boundary.sum() < 2:
        return None
    return {"cent": cent, "xq": xq, "keys": keys, "dis": dis, "nprobe": np.array(nprobe, np.int64)}


def run_coarse_int():
    exe = build_driver()
    z = {}
    for tag, args in (("a", (3100, 32, 16, 40, 5, 8, 3)), ("b", (3300, 64, 256, 40, 8, 4, 6))):
        r = coarse_int_set(exe, *args)
        if r is None:
            refuse("ip_coarse_int", "set %s: no seed where the reference's SSE path, its BLAS path and the int64 products agree "
                   "on the (largest ip, lowest id) order with a boundary tie" % tag)
        for nm, v in r.items():
            z[tag + "_" + nm] = v
    path = os.path.join(DEST, "ip_coarse_int.npz")
    np.savez_compressed(path, **z)
    print("%-18s %8.1f KB" % ("ip_coarse_int", os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    os.makedirs(DEST, exist_ok=True)
    for n in sys.argv[1:] or list(IP_CASES) + ["ip_coarse_int"]:
        run_coarse_int() if n == "ip_coarse_int" else run_case(n)
