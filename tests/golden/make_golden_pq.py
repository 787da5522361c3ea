#!/usr/bin/env python3
"""Generate the flat PQ fixtures tests/golden/pq/*.npz (a directory of their own: tests/util.py takes every .npz directly
under tests/golden/ for an IVFPQ fixture of make_golden.py).

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/pq_driver.cpp (our driver
over the reference's public API, compiled here into oracle/_ref/) builds a faiss::IndexPQ over given centroids, adds (or takes
given codes), searches once per polysemous_ht and records: the codes, D / I, indexPQ_stats, the queries' tables and codes and,
for one fixture, the bytes write_index wrote.  Fixtures are data only.

Every fixture is checked against the numpy restatement (tests/pq_ref.py) and for the conditions the tests rely on; a fixture
that misses one is not written.

  discriminating    grouped order (M % 4 == 0, M > 4): a plain left-to-right sum differs in bits from the reference's D in at
                    least one slot; M % 4 != 0: the grouped sum would differ
  no accidental ties  outside pq_ties no returned row holds two equal distances
  pq_ties           built from duplicated codes; at least a third of its rows have no tie group across the k-th place
  polysemous        at the low threshold between 0.5 % and 20 % of the codes pass per query on average, and some query leaves
                    fewer than k passers

    python tests/golden/make_golden_pq.py                  # all cases
    python tests/golden/make_golden_pq.py pq_m4_d16        # one case
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import pq_ref as pr  # noqa: E402
from tagged import read_tagged, write_tagged  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref")
DEST = os.path.join(HERE, "pq")
MET = {"ip": 0, "l2": 1}
TABLE_ROWS = 4          # queries whose tables a fixture carries (all of them in pq_blas_d128_m4)

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def data(seed, d, M, nbits, nb, nq, nc=24, sigma=1.0):
    """General floats: a Gaussian mixture; the centroids of sub-quantizer m are stored sub-vectors, slightly moved."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((nc, d))
    xb = (centres[rng.integers(0, nc, nb)] + sigma * rng.standard_normal((nb, d))).astype(np.float32)
    xq = (centres[rng.integers(0, nc, nq)] + sigma * rng.standard_normal((nq, d))).astype(np.float32)
    ksub, dsub = 1 << nbits, d // M
    pool = (centres[rng.integers(0, nc, ksub)] + sigma * rng.standard_normal((ksub, d))).astype(np.float32)
    cent = np.ascontiguousarray(pool.reshape(ksub, M, dsub).transpose(1, 0, 2))
    cent = (cent + 0.02 * rng.standard_normal(cent.shape)).astype(np.float32)
    return cent, xb, xq


def spec(d, M, k, metric="l2", nbits=8, st=pr.ST_PQ, nb=2000, nq=32, seed=0, keep_xb=False, want_bytes=False, hts=None, dup=False,
         small_nb=0, blas=False):
    return dict(d=d, M=M, k=k, metric=metric, nbits=nbits, st=st, nb=nb, nq=nq, seed=seed, keep_xb=keep_xb, want_bytes=want_bytes, hts=hts,
                dup=dup, small_nb=small_nb, blas=blas)


@case
def pq_m4_d16():
    """M == 4: ((t0 + t1) + t2) + t3.  Keeps the stored vectors (add on the device) and the bytes write_index wrote."""
    return spec(16, 4, 10, seed=5101, keep_xb=True, want_bytes=True)


@case
def pq_m16_d64_l2():
    """the grouped order, L2"""
    return spec(64, 16, 10, seed=5102, nb=3000)


@case
def pq_m16_d64_ip():
    return spec(64, 16, 10, metric="ip", seed=5102, nb=3000)


@case
def pq_m6_d30():
    """M % 4 != 0: from 0, left to right; dsub 5.  Keeps the stored vectors."""
    return spec(30, 6, 10, seed=5103, keep_xb=True)


@case
def pq_m8_nbits6():
    """ksub 64"""
    return spec(32, 8, 10, nbits=6, seed=5104)


@case
def pq_kwide():
    """k 1024 over 1500 codes; and over the first 600 of them: k > ntotal"""
    return spec(32, 8, 1024, seed=5105, nb=1500, nq=30, small_nb=600)


@case
def pq_ties():
    """half of the codes stored twice: exact ties; odd k, so that a pair can lie across the k-th place"""
    return spec(32, 8, 47, seed=5106, nb=1600, dup=True)


def _poly(M, seed):
    return spec(4 * M, M, 40, st=pr.ST_POLYSEMOUS, seed=seed, hts="poly")


@case
def pq_poly_m8():
    return _poly(8, 5108)


@case
def pq_poly_m16():
    return _poly(16, 5116)


@case
def pq_poly_m24():
    return _poly(24, 5124)


@case
def pq_poly_m32():
    return _poly(32, 5132)


@case
def pq_polygen_m16():
    """the generalized-Hamming filter: hd = differing bytes"""
    return spec(64, 16, 150, st=pr.ST_POLYSEMOUS_GENERALIZE, seed=5140, hts="gen")


@case
def pq_sdc_m8():
    return spec(32, 8, 10, st=pr.ST_SDC, seed=5150)


@case
def pq_blas_d128_m4():
    """dsub 32: the reference's tables come from BLAS; the fixture carries all of them"""
    return spec(128, 4, 10, seed=5160, nb=1500, blas=True)


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "pq_driver")
    src = os.path.join(HERE, "pq_driver.cpp")
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


def run(exe, s, cent, xq, k, xb=None, codes=None, hts=None):
    arrays = {"cfg": np.array([s["d"], s["M"], s["nbits"], (xb if codes is None else codes).shape[0], xq.shape[0], k, MET[s["metric"]], s["st"]],
                              np.int64), "cent": cent, "xq": xq}
    if codes is None:
        arrays["xb"] = xb
    else:
        arrays["codes"] = codes
    if hts is not None:
        arrays["hts"] = np.asarray(hts, np.int64)
    if s["want_bytes"]:
        arrays["bytes"] = np.zeros(1, np.uint8)
    out = drive(exe, arrays)
    again = drive(exe, arrays)
    for nm in out:
        if not np.array_equal(out[nm].view(np.uint8), again[nm].view(np.uint8)):
            raise SystemExit("not reproducible in %s" % nm)
    return out


def tied_rows(D, I):
    out = np.zeros(D.shape[0], bool)
    for r in range(D.shape[0]):
        v = D[r][I[r] != -1]
        out[r] = np.unique(v).size != v.size
    return out


def pick_hts(name, s, cent, codes, xq):
    """low (0.5 % .. 20 % pass on average, some query with fewer than k passers), middle, all pass"""
    M, gen = s["M"], s["st"] == pr.ST_POLYSEMOUS_GENERALIZE
    qc = pr.first_argmin_codes(pr.tables(xq, cent, "l2"))
    hd = np.stack([pr.hamming(codes, q, gen) for q in qc])          # [nq][nb]
    top = M + 1 if gen else 8 * M + 1
    low = None
    for ht in range(1, top):
        npass = (hd < ht).sum(axis=1)
        if npass.mean() > 0.20 * codes.shape[0]:
            break
        if npass.mean() >= 0.005 * codes.shape[0] and npass.min() < s["k"]:
            low = ht
    if low is None:
        refuse(name, "no threshold passes 0.5 %% .. 20 %% of the codes with a query short of k = %d passers" % s["k"])
    # middle: half of the bits may differ (about half of the codes pass); the byte filter has no such middle
    return [low, top] if gen else [low, 4 * M, top]


class AccidentalTie(Exception):
    pass


def run_case(name):
    """the first of the seeds seed, seed + 1, ... whose results hold no accidental tie (k = 1024 float sums collide now and then)"""
    s = CASES[name]()
    for attempt in range(40):
        try:
            return run_seed(name, dict(s, seed=s["seed"] + attempt))
        except AccidentalTie:
            continue
    refuse(name, "an accidental tie among the results at every seed tried")


def run_seed(name, s):
    exe = build_driver()
    cent, xb, xq = data(s["seed"], s["d"], s["M"], s["nbits"], s["nb"], s["nq"])
    M, k, metric, st = s["M"], s["k"], s["metric"], s["st"]
    # two stored vectors with one code are an exact tie: outside pq_ties only the first of them stays
    first = np.sort(np.unique(pr.compute_codes(xb, cent), axis=0, return_index=True)[1])
    xb = np.ascontiguousarray(xb[first])
    s["nb"] = xb.shape[0]
    codes_in = None
    if s["dup"]:
        c0 = pr.compute_codes(xb, cent)
        rng = np.random.default_rng(s["seed"])
        codes_in = np.concatenate([c0, c0[: s["nb"] // 2]])[rng.permutation(s["nb"] + s["nb"] // 2)]
    hts = None
    if s["hts"]:
        hts = pick_hts(name, s, cent, pr.compute_codes(xb, cent), xq)
    out = run(exe, s, cent, xq, k, xb=xb, codes=codes_in, hts=hts)
    codes = out["codes"]
    z = {"centroids": cent, "xq": xq, "codes": codes, "q_codes": out["q_codes"]}
    if st != pr.ST_SDC:       # (sdc_table is 4 * M * ksub^2 bytes: the tests restate it)
        z["tables"] = out["tables"] if s["blas"] else out["tables"][:TABLE_ROWS]
    for nm, v in (("d", s["d"]), ("M", M), ("nbits", s["nbits"]), ("k", k), ("metric", MET[metric]), ("search_type", st)):
        z[nm] = np.array(v, np.int64)
    if s["keep_xb"]:
        z["xb"] = xb
    if s["want_bytes"]:
        z["index_bytes"] = out["index_bytes"]
    nruns = len(hts) if hts else 1
    if hts:
        z["hts"] = np.asarray(hts, np.int64)
    for i in range(nruns):
        for nm in ("D", "I", "stats"):
            z["%s%d" % (nm, i)] = out["%s%d" % (nm, i)]

    # --- what the tests rely on
    if codes_in is None and not s["blas"] and not np.array_equal(codes, pr.compute_codes(xb, cent)):
        refuse(name, "the restatement's compute_codes differs from the reference's add")
    tabs = None
    if s["blas"]:
        # the reference's tables are BLAS's: the scan is checked over them, the tables to the rounding bound
        tabs = out["tables"]
        mine = pr.tables(xq, cent, metric)
        xn = (xq.reshape(-1, M, 1, s["d"] // M).astype(np.float64) ** 2).sum(-1)
        cn = (cent.astype(np.float64) ** 2).sum(-1)[None]
        bound = 2 * (s["d"] // M + 3) * 2.0 ** -24 * (xn + cn)
        if (np.abs(mine.astype(np.float64) - tabs) > bound).any():
            refuse(name, "a table entry of the restatement is outside the rounding bound of the reference's")
    for i in range(nruns):
        ht = hts[i] if hts else None
        Dn, In, npass, tn, qcn = pr.search(cent, codes, xq, k, metric, st, ht, tabs=tabs)
        if not pr.same_rows(Dn, In, z["D%d" % i], z["I%d" % i]):
            refuse(name, "the restatement (tests/pq_ref.py) does not reproduce D / I of search %d" % i)
        if list(z["stats%d" % i]) != [s["nq"], s["nq"] * codes.shape[0], npass]:
            refuse(name, "indexPQ_stats of search %d differ from the restatement: %s" % (i, list(z["stats%d" % i])))
        if not s["blas"]:
            ref_t = out["tables"] if st != pr.ST_SDC else None
            if ref_t is not None and not np.array_equal(tn.view(np.uint32), ref_t.view(np.uint32)):
                refuse(name, "the restatement's tables differ from the reference's")
            if st == pr.ST_SDC and not np.array_equal(pr.sdc_table(cent).view(np.uint32), out["tables"].view(np.uint32)):
                refuse(name, "the restatement's sdc_table differs from the reference's")
            if qcn is not None and not np.array_equal(qcn, out["q_codes"]):
                refuse(name, "the restatement's query codes differ from the reference's")
    D, I = z["D0"], z["I0"]
    if st == pr.ST_PQ and M % 4 == 0 and M > 4:
        Dl = pr.search(cent, codes, xq, k, metric, st, tabs=tabs, order="left")[0]
        if np.array_equal(Dl.view(np.uint32), D.view(np.uint32)):
            refuse(name, "a plain left-to-right sum reproduces D: the data cannot tell the summation orders apart")
    if st == pr.ST_PQ and M % 4 != 0:
        Dg = pr.search(cent, codes, xq, k, metric, st, tabs=tabs, order="group4")[0]
        if np.array_equal(Dg.view(np.uint32), D.view(np.uint32)):
            refuse(name, "the grouped sum reproduces D: the data cannot tell the summation orders apart")
    if not s["dup"]:
        for i in range(nruns):
            if tied_rows(z["D%d" % i], z["I%d" % i]).any():
                raise AccidentalTie()
    else:
        Dk1, Ik1 = pr.search(cent, codes, xq, k + 1, metric, st)[:2]
        across = (Dk1[:, k] == Dk1[:, k - 1]) & (Ik1[:, k] != -1)
        if not across.any():
            refuse(name, "no tie across the k-th place")
        if (~across).sum() * 3 < across.size:
            refuse(name, "fewer than a third of the rows are free of a tie across the k-th place")
        if not tied_rows(D, I).any():
            refuse(name, "no exact tie among the results")
    if hts:
        rate = z["stats0"][2] / float(s["nq"] * codes.shape[0])
        if not (0.005 <= rate <= 0.20):
            refuse(name, "the low threshold passes %.3f of the codes" % rate)
        if not (z["I0"] == -1).any():
            refuse(name, "no query is left with fewer than k passers at the low threshold")
        if z["stats%d" % (nruns - 1)][2] != s["nq"] * codes.shape[0]:
            refuse(name, "the last threshold does not pass every code")
    if s["small_nb"]:
        o2 = run(exe, s, cent, xq, k, codes=np.ascontiguousarray(codes[: s["small_nb"]]))
        Dn, In = pr.search(cent, codes[: s["small_nb"]], xq, k, metric, st)[:2]
        if not pr.same_rows(Dn, In, o2["D0"], o2["I0"]):
            refuse(name, "the restatement does not reproduce the k > ntotal rows")
        if not (o2["I0"][:, s["small_nb"]:] == -1).all() or (z["I0"] == -1).any():
            refuse(name, "padding is not where it should be")
        z["small_nb"] = np.array(s["small_nb"], np.int64)
        z["D_small"], z["I_small"] = o2["D0"], o2["I0"]
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    if os.path.getsize(path) > 1000000:
        refuse(name, "larger than 1 MB")
    print("%-18s seed %d %8.1f KB  ntotal %d%s" % (name, s["seed"], os.path.getsize(path) / 1024.0, codes.shape[0], "  hts %s pass %s" % (hts, [int(z["stats%d" % i][2]) for i in range(nruns)]) if hts else ""))


if __name__ == "__main__":
    os.makedirs(DEST, exist_ok=True)
    for n in sys.argv[1:] or list(CASES):
        run_case(n)
