#!/usr/bin/env python3
"""Generate the IVF scalar-quantizer fixtures tests/golden/ivfsq/*.npz (a directory of their own: tests/util.py takes every
.npz directly under tests/golden/ for an IVFPQ fixture of make_golden.py).

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/ivfsq_driver.cpp (our
driver over the reference's public API, compiled here into oracle/_ref/) builds IndexFlatL2 / IndexFlatIP +
IndexIVFScalarQuantizer over given centroids, trains the range (RS_minmax) on the first rows of the stored vectors, adds, and
records: trained, the lists, quantizer->search keys and distances, D / I of search, sq.decode of the stored codes and, for one
fixture, the bytes write_index wrote.

Every fixture is checked against the numpy restatement (tests/ivfsq_ref.py) and for the conditions the tests rely on; a
fixture that misses one is not written.  Fixtures are data only.

  restated              D bit for bit, the stored codes byte for byte, trained bit for bit, decoded bit for bit
  discriminating data   the OTHER operation order (scalar where d % 8 == 0, eight accumulators otherwise) must differ in bits
                        from the reference's D in at least one slot
  no accidental ties    without deliberate duplicates no returned row holds two equal distances
  checkable tie rows    sq_ties_*: at most half of the rows have a group of equal distances across the k-th place

    python tests/golden/make_golden_ivfsq.py                  # all cases
    python tests/golden/make_golden_ivfsq.py sq_8bit_l2_d32   # one case
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import ivfsq_ref as sr  # noqa: E402
from make_golden_ivfflat import OUT, REF, drive, mixture  # noqa: E402

DEST = os.path.join(HERE, "ivfsq")
MET = {"ip": 0, "l2": 1}

CASES = {}


def spec(qtype, metric, nprobe, k, keep_xb=False, dup=False, want_bytes=False, assign=None, extra_k=(), long_list=False):
    return dict(qtype=sr.QTYPES[qtype], metric=metric, nprobe=nprobe, k=k, keep_xb=keep_xb, dup=dup, want_bytes=want_bytes,
                assign=assign, extra_k=extra_k, long_list=long_list)


def _add(name, fn):
    CASES[name] = fn


# AVX order (d % 8 == 0): d 32 and d 128, all four types, both metrics.  d 32 keeps the stored vectors (add / encode on the device).
for _qt in sr.QTYPES:
    for _m in MET:
        _add("sq_%s_%s_d32" % (_qt, _m), lambda qt=_qt, m=_m: (spec(qt, m, 5, 10, keep_xb=True, want_bytes=(qt, m) == ("4bit_uniform", "ip")),
                                                               mixture(5101, 32, 16, 1000, 30)))
        _add("sq_%s_%s_d128" % (_qt, _m), lambda qt=_qt, m=_m: (spec(qt, m, 4, 10), mixture(5102, 128, 8, 500, 20)))
# scalar order: d 30 and d 33 (4 bits at odd d: the last nibble is unused)
for _qt in ("8bit", "4bit"):
    for _m in MET:
        for _d in (30, 33):
            _add("sq_%s_%s_d%d" % (_qt, _m, _d), lambda qt=_qt, m=_m, d=_d: (spec(qt, m, 3, 10, keep_xb=True, want_bytes=(qt, m, d) == ("4bit", "l2", 33)),
                                                                           mixture(5200 + d, d, 8, 400, 20)))
# ragged rows: code_size 40 (AVX order, rows not 16-byte aligned) and code_size 24
_add("sq_8bit_l2_d40", lambda: (spec("8bit", "l2", 4, 10), mixture(5301, 40, 8, 600, 20)))
_add("sq_4bit_ip_d48", lambda: (spec("4bit", "ip", 4, 10), mixture(5302, 48, 8, 600, 20)))
# tiny
_add("sq_8bit_l2_d8", lambda: (spec("8bit", "l2", 3, 10, keep_xb=True), mixture(5401, 8, 8, 400, 20)))
_add("sq_8bit_l2_d5", lambda: (spec("8bit", "l2", 3, 10, keep_xb=True, want_bytes=True), mixture(5402, 5, 8, 400, 20)))


def _long():
    """d 128, 16 lists, 1200 vectors, a given assignment: the vectors of two probed lists go to list 0, so that one list is
    longer than two trips of the kernel's 256 lanes and two lists are empty."""
    cent, xb, xq = mixture(5502, 128, 16, 1200, 20, heavy=420)
    a = np.argmin(((xb[:, None, :].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(-1), axis=1).astype(np.int64)
    aq = np.argsort(((xq[:, None, :].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(-1), axis=1)[:, :6]
    probed = [c for c in np.unique(aq) if c != 0]
    a[np.isin(a, probed[:2])] = 0
    return spec("8bit", "l2", 6, 10, assign=a, long_list=True), (cent, xb, xq)


_add("sq_8bit_l2_d128_long", _long)
# wide k: k 1024 (every row padded) and k 100 (some rows padded) on the same data
_add("sq_8bit_l2_d32_kwide", lambda: (spec("8bit", "l2", 2, 1024, extra_k=(100,)), mixture(5601, 32, 16, 800, 20)))


def _ties(qt, m):
    cent, xb, xq = mixture(5701, 32, 8, 600, 40)
    rng = np.random.default_rng(57)
    n4 = xb.shape[0] // 4
    xb[-n4:] = xb[rng.integers(0, xb.shape[0] - n4, n4)]      # a quarter of the stored vectors repeat earlier ones
    return spec(qt, m, 4, 10, dup=True), (cent, xb, xq)


for _qt in ("8bit", "4bit"):
    for _m in MET:
        _add("sq_ties_%s_%s" % (_qt, _m), lambda qt=_qt, m=_m: _ties(qt, m))


def _coarse_int(metric, seed, d=16, nlist=16, nb=600, nq=24, nprobe=4):
    """Integer-valued centroids and queries: every coarse distance is exact in fp32 in any summation order, so the reference's
    BLAS coarse path (20 queries and more) gives the keys and the distances any exact method gives, and the whole search() can
    be compared -- under inner product the coarse distance is accu0 and enters D.  The stored vectors are general floats.  No
    query has a tie among its nprobe + 1 best centroids."""
    rng = np.random.default_rng(seed)
    cent = rng.integers(-100, 101, size=(nlist, d)).astype(np.float32)
    xb = (cent[rng.integers(0, nlist, nb)] + 25 * rng.standard_normal((nb, d))).astype(np.float32)
    pool = (cent[rng.integers(0, nlist, 4 * nq)] + rng.integers(-40, 41, size=(4 * nq, d))).astype(np.float32)
    score = pool.astype(np.int64) @ cent.astype(np.int64).T if metric == "ip" else \
        -((pool.astype(np.int64)[:, None, :] - cent.astype(np.int64)[None]) ** 2).sum(-1)
    srt = -np.sort(-score, axis=1)
    xq = pool[(np.diff(srt[:, :nprobe + 1], axis=1) != 0).all(axis=1)][:nq]
    assert xq.shape[0] == nq
    return spec("8bit", metric, nprobe, 10, keep_xb=True), (cent, xb, xq)


_add("sq_coarse_int_l2", lambda: _coarse_int("l2", 5801))
_add("sq_coarse_int_ip", lambda: _coarse_int("ip", 5802))


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "ivfsq_driver")
    src = os.path.join(HERE, "ivfsq_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + REF, "-o", exe, src, os.path.join(OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def refuse(name, why):
    path = os.path.join(DEST, name + ".npz")
    if os.path.exists(path):
        os.remove(path)
    raise SystemExit("%s: %s -- fixture not written" % (name, why))


def run(exe, s, cent, xb, xq, k, nt):
    arrays = {"cfg": np.array([cent.shape[1], cent.shape[0], xb.shape[0], xq.shape[0], s["nprobe"], k, MET[s["metric"]], s["qtype"], nt], np.int64),
              "cent": cent, "xb": xb, "xq": xq}
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


def check_rows(name, s, z, xq, k, D, I):
    """the restatement against the reference's rows; returns the rows left out of the label comparison"""
    Dn, In = sr.search_preassigned(z, xq, z["keys"], z["cdis"], k, s["metric"], s["qtype"])
    if not np.array_equal(Dn.view(np.uint32), D.view(np.uint32)):
        refuse(name, "the restatement (tests/ivfsq_ref.py) does not reproduce D at k = %d" % k)
    across = sr.tie_across_kth(z, xq, z["keys"], z["cdis"], k, s["metric"], s["qtype"]) if s["dup"] else np.zeros(xq.shape[0], bool)
    if not sr.same_pairs(Dn, In, D, I, ~across):
        refuse(name, "the restatement does not reproduce the labels at k = %d" % k)
    return across


def run_case(name):
    s, (cent, xb, xq) = CASES[name]()
    exe = build_driver()
    d, nlist, qtype = cent.shape[1], cent.shape[0], s["qtype"]
    nt = xb.shape[0] * 3 // 4          # the range is trained on three quarters of the vectors: some codes clamp
    out = run(exe, s, cent, xb, xq, s["k"], nt)
    z = {nm: out[nm] for nm in ("trained", "list_offsets", "codes", "ids", "keys", "cdis", "D", "I")}
    z["coarse_centroids"] = cent
    z["xq"] = xq
    for nm, v in (("d", d), ("nlist", nlist), ("nprobe", s["nprobe"]), ("k", s["k"]), ("metric", MET[s["metric"]]), ("qtype", qtype),
                  ("nt", nt)):
        z[nm] = np.array(v, np.int64)
    if s["keep_xb"]:
        z["xb"] = xb
    if s["assign"] is not None:
        z["assign"] = s["assign"]        # (the stored vectors themselves are not kept: the file would pass the size limit)
    if s["want_bytes"]:
        z["index_bytes"] = out["index_bytes"]
        z["decoded"] = out["decoded"]          # sq.decode of the stored codes (tests/test_cpp_ivfsq.py)
    lens = np.diff(z["list_offsets"])

    # --- what the tests rely on
    if z["codes"].shape != (lens.sum(), sr.code_size(d, qtype)):
        refuse(name, "codes of shape %r" % (z["codes"].shape,))
    across = check_rows(name, s, z, xq, s["k"], z["D"], z["I"])
    for ek in s["extra_k"]:
        o2 = run(exe, s, cent, xb, xq, ek, nt)
        if not np.array_equal(o2["keys"], z["keys"]):
            refuse(name, "keys differ between the runs")
        z["D_k%d" % ek], z["I_k%d" % ek] = o2["D"], o2["I"]
        check_rows(name, s, z, xq, ek, o2["D"], o2["I"])
    if (z["I"] == -1).all():
        refuse(name, "no result at all")
    if (z["keys"] < 0).any():
        refuse(name, "the quantizer returned a key < 0")
    if not sr.other_order_differs(z, xq, z["keys"], z["cdis"], s["k"], s["metric"], qtype, z["D"]):
        refuse(name, "the other operation order reproduces D: the data cannot tell the two apart")
    if not s["dup"] and sr.tied_rows(z["D"], z["I"]).any():
        refuse(name, "an accidental tie among the results")
    # the stored codes, the range and sq.decode: restated byte for byte / bit for bit
    assign = np.empty(xb.shape[0], np.int64)
    assign[z["ids"]] = np.repeat(np.arange(nlist), lens)
    if s["assign"] is not None and not np.array_equal(assign, s["assign"]):
        refuse(name, "the lists are not the given assignment")
    for li in range(nlist):
        o0, o1 = z["list_offsets"][li], z["list_offsets"][li + 1]
        if not np.array_equal(z["ids"][o0:o1], np.nonzero(assign == li)[0]):
            refuse(name, "list %d is not in input order" % li)
    res = (xb - cent[assign]).astype(np.float32)
    if not np.array_equal(sr.encode(res[z["ids"]], qtype, z["trained"]), z["codes"]):
        refuse(name, "the restatement does not reproduce the stored codes")
    if s["assign"] is None and not np.array_equal(sr.train(res[:nt], qtype).view(np.uint32), z["trained"].view(np.uint32)):
        refuse(name, "the restatement does not reproduce trained")
    if not np.array_equal(sr.decode_scalar(z["codes"], d, qtype, z["trained"]).view(np.uint32), out["decoded"].view(np.uint32)):
        refuse(name, "the restatement does not reproduce sq.decode")
    if not (z["trained"][z["trained"].size // 2:] > 0).all():
        refuse(name, "a constant dimension (vdiff == 0)")
    comp = sr.components(z["codes"], d, qtype)
    top = 255 if sr.bits_of(qtype) == 8 else 15
    if s["keep_xb"] and not ((comp == 0).any() and (comp == top).any()):
        refuse(name, "no code at either end of the range")
    if name.startswith("sq_coarse_int"):
        c64, q64 = cent.astype(np.int64), xq.astype(np.int64)
        score = q64 @ c64.T if s["metric"] == "ip" else -((q64[:, None, :] - c64[None]) ** 2).sum(-1)
        exact = np.argsort(-score, axis=1, kind="stable")[:, :s["nprobe"]]
        want = np.take_along_axis(score, exact, axis=1)
        if not np.array_equal(exact, z["keys"]) or not np.array_equal(z["cdis"].astype(np.int64), want if s["metric"] == "ip" else -want):
            refuse(name, "the reference's coarse keys / distances are not the exact ones")
    if s["long_list"]:
        kk = z["keys"][z["keys"] >= 0]
        if lens.max() < 520 or (lens == 0).sum() < 2 or not (lens[kk] == 0).any() or not (lens[kk] >= 520).any():
            refuse(name, "needs a probed list of 520 codes and two empty lists, one probed (longest %d, %d empty)" % (lens.max(), (lens == 0).sum()))
    if s["extra_k"]:
        if not (z["I"] == -1).any(axis=1).all():
            refuse(name, "a k = %d row is not padded" % s["k"])
        Ie = z["I_k%d" % s["extra_k"][0]]
        if not ((Ie == -1).any(axis=1).any() and (Ie != -1).all(axis=1).any()):
            refuse(name, "k = %d: needs padded rows and full rows" % s["extra_k"][0])
        pad = np.float32(-sr.FLT_MAX if s["metric"] == "ip" else sr.FLT_MAX)
        if not (z["D"][z["I"] == -1].view(np.uint32) == pad.view(np.uint32)).all():
            refuse(name, "padding is not %r" % pad)
    if s["dup"]:
        if not sr.tied_rows(z["D"], z["I"]).any():
            refuse(name, "no exact tie among the results")
        if across.sum() * 2 > across.size:
            refuse(name, "more than half of the rows (%d of %d) have a tie across the k-th place" % (across.sum(), across.size))
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    if os.path.getsize(path) > 600000:
        refuse(name, "larger than 600 KB")
    print("%-24s %7.1f KB  ntotal %d longest list %d, %d empty, %d rows with a tie across k" % (
        name, os.path.getsize(path) / 1024.0, lens.sum(), lens.max(), (lens == 0).sum(), across.sum()))


if __name__ == "__main__":
    os.makedirs(DEST, exist_ok=True)
    for n in sys.argv[1:] or list(CASES):
        run_case(n)
