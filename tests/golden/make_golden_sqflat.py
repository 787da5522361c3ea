#!/usr/bin/env python3
"""Generate the flat scalar-quantizer fixtures tests/golden/sqflat/*.npz (a directory of their own: tests/util.py takes every
.npz directly under tests/golden/ for an IVFPQ fixture of make_golden.py).

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/sqflat_driver.cpp (our
driver over the reference's public API, compiled here into oracle/_ref/) builds an IndexScalarQuantizer, trains the range
(RS_minmax) on the first rows of the stored vectors, adds, and records: trained, the stored codes, the raw D / I of search (in
the reference's heap order: it never reorders the heap in this search), reconstruct_n of the stored codes and, for two cases,
the bytes write_index wrote.

Every fixture is checked against the numpy restatement (tests/sqflat_ref.py) and for the conditions the tests rely on; a
fixture that misses one is not written.  Fixtures are data only.

  restated              the fixture's D, sorted, bit for bit; the stored codes byte for byte; trained and the decoded vectors
                        bit for bit
  discriminating data   the OTHER operation order (scalar where d % 8 == 0, eight accumulators otherwise) must differ in bits
                        from the reference's D in at least one slot
  no accidental ties    without deliberate duplicates no returned row holds two equal distances (the k 1024 rows return every
                        stored code: there no tie may cross the k-th place of the k 100 rows)
  checkable tie rows    sqf_ties_*: at most half of the rows have a group of equal distances across the k-th place

    python tests/golden/make_golden_sqflat.py                  # all cases
    python tests/golden/make_golden_sqflat.py sqf_8bit_l2_d32  # one case
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import ivfsq_ref as sr  # noqa: E402
import sqflat_ref as fr  # noqa: E402
from make_golden_ivfflat import OUT, REF, drive, mixture  # noqa: E402

DEST = os.path.join(HERE, "sqflat")
MET = {"ip": 0, "l2": 1}

CASES = {}


def spec(qtype, metric, k, keep_xb=False, dup=False, want_bytes=False, extra_k=()):
    return dict(qtype=sr.QTYPES[qtype], metric=metric, k=k, keep_xb=keep_xb, dup=dup, want_bytes=want_bytes, extra_k=extra_k)


def _add(name, fn):
    CASES[name] = fn


def data(seed, d, nb, nq, nc=16):
    _cent, xb, xq = mixture(seed, d, nc, nb, nq)
    return xb, xq


# AVX order (d % 8 == 0): d 32, all four types, both metrics; the stored vectors are kept (train / add / encode on the device)
for _qt in sr.QTYPES:
    for _m in MET:
        _add("sqf_%s_%s_d32" % (_qt, _m), lambda qt=_qt, m=_m: (spec(qt, m, 10, keep_xb=True, want_bytes=(qt, m) == ("8bit", "l2")),
                                                                data(6101, 32, 1000, 30)))
for _qt in ("8bit", "4bit"):
    for _m in MET:
        _add("sqf_%s_%s_d128" % (_qt, _m), lambda qt=_qt, m=_m: (spec(qt, m, 10), data(6102, 128, 500, 20, 8)))
# scalar order: d 30 and d 33 (4 bits at odd d: the last nibble is unused)
for _qt in ("8bit", "4bit"):
    for _m in MET:
        for _d in (30, 33):
            _add("sqf_%s_%s_d%d" % (_qt, _m, _d), lambda qt=_qt, m=_m, d=_d: (spec(qt, m, 10, keep_xb=True, want_bytes=(qt, m, d) == ("4bit", "ip", 33)),
                                                                            data(6200 + d, d, 400, 20, 8)))
# ragged rows: code_size 40 (AVX order, rows not 16-byte aligned) and code_size 24
_add("sqf_8bit_l2_d40", lambda: (spec("8bit", "l2", 10), data(6301, 40, 600, 20, 8)))
_add("sqf_4bit_ip_d48", lambda: (spec("4bit", "ip", 10), data(6302, 48, 600, 20, 8)))
# tiny
_add("sqf_8bit_l2_d8", lambda: (spec("8bit", "l2", 10, keep_xb=True), data(6401, 8, 400, 20, 8)))
_add("sqf_8bit_l2_d5", lambda: (spec("8bit", "l2", 10, keep_xb=True), data(6402, 5, 400, 20, 8)))
# wide k: k 1024 over 800 stored (every row padded) and k 100 on the same data
_add("sqf_8bit_l2_d32_kwide", lambda: (spec("8bit", "l2", 1024, extra_k=(100,)), data(6601, 32, 800, 20)))


def _ties(qt, m):
    xb, xq = data(6701, 32, 600, 40, 8)
    rng = np.random.default_rng(67)
    n4 = xb.shape[0] // 4
    xb[-n4:] = xb[rng.integers(0, xb.shape[0] - n4, n4)]      # a quarter of the stored vectors repeat earlier ones
    return spec(qt, m, 10, dup=True), (xb, xq)


_add("sqf_ties_8bit_l2", lambda: _ties("8bit", "l2"))
_add("sqf_ties_4bit_ip", lambda: _ties("4bit", "ip"))
# longer: more than two 1024-row trips of a workgroup
_add("sqf_8bit_l2_d32_long", lambda: (spec("8bit", "l2", 10), data(6801, 32, 2600, 20)))


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(OUT, "sqflat_driver")
    src = os.path.join(HERE, "sqflat_driver.cpp")
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


def run(exe, s, xb, xq, k, nt):
    arrays = {"cfg": np.array([xb.shape[1], xb.shape[0], xq.shape[0], k, MET[s["metric"]], s["qtype"], nt], np.int64), "xb": xb, "xq": xq}
    if s["want_bytes"]:
        arrays["bytes"] = np.zeros(1, np.uint8)
    out = drive(exe, arrays)
    again = drive(exe, arrays)
    for nm in out:
        if not np.array_equal(out[nm].view(np.uint8), again[nm].view(np.uint8)):
            raise SystemExit("not reproducible in %s" % nm)
    return out


def check_rows(name, s, dis, k, D, I):
    """the restatement against the reference's rows, sorted; returns the rows left out of the label comparison"""
    Dn, In = fr.rows_of(dis, k, s["metric"])
    Ds, Is = fr.sorted_rows(D, I, s["metric"])
    if not np.array_equal(Dn.view(np.uint32), Ds.view(np.uint32)):
        refuse(name, "the restatement (tests/sqflat_ref.py) does not reproduce the sorted D at k = %d" % k)
    across = fr.tie_across_kth(dis, k, s["metric"]) if s["dup"] else np.zeros(D.shape[0], bool)
    if not sr.same_pairs(Dn, In, Ds, Is, ~across):
        refuse(name, "the restatement does not reproduce the labels at k = %d" % k)
    return across


def run_case(name):
    s, (xb, xq) = CASES[name]()
    exe = build_driver()
    d, qtype, k = xb.shape[1], s["qtype"], s["k"]
    nt = xb.shape[0] * 3 // 4          # the range is trained on three quarters of the vectors: some codes clamp
    out = run(exe, s, xb, xq, k, nt)
    z = {nm: out[nm] for nm in ("trained", "codes", "D", "I")}
    z["xq"] = xq
    for nm, v in (("d", d), ("k", k), ("metric", MET[s["metric"]]), ("qtype", qtype), ("nt", nt)):
        z[nm] = np.array(v, np.int64)
    if s["keep_xb"]:
        z["xb"] = xb
        z["decoded"] = out["decoded"]          # reconstruct_n of the stored codes
    if s["want_bytes"]:
        z["index_bytes"] = out["index_bytes"]

    # --- what the tests rely on
    if z["codes"].shape != (xb.shape[0], sr.code_size(d, qtype)):
        refuse(name, "codes of shape %r" % (z["codes"].shape,))
    dis = fr.all_distances(z["codes"], xq, s["metric"], qtype, z["trained"])
    across = check_rows(name, s, dis, k, z["D"], z["I"])
    for ek in s["extra_k"]:
        o2 = run(exe, s, xb, xq, ek, nt)
        z["D_k%d" % ek], z["I_k%d" % ek] = o2["D"], o2["I"]
        check_rows(name, s, dis, ek, o2["D"], o2["I"])
    if (z["I"] == -1).all():
        refuse(name, "no result at all")
    other = fr.all_distances(z["codes"], xq, s["metric"], qtype, z["trained"], order8=(d % 8 != 0))
    if np.array_equal(fr.rows_of(other, k, s["metric"])[0].view(np.uint32), fr.sorted_rows(z["D"], z["I"], s["metric"])[0].view(np.uint32)):
        refuse(name, "the other operation order reproduces D: the data cannot tell the two apart")
    # (a padded row holds every stored code: equal distances among all of them are likely and harmless there, both sides order
    # them by position; what must not happen by accident is a tie across the k-th place of a full row)
    if not s["dup"] and not s["extra_k"] and sr.tied_rows(z["D"], z["I"]).any():
        refuse(name, "an accidental tie among the results")
    for ek in s["extra_k"]:
        if fr.tie_across_kth(dis, ek, s["metric"]).any():
            refuse(name, "an accidental tie across the k-th place at k = %d" % ek)
    # the stored codes, the range and reconstruct_n: restated byte for byte / bit for bit
    if not np.array_equal(sr.encode(xb, qtype, z["trained"]), z["codes"]):
        refuse(name, "the restatement does not reproduce the stored codes")
    if not np.array_equal(sr.train(xb[:nt], qtype).view(np.uint32), z["trained"].view(np.uint32)):
        refuse(name, "the restatement does not reproduce trained")
    if not np.array_equal(sr.decode_scalar(z["codes"], d, qtype, z["trained"]).view(np.uint32), out["decoded"].view(np.uint32)):
        refuse(name, "the restatement does not reproduce reconstruct_n")
    if not (z["trained"][z["trained"].size // 2:] > 0).all():
        refuse(name, "a constant dimension (vdiff == 0)")
    comp = sr.components(z["codes"], d, qtype)
    top = 255 if sr.bits_of(qtype) == 8 else 15
    if s["keep_xb"] and not ((comp == 0).any() and (comp == top).any()):
        refuse(name, "no code at either end of the range")
    if s["extra_k"]:
        if not (z["I"] == -1).any(axis=1).all():
            refuse(name, "a k = %d row is not padded" % k)
        pad = np.float32(-sr.FLT_MAX if s["metric"] == "ip" else sr.FLT_MAX)
        if not (z["D"][z["I"] == -1].view(np.uint32) == pad.view(np.uint32)).all():
            refuse(name, "padding is not %r" % pad)
    if s["dup"]:
        if not sr.tied_rows(z["D"], z["I"]).any():
            refuse(name, "no exact tie among the results")
        if not across.any():
            refuse(name, "no row with a tie across the k-th place")
        if across.sum() * 2 > across.size:
            refuse(name, "more than half of the rows (%d of %d) have a tie across the k-th place" % (across.sum(), across.size))
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **z)
    if os.path.getsize(path) > 600000:
        refuse(name, "larger than 600 KB")
    print("%-24s %7.1f KB  ntotal %d, %d rows with a tie across k" % (name, os.path.getsize(path) / 1024.0, xb.shape[0], across.sum()))


if __name__ == "__main__":
    os.makedirs(DEST, exist_ok=True)
    for n in sys.argv[1:] or list(CASES):
        run_case(n)
