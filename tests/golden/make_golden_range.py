#!/usr/bin/env python3
"""Generate the IVFFlat range-search fixtures tests/golden/ivfflat_range/*.npz.

Runs ONLY where the reference tree and its compiled CPU library (oracle/ref.mk) exist.  tests/golden/range_driver.cpp (our
driver over the reference's public API, compiled here into oracle/_ref/) rebuilds the index of a case of
make_golden_ivfflat.py and records IndexIVFFlat::range_search at several radii, together with the quantizer->assign keys
range_search computes for itself.  A case is refused unless the lists and keys the reference produces are bit-equal to the
committed tests/golden/ivfflat/<case>.npz, so a range fixture stores only `src` (that fixture's name), the radii and the
results per radius.  flat_padding_ties holds -1 keys, which range_search does not take: its range fixture carries the
recorded assign keys.  Fixtures are data only.

Radii of a case: the distances of all (query, scanned row) pairs, pooled and ordered best first (tests/range_ref.py's
restatement of the scan):
  tight       the value at rank 12 * nq (RANK overrides the 12 for a case whose data miss a condition there)
  tight_next  nextafter of it towards more hits
  wide        the value at rank 100 * nq          (long and ragged cases; and the cases named under `tight` below)
  all         +inf for L2, -inf for inner product (long and ragged cases only)
  none        0 for L2, +inf for inner product
Each finite radius is an observed value, so the strict comparison decides at least one pair.

Conditions (a fixture that misses one is not written; tests/test_range_ref.py checks them again):
  - the restatement reproduces lims, D (as bits) and I at every radius
  - tight: at least one query has no hit and at least one has hits from two different probes.  In seven cases the data
    allow no such radius at any rank: the clusters are well apart, so every query finds its own cluster's vectors in one
    list long before any query reaches a second list (range_ref.one_radius_can states the test: the smallest
    second-probe distance of any query lies above the largest best distance of any query).  The generator establishes
    that from the data; such a case must show the first half at `tight` and the second half at `wide`, which it then
    carries as well.  Where one radius can show both, `tight` must.
  - tight_next holds at least one more hit than tight, whose distance is bit-equal to the radius tight
  - wide (long and ragged cases): some query's hits in one list fall into at least 2 different 256-row trips and at least 3
    different 64-row groups, at least one of them only partly hit
  - two runs of the driver agree byte for byte (OMP_NUM_THREADS=4)
  - over all cases with d >= 4: a plain left-to-right sum gives a different lims or different D bits for at least one

    python tests/golden/make_golden_range.py                  # all cases
    python tests/golden/make_golden_range.py flat_l2_d32      # one case
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden_ivfflat as mg  # noqa: E402
import range_ref as rr  # noqa: E402

DEST = rr.RANGE_DIR
# case -> rank per query of `tight`, where 12 misses a condition.  The ranks per query at which the case's data can meet the
# `tight` conditions, from its pooled distances: flat_l2_d128_long 97 .. 123 (two lists' hits start at 97: there `tight` lies
# beyond `wide`), flat_coarse_int_ip 20 .. 32; an empty query needs flat_tail_d30_l2 <= 11, flat_padding_ties_l2 <= 6 and
# flat_coarse_int_l2 <= 4.
RANK = {"flat_l2_d128_long": 110, "flat_padding_ties_l2": 4, "flat_coarse_int_ip": 24, "flat_tail_d30_l2": 8, "flat_coarse_int_l2": 4}
# ... and of `wide`: flat_padding_ties_l2 scans 74 rows per query (two lists' hits start at rank 18)
WIDE_RANK = {"flat_padding_ties_l2": 40}


def build_driver():
    subprocess.check_call(["make", "-s", "-f", "oracle/ref.mk"], cwd=ROOT)
    exe = os.path.join(mg.OUT, "range_driver")
    src = os.path.join(HERE, "range_driver.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        mkl = os.environ.get("MKLDIR", "/opt/conda/lib")
        subprocess.check_call(
            ["g++", "-std=c++11", "-fPIC", "-m64", "-O2", "-mavx", "-msse4", "-mpopcnt", "-fopenmp", "-w", "-DFINTEGER=int",
             "-I" + mg.REF, "-o", exe, src, os.path.join(mg.OUT, "libfaiss_ref.so"), "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed",
             mkl + "/libmkl_gf_lp64.so", mkl + "/libmkl_gnu_thread.so", mkl + "/libmkl_core.so", "-lgomp", "-lpthread", "-lm", "-ldl"])
    return exe


def refuse(name, why):
    path = os.path.join(DEST, name + ".npz")
    if os.path.exists(path):
        os.remove(path)
    raise SystemExit("%s: %s -- fixture not written" % (name, why))


def case_data(name):
    """(cent, xb, xq, assign or None, nprobe, n_small) of a case, rebuilt the way make_golden_ivfflat.py builds it"""
    src, prefix, metric = rr.CASES[name]
    z = np.load(os.path.join(rr.SRC_DIR, src + ".npz"))
    if src == "flat_coarse_int":        # (its data are drawn inside run_coarse_int; the fixture keeps all of them)
        return z[prefix + "coarse_centroids"], z[prefix + "xb"], z[prefix + "xq"], None, int(z["nprobe"]), int(z["n_small"])
    s, (cent, xb, xq) = mg.CASES[src]()
    assert s["metric"] == metric
    return cent, xb, xq, s["assign"], s["nprobe"], 0


def radii_of(name, z, prefix, xq, keys, metric):
    nq = xq.shape[0]
    everything = np.float32(-np.inf if metric == "ip" else np.inf)
    _l, D, _i = rr.range_search_preassigned(z, xq, keys, everything, metric, prefix=prefix)
    pool = np.sort(-D if metric == "ip" else D)
    sign = np.float32(-1 if metric == "ip" else 1)

    def at(rank):
        if rank >= pool.size:
            refuse(name, "rank %d beyond the %d scanned pairs" % (rank, pool.size))
        return np.float32(sign * pool[rank])

    tight = at(RANK.get(name, 12) * nq)
    out = [("tight", tight), ("tight_next", np.nextafter(tight, everything))]
    if name in rr.WIDE_CASES or not rr.one_radius_can(z, xq, keys, metric, prefix):
        out.append(("wide", at(WIDE_RANK.get(name, 100) * nq)))
    if name in rr.WIDE_CASES:
        out.append(("all", everything))
    out.append(("none", np.float32(np.inf if metric == "ip" else 0)))
    return out


def wide_spread(P, J, lims):
    """some query's hits in one list: >= 2 trips of 256 rows, >= 3 groups of 64 rows, one group only partly hit (a group of
    the list that holds a hit and a row that is none -- rows of a group past the hits' last one are not counted)"""
    for q in range(lims.size - 1):
        p, j = P[lims[q]:lims[q + 1]], J[lims[q]:lims[q + 1]]
        for ik in np.unique(p):
            jj = j[p == ik]
            groups, counts = np.unique(jj // 64, return_counts=True)
            if np.unique(jj // 256).size >= 2 and groups.size >= 3 and (counts[:-1] < 64).any():
                return True
    return False


def conditions(name, metric, z, prefix, xq, keys, res, say):
    """res: radius name -> (radius, lims, D, I).  say(why) is called with the first condition missed."""
    bits = lambda a: a.view(np.uint32)
    for rn, (radius, lims, D, I) in res.items():
        ln, Dn, In = rr.range_search_preassigned(z, xq, keys, radius, metric, prefix=prefix)
        if not (np.array_equal(ln, lims) and np.array_equal(bits(Dn), bits(D)) and np.array_equal(In, I)):
            return say("the restatement (tests/range_ref.py) does not reproduce the result at `%s`" % rn)
    radius, lims, D, I = res["tight"]
    if not (np.diff(lims) == 0).any():
        return say("tight: no query without a hit")
    if rr.one_radius_can(z, xq, keys, metric, prefix):
        if not rr.hits_from_two_probes(z, xq, keys, radius, metric, prefix):
            return say("tight: no query with hits from two probes")
    elif "wide" not in res or not rr.hits_from_two_probes(z, xq, keys, res["wide"][0], metric, prefix):
        return say("no radius can show an empty query beside one with hits from two probes, and `wide` shows no such hits")
    r2, lims2, D2, _I2 = res["tight_next"]
    if lims2[-1] <= lims[-1]:
        return say("tight_next holds no more hits than tight")
    if not (bits(D2) == bits(np.array([radius], np.float32))[0]).any():
        return say("tight_next: no hit whose distance is the radius tight")
    if (D == radius).any():
        return say("tight: a hit at the radius itself (the comparison is not strict)")
    if name in rr.WIDE_CASES:
        radius, lims, D, I = res["wide"]
        _l, _D, _I, P, J = rr.range_search_preassigned(z, xq, keys, radius, metric, where=True, prefix=prefix)
        if not wide_spread(P, J, lims):
            return say("wide: no query whose hits in one list span 2 trips and 3 groups, one of them partly hit")
        if res["all"][1][-1] <= lims[-1]:
            return say("all holds no more hits than wide")
    if res["none"][1][-1] != 0:
        return say("none: hits")
    return True


def discriminates(metric, z, prefix, xq, keys, res):
    """a plain left-to-right sum gives a different lims or different D bits at some radius"""
    for rn, (radius, lims, D, _I) in res.items():
        lp, Dp, _Ip = rr.range_search_preassigned(z, xq, keys, radius, metric, dist=rr.plain(metric), prefix=prefix)
        if not (np.array_equal(lp, lims) and np.array_equal(Dp.view(np.uint32), D.view(np.uint32))):
            return True
    return False


def results_of(r, small=False):
    tag = "small_" if small else ""
    return {rn: (r["radii"][i], r["lims_%s%s" % (tag, rn)], r["D_%s%s" % (tag, rn)], r["I_%s%s" % (tag, rn)])
            for i, rn in enumerate(rr.radius_names(r))}


def run_case(name):
    src, prefix, metric = rr.CASES[name]
    exe = build_driver()
    z = np.load(os.path.join(rr.SRC_DIR, src + ".npz"))
    cent, xb, xq, assign, nprobe, n_small = case_data(name)
    if not np.array_equal(xq.view(np.uint32), z[prefix + "xq"].view(np.uint32)):
        refuse(name, "the rebuilt queries are not the committed fixture's")
    keys_fix = z[prefix + "keys"]
    nq = xq.shape[0]

    # the radii come from the committed lists; the keys of the first run are the reference's own
    arrays = {"cfg": np.array([cent.shape[1], cent.shape[0], xb.shape[0], nq, nprobe, mg.MET[metric], n_small], np.int64),
              "cent": cent, "xb": xb, "xq": xq, "radii": np.zeros(0, np.float32)}
    if assign is not None:
        arrays["assign"] = assign
    probe = mg.drive(exe, arrays)
    for nm in ("list_offsets", "vecs", "ids"):
        if not np.array_equal(probe[nm].view(np.uint8), z[prefix + nm].view(np.uint8)):
            refuse(name, "the reference's %s are not the committed fixture's" % nm)
    keys = probe["keys"]
    live = keys_fix >= 0
    if not np.array_equal(keys[live], keys_fix[live]):
        refuse(name, "the reference's assign keys are not the committed fixture's")
    if n_small and not np.array_equal(probe["keys_small"], keys[:n_small]):
        refuse(name, "the keys of the small batch differ from the whole batch's")
    rad = radii_of(name, z, prefix, xq, keys, metric)
    arrays["radii"] = np.array([v for _n, v in rad], np.float32)
    out = mg.drive(exe, arrays)
    again = mg.drive(exe, arrays)
    for nm in out:
        if not np.array_equal(out[nm].view(np.uint8), again[nm].view(np.uint8)):
            refuse(name, "not reproducible in %s" % nm)
    if not np.array_equal(out["keys"], keys):
        refuse(name, "keys differ between the runs")

    fx = {"src": np.array(src), "radius_names": np.array([n for n, _v in rad]), "radii": arrays["radii"]}
    if not live.all():
        fx["keys"] = keys
    for i, (rn, _v) in enumerate(rad):
        for a in ("lims", "D", "I"):
            fx["%s_%s" % (a, rn)] = out["%s_%d" % (a, i)]
            if n_small:
                fx["%s_small_%s" % (a, rn)] = out["%s_small_%d" % (a, i)]
    if n_small:
        fx["n_small"] = np.array(n_small, np.int64)

    ok = conditions(name, metric, z, prefix, xq, keys, results_of(fx), lambda why: refuse(name, why))
    assert ok is True
    if n_small:
        # the small batch's coarse stage takes the reference's other path: same keys, so the same hits as the first rows
        for rn, (_r, lims, D, I) in results_of(fx, small=True).items():
            _r2, l0, D0, I0 = results_of(fx)[rn]
            t = l0[n_small]
            if not (np.array_equal(lims, l0[:n_small + 1]) and np.array_equal(D.view(np.uint32), D0[:t].view(np.uint32)) and
                    np.array_equal(I, I0[:t])):
                refuse(name, "range_search of the first %d queries differs from the whole batch's rows at `%s`" % (n_small, rn))
    os.makedirs(DEST, exist_ok=True)
    path = os.path.join(DEST, name + ".npz")
    np.savez_compressed(path, **fx)
    if os.path.getsize(path) > 1000000:
        refuse(name, "larger than 1 MB")
    disc = cent.shape[1] >= 4 and discriminates(metric, z, prefix, xq, keys, results_of(fx))
    print("%-22s %8.1f KB  hits %s%s" % (name, os.path.getsize(path) / 1024.0,
                                        " ".join("%s=%d" % (rn, fx["lims_" + rn][-1]) for rn, _v in rad),
                                        "  (tells the summation orders apart)" if disc else ""))
    return disc


if __name__ == "__main__":
    names = sys.argv[1:] or list(rr.CASES)
    disc = [run_case(n) for n in names]
    if not sys.argv[1:] and not any(disc):
        raise SystemExit("no case tells the four-accumulator order from a plain left-to-right sum")
