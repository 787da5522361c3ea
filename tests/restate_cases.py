"""The worlds, walks, fresh-handle recipes and CPU references of tests/test_gpu_restate.py: handles that are retrained, re-moded
or reloaded AFTER a search; tests/test_restate_cases.py holds this module to its promises without a GPU.

TEST INFRASTRUCTURE ONLY.  Nothing here touches a device at import or while a walk is built: a walk is host arrays plus functions
that a GPU test applies to a live handle.

  state     a dict: everything a handle of the kind holds after a step -- centroids, codebooks, lists / codes (host arrays, as the
            kind's CPU encoder gives them), options, metric, mode -- plus "history" (the labels of the steps so far) and
            "stream", which no recipe and no reference reads.
  Step      label, fn(handle) applied to the live handle, the state after it, and `stale`: the same state with the component the
            step changed left at its old value (what a handle that missed the invalidation would answer from).  noop: a toggle
            that must not change a row.  refuse: the error code a step that must be refused raises (its state is the one the
            following clean search runs in).
  Kind      walk() -> [Step]; start(state) -> the live handle, built in canonical order; recipe(state) -> the calls that build a
            fresh handle of that state (constructor, trained state, options, set_lists / set_codes), a pure function of the
            state; fresh(state) runs it; read(g) -> what the live handle stores; with_stored(state, stored) -> the state over
            exactly that; search(g, state, xq); coarse(g, state, xq) -> the device's own coarse (or first) stage where the kind's
            tests feed it to the restatement; reference(state, xq, coarse=None) -> the CPU rows; rule(state) -> the kind's
            comparison rule in that state; extras(g, state) -> further (what, got, want) triples compared exactly (reconstruct_n,
            range_search); ran(g, state) -> asserts from last_scan_info() and the state getters that the intended kernel ran.
            check_stored(state, stored) -> what the live handle stores IS what the walk's host-side state says (bytes, or shapes
            where the CPU encoder is not bit-compatible).
  Step.pre  calls that prepare a refusal (set_refine_pq before set_refine_codes, new centroids before a new graph);
  resize    a step that changes the batch of queries (their number, or k) only.

World B is chosen so that every step moves the answer (tests/test_restate_cases.py measures it): pq * 1.25 + 0.5 and coarse + 1.5
as in scan_sums_cases.case_stale; where only the coarse centroids of an index without residual-free codes change, the rows of the
centroid table rolled by one with nprobe < nlist: the probed lists change, the lists themselves stay.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]

import ip_ref  # noqa: E402
import ivfflat_ref  # noqa: E402
import ivfsq_ref  # noqa: E402
import knn_ref  # noqa: E402
import lsh_ref  # noqa: E402
import polysemous_ref  # noqa: E402
import pq_ref  # noqa: E402
import range_ref  # noqa: E402
import refine_ref  # noqa: E402
import refineflat_ref  # noqa: E402
import sqflat_ref  # noqa: E402
from oracle.pyoracle import OracleIndex, OracleVLQ  # noqa: E402
from util import assert_same_topk  # noqa: E402

F32 = np.float32
ERR_UNSUPPORTED, ERR_STATE = 3, 4
# toggles that must not change a row: every step that names one of these components is a no-op on the reference side
# ("capacity": reserve_memory / reclaim_memory move the lists and keep their contents)
NOOP_COMPONENTS = ("stream", "scan_schedule", "scan_sums", "coarse_screen", "row_mode", "scan_parts", "scan_split", "capacity")


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def same_stored(got, want, as_bytes, what=""):
    """arrays, or tuples of arrays, of the same shapes and types -- and, as_bytes, the same contents"""
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == len(want), what
        for g, w in zip(got, want):
            same_stored(g, w, as_bytes, what)
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if as_bytes and want.size:
        n = want.shape[0]
        bad = np.nonzero((np.ascontiguousarray(got).reshape(n, -1).view(np.uint8) != np.ascontiguousarray(want).reshape(n, -1).view(np.uint8)).any(axis=1))[0]
        assert bad.size == 0, "%s: %d of %d rows differ, first row %d" % (what, bad.size, n, bad[0] if bad.size else -1)


def rows_differ(a, b):
    """[nq] bool: the row differs in the bits of D or in I"""
    return (bits(a[0]) != bits(b[0])).any(axis=1) | (np.asarray(a[1]) != np.asarray(b[1])).any(axis=1)


def exact(got, want, what=""):
    """D as bits and I in every slot: the rule where the order of a row is the defined one"""
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    bad = np.nonzero(rows_differ(got, want))[0]
    assert bad.size == 0, "%s: %d of %d rows differ, first row %d" % (what, bad.size, got[0].shape[0], bad[0] if bad.size else -1)


def topk_rule(got, want, what=""):
    assert_same_topk(np.asarray(got[0]), np.asarray(got[1]), want[0], want[1], what)


class Step:
    def __init__(self, label, fn, state, stale=None, noop=False, refuse=None, pre=(), resize=False):
        self.label, self.fn, self.state, self.stale, self.noop, self.refuse = label, fn, state, stale, noop, refuse
        self.pre = tuple(pre)          # calls that prepare a refusal: applied before fn, expected to succeed
        self.resize = resize           # only the batch of queries changes: nothing of the handle's state does

    def __repr__(self):
        return "Step(%r)" % self.label


def to_torch_stream(g):
    import torch
    g.set_stream(torch.cuda.current_stream().cuda_stream)


def to_own_stream(g):
    import torch
    g._restate_stream = torch.cuda.Stream()          # (kept alive with the handle)
    g.set_stream(g._restate_stream.cuda_stream)


class Walk:
    """builds the steps of one walk: every step's state is the one before it with the named components replaced"""

    def __init__(self, **first):
        self.state = dict(first, history=("A",), stream="own")
        self.steps = [Step("A", None, self.state)]

    def step(self, label, fn, old=None, **new):
        prev = self.state
        self.state = dict(prev, **new)
        self.state["history"] = prev["history"] + (label,)
        noop = all(c in NOOP_COMPONENTS for c in new)
        stale = dict(self.state, **({c: prev[c] for c in new} if old is None else old))
        self.steps.append(Step(label, fn, self.state, stale, noop=noop))

    def to_torch(self):
        self.step("set_stream(torch's current stream)", to_torch_stream, stream="torch")

    def to_own(self):
        self.step("set_stream(a stream of its own)", to_own_stream, stream="own")


class Kind:
    name = None
    k = 10
    compare = staticmethod(exact)

    def __repr__(self):
        return self.name

    def rule(self, state):
        """the comparison with the CPU reference in this state: the one the kind's own test_gpu_*.py uses"""
        return self.compare

    def fresh(self, state):
        calls = self.recipe(state)
        g = calls[0][1](*calls[0][2])
        for name, fn, args in calls[1:]:
            fn(g, *args)
        return g

    def start(self, state):
        return self.fresh(state)

    def recipe_key(self, state):
        """the recipe as comparable data: call names and the bytes of their arguments"""
        out = []
        for name, _fn, args in self.recipe(state):
            out.append((name,) + tuple(a.tobytes() + str(a.shape).encode() if isinstance(a, np.ndarray) else repr(a) for a in args))
        return out

    def queries(self, state):
        return self.world()["xq"]

    def coarse(self, g, state, xq):
        return None

    def extras(self, g, state):
        return []

    def ran(self, g, state):
        """asserts that the kernel the walk is about ran, where the handle tells (last_scan_info and the state getters)"""

    # The live handle's stored rows are what the fresh handle and the reference are given, so a reset that cleared nothing or an
    # add that appended the wrong rows would make all three agree.  Every kind's CPU encoder is one an existing GPU test
    # already holds the device's add to bit for bit (test_gpu_flatknn, test_gpu_lsh, test_gpu_sqflat*, test_gpu_pq,
    # test_gpu_write_pages for the IVF kinds under L2), so the bytes are compared; False where only shapes can be (float data
    # assigned by inner product: the device's sum order may break a near-tie between two lists the other way).
    stored_bytes = True

    def check_stored(self, state, stored, what=""):
        want = self.with_stored(state, stored)
        for c in want:
            if want[c] is not state[c]:
                same_stored(want[c], state[c], self.stored_bytes, "%s: the handle's %s against the walk's" % (what, c))

    def close(self, g):
        g.close()


def vlq():
    import vector_line_quantization_amd
    return vector_line_quantization_amd


def call(name):
    return name, (lambda g, *a: getattr(g, name)(*a))


def setter(name):
    return name, (lambda g, v: setattr(g, name, v))


# ----------------------------------------------------------------------------------------------------------------------
# GpuFlat: the stored norms (add extends them, reset + add rebuilds them)
# ----------------------------------------------------------------------------------------------------------------------
class FlatKind(Kind):
    def __init__(self, d, metric, nq):
        self.d, self.metric, self.nq = d, metric, nq
        self.name = "flat-%s-d%d-nq%d" % (metric, d, nq)

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(800 + self.d)
        return dict(xa=rng.standard_normal((400, self.d)).astype(F32), xo=(0.5 + rng.standard_normal((300, self.d))).astype(F32),
                    xq=rng.standard_normal((25, self.d)).astype(F32)[:self.nq])

    def walk(self):
        w = self.world()
        xa, xo = w["xa"], w["xo"]
        wk = Walk(xb=xa[:150], scan_split=(0, 0))
        wk.step("add: the norms are extended", lambda g: g.add(xa[150:]), xb=xa)
        wk.to_torch()
        wk.step("reset", lambda g: g.reset(), xb=np.zeros((0, self.d), F32))
        wk.step("add of other vectors: the norms are rebuilt", lambda g: g.add(xo), old=dict(xb=xa), xb=xo)
        wk.to_own()
        wk.step("add once more behind them", lambda g: g.add(xa[:70]), xb=np.concatenate([xo, xa[:70]]))
        wk.step("scan_split(32, 2)", lambda g: g.scan_split(32, 2), scan_split=(32, 2))
        wk.step("scan_split(0, 0)", lambda g: g.scan_split(0, 0), scan_split=(0, 0))
        return wk.steps

    def recipe(self, state):
        calls = [("GpuFlat", lambda d, m: vlq().GpuFlat(d, metric=m), (self.d, self.metric))]
        if state["xb"].shape[0]:
            calls.append(call("add") + ((state["xb"],),))
        return calls

    def start(self, state):
        return self.fresh(state)             # (the first step IS an add)

    def read(self, g):
        return g.reconstruct_n() if g.ntotal else np.zeros((0, self.d), F32)

    def with_stored(self, state, stored):
        return dict(state, xb=stored)

    def search(self, g, state, xq):
        return g.search(xq, self.k)

    def reference(self, state, xq, coarse=None):
        return knn_ref.search(xq, state["xb"], self.k, self.metric)


# ----------------------------------------------------------------------------------------------------------------------
# GpuLSH: stored codes under a new rotation / new thresholds
# ----------------------------------------------------------------------------------------------------------------------
def rotation(seed, d, nbits):
    m = max(d, nbits)
    q, _r = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, m)))
    return np.ascontiguousarray(q[:nbits, :d], dtype=F32)


class LshKind(Kind):
    name = "lsh-64bit-d32"
    d, nbits = 32, 64

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(900)
        w = dict(xa=rng.standard_normal((500, self.d)).astype(F32), xo=rng.standard_normal((500, self.d)).astype(F32),
                 xq=rng.standard_normal((64, self.d)).astype(F32))
        w["A"], w["bA"] = rotation(1, self.d, self.nbits), (0.1 * rng.standard_normal(self.nbits)).astype(F32)
        w["B"], w["bB"] = rotation(2, self.d, self.nbits), (0.1 * rng.standard_normal(self.nbits)).astype(F32)
        w["thrA"] = (0.2 * rng.standard_normal(self.nbits)).astype(F32)
        w["thrB"] = (0.4 * rng.standard_normal(self.nbits)).astype(F32)
        w["xt"] = (0.3 + rng.standard_normal((301, self.d))).astype(F32)          # the second training set: its medians are off zero
        return w

    def walk(self):
        w = self.world()
        enc = lambda x, s: lsh_ref.encode(x, self.nbits, s["A"], s["b"], s["thr"])  # noqa: E731
        first = dict(A=w["A"], b=w["bA"], thr=w["thrA"])
        wk = Walk(codes=enc(w["xa"], first), scan_split=(0, 0), **first)
        wk.step("set_rotation(B): stored codes stay, query codes are new", lambda g: g.set_rotation(w["B"], w["bB"]), A=w["B"], b=w["bB"])
        wk.to_torch()
        wk.step("set_thresholds(B)", lambda g: g.set_thresholds(w["thrB"]), thr=w["thrB"])
        wk.step("train again", lambda g: g.train(w["xt"]), thr=lsh_ref.train(w["xt"], self.nbits, w["B"], w["bB"]))
        wk.to_own()
        wk.step("reset + add of other vectors", lambda g: (g.reset(), g.add(w["xo"])), codes=enc(w["xo"], wk.state))
        wk.step("scan_split(2, 3)", lambda g: g.scan_split(2, 3), scan_split=(2, 3))
        wk.step("scan_split(0, 0)", lambda g: g.scan_split(0, 0), scan_split=(0, 0))
        return wk.steps

    def recipe(self, state):
        return [("GpuLSH", lambda d, n: vlq().GpuLSH(d, n, rotate_data=True, train_thresholds=True), (self.d, self.nbits)),
                call("set_rotation") + ((state["A"], state["b"]),), call("set_thresholds") + ((state["thr"],),),
                call("add_codes") + ((state["codes"],),)]

    def start(self, state):
        g = vlq().GpuLSH(self.d, self.nbits, rotate_data=True, train_thresholds=True)
        g.set_rotation(state["A"], state["b"])
        g.set_thresholds(state["thr"])
        g.add(self.world()["xa"])
        return g

    def read(self, g):
        return g.get_codes()

    def with_stored(self, state, stored):
        return dict(state, codes=stored)

    def search(self, g, state, xq):
        return g.search(xq, self.k)

    def reference(self, state, xq, coarse=None):
        return lsh_ref.search_codes(lsh_ref.encode(xq, self.nbits, state["A"], state["b"], state["thr"]), state["codes"], self.k)


# ----------------------------------------------------------------------------------------------------------------------
# GpuSQ: a second set_trained over stored codes
# ----------------------------------------------------------------------------------------------------------------------
def other_range(trained):
    """world B of a scalar quantizer's range: vmin lower by 0.3, vdiff 1.25 times as wide"""
    t = np.asarray(trained, F32)
    h = t.size // 2
    return np.concatenate([t[:h] - F32(0.3), t[h:] * F32(1.25)]).astype(F32)


class SqKind(Kind):
    def __init__(self, d, qtype):
        self.d, self.qtype, self.qt = d, qtype, ivfsq_ref.QTYPES[qtype]
        self.name = "sq-%s-d%d" % (qtype, d)

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(700 + self.d)
        w = dict(xa=rng.standard_normal((300, self.d)).astype(F32), xo=rng.standard_normal((300, self.d)).astype(F32),
                 xq=rng.standard_normal((64, self.d)).astype(F32))
        w["tA"] = ivfsq_ref.train(w["xa"], self.qt)
        w["tB"] = other_range(w["tA"])
        return w

    def walk(self):
        w = self.world()
        enc = lambda x, t: ivfsq_ref.encode(x, self.qt, t)  # noqa: E731
        wk = Walk(trained=w["tA"], codes=enc(w["xa"], w["tA"]), scan_split=(0, 0))
        wk.step("set_trained(B) over the stored codes", lambda g: g.set_trained(w["tB"]), trained=w["tB"])
        wk.to_torch()
        other = enc(w["xo"], w["tB"])
        wk.step("set_codes of other codes", lambda g: g.set_codes(other), codes=other)
        wk.to_own()
        wk.step("reset + add", lambda g: (g.reset(), g.add(w["xa"])), codes=enc(w["xa"], w["tB"]))
        wk.step("set_scan_split(4, 5)", lambda g: g.set_scan_split(4, 5), scan_split=(4, 5))
        wk.step("set_scan_split(0, 0)", lambda g: g.set_scan_split(0, 0), scan_split=(0, 0))
        return wk.steps

    def recipe(self, state):
        return [("GpuSQ", lambda d, q: vlq().GpuSQ(d, q), (self.d, self.qtype)), call("set_trained") + ((state["trained"],),),
                call("set_codes") + ((state["codes"],),)]

    def start(self, state):
        g = vlq().GpuSQ(self.d, self.qtype)
        g.set_trained(state["trained"])
        g.add(self.world()["xa"])
        return g

    def read(self, g):
        return g.codes()

    def with_stored(self, state, stored):
        return dict(state, codes=stored)

    def search(self, g, state, xq):
        return g.search(xq, self.k)

    def reference(self, state, xq, coarse=None):
        return sqflat_ref.search(state["codes"], state["trained"], xq, self.k, "l2", self.qt)

    def extras(self, g, state):
        return [("reconstruct_n", bits(g.reconstruct_n()), bits(ivfsq_ref.decode_scalar(state["codes"], self.d, self.qt, state["trained"])))]


# ----------------------------------------------------------------------------------------------------------------------
# GpuPQ: a second set_centroids under every search type (the SDC table among them)
# ----------------------------------------------------------------------------------------------------------------------
class PqKind(Kind):
    d, M, nbits, HT = 32, 8, 8, 33
    compare = staticmethod(topk_rule)

    def __init__(self, metric):
        self.metric = metric
        self.name = "pq-%s" % metric

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(600)
        cA = (0.5 * rng.standard_normal((self.M, 256, self.d // self.M))).astype(F32)
        return dict(cA=cA, cB=(cA * F32(1.25) + F32(0.5)).astype(F32), xa=(0.7 * rng.standard_normal((500, self.d))).astype(F32),
                    xo=(0.3 + 0.7 * rng.standard_normal((500, self.d))).astype(F32), xq=(0.7 * rng.standard_normal((64, self.d))).astype(F32))

    def walk(self):
        w = self.world()
        cA, cB = w["cA"], w["cB"]
        wk = Walk(cent=cA, codes=pq_ref.compute_codes(w["xa"], cA), search_type=pq_ref.ST_PQ, ht=self.nbits * self.M + 1, scan_split=(0, 0))
        wk.step("set_centroids(B) under ST_PQ", lambda g: g.set_centroids(cB), cent=cB)
        if self.metric == "l2":
            wk.step("search_type = sdc with B loaded", lambda g: setattr(g, "search_type", "sdc"), search_type=pq_ref.ST_SDC)
            wk.to_torch()
            wk.step("set_centroids(A) under ST_SDC", lambda g: g.set_centroids(cA), cent=cA)

            def poly(g):
                g.polysemous_ht = self.HT
                g.search_type = "polysemous"
            wk.step("search_type = polysemous", poly, search_type=pq_ref.ST_POLYSEMOUS, ht=self.HT)
            wk.step("set_centroids(B) under ST_polysemous", lambda g: g.set_centroids(cB), cent=cB)
        else:
            wk.to_torch()
        other = pq_ref.compute_codes(w["xo"], cB)
        wk.step("set_codes of other codes", lambda g: g.set_codes(other), codes=other)
        wk.to_own()
        wk.step("reset + add", lambda g: (g.reset(), g.add(w["xa"])), codes=pq_ref.compute_codes(w["xa"], wk.state["cent"]))
        wk.step("set_scan_split(2, 3)", lambda g: g.set_scan_split(2, 3), scan_split=(2, 3))
        wk.step("set_scan_split(0, 0)", lambda g: g.set_scan_split(0, 0), scan_split=(0, 0))
        return wk.steps

    def recipe(self, state):
        return [("GpuPQ", lambda d, M, nb, m: vlq().GpuPQ(d, M, nb, metric=m), (self.d, self.M, self.nbits, self.metric)),
                call("set_centroids") + ((state["cent"],),), setter("polysemous_ht") + ((state["ht"],),),
                setter("search_type") + ((state["search_type"],),), call("set_codes") + ((state["codes"],),)]

    def start(self, state):
        g = vlq().GpuPQ(self.d, self.M, self.nbits, metric=self.metric)
        g.set_centroids(state["cent"])
        g.add(self.world()["xa"])
        return g

    def read(self, g):
        return g.codes()

    def with_stored(self, state, stored):
        return dict(state, codes=stored)

    def search(self, g, state, xq):
        return g.search(xq, self.k)

    def reference(self, state, xq, coarse=None):
        return pq_ref.search(state["cent"], state["codes"], xq, self.k, self.metric, state["search_type"], state["ht"])[:2]


# ----------------------------------------------------------------------------------------------------------------------
# the host side of an IVF index: assignment, lists, coarse stage
# ----------------------------------------------------------------------------------------------------------------------
def flat_quantizer(coarse):
    nlist, d = coarse.shape
    return OracleIndex(d, nlist, 1, 1, coarse, np.zeros((1, 2, d), F32), by_residual=False)


def host_coarse(coarse, x, nprobe, metric):
    """(coarse_dis, keys) of the flat quantizer on the host: the C++ oracle under L2, ip_ref under inner product"""
    if metric == "ip":
        keys, dis = ip_ref.coarse_search(coarse, x, nprobe)
        return dis, keys
    return flat_quantizer(coarse).coarse_search(x, nprobe, canonical=True)


def append(lists, assign, rows, ids=None):
    """lists = (rows, ids, offsets) after a stable append of a batch (start from empty_lists()); sequential ids where none are given"""
    old_rows, old_ids, off = lists
    nlist = off.shape[0] - 1
    if ids is None:
        ids = np.arange(old_ids.shape[0], old_ids.shape[0] + rows.shape[0], dtype=np.int64)
    all_assign = np.concatenate([np.repeat(np.arange(nlist), np.diff(off)), np.asarray(assign, np.int64)])
    order = np.argsort(all_assign, kind="stable")
    out_off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(all_assign, minlength=nlist), out=out_off[1:])
    return np.ascontiguousarray(np.concatenate([old_rows, rows])[order]), np.concatenate([old_ids, ids])[order], out_off


def empty_lists(nlist, width, dtype):
    return np.zeros((0, width), dtype), np.zeros((0,), np.int64), np.zeros((nlist + 1,), np.int64)


def read_ivf_lists(g, nlist):
    got = [g.get_list(i) for i in range(nlist)]
    lens = np.array([len(x[-1]) for x in got], np.int64)
    return tuple(np.concatenate([x[j] for x in got]) for j in range(len(got[0]))) + (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),)


def clustered(rng, centres, n, spread):
    return (centres[rng.integers(0, centres.shape[0], n)] + spread * rng.standard_normal((n, centres.shape[1]))).astype(F32)


# ----------------------------------------------------------------------------------------------------------------------
# GpuIVFFlat (search and range_search) and GpuIVFSQ
# ----------------------------------------------------------------------------------------------------------------------
class IvfFlatKind(Kind):
    nlist, nprobe, d = 16, 4, 32
    compare = staticmethod(topk_rule)

    def __init__(self, metric):
        self.metric = metric
        self.name = "ivfflat-%s" % metric
        self.stored_bytes = metric == "l2"

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(500)
        centres = rng.standard_normal((self.nlist, self.d)).astype(F32)
        w = dict(cA=centres, cR=np.ascontiguousarray(np.roll(centres, 1, 0)), xa=clustered(rng, centres, 1500, 0.5),
                 xo=clustered(rng, centres, 1200, 0.5), xm=clustered(rng, centres, 300, 0.5), xq=clustered(rng, centres, 64, 0.5))
        first = self.add(empty_lists(self.nlist, self.d, F32), centres, w["xa"])
        cd, keys = host_coarse(centres, w["xq"], self.nprobe, self.metric)
        D, _I = self.rows(dict(coarse=centres, lists=first), w["xq"], keys)
        w["radius"] = float(np.median(D[:, 4]))          # about five hits a query in world A
        return w

    def add(self, lists, coarse, x):
        return append(lists, host_coarse(coarse, x, 1, self.metric)[1][:, 0], x)

    def walk(self):
        w = self.world()
        cA, cR = w["cA"], w["cR"]
        empty = empty_lists(self.nlist, self.d, F32)
        wk = Walk(coarse=cA, lists=self.add(empty, cA, w["xa"]), range=False)
        wk.step("set_coarse_centroids(rolled): the lists stay", lambda g: g.set_coarse_centroids(cR), coarse=cR, range=True)
        wk.to_torch()
        wk.step("reset", lambda g: g.reset(), lists=empty, range=False)
        wk.step("add of other vectors", lambda g: g.add(w["xo"]), old=dict(lists=wk.steps[1].state["lists"]),
                lists=self.add(empty, cR, w["xo"]), range=True)
        wk.to_own()
        wk.step("add again", lambda g: g.add(w["xm"]), lists=self.add(wk.state["lists"], cR, w["xm"]), range=False)
        return wk.steps

    def recipe(self, state):
        return [("GpuIVFFlat", lambda d, n, m: vlq().GpuIVFFlat(d, n, metric=m), (self.d, self.nlist, self.metric)),
                call("set_coarse_centroids") + ((state["coarse"],),), call("set_lists") + (state["lists"],)]

    def start(self, state):
        g = vlq().GpuIVFFlat(self.d, self.nlist, metric=self.metric)
        g.set_coarse_centroids(state["coarse"])
        g.add(self.world()["xa"])
        return g

    def read(self, g):
        return read_ivf_lists(g, self.nlist)

    def with_stored(self, state, stored):
        return dict(state, lists=stored)

    def search(self, g, state, xq):
        return g.search(xq, self.nprobe, self.k)

    def coarse(self, g, state, xq):
        return g.coarse_search(xq, self.nprobe)

    def rows(self, state, xq, keys):
        vecs, ids, off = state["lists"]
        return ivfflat_ref.search_preassigned(dict(vecs=vecs, ids=ids, list_offsets=off), xq, keys, self.k, self.metric)[:2]

    def reference(self, state, xq, coarse=None):
        cd, keys = host_coarse(state["coarse"], xq, self.nprobe, self.metric) if coarse is None else coarse
        return self.rows(state, xq, keys)

    def extras(self, g, state):
        if not state["range"]:
            return []
        w = self.world()
        xq = w["xq"][:40]
        vecs, ids, off = state["lists"]
        _cd, keys = g.coarse_search(xq, self.nprobe)
        lims, D, I = range_ref.range_search_preassigned(dict(vecs=vecs, ids=ids, list_offsets=off), xq, keys, w["radius"], self.metric)
        gl, gD, gI = g.range_search(xq, self.nprobe, w["radius"])
        assert lims[-1] > 0, "the radius leaves no hit"
        return [("range lims", host(gl), lims), ("range D", bits(host(gD)), bits(D)), ("range I", host(gI), I)]


class IvfSqKind(Kind):
    nlist, nprobe = 16, 4

    def __init__(self, d, qtype):
        self.d, self.qtype, self.qt = d, qtype, ivfsq_ref.QTYPES[qtype]
        self.name = "ivfsq-%s-d%d" % (qtype, d)

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(400 + self.d)
        centres = rng.standard_normal((self.nlist, self.d)).astype(F32)
        w = dict(cA=centres, cR=np.ascontiguousarray(np.roll(centres, 1, 0)), xa=clustered(rng, centres, 1500, 0.5),
                 xo=clustered(rng, centres, 1200, 0.5), xm=clustered(rng, centres, 300, 0.5), xq=clustered(rng, centres, 64, 0.5))
        a = host_coarse(centres, w["xa"], 1, "l2")[1][:, 0]
        w["tA"] = ivfsq_ref.train((w["xa"] - centres[a]).astype(F32), self.qt)
        w["tB"] = other_range(w["tA"])
        return w

    def add(self, lists, coarse, trained, x):
        a = host_coarse(coarse, x, 1, "l2")[1][:, 0]
        return append(lists, a, ivfsq_ref.encode((x - coarse[a]).astype(F32), self.qt, trained))

    def walk(self):
        w = self.world()
        cA, cR, tA, tB = w["cA"], w["cR"], w["tA"], w["tB"]
        empty = empty_lists(self.nlist, ivfsq_ref.code_size(self.d, self.qt), np.uint8)
        wk = Walk(coarse=cA, trained=tA, lists=self.add(empty, cA, tA, w["xa"]))
        wk.step("set_coarse_centroids(rolled): the lists stay", lambda g: g.set_coarse_centroids(cR), coarse=cR)
        wk.to_torch()
        wk.step("set_trained(B) over the stored codes", lambda g: g.set_trained(tB), trained=tB)
        loaded = wk.state["lists"]
        wk.step("reset", lambda g: g.reset(), lists=empty)
        wk.step("add of other vectors", lambda g: g.add(w["xo"]), old=dict(lists=loaded), lists=self.add(empty, cR, tB, w["xo"]))
        wk.to_own()
        wk.step("add again", lambda g: g.add(w["xm"]), lists=self.add(wk.state["lists"], cR, tB, w["xm"]))
        return wk.steps

    def recipe(self, state):
        return [("GpuIVFSQ", lambda d, n, q: vlq().GpuIVFSQ(d, n, q), (self.d, self.nlist, self.qtype)),
                call("set_coarse_centroids") + ((state["coarse"],),), call("set_trained") + ((state["trained"],),),
                call("set_lists") + (state["lists"],)]

    def start(self, state):
        g = vlq().GpuIVFSQ(self.d, self.nlist, self.qtype)
        g.set_coarse_centroids(state["coarse"])
        g.set_trained(state["trained"])
        g.add(self.world()["xa"])
        return g

    def read(self, g):
        return read_ivf_lists(g, self.nlist)

    def with_stored(self, state, stored):
        return dict(state, lists=stored)

    def search(self, g, state, xq):
        return g.search(xq, self.nprobe, self.k)

    def coarse(self, g, state, xq):
        return g.coarse_search(xq, self.nprobe)

    def reference(self, state, xq, coarse=None):
        cd, keys = host_coarse(state["coarse"], xq, self.nprobe, "l2") if coarse is None else coarse
        codes, ids, off = state["lists"]
        z = dict(coarse_centroids=state["coarse"], trained=state["trained"], codes=codes, ids=ids, list_offsets=off)
        return ivfsq_ref.search_preassigned(z, xq, keys, cd, self.k, "l2", self.qt)


# ----------------------------------------------------------------------------------------------------------------------
# GpuIVFPQ: the generic kernel, flat <-> multi-index, IVFPQR
# ----------------------------------------------------------------------------------------------------------------------
class IvfPqBase(Kind):
    """state: coarse (None under a multi-index quantizer), imi, pq, lists (codes, ids, offsets), by_residual, table, metric, ht,
    fp16, nq; the speed-only toggles ride along and are read by nobody"""
    imi_nbits = 0
    DEFAULTS = dict(imi=None, by_residual=True, table=1, metric="l2", ht=0, fp16=False, nq=64)

    def k_of(self, state):
        """the k of the state's searches (a walk may change it: it is part of the handle's walk key, not of its trained state)"""
        return state.get("k", self.k)

    def oracle(self, state, lists=True):
        codes, ids, off = state["lists"] if lists else (None, None, None)
        imi = state["imi"]
        ox = OracleIndex(self.d, self.nlist, self.M, self.nbits, None if imi is not None else state["coarse"], state["pq"], codes=codes, ids=ids,
                         list_offsets=off, by_residual=state["by_residual"], use_precomputed_table=state["table"], imi_centroids=imi,
                         imi_nbits=self.imi_nbits if imi is not None else 0)
        ox.float16_tables = bool(state["fp16"])
        return ox

    def encode_lists(self, state, x, ids=None, base=None):
        """the lists of `base` (None: empty) with x appended as the oracle encodes it under the state's trained components"""
        ox = self.oracle(dict(state, lists=base if base is not None else empty_lists(self.nlist, self.M, np.uint8)))
        ox.add(x, ids, canonical=True)
        return ox.codes, ox.ids, ox.list_offsets

    def quantizer_calls(self, state):
        if state["imi"] is not None:
            return [call("set_imi_centroids") + ((self.imi_nbits, state["imi"]),)]
        return [call("set_coarse_centroids") + ((state["coarse"],),)]

    def recipe(self, state):
        calls = [("GpuIVFPQ", lambda d, n, M, nb, m: vlq().GpuIVFPQ(d, n, M, nb, metric=m), (self.d, self.nlist, self.M, self.nbits, state["metric"]))]
        calls += self.quantizer_calls(state)
        calls.append(call("set_pq_centroids") + ((state["pq"],),))
        calls.append(call("set_search_options") + ((state["by_residual"], state["table"], 0),))
        if state["fp16"]:
            calls.append(call("set_float16_tables") + ((True,),))
        if state["ht"]:
            calls.append(call("set_polysemous_ht") + ((state["ht"],),))
        calls.append(call("set_lists") + (state["lists"],))
        return calls

    def queries(self, state):
        return self.world()["xq"][:state["nq"]]

    def read(self, g):
        return read_ivf_lists(g, self.nlist)

    def with_stored(self, state, stored):
        return dict(state, lists=stored)

    def search(self, g, state, xq):
        return g.search(xq, self.nprobe, self.k_of(state))

    def needs_coarse(self, state):
        return state["metric"] == "ip" or bool(state["ht"])

    def coarse(self, g, state, xq):
        return g.coarse_search(xq, self.nprobe) if self.needs_coarse(state) else None

    def rule(self, state):
        """bit for bit against the oracle's canonical labels; tests/util.py's assert_same_topk where the kind's own tests use it
        (inner product, the polysemous filter, a multi-index quantizer)"""
        return topk_rule if self.needs_coarse(state) or state["imi"] is not None else exact

    def reference(self, state, xq, coarse=None):
        codes, ids, off = state["lists"]
        if state["metric"] == "ip":
            cd, keys = host_coarse(state["coarse"], xq, self.nprobe, "ip") if coarse is None else coarse
            z = dict(coarse_centroids=state["coarse"], pq_centroids=state["pq"], codes=codes, ids=ids, list_offsets=off,
                     by_residual=int(state["by_residual"]), max_codes=0)
            return ip_ref.search_preassigned(z, xq, keys, self.k_of(state))[:2]
        ox = self.oracle(state)
        if state["ht"]:
            cd, keys = ox.coarse_search(xq, self.nprobe, canonical=True) if coarse is None else coarse
            D, P, _npass, _ncode = polysemous_ref.oracle_filtered(polysemous_ref.oracle_scan(ox, xq, keys, cd), state["ht"], self.k_of(state))
            return D, polysemous_ref.labels_to_ids(off, ids, P)
        return ox.search(xq, self.nprobe, self.k_of(state), canonical=True)


def options(by_residual, table):
    return lambda g: g.set_search_options(by_residual, table, 0)


class IvfPqGenericKind(IvfPqBase):
    """d 32, nlist 16, M 8 x 8 bit: the generic scan kernel, with the IP and polysemous kernels of the same shape"""
    name = "ivfpq-generic"
    d, nlist, M, nbits, nprobe, HT = 32, 16, 8, 8, 4, 34

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(1234)
        centres = rng.standard_normal((40, self.d)).astype(F32)
        xa = clustered(rng, centres, 2000, 0.6)
        cA = xa[rng.permutation(2000)[:self.nlist]].copy()
        pA = (0.5 * rng.standard_normal((self.M, 256, self.d // self.M))).astype(F32)
        return dict(xa=xa, xo=clustered(rng, centres, 1800, 0.6), xm=clustered(rng, centres, 300, 0.6), xq=clustered(rng, centres, 64, 0.6),
                    cA=cA, cB=(cA + F32(1.5)).astype(F32), pA=pA, pB=(pA * F32(1.25) + F32(0.5)).astype(F32))

    def walk(self):
        w = self.world()
        cA, cB, pA, pB = w["cA"], w["cB"], w["pA"], w["pB"]
        first = dict(self.DEFAULTS, coarse=cA, pq=pA, capacity="packed")
        wk = Walk(lists=self.encode_lists(first, w["xa"]), **first)
        wk.step("set_pq_centroids(B)", lambda g: g.set_pq_centroids(pB), pq=pB)
        wk.step("set_coarse_centroids(B): the lists keep their codes", lambda g: g.set_coarse_centroids(cB), coarse=cB)
        wk.step("use_precomputed_table 1 -> 0", options(True, 0), table=0)
        wk.step("use_precomputed_table 0 -> 1", options(True, 1), table=1)
        wk.to_torch()
        wk.steps.append(Step("set_float16_tables(True) at M = 8", lambda g: g.set_float16_tables(True), wk.state, refuse=ERR_UNSUPPORTED))
        wk.step("by_residual True -> False", options(False, 1), by_residual=False)
        wk.step("by_residual False -> True", options(True, 1), by_residual=True)
        wk.step("metric l2 -> ip", lambda g: setattr(g, "metric", "ip"), metric="ip")
        wk.step("set_pq_centroids(A) under ip", lambda g: g.set_pq_centroids(pA), pq=pA)
        # (the stale answer of this step: term 2 of the codebook that was loaded when the table was released)
        wk.step("metric ip -> l2: term 2 is rebuilt from A", lambda g: setattr(g, "metric", "l2"), old=dict(pq=pB), metric="l2")
        wk.step("set_polysemous_ht(%d)" % self.HT, lambda g: g.set_polysemous_ht(self.HT), ht=self.HT)
        wk.step("set_pq_centroids(B) under the filter", lambda g: g.set_pq_centroids(pB), pq=pB)
        wk.step("polysemous_ht = 0", lambda g: g.set_polysemous_ht(0), ht=0)
        wk.to_own()
        other = self.encode_lists(wk.state, w["xo"], ids=np.arange(1800, dtype=np.int64))
        wk.step("set_lists of a different database", lambda g: g.set_lists(*other), lists=other)
        wk.step("add", lambda g: g.add(w["xm"]), lists=self.encode_lists(wk.state, w["xm"], base=other))
        wk.step("reserve_memory", lambda g: g.reserve_memory(8000), capacity="reserved")
        wk.step("reclaim_memory", lambda g: g.reclaim_memory(), capacity="packed")
        return wk.steps

    def start(self, state):
        g = vlq().GpuIVFPQ(self.d, self.nlist, self.M, self.nbits)
        g.set_coarse_centroids(state["coarse"])
        g.set_pq_centroids(state["pq"])
        g.add(self.world()["xa"])
        return g


class IvfPq16Kind(IvfPqBase):
    """d 128, nlist 64, M 16 x 8 bit, the lists of scan_sums_cases.common_world() and batches of 2 048 queries: the engineered
    16-byte kernel with its stored table sums, half(term 2) and walk order.  The generator's byte-valued coordinates are divided
    by 255 (centroids, codebook and queries alike; the codes stay): half tables of byte-valued data are refused (|term 2| beyond
    the half range, include/vlq_ivfpq.h), and the walk needs them.  World B is case_stale's, on that scale."""
    name = "ivfpq-16byte"
    d, nlist, M, nbits, nprobe = 128, 64, 16, 8, 16
    TOGGLES = dict(scan_schedule=0, scan_sums=1, coarse_screen=1)

    @functools.lru_cache(maxsize=None)
    def world(self):
        import scan_sums_cases as ssc
        _rng, ox, coarse, pq, xq, _gen = ssc.common_world()
        s = F32(1.0 / 255.0)
        cA, pA = (coarse * s).astype(F32), (pq * s).astype(F32)
        return dict(cA=cA, pA=pA, cB=(cA + F32(1.5) * s).astype(F32), pB=(pA * F32(1.25) + F32(0.5) * s).astype(F32),
                    xq=(xq[:2048] * s).astype(F32), lists=(ox.codes, ox.ids, ox.list_offsets))

    def walk(self):
        w = self.world()
        wk = Walk(**dict(self.DEFAULTS, coarse=w["cA"], pq=w["pA"], lists=w["lists"], nq=2048, k=10, **self.TOGGLES))
        wk.step("set_float16_tables(True)", lambda g: g.set_float16_tables(True), fp16=True)
        wk.step("set_pq_centroids(B) while fp16: half(term 2)", lambda g: g.set_pq_centroids(w["pB"]), pq=w["pB"])
        wk.step("set_float16_tables(False)", lambda g: g.set_float16_tables(False), fp16=False)
        wk.to_torch()
        wk.step("set_coarse_centroids(B)", lambda g: g.set_coarse_centroids(w["cB"]), coarse=w["cB"])
        for mode in (2, 3, 4, 1, 0):
            wk.step("set_scan_schedule(%d)" % mode, lambda g, mode=mode: g.set_scan_schedule(mode), scan_schedule=mode)
        for mode in (0, 1):
            wk.step("set_scan_sums(%d)" % mode, lambda g, mode=mode: g.set_scan_sums(mode), scan_sums=mode)
        for mode in (0, 1):
            wk.step("set_coarse_screen(%d)" % mode, lambda g, mode=mode: g.set_coarse_screen(mode), coarse_screen=mode)
        wk.to_own()
        # The handle keeps the walk times it measured under walk_key = (nprobe, k, batch class) and starts afresh when the key of
        # a search differs (csrc/scan_stage.hip).  The class is 1 for every batch below 4 096 queries, the 64-query batch takes
        # no walk at all, so the key moves with k: 20 here (<= 32: the stored sums stay live), and back to 10 afterwards.
        for nq, k, what in ((64, 10, "a batch of 64 queries: the split scan"), (2048, 20, "2 048 queries again at k = 20: another walk key"),):
            wk.state = dict(wk.state, nq=nq, k=k, history=wk.state["history"] + (what,))
            wk.steps.append(Step(what, lambda g: None, wk.state, resize=True))
        wk.step("set_pq_centroids(A) under the new walk key", lambda g: g.set_pq_centroids(w["pA"]), pq=w["pA"])
        what = "k = 10 again: the first walk key once more"
        wk.state = dict(wk.state, k=10, history=wk.state["history"] + (what,))
        wk.steps.append(Step(what, lambda g: None, wk.state, resize=True))
        wk.step("set_coarse_centroids(A) under the first walk key", lambda g: g.set_coarse_centroids(w["cA"]), coarse=w["cA"])
        return wk.steps

    def start(self, state):
        return self.fresh(state)

    def ran(self, g, state):
        """What last_scan_info() and scan_sums_state() tell of the path that answered.  The text names the kernel template and
        ends in the rows it read; it does not name the half tables or the split (the rows themselves do: they are the fp16
        oracle's, which differ from the fp32 ones in every row, tests/test_restate_cases.py).
          2 048 queries, fp32, sums on, query-major schedule: rows=sums, and scan_sums_state counts exactly this batch
          half tables, the other schedules, sums off, 64 queries: rows=stored, and the counter stands still
          64 queries: no walk order is taken (first=-1) -- the batch is below the walk's size, the scan is split over workgroups
          2 048 queries: the walk statistic ran (first >= 0)"""
        info, sums = g.last_scan_info(), g.scan_sums_state()
        seen = getattr(g, "_restate_seen", 0)
        g._restate_seen = sums[1]
        assert "kernel=scan16_kernel<" in info, info
        on_sums = state["nq"] == 2048 and not state["fp16"] and state["scan_sums"] == 1 and state["scan_schedule"] < 2
        assert info.endswith(" rows=sums" if on_sums else " rows=stored"), (state["history"][-1], info)
        assert sums[1] - seen == (state["nq"] if on_sums else 0), (state["history"][-1], sums, seen)
        assert sums[0] == (state["scan_sums"] == 1), sums
        assert (" first=-1 " in info) == (state["nq"] == 64), (state["history"][-1], info)


class IvfPqImiKind(IvfPqBase):
    """nlist 64 = 2 x 3 bits, d 32, M 8: one handle under a flat quantizer, a multi-index quantizer, and the flat one again"""
    name = "ivfpq-flat-imi"
    d, nlist, M, nbits, nprobe, imi_nbits = 32, 64, 8, 8, 8, 3

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(4321)
        centres = rng.random((40, self.d)).astype(F32)
        xa = clustered(rng, centres, 3000, 0.08)
        h = self.d // 2
        imi = np.stack([xa[rng.choice(3000, 8, replace=False), :h], xa[rng.choice(3000, 8, replace=False), h:]]).astype(F32)
        return dict(xa=xa, xq=clustered(rng, centres, 2048, 0.08), cA=xa[rng.permutation(3000)[:self.nlist]].copy(), imi=imi,
                    pq=(0.05 * rng.standard_normal((self.M, 256, self.d // self.M))).astype(F32))

    def walk(self):
        w = self.world()
        flat = dict(self.DEFAULTS, coarse=w["cA"], pq=w["pq"])
        multi = dict(flat, coarse=None, imi=w["imi"])
        lf, lm = self.encode_lists(flat, w["xa"]), self.encode_lists(multi, w["xa"])
        wk = Walk(lists=lf, **flat)
        wk.step("set_imi_centroids + set_lists of the multi-index assignment", lambda g: (g.set_imi_centroids(self.imi_nbits, w["imi"]), g.set_lists(*lm)),
                coarse=None, imi=w["imi"], lists=lm)
        wk.to_torch()
        wk.step("set_coarse_centroids(A) + set_lists: as if the multi-index had never been set", lambda g: (g.set_coarse_centroids(w["cA"]), g.set_lists(*lf)),
                coarse=w["cA"], imi=None, lists=lf)
        wk.steps.append(Step("2 048 queries", lambda g: None, dict(wk.state, nq=2048, history=wk.state["history"] + ("2 048 queries",)), resize=True))
        wk.state = wk.steps[-1].state
        wk.to_own()
        wk.step("the multi-index quantizer once more, 2 048 queries", lambda g: (g.set_imi_centroids(self.imi_nbits, w["imi"]), g.set_lists(*lm)),
                coarse=None, imi=w["imi"], lists=lm)
        return wk.steps

    def start(self, state):
        return self.fresh(state)


class IvfPqScreenKind(IvfPqImiKind):
    """nlist 256 = 2 x 4 bits, d 32, M 8, batches of 2 048 queries: the smallest flat quantizer whose float16 coarse screen is
    live (256 centroids, 2 048 rows; include/vlq_ivfpq.h), under new centroids, a visit to a multi-index quantizer (whose halves
    of 16 centroids have no screen) and back"""
    name = "ivfpq-screen"
    nlist, imi_nbits = 256, 4

    @functools.lru_cache(maxsize=None)
    def world(self):
        rng = np.random.default_rng(8765)
        centres = rng.random((60, self.d)).astype(F32)
        xa = clustered(rng, centres, 4000, 0.08)
        h = self.d // 2
        imi = np.stack([xa[rng.choice(4000, 16, replace=False), :h], xa[rng.choice(4000, 16, replace=False), h:]]).astype(F32)
        rows = rng.permutation(4000)
        # (world B: 256 other rows of the data.  Centroids 1.5 away from every query in every coordinate leave the half-precision
        # bound nothing to decide, and the handle then drops the screen by itself: the state this walk is about would be gone)
        cA, cB = xa[rows[:self.nlist]].copy(), xa[rows[self.nlist:2 * self.nlist]].copy()
        return dict(xa=xa, xq=clustered(rng, centres, 2048, 0.08), cA=cA, cB=cB, imi=imi,
                    pq=(0.05 * rng.standard_normal((self.M, 256, self.d // self.M))).astype(F32))

    def walk(self):
        w = self.world()
        flat = dict(self.DEFAULTS, coarse=w["cA"], pq=w["pq"], nq=2048, coarse_screen=1)
        multi = dict(flat, coarse=None, imi=w["imi"])
        lf, lm = self.encode_lists(flat, w["xa"]), self.encode_lists(multi, w["xa"])
        wk = Walk(lists=lf, **flat)
        wk.step("set_coarse_centroids(B): the lists keep their codes", lambda g: g.set_coarse_centroids(w["cB"]), coarse=w["cB"])
        wk.to_torch()
        wk.step("set_imi_centroids + set_lists of the multi-index assignment", lambda g: (g.set_imi_centroids(self.imi_nbits, w["imi"]), g.set_lists(*lm)),
                coarse=None, imi=w["imi"], lists=lm)
        wk.step("set_coarse_centroids(A) + set_lists: as if the multi-index had never been set", lambda g: (g.set_coarse_centroids(w["cA"]), g.set_lists(*lf)),
                coarse=w["cA"], imi=None, lists=lf)
        wk.to_own()
        for mode in (0, 1):
            wk.step("set_coarse_screen(%d)" % mode, lambda g, mode=mode: g.set_coarse_screen(mode), coarse_screen=mode)
        wk.step("set_coarse_centroids(B) behind the toggles", lambda g: g.set_coarse_centroids(w["cB"]), coarse=w["cB"])
        return wk.steps

    def ran(self, g, state):
        en, rows, und = g.coarse_screen_state()
        if state["imi"] is None and state["coarse_screen"] == 1:
            assert en and rows >= state["nq"], "the coarse screen is not live at this shape: %s" % ((en, rows, und),)
        if state["coarse_screen"] == 0:
            assert not en


class IvfPqrKind(IvfPqBase):
    """IVFPQR: a second set_refine_pq on a loaded index; state adds rpq (the refine centroids) and rcodes (in list order)"""
    name = "ivfpqr"
    d, nlist, M, nbits, nprobe, Mr, nbits_r, k_factor = 32, 16, 8, 8, 4, 8, 8, 2.0

    @functools.lru_cache(maxsize=None)
    def world(self):
        w = dict(IvfPqGenericKind().world())
        rng = np.random.default_rng(77)
        w["rA"] = (0.1 * rng.standard_normal((self.Mr, 1 << self.nbits_r, self.d // self.Mr))).astype(F32)
        w["rB"] = (w["rA"] * F32(1.25) + F32(0.05)).astype(F32)
        return w

    def refine_codes(self, state, lists, x_by_id):
        """refine codes in list order: the first-minimum code of (x - coarse[list]) - decode(code), float32 steps"""
        codes, ids, off = lists
        a = np.repeat(np.arange(self.nlist), np.diff(off))
        r1 = (x_by_id[ids] - state["coarse"][a]).astype(F32)
        r2 = (r1 - refine_ref.pq_decode(state["pq"], codes)).astype(F32)
        return pq_ref.compute_codes(r2, state["rpq"])

    def walk(self):
        w = self.world()
        first = dict(self.DEFAULTS, coarse=w["cA"], pq=w["pA"], rpq=w["rA"])
        lists = self.encode_lists(first, w["xa"])
        xall = np.concatenate([w["xa"], w["xm"]])
        wk = Walk(lists=lists, rcodes=self.refine_codes(first, lists, xall), **first)
        rB = self.refine_codes(dict(first, rpq=w["rB"]), lists, xall)
        wk.to_torch()
        wk.steps.append(Step("search_refined after set_refine_pq(B), before set_refine_codes", lambda g: g.search_refined(w["xq"], self.nprobe, self.k, self.k_factor),
                             wk.state, refuse=ERR_STATE, pre=[lambda g: g.set_refine_pq(self.Mr, self.nbits_r, w["rB"])]))
        wk.step("set_refine_codes", lambda g: g.set_refine_codes(rB), rpq=w["rB"], rcodes=rB)
        wk.to_own()
        more = self.encode_lists(wk.state, w["xm"], base=lists)
        wk.step("add after it", lambda g: g.add(w["xm"]), lists=more, rcodes=self.refine_codes(wk.state, more, xall))
        return wk.steps

    def recipe(self, state):
        calls = IvfPqBase.recipe(self, state)
        calls.insert(len(calls) - 1, call("set_refine_pq") + ((self.Mr, self.nbits_r, state["rpq"]),))
        calls.append(call("set_refine_codes") + ((state["rcodes"],),))
        return calls

    def start(self, state):
        return self.fresh(state)

    def read(self, g):
        return read_ivf_lists(g, self.nlist), np.concatenate([g.get_list_refine_codes(i) for i in range(self.nlist)])

    def with_stored(self, state, stored):
        return dict(state, lists=stored[0], rcodes=stored[1])

    def search(self, g, state, xq):
        return g.search_refined(xq, self.nprobe, self.k, self.k_factor)

    def rule(self, state):
        return exact

    def reference(self, state, xq, coarse=None):
        codes, ids, off = state["lists"]
        ox = self.oracle(state)
        cd, keys = ox.coarse_search(xq, self.nprobe, canonical=True)
        _D, sl = ox.search_preassigned(xq, keys, cd, int(F32(self.k) * F32(self.k_factor)), store_pairs=True, canonical=True)
        return refine_ref.refine_ref(xq, sl, self.k, state["coarse"], state["pq"], codes, state["rpq"], state["rcodes"], ids, off)


# ----------------------------------------------------------------------------------------------------------------------
# GpuVLQ: the stored per-code constants of line16c, half(term 2), the graph
# ----------------------------------------------------------------------------------------------------------------------
class VlqKind(Kind):
    """shape "small": make_vlq's M 8 x 6 bit; "m16": d 96, M 16 x 8 bit, nlist 64, 6 000 vectors (line16 / line16r / line16c)"""
    SHAPES = {"small": dict(seed=21, d=32, nlist=24, M=8, nbits=6, nedge=6, nlambda=16, nb=3000),
              "m16": dict(seed=22, d=96, nlist=64, M=16, nbits=8, nedge=8, nlambda=64, nb=6000)}
    nprobe, w1 = 8, 32

    def __init__(self, shape, row_mode, fp16):
        self.shape, self.row_mode, self.fp16 = shape, row_mode, fp16
        self.p = self.SHAPES[shape]
        self.name = "vlq-%s-rows%d%s" % (shape, row_mode, "-fp16" if fp16 else "")

    def world(self):
        return vlq_world(self.shape)

    def walk(self):
        w = self.world()
        v = w["v"]
        wk = Walk(coarse=v.coarse, graph=(v.edge_info, v.edge_dist), lam=v.lambda_info, pq=v.pq_centroids,
                  lines=(v.codes, v.lambdas, v.ids, v.line_off), row_mode=self.row_mode, scan_parts=0)
        wk.step("set_lambda_codebook(B)", lambda g: g.set_lambda_codebook(w["lamB"]), lam=w["lamB"])
        wk.step("set_pq_centroids(B)", lambda g: g.set_pq_centroids(w["pqB"]), pq=w["pqB"])
        wk.to_torch()
        wk.step("set_graph(B's graph)", lambda g: g.set_graph(*w["graphB"]), graph=w["graphB"])
        wk.steps.append(Step("search after set_coarse_centroids(B), before a new graph", lambda g: g.search(w["xq"], self.nprobe, self.w1, self.k),
                             wk.state, refuse=ERR_STATE, pre=[lambda g: g.set_coarse_centroids(w["cB"])]))
        wk.step("build_graph over B's centroids", lambda g: g.build_graph(), old=dict(coarse=v.coarse), coarse=w["cB"])
        wk.step("set_scan_parts(3)", lambda g: g.set_scan_parts(3), scan_parts=3)
        wk.to_own()
        if self.p["M"] != 16:
            wk.steps.append(Step("set_float16_tables(True) at M = 8", lambda g: g.set_float16_tables(True), wk.state, refuse=ERR_UNSUPPORTED))
        # the fresh handle of every state stays in the kind's row mode: the toggles are compared across row modes, too
        for mode in [m for m in (1, 2, 3) if m != self.row_mode] + [self.row_mode]:
            wk.step("set_row_mode(%d)" % mode, lambda g, mode=mode: g.set_row_mode(mode), row_mode=mode)
        wk.step("set_lambda_codebook(A) in the kind's row mode again", lambda g: g.set_lambda_codebook(v.lambda_info), lam=v.lambda_info)
        return wk.steps

    def recipe(self, state):
        p = self.p
        calls = [("GpuVLQ", lambda *a: vlq().GpuVLQ(*a), (p["d"], p["nlist"], p["M"], p["nbits"], p["nedge"], p["nlambda"])),
                 call("set_coarse_centroids") + ((state["coarse"],),), call("set_graph") + (state["graph"],),
                 call("set_lambda_codebook") + ((state["lam"],),), call("set_pq_centroids") + ((state["pq"],),),
                 call("set_row_mode") + ((self.row_mode,),)]
        if self.fp16:
            calls.append(call("set_float16_tables") + ((True,),))
        calls.append(call("set_lists") + (state["lines"],))
        return calls

    def read(self, g):
        p = self.p
        got = [g.get_list(i) for i in range(p["nlist"] * p["nedge"])]
        lens = np.array([len(x[2]) for x in got], np.int64)
        return tuple(np.concatenate([x[j] for x in got]) for j in range(3)) + (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),)

    def with_stored(self, state, stored):
        return dict(state, lines=stored)

    def search(self, g, state, xq):
        return g.search(xq, self.nprobe, self.w1, self.k)

    def reference(self, state, xq, coarse=None):
        p = self.p
        o = OracleVLQ(p["d"], p["nlist"], p["M"], p["nbits"], p["nedge"], p["nlambda"], state["coarse"], state["pq"], state["graph"][0],
                      state["graph"][1], state["lam"])
        o.codes, o.lambdas, o.ids, o.line_off = (np.ascontiguousarray(a) for a in state["lines"])
        return o.search(xq, self.nprobe, self.w1, self.k, fp16=self.fp16)


@functools.lru_cache(maxsize=None)
def vlq_world(shape):
    from test_vlq_oracle import make_vlq
    p = VlqKind.SHAPES[shape]
    v, _xb, xq = make_vlq(**p)
    rng = np.random.default_rng(p["seed"])
    cB = (v.coarse + 0.15 * rng.standard_normal(v.coarse.shape)).astype(F32)
    vB = OracleVLQ(p["d"], p["nlist"], p["M"], p["nbits"], p["nedge"], p["nlambda"], cB)
    return dict(v=v, xq=xq, cB=cB, graphB=(vB.edge_info, vB.edge_dist), lamB=(v.lambda_info * F32(0.8) + F32(0.15)).astype(F32),
                pqB=(v.pq_centroids * F32(1.25) + F32(0.05)).astype(F32))


# ----------------------------------------------------------------------------------------------------------------------
# GpuRefineFlat over GpuPQ and over GpuIVFSQ: reset() and a second add
# ----------------------------------------------------------------------------------------------------------------------
class RefineFlatKind(Kind):
    """state: xb (the refine store) and the base's stored codes / lists; the base's trained state never changes"""
    k, k_factor = 5, 3.0

    def __init__(self, base):
        self.base = base
        self.bk = PqKind("l2") if base == "pq" else IvfSqKind(32, "8bit")
        self.name = "refineflat-over-%s" % base
        self.kb = refineflat_ref.k_base(self.k, self.k_factor)

    def world(self):
        return self.bk.world()

    def stored_of(self, x, base=None):
        w = self.world()
        if self.base == "pq":
            c = pq_ref.compute_codes(x, w["cA"])
            return c if base is None else np.concatenate([base, c])
        empty = empty_lists(self.bk.nlist, ivfsq_ref.code_size(self.bk.d, self.bk.qt), np.uint8)
        return self.bk.add(empty if base is None else base, w["cA"], w["tA"], x)

    def walk(self):
        w = self.world()
        xa, xo, extra = w["xa"], w["xo"], (w["xa"][:400] + F32(0.01)).astype(F32)
        wk = Walk(xb=xa, stored=self.stored_of(xa))
        wk.to_torch()
        wk.step("reset() + add of other vectors", lambda r: (r.reset(), r.add(xo)), xb=xo, stored=self.stored_of(xo))
        wk.to_own()
        wk.step("add again", lambda r: r.add(extra), xb=np.concatenate([xo, extra]), stored=self.stored_of(extra, wk.state["stored"]))
        return wk.steps

    def base_state(self, state):
        w = self.world()
        if self.base == "pq":
            return dict(cent=w["cA"], codes=state["stored"], search_type=pq_ref.ST_PQ, ht=self.bk.nbits * self.bk.M + 1)
        return dict(coarse=w["cA"], trained=w["tA"], lists=state["stored"])

    def recipe(self, state):
        return self.bk.recipe(self.base_state(state)) + [call("set_store") + ((state["xb"],),)]

    def fresh(self, state):
        r = vlq().GpuRefineFlat(self.bk.fresh(self.base_state(state)))
        r.k_factor = self.k_factor
        r.set_store(state["xb"])
        return r

    def start(self, state):
        calls = self.bk.recipe(self.base_state(state))[:-1]          # the trained base, nothing stored
        base = calls[0][1](*calls[0][2])
        for _name, fn, args in calls[1:]:
            fn(base, *args)
        r = vlq().GpuRefineFlat(base)
        r.k_factor = self.k_factor
        r.add(state["xb"])
        return r

    def read(self, r):
        return r.store.reconstruct_n(), self.bk.read(r.base)

    def with_stored(self, state, stored):
        return dict(state, xb=stored[0], stored=stored[1])

    def search(self, r, state, xq):
        return r.search(xq, self.k, self.bk.nprobe) if self.base != "pq" else r.search(xq, self.k)

    def coarse(self, r, state, xq):
        """the device's own first stage, as tests/test_gpu_refine_flat.py's test_whole_search feeds the restatement"""
        return r.base.search(xq, self.kb) if self.base == "pq" else r.base.search(xq, self.bk.nprobe, self.kb)

    def first_stage(self, state, xq):
        bk, self.bk.k = self.bk.k, self.kb
        try:
            return self.bk.reference(self.base_state(state), xq)
        finally:
            self.bk.k = bk

    def reference(self, state, xq, coarse=None):
        bD, bI = self.first_stage(state, xq) if coarse is None else coarse
        return refineflat_ref.refine(state["xb"], xq, bD, bI, self.k, "l2")

    def close(self, r):
        r.base.close()
        r.store.close()


KINDS = ([FlatKind(d, m, nq) for d in (20, 33) for m in ("l2", "ip") for nq in (25, 3)]
         + [LshKind(), SqKind(32, "8bit"), SqKind(12, "4bit"), PqKind("l2"), PqKind("ip"), IvfFlatKind("l2"), IvfFlatKind("ip"),
            IvfSqKind(32, "8bit"), IvfSqKind(12, "4bit"), IvfPqGenericKind(), IvfPq16Kind(), IvfPqImiKind(), IvfPqScreenKind(), IvfPqrKind()]
         + [VlqKind("small", r, False) for r in (1, 2, 3)] + [VlqKind("m16", r, f) for r in (1, 2, 3) for f in (False, True)]
         + [RefineFlatKind("pq"), RefineFlatKind("ivfsq")])


@functools.lru_cache(maxsize=None)
def walk_of(name):
    kind = next(k for k in KINDS if k.name == name)
    return kind, kind.walk()
