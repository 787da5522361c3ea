"""The table, the calls and the decoys of tests/test_gpu_async_streams.py: stream-ordered use of every handle that has a
set_stream -- device inputs that arrive LATE on a non-blocking stream, results consumed on that stream.
tests/test_async_cases.py holds this module to its promises without a GPU.

TEST INFRASTRUCTURE ONLY.  Nothing here touches a device: a Call is host arrays plus a function that a GPU test applies to a live
handle, with host arrays (the warm, synchronous form) or with device tensors (the measured form).

  TABLE    per handle kind (the prefix of its vlq_<kind>_set_stream) the entry points the GPU file exercises, classified from the
           WORDS of the headers: class B = the entry point's comment says "Synchronises the stream" (complete on return), class A =
           device-resident buffers and no such sentence (asynchronous on the handle's stream).
  Call     what / entry / klass; issue(g, b) makes the library call(s) on the buffers b[name]; ins: the real inputs; decoys: a
           DIFFERENT BUT VALID input of the same shapes (other rows of the query set, other valid list ids, labels 0, shortlist
           entries -1, codes of other vectors): a library that reads an input early computes a wrong answer, never an address out
           of range; outs: name -> (shape, dtype); inout: inputs the call updates in place.
  AKind    one handle in one mode over a world of tests/restate_cases.py: fresh(), the main search Call, the further Calls.
"""
import os
import re

import numpy as np

import restate_cases as rc
from restate_cases import F32

I64 = np.int64
U8 = np.uint8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("include/vlq_ivfpq.h", "include/vlq_line.h")
SYNC_SENTENCE = re.compile(r"synchronises[\s*]+the[\s*]+stream", re.I)          # (a comment's line break brings a " * " with it)

# ----------------------------------------------------------------------------------------------------------------------
# the contract, as the GPU file reads it
# ----------------------------------------------------------------------------------------------------------------------
TABLE = {
    "ivfpq": dict(handle="GpuIVFPQ",
                  A=("vlq_ivfpq_search", "vlq_ivfpq_search_preassigned", "vlq_ivfpq_coarse_search", "vlq_ivfpq_search_refined",
                     "vlq_ivfpq_refine", "vlq_ivfpq_encode"),
                  B=("vlq_ivfpq_add", "vlq_ivfpq_stats", "vlq_ivfpq_polysemous_stats", "vlq_ivfpq_last_scan_info")),
    "ivfflat": dict(handle="GpuIVFFlat",
                    A=("vlq_ivfflat_search", "vlq_ivfflat_search_preassigned", "vlq_ivfflat_coarse_search"),
                    B=("vlq_ivfflat_range_search", "vlq_ivfflat_add", "vlq_ivfflat_stats", "vlq_ivfflat_last_scan_info")),
    "ivfsq": dict(handle="GpuIVFSQ",
                  A=("vlq_ivfsq_search", "vlq_ivfsq_search_preassigned", "vlq_ivfsq_coarse_search"),
                  B=("vlq_ivfsq_add", "vlq_ivfsq_encode", "vlq_ivfsq_last_scan_info")),
    "pq": dict(handle="GpuPQ", A=("vlq_pq_search",), B=("vlq_pq_add", "vlq_pq_encode", "vlq_pq_stats", "vlq_pq_last_scan_info")),
    "sq": dict(handle="GpuSQ", A=("vlq_sq_search",), B=("vlq_sq_add", "vlq_sq_encode", "vlq_sq_last_scan_info")),
    "flat": dict(handle="GpuFlat", A=("vlq_flat_search",),
                 B=("vlq_flat_refine", "vlq_flat_compute_distance_subset", "vlq_flat_add", "vlq_flat_last_scan_info")),
    "lsh": dict(handle="GpuLSH", A=("vlq_lsh_search", "vlq_lsh_search_codes"), B=("vlq_lsh_add", "vlq_lsh_encode", "vlq_lsh_last_scan_info")),
    "line": dict(handle="GpuVLQ", A=("vlq_line_search",), B=("vlq_line_stats",)),
}
# GpuRefineFlat has no C handle: it chains a base search (class A) and vlq_flat_refine (class B) on one stream, so its search is
# complete on return
PYTHON_ONLY = {"refineflat": dict(handle="GpuRefineFlat", B=("GpuRefineFlat.search",))}


def header_text():
    return "\n".join(open(os.path.join(ROOT, p)).read() for p in HEADERS)


def set_stream_kinds(text=None):
    """the prefixes <kind> of every vlq_<kind>_set_stream the headers declare"""
    return sorted(set(re.findall(r"\bint\s+vlq_(\w+?)_set_stream\s*\(", header_text() if text is None else text)))


def entry_comments(text=None):
    """{function name: the comment that stands in front of its declaration}; declarations that follow one another without a
    comment in between share the one in front of the first"""
    text = header_text() if text is None else text
    out, last, pos = {}, "", 0
    for m in re.finditer(r"/\*(.*?)\*/|\b(?:int|int64_t|void|const char\*)\s+(vlq_\w+)\s*\(", text, re.S):
        if m.group(2) is None:
            # a comment counts for the declarations behind it only if nothing but declarations stands in between
            last, pos = m.group(1), m.end()
        else:
            between = text[pos:m.start()]
            if re.search(r"typedef|#|\{|\}", between):
                last = ""
            out[m.group(2)] = last
            pos = text.find(";", m.end()) + 1
    return out


def says_synchronises(comment):
    return SYNC_SENTENCE.search(comment) is not None


# ----------------------------------------------------------------------------------------------------------------------
# decoys
# ----------------------------------------------------------------------------------------------------------------------
def other_rows(a):
    """other rows of the same set: every row moves down by one"""
    return np.ascontiguousarray(np.roll(a, 1, axis=0))


def other_keys(keys, nlist):
    """valid list ids other than the real ones (a skipped probe, -1, stays skipped)"""
    k = np.asarray(keys, I64)
    return np.where(k < 0, k, (k + 1) % nlist).astype(I64)


def zero_labels(labels):
    return np.zeros_like(labels)


def skipped(shortlist):
    return np.full_like(shortlist, -1)


class Call:
    def __init__(self, what, entry, klass, issue, ins, decoys, outs=(), inout=(), limits=None):
        self.what, self.entry, self.klass, self.issue = what, entry, klass, issue
        self.ins = {k: np.ascontiguousarray(v) for k, v in ins.items()}
        self.decoys = {k: np.ascontiguousarray(v) for k, v in decoys.items()}
        self.outs, self.inout = dict(outs), tuple(inout)
        self.limits = dict(limits or {})         # name -> (lo, hi): the values of that input lie in [lo, hi) (-1 = skip allowed)
        assert self.ins.keys() == self.decoys.keys()

    def __repr__(self):
        return "Call(%s)" % self.what

    def result_names(self):
        return self.inout + tuple(self.outs)


def check_decoys(call):
    """every decoy is a valid input of the call and not the real one"""
    for name, real in call.ins.items():
        d = call.decoys[name]
        assert d.shape == real.shape and d.dtype == real.dtype, (call.what, name)
        assert not np.array_equal(d, real), "%s: the decoy of %s is the real input" % (call.what, name)
        if d.dtype.kind == "f":
            assert np.isfinite(d).all(), (call.what, name)
        if name in call.limits:
            lo, hi = call.limits[name]
            for a in (real, d):
                live = a[a != -1]
                assert ((live >= lo) & (live < hi)).all(), "%s: %s outside [%d, %d)" % (call.what, name, lo, hi)
        else:
            assert d.dtype.kind != "i", "%s: integer input %s without stated limits" % (call.what, name)


def rows(n, k):
    return dict(D=((n, k), F32), I=((n, k), I64))


# ----------------------------------------------------------------------------------------------------------------------
# kinds
# ----------------------------------------------------------------------------------------------------------------------
def raw_ivfpq_encode(g, x, assign, codes):
    """vlq_ivfpq_encode with the caller's outputs (GpuIVFPQ.encode always hands over host arrays)"""
    from vector_line_quantization_amd._lib import check, lib
    from vector_line_quantization_amd.index import _out_ptr, _ptr
    import ctypes as C
    px, _a = _ptr(x, F32)
    check(lib().vlq_ivfpq_encode(g._h, C.c_int64(x.shape[0]), px, _out_ptr(assign, I64)[0], _out_ptr(codes, U8)[0]))


class AKind:
    """one handle in one mode.  prefix: its kind in TABLE; rk: the kind of tests/restate_cases.py whose world it uses."""
    sync = "stats"              # the introspection call documented to synchronise the stream (and to raise a pending error)

    def __init__(self, name, prefix, rk, state=None, nq=None, **over):
        self.name, self.prefix, self.rk, self._state, self.nq, self.over = name, prefix, rk, state, nq, over

    def __repr__(self):
        return self.name

    def state(self):
        if self._state is None:
            self._state = dict(rc.walk_of(self.rk.name)[1][0].state, **self.over)
        return self._state

    def fresh(self):
        return self.rk.fresh(self.state())

    def close(self, g):
        self.rk.close(g)

    def xq(self):
        x = self.rk.queries(self.state())
        return x if self.nq is None else x[:self.nq]

    @property
    def k(self):
        return self.rk.k_of(self.state()) if hasattr(self.rk, "k_of") else self.rk.k

    @property
    def search_entry(self):
        return TABLE[self.prefix]["A"][0]

    search_class = "A"

    def search_into(self, g, x, D, I):
        rk = self.rk
        if isinstance(rk, rc.IvfPqrKind):
            return g.search_refined(x, rk.nprobe, self.k, rk.k_factor, D, I)
        if isinstance(rk, rc.VlqKind):
            return g.search(x, rk.nprobe, rk.w1, self.k, D, I)
        if isinstance(rk, rc.RefineFlatKind):
            return g.search(x, self.k, rk.bk.nprobe if rk.base != "pq" else None, D, I)
        if hasattr(rk, "nprobe"):
            return g.search(x, rk.nprobe, self.k, D, I)
        return g.search(x, self.k, D, I)

    def search_call(self, x=None, tag="search"):
        x = self.xq() if x is None else x
        return Call("%s: %s" % (self.name, tag), self.search_entry, self.search_class,
                    lambda g, b: self.search_into(g, b["x"], b["D"], b["I"]), dict(x=x), dict(x=other_rows(x)), rows(x.shape[0], self.k))

    def two_searches(self):
        """back to back: two searches with different queries into different outputs, the second no larger than the first"""
        x1 = self.xq()
        x2 = np.ascontiguousarray(x1[::-1][:max(2, x1.shape[0] - 3)])

        def issue(g, b):
            self.search_into(g, b["x"], b["D"], b["I"])
            self.search_into(g, b["x2"], b["D2"], b["I2"])
        k = self.k
        return Call("%s: two searches back to back" % self.name, self.search_entry, self.search_class, issue, dict(x=x1, x2=x2),
                    dict(x=other_rows(x1), x2=other_rows(x2)),
                    dict(D=((x1.shape[0], k), F32), I=((x1.shape[0], k), I64), D2=((x2.shape[0], k), F32), I2=((x2.shape[0], k), I64)))

    def reference(self, g):
        """(rule, rows) of the main search on the CPU: what test_gpu_restate.py compares a live handle with"""
        st, x = self.state(), self.xq()
        return self.rk.rule(st), self.rk.reference(st, x, self.rk.coarse(g, st, x))

    def calls(self):
        """the further entry points of the handle, each with late inputs"""
        return []

    def host_keys(self):
        rk, st = self.rk, self.state()
        metric = getattr(rk, "metric", None) or st.get("metric", "l2")
        cd, keys = rc.host_coarse(st["coarse"], self.xq(), rk.nprobe, metric)
        return np.ascontiguousarray(cd, F32), np.ascontiguousarray(keys, I64)


class IvfAKind(AKind):
    """the three IVF handles: coarse_search and search_preassigned beside search, and the chain of the two on the device"""

    def preassigned(self, g, b, D, I):
        if self.prefix == "ivfpq":
            return g.search_preassigned(b["x"], b["keys"], b["cdis"], self.k, False, D, I)
        if self.prefix == "ivfsq":
            return g.search_preassigned(b["x"], b["keys"], None, self.k, D, I)
        return g.search_preassigned(b["x"], b["keys"], self.k, D, I)

    def preassigned_call(self, keys=None, tag="search_preassigned"):
        x, rk = self.xq(), self.rk
        cd, real = self.host_keys()
        keys = real if keys is None else keys
        ins, dec = dict(x=x, keys=keys), dict(x=other_rows(x), keys=other_keys(real, rk.nlist))
        if self.prefix == "ivfpq":
            ins["cdis"], dec["cdis"] = cd, other_rows(cd)
        return Call("%s: %s" % (self.name, tag), "vlq_%s_search_preassigned" % self.prefix, "A",
                    lambda g, b: self.preassigned(g, b, b["D"], b["I"]), ins, dec, rows(x.shape[0], self.k), limits=dict(keys=(0, rk.nlist)))

    def bad_key_calls(self):
        """(the call with one key >= nlist, the same call with that key -1).  IVFSQ ends a query's walk at a key < 0 and skips a
        key >= nlist: the key stands in the last probe slot there, where the two agree."""
        cd, keys = self.host_keys()
        q, p = 5, (keys.shape[1] - 1 if self.prefix == "ivfsq" else 1)
        bad, skip = keys.copy(), keys.copy()
        bad[q, p], skip[q, p] = self.rk.nlist, -1
        c = self.preassigned_call(bad, "search_preassigned with a key >= nlist")
        c.limits = dict(keys=(0, self.rk.nlist + 1))
        return c, self.preassigned_call(skip, "search_preassigned with that key -1")

    def calls(self):
        x, rk, k = self.xq(), self.rk, self.k
        n, P = x.shape[0], rk.nprobe
        probes = dict(cdis=((n, P), F32), keys=((n, P), I64))
        out = [Call("%s: coarse_search" % self.name, "vlq_%s_coarse_search" % self.prefix, "A",
                    lambda g, b: g.coarse_search(b["x"], P, b["cdis"], b["keys"]), dict(x=x), dict(x=other_rows(x)), probes),
               self.preassigned_call()]

        def chain(g, b):
            g.coarse_search(b["x"], P, b["cdis"], b["keys"])
            self.preassigned(g, b, b["D"], b["I"])
        out.append(Call("%s: coarse_search, then search_preassigned on its outputs" % self.name, "vlq_%s_search_preassigned" % self.prefix, "A",
                        chain, dict(x=x), dict(x=other_rows(x)), dict(probes, **rows(n, k))))
        return out


class IvfPqAKind(IvfAKind):
    def calls(self):
        out = IvfAKind.calls(self)
        x, M = self.xq(), self.rk.M
        out.append(Call("%s: encode into device outputs" % self.name, "vlq_ivfpq_encode", "A",
                        lambda g, b: raw_ivfpq_encode(g, b["x"], b["assign"], b["codes"]), dict(x=x), dict(x=other_rows(x)),
                        dict(assign=((x.shape[0],), I64), codes=((x.shape[0], M), U8))))
        return out


class IvfPqrAKind(AKind):
    search_entry = "vlq_ivfpq_search_refined"

    def calls(self):
        rk, st, x, k = self.rk, self.state(), self.xq(), self.k
        ox = rk.oracle(st)
        cd, keys = ox.coarse_search(x, rk.nprobe, canonical=True)
        kc = int(F32(k) * F32(rk.k_factor))
        _D, sl = ox.search_preassigned(x, keys, cd, kc, store_pairs=True, canonical=True)
        sl = np.ascontiguousarray(sl, I64)
        return [Call("%s: refine" % self.name, "vlq_ivfpq_refine", "A", lambda g, b: g.refine(b["x"], b["shortlist"], k, b["D"], b["I"]),
                     dict(x=x, shortlist=sl), dict(x=other_rows(x), shortlist=skipped(sl)), rows(x.shape[0], k),
                     limits=dict(shortlist=(0, int(rk.nlist) << 32)))]


class ImiWideKind(rc.IvfPqImiKind):
    """nlist 65 536 = 2 x 8 bits, d 32, batches of 2 048 queries: the smallest multi-index quantizer whose two halves go through
    the float16 screen (256 sub-centroids of 16 dimensions, 2 048 rows: include/vlq_ivfpq.h), the second half on the handle's
    auxiliary stream, joined by events before the cells are enumerated (csrc/coarse_stage.hip)"""
    name = "ivfpq-imi-two-streams"
    d, nlist, M, nbits, nprobe, imi_nbits = 32, 65536, 8, 8, 8, 8

    def world(self):
        return imi_wide_world()

    def first_state(self):
        w = self.world()
        st = dict(self.DEFAULTS, coarse=None, imi=w["imi"], pq=w["pq"], nq=2048)
        return dict(st, lists=w["lists"](self, st), history=("A",), stream="own")


_imi_wide = {}


def imi_wide_world():
    if not _imi_wide:
        rng = np.random.default_rng(6543)
        d, h = 32, 16
        centres = rng.random((40, d)).astype(F32)
        xa = rc.clustered(rng, centres, 3000, 0.08)
        imi = np.stack([xa[rng.choice(3000, 256, replace=False), :h], xa[rng.choice(3000, 256, replace=False), h:]]).astype(F32)
        _imi_wide.update(xa=xa, xq=rc.clustered(rng, centres, 2048, 0.08), imi=imi, pq=(0.05 * rng.standard_normal((8, 256, 4))).astype(F32))
        cache = {}
        _imi_wide["lists"] = lambda kind, st: cache.setdefault(0, kind.encode_lists(st, xa))
    return _imi_wide


class ImiAKind(IvfAKind):
    def state(self):
        if self._state is None:
            self._state = self.rk.first_state()
        return self._state

    def host_keys(self):
        cd, keys = self.rk.oracle(self.state()).coarse_search(self.xq(), self.rk.nprobe, canonical=True)
        return np.ascontiguousarray(cd, F32), np.ascontiguousarray(keys, I64)

    def calls(self):
        return IvfAKind.calls(self)[:1]          # coarse_search: the two-stream stage alone


class IvfFlatAKind(IvfAKind):
    def calls(self):
        out = IvfAKind.calls(self)
        rk, x = self.rk, self.xq()[:40]
        radius = rk.world()["radius"]
        out.append(Call("%s: range_search" % self.name, "vlq_ivfflat_range_search", "B", lambda g, b: g.range_search(b["x"], rk.nprobe, radius),
                        dict(x=x), dict(x=other_rows(x))))
        return out


class IvfSqAKind(IvfAKind):
    sync = "last_scan_info"


class FlatAKind(AKind):
    sync = "last_scan_info"

    def calls(self):
        import knn_ref
        rk, st, x = self.rk, self.state(), self.xq()
        k, kb = self.k, 2 * self.k
        bD, bI = knn_ref.search(x, st["xb"], kb, rk.metric)
        bD, bI = np.ascontiguousarray(bD, F32), np.ascontiguousarray(bI, I64)
        holes = bI.copy()
        holes[:, 1::3] = -1          # skipped entries keep the distance they carry
        nb = (0, st["xb"].shape[0])
        return [Call("%s: refine" % self.name, "vlq_flat_refine", "B", lambda g, b: g.refine(b["x"], b["base_D"], b["base_I"], k, b["D"], b["I"]),
                     dict(x=x, base_D=bD, base_I=bI), dict(x=other_rows(x), base_D=other_rows(bD), base_I=zero_labels(bI)), rows(x.shape[0], k),
                     limits=dict(base_I=nb)),
                Call("%s: refine in place" % self.name, "vlq_flat_refine", "B",
                     lambda g, b: g.refine(b["x"], b["base_D"], b["base_I"], kb, b["base_D"], b["base_I"]),
                     dict(x=x, base_D=bD, base_I=bI), dict(x=other_rows(x), base_D=other_rows(bD), base_I=zero_labels(bI)),
                     inout=("base_D", "base_I"), limits=dict(base_I=nb)),
                Call("%s: compute_distance_subset" % self.name, "vlq_flat_compute_distance_subset", "B",
                     lambda g, b: g.compute_distance_subset(b["x"], b["labels"], b["distances"]),
                     dict(x=x, labels=holes, distances=bD), dict(x=other_rows(x), labels=zero_labels(holes), distances=other_rows(bD)),
                     inout=("distances",), limits=dict(labels=nb))]


class LshAKind(AKind):
    sync = "last_scan_info"

    def calls(self):
        import lsh_ref
        rk, st, x, k = self.rk, self.state(), self.xq(), self.k
        qc = np.ascontiguousarray(lsh_ref.encode(x, rk.nbits, st["A"], st["b"], st["thr"]), U8)
        return [Call("%s: search_codes" % self.name, "vlq_lsh_search_codes", "A", lambda g, b: g.search_codes(b["qcodes"], k, b["D"], b["I"]),
                     dict(qcodes=qc), dict(qcodes=other_rows(qc)), rows(x.shape[0], k))]


class SqAKind(AKind):
    sync = "last_scan_info"


class RefineFlatAKind(AKind):
    search_class = "B"          # ends in vlq_flat_refine, which synchronises the stream: the rows are complete on return
    search_entry = "GpuRefineFlat.search"
    sync = None


GENERIC, PQR, IMI = rc.IvfPqGenericKind(), rc.IvfPqrKind(), ImiWideKind()
KINDS = [
    IvfPqAKind("ivfpq-l2", "ivfpq", GENERIC),
    IvfPqAKind("ivfpq-ip", "ivfpq", GENERIC, metric="ip"),
    IvfPqAKind("ivfpq-polysemous", "ivfpq", GENERIC, ht=GENERIC.HT),
    ImiAKind("ivfpq-imi", "ivfpq", IMI),
    IvfPqrAKind("ivfpqr", "ivfpq", PQR),
    IvfFlatAKind("ivfflat-l2", "ivfflat", rc.IvfFlatKind("l2")),
    IvfSqAKind("ivfsq-8bit", "ivfsq", rc.IvfSqKind(32, "8bit")),
    AKind("pq-adc", "pq", rc.PqKind("l2")),
    AKind("pq-polysemous", "pq", rc.PqKind("l2"), ht=rc.PqKind.HT, search_type=4),
    SqAKind("sq-8bit", "sq", rc.SqKind(32, "8bit")),
    FlatAKind("flat-l2-gemm", "flat", rc.FlatKind(20, "l2", 25)),
    FlatAKind("flat-ip-direct", "flat", rc.FlatKind(20, "ip", 3)),
    LshAKind("lsh", "lsh", rc.LshKind()),
    RefineFlatAKind("refineflat-over-ivfsq", "refineflat", rc.RefineFlatKind("ivfsq")),
    RefineFlatAKind("refineflat-over-pq", "refineflat", rc.RefineFlatKind("pq")),
    AKind("vlq-small", "line", rc.VlqKind("small", 1, False)),
]
BY_NAME = {a.name: a for a in KINDS}
COUNTED = ("ivfpq-l2", "ivfpq-polysemous", "pq-adc", "pq-polysemous")          # stats(reset) / search / stats
BAD_KEYS = ("ivfpq-l2", "ivfflat-l2", "ivfsq-8bit")
ADDS = ("ivfpq-l2", "ivfflat-l2", "ivfsq-8bit", "pq-adc", "sq-8bit", "flat-l2-gemm", "lsh")
ENCODES = ("ivfsq-8bit", "pq-adc", "sq-8bit", "lsh")


def all_calls(a):
    out = [a.search_call(), a.two_searches()] + a.calls()
    if isinstance(a, IvfAKind) and a.name in BAD_KEYS:
        out += list(a.bad_key_calls())
    return out
