"""The small worlds, expectations and comparison helpers of the write-path tests (tests/test_gpu_write_pages.py,
tests/test_gpu_encode_shapes.py); tests/test_write_cases.py holds them to their promises without a GPU.

TEST INFRASTRUCTURE ONLY.  Nothing here touches a device: a world is host arrays plus the CPU reference of the operation.

  whole_call      every row of every output of ONE call of more than a 32 768-row page, float32 as bits
  expected_lists  the inverted lists a stable append produces (Lists), same_lists compares two of them
  page worlds     32 768 + r rows (r up to R_MAX) around 256 centroids.  The rows at PAGE .. PAGE + 7 are aimed at eight different
                  lists and no row of the last page is aimed at the list of the row one page before it, so a row written one
                  page off, or a page's results laid over another's, cannot pass.  Where the C++ oracle is the reference the
                  rows are all distinct and the oracle sees the whole batch; where a numpy restatement works per row it is
                  evaluated on a pool of 512 distinct rows, the batch is pool[idx] and the expectation ref[idx] (pool_rows).
  integer worlds  inner-product assignment: small-integer centroids and rows, so every product and every partial sum is an
                  integer below 2^24 -- exact in float32 in any summation order -- and ip_ref.coarse_search is an independent
                  reference whatever order the device adds in; equal inner products are frequent and go to the lower list.
"""
import functools
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]

import ip_ref  # noqa: E402
import ivfsq_ref  # noqa: E402
import pq_ref  # noqa: E402
from oracle.pyoracle import OracleIndex  # noqa: E402
from refine_ref import pq_decode  # noqa: E402

PAGE = 32768
POOL = 512
R_MAX = 2048                  # the longest tail any test asks for
TAILS = (7, 1500)             # below the 20-row dispatch boundary; an unscreened tail behind a screened first page
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


# ----------------------------------------------------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------------------------------------------------
def whole_call(got, want, what=""):
    """Every row of every output array of one call of more than a page equals the reference's: float32 arrays as bits, the
    others as they are.  Names the first differing row, the page it lies in and its row within that page."""
    assert len(got) == len(want), "%s: %d outputs, expected %d" % (what, len(got), len(want))
    n = want[0].shape[0]
    assert n > PAGE, "%s: not a call of more than one page" % what
    for j, (g, w) in enumerate(zip(got, want)):
        g = host(g)
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: output %d is %s %s, expected %s %s" % (what, j, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype == np.float32:
            g, w = bits(g), bits(w)
        bad = np.nonzero((g.reshape(n, -1) != w.reshape(n, -1)).any(axis=1))[0]
        assert bad.size == 0, "%s: output %d differs in %d of %d rows, first row %d (page %d, row %d of it)" % (
            what, j, bad.size, n, bad[0], bad[0] // PAGE, bad[0] % PAGE)


class Lists:
    """Inverted lists on the host: parts[i] is a tuple of arrays (the rows of list i and, where the kind has them, their side
    bytes), ids[i] the ids, all in stored order."""

    def __init__(self, parts, ids):
        self.parts, self.ids = parts, ids

    @property
    def nlist(self):
        return len(self.ids)

    @property
    def lens(self):
        return np.array([len(i) for i in self.ids], np.int64)

    @property
    def ntotal(self):
        return int(self.lens.sum())

    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)

    def flat(self):
        """(the parts, each concatenated over the lists; the ids): what set_lists takes"""
        nparts = len(self.parts[0])
        return tuple(np.concatenate([p[j] for p in self.parts]) for j in range(nparts)), np.concatenate(self.ids)


def expected_lists(assign, rows, ids, nlist, base=None):
    """The lists a stable append of a batch produces: per list the rows with that assignment in input order, rows assigned
    outside 0 .. nlist-1 dropped, everything behind the rows of `base` (a Lists) when there is one.  rows: one array [n][..]
    or a tuple of them (codes and side bytes)."""
    rows = rows if isinstance(rows, tuple) else (rows,)
    assign = np.asarray(assign).astype(np.int64)
    ids = np.asarray(ids, np.int64)
    assert all(len(r) == len(assign) for r in rows) and len(ids) == len(assign)
    keep = np.nonzero((assign >= 0) & (assign < nlist))[0]
    order = keep[np.argsort(assign[keep], kind="stable")]
    cuts = np.cumsum(np.bincount(assign[keep], minlength=nlist))[:-1]
    split = [np.split(np.ascontiguousarray(r[order]), cuts) for r in rows]
    sid = np.split(ids[order], cuts)
    parts, out_ids = [], []
    for i in range(nlist):
        p = tuple(s[i] for s in split)
        if base is not None:
            p = tuple(np.concatenate([b, q]) for b, q in zip(base.parts[i], p))
        parts.append(p)
        out_ids.append(sid[i] if base is None else np.concatenate([base.ids[i], sid[i]]))
    return Lists(parts, out_ids)


def read_lists(nlist, get):
    """Lists from a getter: get(i) -> (part, ..., ids) of list i (an index's get_list)"""
    got = [get(i) for i in range(nlist)]
    return Lists([tuple(g[:-1]) for g in got], [g[-1] for g in got])


def same_lists(got, want, what=""):
    """every list of `got` holds the rows, side bytes and ids of `want`, in its order; names the first differing list and row"""
    assert got.nlist == want.nlist, "%s: %d lists, expected %d" % (what, got.nlist, want.nlist)
    for i in range(want.nlist):
        gi, wi = np.asarray(got.ids[i]), want.ids[i]
        assert len(gi) == len(wi), "%s: list %d holds %d rows, expected %d" % (what, i, len(gi), len(wi))
        bad = np.nonzero(gi != wi)[0]
        assert bad.size == 0, "%s: list %d, row %d: id %d, expected %d" % (what, i, bad[0], gi[bad[0]], wi[bad[0]])
        assert len(got.parts[i]) == len(want.parts[i]), "%s: list %d has %d parts" % (what, i, len(got.parts[i]))
        for j, (g, w) in enumerate(zip(got.parts[i], want.parts[i])):
            g = np.asarray(g)
            assert g.dtype == w.dtype and g.shape == w.shape, "%s: list %d part %d is %s %s, expected %s %s" % (what, i, j, g.dtype, g.shape, w.dtype, w.shape)
            if len(wi) == 0:
                continue
            gb = np.ascontiguousarray(g).reshape(len(wi), -1).view(np.uint8)
            wb = np.ascontiguousarray(w).reshape(len(wi), -1).view(np.uint8)
            bad = np.nonzero((gb != wb).any(axis=1))[0]
            assert bad.size == 0, "%s: list %d part %d differs in %d rows, first row %d (id %d)" % (what, i, j, bad.size, bad[0], wi[bad[0]])


# ----------------------------------------------------------------------------------------------------------------------
# batches
# ----------------------------------------------------------------------------------------------------------------------
def pool_rows(seed, n, npool=POOL, labels=None):
    """idx [n] into a pool of distinct rows; no row of the last page repeats the row one page before it -- nor, with the pool's
    labels (the list every pool row goes to) given, a row of the same label"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, npool, n)
    lab = np.arange(npool) if labels is None else np.asarray(labels)
    tail = np.arange(PAGE, n)
    for _ in range(64):
        clash = tail[lab[idx[tail]] == lab[idx[tail - PAGE]]]
        if clash.size == 0:
            break
        idx[clash] = rng.integers(0, npool, clash.size)
    assert (lab[idx[PAGE:]] != lab[idx[:n - PAGE]]).all()
    return idx


def aimed_cells(rng, nlist, n):
    """the cell every row of a batch is generated beside: rows PAGE .. PAGE + 7 at eight different cells, no row of the last
    page at the cell of the row one page before it"""
    cell = rng.integers(0, nlist, n)
    if n <= PAGE:
        return cell
    cell[PAGE:PAGE + 8] = rng.permutation(nlist)[:len(cell[PAGE:PAGE + 8])]
    tail = np.arange(PAGE, n)
    clash = tail[cell[tail] == cell[tail - PAGE]]
    cell[clash - PAGE] = (cell[clash] + 1) % nlist          # (the earlier row moves: the eight different cells stay)
    return cell


def given_ids(seed, n, start=0):
    """ids that are neither sequential nor sorted"""
    return (np.random.default_rng(seed).permutation(n).astype(np.int64) + start) * 3 + 7


def world(**kw):
    return types.SimpleNamespace(**kw)


def l2_world(seed, d, nlist, spread=0.35, n=PAGE + R_MAX, n2=0):
    """distinct float rows beside unit-normal centroids: x [n], a second batch x2 [n2], 64 queries"""
    rng = np.random.default_rng(seed)
    coarse = rng.standard_normal((nlist, d)).astype(F32)

    def beside(cells):
        return (coarse[cells] + spread * rng.standard_normal((len(cells), d))).astype(F32)
    w = world(d=d, nlist=nlist, coarse=coarse, x=beside(aimed_cells(rng, nlist, n)), x2=beside(rng.integers(0, nlist, n2)),
              xq=beside(rng.integers(0, nlist, 64)), rng=rng)
    assert np.unique(w.x, axis=0).shape[0] == n, "the rows of a world the oracle sees whole are all distinct"
    return w


def l2_assign(w, x):
    """the reference's 1-NN over the flat quantizer for a batch of at least 20 rows (knn_L2sqr's GEMM formulation, lower id
    first among equals): the C++ oracle on the whole batch"""
    assert x.shape[0] >= 20
    ox = OracleIndex(w.d, w.nlist, 1, 1, w.coarse, np.zeros((1, 2, w.d), F32), by_residual=False)
    return ox.coarse_search(x, 1, canonical=True)[1][:, 0].copy()


def int_world(seed, d, nlist, npool=POOL):
    """small-integer centroids and a pool of distinct small-integer rows (every inner product is exact in float32)"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(-3, 4, (nlist, d)).astype(F32)
    pool = np.zeros((0, d), F32)
    while pool.shape[0] < npool:
        more = coarse[rng.integers(0, nlist, npool)] + rng.integers(-1, 2, (npool, d))
        pool = np.unique(np.concatenate([pool, more.astype(F32)]), axis=0)
    pool = pool[rng.permutation(pool.shape[0])[:npool]]
    keys, _dis = ip_ref.coarse_search(coarse, pool, 1)
    return world(d=d, nlist=nlist, coarse=coarse, pool=pool, pool_assign=keys[:, 0].copy(), rng=rng)


# ----------------------------------------------------------------------------------------------------------------------
# the page worlds (B)
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ivfpq_l2():
    """IVFPQ, L2, flat quantizer, 16-byte codes: d = 32, nlist = 256 (coarse_argmin_ok and coarse_screen_nn_shape_ok hold)"""
    w = l2_world(101, 32, 256, n2=PAGE + 7)
    w.M, w.nbits = 16, 8
    w.pq = (0.3 * w.rng.standard_normal((w.M, 256, w.d // w.M))).astype(F32)
    w.ids, w.ids2 = given_ids(1, w.x.shape[0]), given_ids(2, w.x2.shape[0], start=w.x.shape[0])
    return w


@functools.lru_cache(maxsize=None)
def ivfpq_matrix():
    """d = 6, nlist = 250, M = 3: fails coarse_argmin_ok (d % 4, nlist % 64) and the screen's shape: distance matrix + select"""
    w = l2_world(102, 6, 250, spread=0.2, n=PAGE + TAILS[-1])
    w.M, w.nbits = 3, 8
    w.pq = (0.2 * w.rng.standard_normal((w.M, 256, w.d // w.M))).astype(F32)
    w.ids = given_ids(3, w.x.shape[0])
    return w


def oracle_of(w, by_residual=True):
    return OracleIndex(w.d, w.nlist, w.M, w.nbits, getattr(w, "coarse", None), w.pq, by_residual=by_residual,
                       use_precomputed_table=1 if by_residual else 0, imi_centroids=getattr(w, "imi", None),
                       imi_nbits=getattr(w, "imi_nbits", 0))


@functools.lru_cache(maxsize=None)
def oracle_encode(name, n=None, by_residual=True, batch="x"):
    """(assign, codes) of the oracle for the whole call of the first n rows (None: all) of a world's batch ("x", or "x2" for the
    second add), canonical order.  name: "ivfpq_l2", "ivfpq_matrix" or "ivfpq_imi"."""
    w = {"ivfpq_l2": ivfpq_l2, "ivfpq_matrix": ivfpq_matrix, "ivfpq_imi": ivfpq_imi}[name]()
    a, c = oracle_of(w, by_residual).encode(getattr(w, batch)[:n], canonical=True)
    a.setflags(write=False)
    c.setflags(write=False)
    return a, c


@functools.lru_cache(maxsize=None)
def ivfpq_imi():
    """IVFPQ over a 2 x 4-bit multi-index quantizer (nlist = 256), d = 16"""
    rng = np.random.default_rng(103)
    d, nb, nlist = 16, 4, 256
    kc = 1 << nb
    imi = rng.standard_normal((2, kc, d // 2)).astype(F32)
    n = PAGE + TAILS[-1]
    cell = aimed_cells(rng, nlist, n)
    centres = np.concatenate([imi[0][cell & (kc - 1)], imi[1][cell >> nb]], axis=1)
    x = (centres + 0.3 * rng.standard_normal((n, d))).astype(F32)
    w = world(d=d, nlist=nlist, M=4, nbits=8, imi=imi, imi_nbits=nb, coarse=None, x=x, ids=given_ids(4, n),
              pq=(0.3 * rng.standard_normal((4, 256, d // 4))).astype(F32))
    return w


@functools.lru_cache(maxsize=None)
def ivfpq_ip():
    """IVFPQ under inner product, integer data, pooled: assignment by ip_ref.coarse_search, codes by pq_ref.compute_codes of the
    residuals (by_residual) to that assignment"""
    w = int_world(104, 16, 256)
    w.M, w.nbits = 4, 8
    w.pq = (0.8 * w.rng.standard_normal((w.M, 256, w.d // w.M))).astype(F32)
    res = (w.pool - w.coarse[w.pool_assign]).astype(F32)
    w.pool_codes = pq_ref.compute_codes(res, w.pq)
    w.idx = pool_rows(14, PAGE + TAILS[-1], labels=w.pool_assign)
    w.ids = given_ids(5, w.idx.shape[0])
    return w


@functools.lru_cache(maxsize=None)
def ivfpqr():
    """IVFPQR, d / M_refine = 4 < 16, pooled: lists and codes by the oracle on the pool (every row of a GEMM-formulation batch
    is independent of the others), refine code = first-minimum PQ code of (x - coarse[a]) - pq_decode(code), float32 steps"""
    w = l2_world(105, 16, 256, n=POOL)
    w.M, w.nbits, w.Mr, w.nbits_r = 4, 8, 4, 6
    w.pq = (0.3 * w.rng.standard_normal((w.M, 256, w.d // w.M))).astype(F32)
    w.rpq = (0.08 * w.rng.standard_normal((w.Mr, 1 << w.nbits_r, w.d // w.Mr))).astype(F32)
    w.pool = w.x
    a, c = oracle_of(w).encode(w.pool, canonical=True)
    r1 = (w.pool - w.coarse[a]).astype(F32)
    r2 = (r1 - pq_decode(w.pq, c)).astype(F32)
    w.pool_assign, w.pool_codes, w.pool_rcodes = a, c, pq_ref.compute_codes(r2, w.rpq)
    w.idx = pool_rows(15, PAGE + TAILS[-1], labels=w.pool_assign)
    w.ids = given_ids(6, w.idx.shape[0])
    return w


@functools.lru_cache(maxsize=None)
def ivfflat_l2():
    w = l2_world(106, 8, 256, spread=0.25, n=PAGE + TAILS[-1])
    w.ids = given_ids(7, w.x.shape[0])
    w.assign = l2_assign(w, w.x)
    w.assign.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def ivfflat_ip():
    w = int_world(107, 8, 256)
    w.idx = pool_rows(17, PAGE + TAILS[-1], labels=w.pool_assign)
    w.ids = given_ids(8, w.idx.shape[0])
    return w


def holes(seed, assign, nlist):
    """an assignment for add_preassigned: a seeded tenth of the rows get -1 and another twentieth nlist or nlist + 5 -- some of
    them on the last page"""
    rng = np.random.default_rng(seed)
    a = np.array(assign, np.int64)
    n = a.shape[0]
    a[rng.random(n) < 0.1] = -1
    big = rng.random(n) < 0.05
    a[big] = nlist + 5 * (np.arange(n)[big] % 2)
    a[PAGE + 1], a[PAGE + 3] = -1, nlist
    return a


@functools.lru_cache(maxsize=None)
def ivfsq(qtype):
    """IVFSQ: "8bit" at d = 16, "4bit" at d = 12; the range is trained on the residuals of the first 4000 rows shrunk to 0.7 of
    their size, so rows of every page reach both clamps"""
    d = {"8bit": 16, "4bit": 12}[qtype]
    w = l2_world(108 + d, d, 256, n=PAGE + TAILS[-1])
    w.qtype, w.qt = qtype, ivfsq_ref.QTYPES[qtype]
    w.ids = given_ids(9, w.x.shape[0])
    w.assign = l2_assign(w, w.x)
    w.assign.setflags(write=False)
    w.res = (w.x - w.coarse[w.assign]).astype(F32)
    w.trained = ivfsq_ref.train((F32(0.7) * w.res[:4000]).astype(F32), w.qt)
    w.codes = ivfsq_ref.encode(w.res, w.qt, w.trained)
    return w


@functools.lru_cache(maxsize=None)
def vlq_world():
    """VLQ: 256 centroids x 2 edges = 512 lines, d = 16, PAGE + 1500 distinct rows.  The rows behind the first page are chosen
    from spare ones by the oracle's own assignment: the first seven lie on seven different lines, none on the line of the row
    one page before it.  v is the trained oracle index (its own lists are not used: fresh_vlq)."""
    from test_vlq_oracle import make_vlq
    n = PAGE + TAILS[-1]
    v, xb, xq = make_vlq(seed=9, d=16, nlist=256, M=4, nbits=6, nedge=2, nlambda=16, nb=n + 512)
    line, _lam = v.assign(xb)
    spare, tail, seen = list(range(PAGE, xb.shape[0])), [], set()
    for i in range(n - PAGE):
        j = next(j for j in spare if line[j] != line[i] and (i >= 7 or line[j] not in seen))
        spare.remove(j)
        tail.append(j)
        seen.add(int(line[j]))
    x = np.ascontiguousarray(np.concatenate([xb[:PAGE], xb[tail]]))
    assert np.unique(x, axis=0).shape[0] == n
    return world(v=v, x=x, xq=xq, nlines=256 * 2, ids=given_ids(10, n))


def fresh_vlq(v):
    """an empty oracle index with v's trained state"""
    from oracle.pyoracle import OracleVLQ
    return OracleVLQ(v.d, v.nlist, v.M, v.nbits, v.nedge, v.nlambda, v.coarse, v.pq_centroids, v.edge_info, v.edge_dist, v.lambda_info)


@functools.lru_cache(maxsize=None)
def offset_tail():
    """Rows far from the origin, where |x|^2 + |c|^2 - 2 <x, c> of the GEMM formulation cancels and the direct (x - c)^2 of the
    reference's batches of fewer than 20 rows does not: the seven rows behind the first page are picked so that the two
    formulations assign EVERY one of them to different lists.  d = 16, nlist = 256."""
    rng = np.random.default_rng(110)
    d, nlist = 16, 256
    coarse = (100 + rng.random((nlist, d))).astype(F32)
    ox = OracleIndex(d, nlist, 1, 1, coarse, np.zeros((1, 2, d), F32), by_residual=False)
    cand = (100 + rng.random((PAGE + 20000, d))).astype(F32)
    k1 = ox.coarse_search(cand[PAGE:], 1, canonical=True, force_path=1)[1][:, 0]
    k2 = ox.coarse_search(cand[PAGE:], 1, canonical=True, force_path=2)[1][:, 0]
    differ = np.nonzero(k1 != k2)[0]
    assert differ.size >= 7, "the two formulations agree on this data"
    x = np.concatenate([cand[:PAGE], cand[PAGE + differ[:7]]])
    w = world(d=d, nlist=nlist, coarse=coarse, x=x, direct=k1[differ[:7]].copy(), gemm=k2[differ[:7]].copy())
    w.assign = l2_assign(w, x)
    return w


# ----------------------------------------------------------------------------------------------------------------------
# the encoder sweep (D)
# ----------------------------------------------------------------------------------------------------------------------
# (d, M, nbits): dsub 1, 2, 3, 4, 6, 8; nbits 4 .. 8; d from 4 to 72 (above 64, no multiple of 64)
# M % 8 == 0 (the polysemous search type, whose query codes come from pq_table_argmin_kernel) at nbits 4, 5, 6, 7 and 8
PQ_SHAPES = ((4, 4, 4), (6, 6, 5), (12, 4, 4), (20, 5, 6), (12, 6, 7), (32, 8, 8), (48, 8, 7), (24, 3, 5), (64, 16, 6), (72, 12, 8), (72, 9, 4),
             (8, 8, 4), (16, 8, 5))
PQ_ROWS = (1, 3, 4, 5, 257)
PQ_NLIST = 7


@functools.lru_cache(maxsize=None)
def pq_shape(d, M, nbits):
    """A PQ with two duplicated centroids per sub-quantizer (j1 is a copy of j0, j0 < j1) and 257 rows whose every sub-vector of
    rows 0 .. 63 lies EXACTLY on a duplicated centroid (after the residual, too: the coarse centroids and those rows are
    small integers over 4, so x - c is exact): the lower index must win.  A small flat coarse quantizer for the IVFPQ side."""
    rng = np.random.default_rng(1000 * d + 10 * M + nbits)
    ksub, dsub = 1 << nbits, d // M
    pq = (rng.integers(-8, 9, (M, ksub, dsub)) / 4.0).astype(F32)
    pq += (rng.standard_normal(pq.shape) * 0.01).astype(F32)
    dup = np.zeros((M, 2), np.int64)
    for m in range(M):
        j0, j1 = np.sort(rng.permutation(ksub)[:2])
        pq[m, j0] = (rng.integers(-8, 9, dsub) / 4.0).astype(F32)
        pq[m, j1] = pq[m, j0]
        dup[m] = j0, j1
    coarse = (rng.integers(-8, 9, (PQ_NLIST, d)) / 4.0).astype(F32)
    n = PQ_ROWS[-1]
    cells = rng.integers(0, PQ_NLIST, n).astype(np.int64)
    x = (coarse[cells] + 0.6 * rng.standard_normal((n, d))).astype(F32)
    on = np.concatenate([pq[m, dup[m, rng.integers(0, 2, 64)]] for m in range(M)], axis=1)      # [64][d]: on the duplicates
    x_flat = x.copy()
    x_flat[:64] = on                                                  # by_residual off / GpuPQ: the row itself is encoded
    x_res = x.copy()
    x_res[:64] = on + coarse[cells[:64]]                              # the residual to cells: exact sums of multiples of 1/4
    return world(d=d, M=M, nbits=nbits, nlist=PQ_NLIST, pq=pq, dup=dup, coarse=coarse, x_flat=x_flat, x_res=x_res, cells=cells)


def residual_codes(w, x, assign, codes_of):
    """what encode_preassigned stores: the code of x - coarse[assign] (one float32 subtraction), of a zero row where assign < 0"""
    a = np.asarray(assign, np.int64)
    res = np.where((a >= 0)[:, None], (x - w.coarse[np.maximum(a, 0)]).astype(F32), F32(0)).astype(F32)
    return codes_of(res)


def oracle_flat_codes(w, rows):
    """the oracle's PQ codes of the rows themselves (by_residual off)"""
    return oracle_of(w, by_residual=False).encode(rows, canonical=True)[1]


SQ_DIMS = (1, 3, 5, 33, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def sq_shape(d, qt, seed=0):
    """Residuals for the scalar-quantizer encoders at dimension d: trained range, rows inside it, rows below vmin and above
    vmin + vdiff in every component (both clamps), rows exactly on both ends.  A flat coarse quantizer of 4 centroids 64 apart
    in every component: a row res + coarse[i] has centroid i as its nearest by far, and for the end rows, whose entries are
    multiples of 1/8, the sum and the residual taken from it are exact."""
    rng = np.random.default_rng(7000 + 10 * d + qt + seed)
    uniform = ivfsq_ref.is_uniform(qt)
    vmin = (rng.integers(-16, -3, 1 if uniform else d) / 8.0).astype(F32)
    vdiff = (rng.integers(4, 40, 1 if uniform else d) / 8.0).astype(F32)
    trained = np.concatenate([vmin, vdiff]).astype(F32)
    lo, hi = np.broadcast_to(vmin, (d,)), np.broadcast_to((vmin + vdiff).astype(F32), (d,))
    inside = (lo + rng.random((150, d)) * (hi - lo)).astype(F32)
    below = (lo - rng.random((10, d)) - 0.01).astype(F32)
    above = (hi + rng.random((10, d)) + 0.01).astype(F32)
    mixed = np.where(rng.random((20, d)) < 0.5, below[rng.integers(0, 10, 20)], above[rng.integers(0, 10, 20)]).astype(F32)
    ends = np.stack([lo, hi, np.where(np.arange(d) % 2 == 0, lo, hi), np.where(np.arange(d) % 2 == 0, hi, lo)]).astype(F32)
    res = np.concatenate([ends, inside, below, above, mixed])
    coarse = np.repeat(64.0 * np.arange(4)[:, None], d, axis=1).astype(F32)
    cells = rng.integers(0, 4, res.shape[0]).astype(np.int64)
    return world(d=d, qt=qt, nlist=4, trained=trained, res=res, coarse=coarse, cells=cells, x=(res + coarse[cells]).astype(F32), nends=4)


LSH_BITS = (1, 7, 8, 9, 60, 64, 65, 128, 130)


@functools.lru_cache(maxsize=None)
def lsh_shape(nbits, rotate):
    """rows for the LSH packer at nbits: d = nbits + 3 without a rotation (the first nbits components are the bits), d = 24
    with one; components that are exactly 0.0 and -0.0 (both set their bit) among ordinary ones"""
    rng = np.random.default_rng(9000 + 2 * nbits + int(rotate))
    d = 24 if rotate else nbits + 3
    x = rng.standard_normal((67, d)).astype(F32)
    if not rotate:
        x[rng.random(x.shape) < 0.15] = 0.0
        x[rng.random(x.shape) < 0.15] = -0.0
    else:
        x[:4] = 0.0                     # rotated zero rows: every xt is +0.0 (or the bias)
        x[4:8] = -0.0
    A = b = None
    if rotate:
        q, _r = np.linalg.qr(rng.standard_normal((max(d, nbits), max(d, nbits))))
        A = np.ascontiguousarray(q[:nbits, :d], dtype=F32)
        b = (0.1 * rng.standard_normal(nbits)).astype(F32)
    thr = (0.2 * rng.standard_normal(nbits)).astype(F32)
    return world(d=d, nbits=nbits, x=x, A=A, b=b, thr=thr)


# ----------------------------------------------------------------------------------------------------------------------
# list growth (C): the lengths loaded into 300 lists and the batches added afterwards, as (list -> rows) counts
# ----------------------------------------------------------------------------------------------------------------------
GROWTH_NLIST = 300                    # two workgroups of the relayout kernel: 256 + 44 lists
GROWTH_SHORT = 32                     # lists.hip's kShortList: up to here a list is copied by its own thread
# (list 0 starts at offset 0 in every layout: a long list whose offsets are always 16-byte aligned)
GROWTH_SPECIAL = {0: 37, 3: 0, 10: 1, 17: 31, 24: 32, 31: 33, 38: 40, 45: 255, 52: 256, 59: 257, 66: 1000, 73: 31,      # first workgroup
                  262: 0, 270: 500, 280: 33, 299: 40}                                                          # second workgroup
GROWTH_LONG, GROWTH_SHORT_TO_LONG, GROWTH_SECOND = 66, 73, 59
# (what the step is for, rows per list, reclaim_memory behind it -- where the kind has one: its byte count is the one place the
# capacities show, so it is taken while they still carry the slack of the growth)
GROWTH_STEPS = (("a long list overflows: every list moves", {GROWTH_LONG: 3}, True),
                ("once more (packed again where reclaim_memory ran: an overflow; else it fits the slack)", {GROWTH_LONG: 2}, False),
                ("the batch fits the slack: nothing moves", {GROWTH_LONG: 10, 270: 20, 24: 5}, True),
                ("a short list overflows and becomes long", {GROWTH_SHORT_TO_LONG: 10}, False),
                ("another overflow moves the list that became long", {GROWTH_SECOND: 80}, True))
GROWTH_ROW_BYTES = {"ivfpq-M16": 16, "ivfpq-M8": 8, "ivfpq-M5": 5, "ivfpqr": 2, "ivfflat-d3": 12, "ivfflat-d4": 16, "ivfsq-4bit": 3, "vlq": 2}


def growth_lens():
    """lengths of the 300 lists as loaded: 0 .. 4 rows each, long and boundary lengths in between"""
    lens = np.array([(i * 7) % 5 for i in range(GROWTH_NLIST)], np.int64)
    for i, n in GROWTH_SPECIAL.items():
        lens[i] = n
    return lens


def growth_counts(step):
    cnt = np.zeros(GROWTH_NLIST, np.int64)
    for i, n in GROWTH_STEPS[step][1].items():
        cnt[i] = n
    return cnt


def grow(lens, cap, cnt):
    """lists.hip's append: (lengths, capacities, overflowed) after cnt more rows per list -- when one list overflows, EVERY
    list gets max(capacity, need + need // 4)"""
    need = lens + cnt
    over = bool((need > cap).any())
    return need, (np.maximum(cap, need + need // 4) if over else cap), over


def growth_run(reclaims=True):
    """The growth test on the host, from the packed load on.  reclaims: the kind has reserve_memory / reclaim_memory (all but
    VLQ).  Returns (steps, relayouts): per step of GROWTH_STEPS a dict of counts, overflows, lens / cap before and after and
    the bytes-free row count reclaim_memory gives back behind it (None: no reclaim); and every relayout of the run as
    (what, lengths at the time, old capacities, new capacities) -- the overflowing adds, the reclaims, and the last round of
    reserve_memory to max(capacity) + 3 rows a list and reclaim_memory."""
    lens = growth_lens()
    cap = lens.copy()
    steps, relayouts = [], []
    for step, (what, _rows, reclaim) in enumerate(GROWTH_STEPS):
        cnt = growth_counts(step)
        new_lens, new_cap, over = grow(lens, cap, cnt)
        if over:
            relayouts.append((what, lens, cap, new_cap))
        s = dict(what=what, counts=cnt, overflows=over, lens_before=lens, cap_before=cap, lens=new_lens, cap=new_cap, reclaimed=None)
        lens, cap = new_lens, new_cap
        if reclaim and reclaims:
            s["reclaimed"] = int(cap.sum() - lens.sum())
            relayouts.append(("reclaim_memory after: " + what, lens, cap, lens))
            cap = lens
        steps.append(s)
    if reclaims:
        per = int(cap.max()) + 3
        relayouts.append(("reserve_memory", lens, cap, np.maximum(cap, per)))
        relayouts.append(("last reclaim_memory", lens, np.maximum(cap, per), lens))
    return steps, relayouts


def relayout_paths(relayouts, row_bytes):
    """how many list copies the relayouts make on each path of relayout_kernel: "aligned" -- a list longer than GROWTH_SHORT
    rows whose old and new byte offsets are both multiples of 16, copied by the workgroup in 16-byte words ("tail": of those,
    the ones whose byte count leaves single bytes behind the words); "unaligned" -- such a list at other offsets, copied by
    bytes; "short" -- a list copied by its own thread"""
    n = dict(aligned=0, tail=0, unaligned=0, short=0)
    for _what, lens, old_cap, new_cap in relayouts:
        old_off = np.concatenate([[0], np.cumsum(old_cap)[:-1]]) * row_bytes
        new_off = np.concatenate([[0], np.cumsum(new_cap)[:-1]]) * row_bytes
        long_ = lens > GROWTH_SHORT
        ok = ((old_off | new_off) % 16 == 0)
        n["aligned"] += int((long_ & ok).sum())
        n["tail"] += int((long_ & ok & ((lens * row_bytes) % 16 != 0)).sum())
        n["unaligned"] += int((long_ & ~ok).sum())
        n["short"] += int(((lens > 0) & ~long_).sum())
    return n
