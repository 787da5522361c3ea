"""GPU (run with -m gpu on an MI355X): the life cycle of the inverted lists (csrc/lists.h) through the Python classes of every
kind of index -- loading, reloading, adding with and without growth, reserving and reclaiming, resetting -- against a host
model kept in numpy: for each list the rows, side bytes and ids in arrival order, and its capacity.  The capacities follow
lists.hip exactly (packed after set_lists, max(capacity, num_vecs // nlist) after reserve_memory, max(capacity, need + need // 4)
for EVERY list when one list of an add overflows, length after reclaim_memory, nothing after reset), so reclaim_memory's byte
count is asserted, not only its second call.  A search after the adds must return, bit for bit, the rows of a fresh index
that got the model through set_lists: that ties the store to what the scans read.
The bytes a row is stored as come from the kind's own encode call (for the refine codes, which have none: from one add of the
rows to a scratch index, read back by id); where they go, in which order and under which id is the model's.
The geometry -- d, the number of lists, the code width, the side bytes -- is a parameter (Geometry): this file runs the small
one (5 lists of at most about 20 rows), tests/test_gpu_list_growth.py the ones that reach the relayout kernel's other paths."""
import numpy as np
import pytest

import vector_line_quantization_amd as vlq

pytestmark = pytest.mark.gpu

KINDS = ("ivfpq", "ivfpqr", "ivfflat", "ivfsq", "vlq")


class Geometry:
    """What the list store sees of an index: d, the coarse lists (a VLQ index has nedge lines per list), the PQ code width M
    (8 bits), the refine codes (mr bytes of nbits_r bits), the scalar quantizer's type.  The trained state is seeded."""

    def __init__(self, d=8, nlist=5, M=2, nedge=2, nlambda=16, mr=2, nbits_r=4, qtype="8bit", k=5, nq=7, seed=77):
        self.d, self.nlist, self.M, self.nedge, self.nlambda = d, nlist, M, nedge, nlambda
        self.mr, self.nbits_r, self.qtype, self.k, self.nq, self.seed = mr, nbits_r, qtype, k, nq, seed
        self._world = {}

    def world(self):
        w = self._world
        if not w:
            rng = np.random.RandomState(self.seed)
            w["coarse"] = (4 * rng.randn(self.nlist, self.d)).astype(np.float32)
            w["pq"] = (0.5 * rng.randn(self.M, 256, self.d // self.M)).astype(np.float32)
            w["rpq"] = (0.1 * rng.randn(self.mr, 1 << self.nbits_r, self.d // self.mr)).astype(np.float32)
            w["lambda"] = np.linspace(0.0, 1.0, self.nlambda).astype(np.float32)
            w["train"] = near(rng, rng.randint(0, self.nlist, 64), self)
            w["xq"] = near(rng, rng.randint(0, self.nlist, self.nq), self)
        return w


BASE = Geometry()
D_, NLIST, M_, NEDGE, NLAMBDA, MR, NBITS_R, K, NQ = BASE.d, BASE.nlist, BASE.M, BASE.nedge, BASE.nlambda, BASE.mr, BASE.nbits_r, BASE.k, BASE.nq


def world(geo=BASE):
    return geo.world()


def near(rng, cells, geo=BASE):
    """one row beside the coarse centroid of each given cell"""
    return (geo._world["coarse"][np.asarray(cells)] + 0.3 * rng.randn(len(cells), geo.d)).astype(np.float32)


def make(kind, geo=BASE):
    w = world(geo)
    if kind == "ivfflat":
        g = vlq.GpuIVFFlat(geo.d, geo.nlist)
    elif kind == "ivfsq":
        g = vlq.GpuIVFSQ(geo.d, geo.nlist, geo.qtype)
    elif kind == "vlq":
        g = vlq.GpuVLQ(geo.d, geo.nlist, geo.M, 8, geo.nedge, geo.nlambda)
    else:
        g = vlq.GpuIVFPQ(geo.d, geo.nlist, geo.M, 8)
    g.set_coarse_centroids(w["coarse"])
    if kind == "ivfsq":
        if "sq_trained" not in w:
            g.train(w["train"])
            w["sq_trained"] = g.trained
        g.set_trained(w["sq_trained"])
    if kind in ("ivfpq", "ivfpqr", "vlq"):
        g.set_pq_centroids(w["pq"])
    if kind == "ivfpqr":
        g.set_refine_pq(geo.mr, geo.nbits_r, w["rpq"])
    if kind == "vlq":
        g.build_graph()
        g.set_lambda_codebook(w["lambda"])
    return g


def shape_of(kind, geo=BASE):
    """(number of lists, row dtype, row width, side bytes per row)"""
    if kind == "ivfflat":
        return geo.nlist, np.float32, geo.d, 0
    if kind == "vlq":
        return geo.nlist * geo.nedge, np.uint8, geo.M, 1
    if kind == "ivfsq":
        return geo.nlist, np.uint8, geo.d if geo.qtype.startswith("8bit") else (geo.d + 1) // 2, 0
    return geo.nlist, np.uint8, geo.M, geo.mr if kind == "ivfpqr" else 0


def stored_as(kind, g, x, geo=BASE):
    """(list of every row or -1, the rows as stored, their side bytes [n][side]) for the rows x"""
    n = len(x)
    side = np.zeros((n, 0), np.uint8)
    if kind == "ivfflat":
        _cd, keys = g.coarse_search(x, 1)
        return keys[:, 0].copy(), x.copy(), side
    if kind == "ivfsq":
        codes, assign = g.encode(x)
        return assign, codes, side
    if kind == "vlq":
        line, lam, codes = g.encode(x)
        return line.astype(np.int64), codes, lam.reshape(n, 1)
    assign, codes = g.encode(x)
    if kind == "ivfpqr":        # ids of an empty index's first add are the row numbers
        s = make(kind, geo)
        s.add(x)
        side = np.zeros((n, geo.mr), np.uint8)
        for i in np.unique(assign[assign >= 0]):
            side[s.get_list(i)[1]] = s.get_list_refine_codes(i)
    return assign, codes, side


class Model:
    def __init__(self, kind, geo=BASE):
        self.kind, self.geo = kind, geo
        self.nlists, self.dtype, self.width, self.side = shape_of(kind, geo)
        self.row_bytes = self.width * np.dtype(self.dtype).itemsize + 8 + self.side
        self.side_values = geo.nlambda if kind == "vlq" else 1 << geo.nbits_r      # (a lambda index, a refine code)
        self.grown = 0
        self.reset()

    def reset(self):
        self.rows = [np.zeros((0, self.width), self.dtype) for _ in range(self.nlists)]
        self.sides = [np.zeros((0, self.side), np.uint8) for _ in range(self.nlists)]
        self.ids = [np.zeros((0,), np.int64) for _ in range(self.nlists)]
        self.cap = np.zeros(self.nlists, np.int64)
        self.next_id = 0        # sequential ids continue from the vectors loaded / handed to add so far
        self.ntotal = 0

    @property
    def lens(self):
        return np.array([len(i) for i in self.ids], np.int64)

    def load(self, rng, lens):
        assert len(lens) == self.nlists
        nt = int(sum(lens))
        rows = rng.randn(nt, self.width).astype(np.float32) if self.dtype == np.float32 else rng.randint(0, 256, (nt, self.width)).astype(np.uint8)
        sides = rng.randint(0, self.side_values, (nt, self.side)).astype(np.uint8)
        ids = (rng.permutation(nt) * 3 + 1000).astype(np.int64)
        cuts = np.cumsum(lens)[:-1]
        self.rows, self.sides, self.ids = np.split(rows, cuts), np.split(sides, cuts), np.split(ids, cuts)
        self.cap = np.array(lens, np.int64)
        self.next_id = self.ntotal = nt

    def reserve(self, num_vecs):
        per = num_vecs // self.nlists
        if per >= 1:
            self.cap = np.maximum(self.cap, per)

    def reclaim(self):
        freed = int(self.cap.sum() - self.lens.sum()) * self.row_bytes
        self.cap = self.lens
        return freed

    def add(self, assign, rows, sides):
        n = len(assign)
        ok = assign >= 0
        need = self.lens + np.bincount(assign[ok], minlength=self.nlists)
        if (need > self.cap).any():
            self.cap = np.maximum(self.cap, need + need // 4)
            self.grown += 1
        for i in np.nonzero(ok)[0]:
            l = assign[i]
            self.rows[l] = np.concatenate([self.rows[l], rows[i:i + 1]])
            self.sides[l] = np.concatenate([self.sides[l], sides[i:i + 1]])
            self.ids[l] = np.concatenate([self.ids[l], [self.next_id + i]])
        self.next_id += n
        self.ntotal += n if self.kind in ("ivfpq", "ivfpqr") else int(ok.sum())

    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)

    def load_into(self, g):
        rows, sides, ids = np.concatenate(self.rows), np.concatenate(self.sides), np.concatenate(self.ids)
        if self.kind == "vlq":
            g.set_lists(rows, sides[:, 0], ids, self.offsets())
        else:
            g.set_lists(rows, ids, self.offsets())
        if self.kind == "ivfpqr":
            g.set_refine_codes(sides)

    def check(self, g, step):
        assert g.ntotal == self.ntotal, step
        for i in range(self.nlists):
            got = g.get_list(i)
            if self.kind != "vlq":
                assert g.list_length(i) == len(self.ids[i]), (step, i)
            rows, ids = got[0], got[-1]
            assert rows.dtype == self.dtype and rows.shape == self.rows[i].shape, (step, i, rows.shape, self.rows[i].shape)
            assert rows.tobytes() == self.rows[i].tobytes(), (step, i, "rows")
            assert np.array_equal(ids, self.ids[i]), (step, i, ids, self.ids[i])
            if self.kind == "vlq":
                assert np.array_equal(got[1], self.sides[i][:, 0]), (step, i, "lambdas")
            if self.kind == "ivfpqr":
                assert np.array_equal(g.get_list_refine_codes(i), self.sides[i]), (step, i, "refine codes")


def search(kind, g, geo=BASE):
    xq = world(geo)["xq"]
    if kind == "vlq":
        return g.search(xq, geo.nlist, geo.nlist * geo.nedge, geo.k)
    if kind == "ivfpqr":
        return g.search_refined(xq, geo.nlist, geo.k, 2.0)
    return g.search(xq, geo.nlist, geo.k)


def check_search(kind, g, model, step):
    """the rows of g == the rows of a fresh index that got the model through set_lists, bit for bit"""
    geo = model.geo
    fresh = make(kind, geo)
    model.load_into(fresh)
    D, I = search(kind, g, geo)
    Df, If = search(kind, fresh, geo)
    assert (If[:, geo.k - 1] >= 0).all(), (step, "every query has K results")
    assert np.array_equal(D.view(np.uint32), Df.view(np.uint32)), (step, D, Df)
    assert np.array_equal(I, If), (step, I, If)


def add(kind, g, model, x):
    assign, rows, sides = stored_as(kind, g, x, model.geo)
    g.add(x)
    model.add(assign, rows, sides)


@pytest.mark.parametrize("kind", KINDS)
def test_list_life_cycle(kind):
    w = world()
    rng = np.random.RandomState(5)
    g = make(kind)
    model = Model(kind)
    per_cell = model.nlists // NLIST
    has_reserve = kind != "vlq"

    # 1. loading: one empty list, one list of a single row
    model.load(rng, [0, 1, 7, 5, 4] * per_cell)
    model.load_into(g)
    model.check(g, "load")
    # 2. reloading: fewer rows, then more rows than the first time
    model.load(rng, [2, 0, 3, 1, 0] * per_cell)
    model.load_into(g)
    model.check(g, "reload with fewer rows")
    model.load(rng, [6, 9, 0, 8, 7] if per_cell == 1 else [3, 3, 5, 4, 0, 0, 8, 0, 4, 3])
    model.load_into(g)
    model.check(g, "reload with more rows")
    assert model.ntotal == 30

    # 3. adding without growth: room for 4 more rows in every list first
    if has_reserve:
        room = (int(model.lens.max()) + 4) * model.nlists
        g.reserve_memory(room)
        model.reserve(room)
        model.check(g, "reserve_memory")
        grown = model.grown
        add(kind, g, model, near(rng, [0, 2, 2, 4]))
        assert model.grown == grown, "the batch fits the reserved room"
        model.check(g, "add without growth")
        g.reserve_memory(room)
        model.reserve(room)
        model.check(g, "reserve_memory again")

    # 4. adding with growth: ten rows beside one centroid overflow its list(s); input order is kept (the ids ascend)
    grown = model.grown
    add(kind, g, model, near(rng, [1] * 10 + [3, 0]))
    assert model.grown == grown + 1, "the batch overflows a list"
    model.check(g, "add with growth")
    for ids in model.ids:
        new = ids[ids < 1000]
        assert (np.diff(new) > 0).all()
    check_search(kind, g, model, "search after the adds")
    if has_reserve:
        assert model.cap.sum() > model.lens.sum()
        assert g.reclaim_memory() == model.reclaim(), "reclaim_memory"
        assert g.reclaim_memory() == 0, "second reclaim_memory"
        model.check(g, "reclaim_memory")
        check_search(kind, g, model, "search after reclaim_memory")

    # 5. resetting: every list empty, the next add starts afresh with ids from 0
    if kind in ("ivfflat", "ivfsq"):
        g.reset()
        model.reset()
        model.check(g, "reset")
        assert g.ntotal == 0
        add(kind, g, model, near(rng, [4, 4, 0, 1, 3, 3, 3, 2]))
        model.check(g, "add after reset")
        assert sorted(np.concatenate(model.ids)) == list(range(8))
        check_search(kind, g, model, "search after reset")
