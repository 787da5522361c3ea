"""Product-quantizer training on the device (vlq.GpuPQTrainer): the batched assignment against the flat search's restatement
(knn_ref.py), the training against M GpuKMeans runs over contiguous slices, IndexIVFPQ::train / IndexPQ::train against their
composition.  Everything bit for bit."""
import numpy as np
import pytest

import kmeans_ref
import knn_ref
import vector_line_quantization_amd as vlq

pytestmark = pytest.mark.gpu
F32 = np.float32


def check_assign(x, cb, nbits):
    (n, d), (M, ksub, dsub) = x.shape, cb.shape
    tr = vlq.GpuPQTrainer(d, M, nbits)
    tr.set_centroids(cb)
    D, I = tr.assign(x)
    print(tr.last_info())
    assert "route=batched" in tr.last_info()
    for m in range(M):
        Dm, Im = knn_ref.search(x[:, m * dsub:(m + 1) * dsub], cb[m], 1, "l2", nq_call=n)
        assert np.array_equal(I[:, m], Im[:, 0] + m * ksub), m
        assert knn_ref.same_bits(D[m], Dm[:, 0]), m
    return D, I


ASSIGN_SHAPES = {                       # (d, M, nbits, n)
    "ksub 4 < 32 columns, dsub 4": (8, 2, 2, 40),
    "dsub 6, d no multiple of 32 floats": (30, 5, 4, 300),
    "odd dsub 3, one row past a tile": (24, 8, 3, 257),
    "the real shape, several slice groups": (128, 16, 8, 1000),
    "M = 1, dsub 64": (64, 1, 8, 300),
    "dsub 48": (96, 2, 8, 300),
    "n == ksub": (12, 3, 8, 256),
}


@pytest.mark.parametrize("edge", sorted(ASSIGN_SHAPES))
def test_assign_is_the_flat_search_per_slice(edge):
    d, M, nbits, n = ASSIGN_SHAPES[edge]
    rng = np.random.default_rng(d * 1000 + M * 10 + nbits)
    x = (rng.standard_normal((n, d)) * 3 + 1).astype(F32)
    cb = (rng.standard_normal((M, 1 << nbits, d // M)) * 3 + 1).astype(F32)
    check_assign(x, cb, nbits)


def test_assign_ties_go_to_the_lower_index():
    rng = np.random.default_rng(5)
    x = rng.integers(-2, 3, (200, 8)).astype(F32)
    cb = rng.integers(-2, 3, (2, 8, 4)).astype(F32)
    x[0] = 0
    cb[:, 2] = 0
    cb[:, 5] = cb[:, 1]                 # a duplicate never wins
    D, I = check_assign(x, cb, 3)
    assert not (I % 8 == 5).any() and (D[:, 0].view(np.uint32) == 0).all()


def composed(x, M, nbits, init=None, **kw):
    """(codebook, objectives) of M GpuKMeans runs over contiguous slices"""
    dsub = x.shape[1] // M
    cb, obj = [], []
    for m in range(M):
        km = vlq.GpuKMeans(dsub, 1 << nbits, **kw)
        cb.append(km.train(np.ascontiguousarray(x[:, m * dsub:(m + 1) * dsub]), init=None if init is None else init[m]))
        obj.append(km.obj)
        km.close()
    return np.stack(cb), np.stack(obj)


def few_rows(rng, n, d, distinct):
    return rng.standard_normal((distinct, d)).astype(F32)[rng.integers(0, distinct, n)]


TRAIN_CASES = {                         # (d, M, nbits, n), the clustering parameters, what else the case does
    "plain": ((16, 4, 4, 3000), dict(niter=3), ""),
    "subsampled": ((32, 4, 5, 600), dict(niter=3, max_points_per_centroid=8), ""),
    "empty clusters": ((8, 2, 3, 200), dict(niter=3), "few rows"),
    "spherical": ((24, 3, 3, 500), dict(niter=3, spherical=True), ""),
    "nredo=2": ((16, 4, 4, 2000), dict(niter=2, nredo=2), ""),
    "hot_start": ((16, 4, 4, 1000), dict(niter=2), "hot"),
    "loop route": ((8, 2, 3, 16), dict(niter=3), "loop"),
}


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_train_is_m_kmeans_runs(name):
    (d, M, nbits, n), kw, what = TRAIN_CASES[name]
    ksub, dsub = 1 << nbits, d // M
    rng = np.random.default_rng(d * 100 + n)
    x = few_rows(rng, n, d, ksub // 2) if what == "few rows" else rng.standard_normal((n, d)).astype(F32)
    tr = vlq.GpuPQTrainer(d, M, nbits, **kw)
    c = tr.train(x)
    info = tr.last_info()
    print(name, info)
    want_c, want_obj = composed(x, M, nbits, **kw)
    assert knn_ref.same_bits(c, want_c) and np.array_equal(tr.obj, want_obj)
    assert ("route=loop" if what == "loop" else "route=batched") in info
    if what == "few rows":              # the reference alone splits in the first step of slice 0
        x0 = np.ascontiguousarray(x[:, :dsub])
        start = x0[kmeans_ref.rand_perm(n, 1234 + 1)[:ksub]]
        labels = knn_ref.search(x0, start, 1, "l2", nq_call=n)[1][:, 0]
        assert kmeans_ref.update(x0, labels, ksub)[2] >= 1
        assert int(info.split("nsplit=")[1].split()[0]) > 0
    if what == "hot":                   # a second train from the first result
        tr.train_type = "hot_start"
        c2 = tr.train(x)
        want_c2, want_obj2 = composed(x, M, nbits, init=want_c, **kw)
        assert knn_ref.same_bits(c2, want_c2) and np.array_equal(tr.obj, want_obj2)
    if name == "plain":                 # a second run: the same bits
        assert knn_ref.same_bits(tr.train(x), c)


def test_train_shared_is_one_kmeans_over_all_slices():
    d, M, nbits, n = 16, 4, 4, 1000
    x = np.random.default_rng(7).standard_normal((n, d)).astype(F32)
    tr = vlq.GpuPQTrainer(d, M, nbits, niter=3, train_type="shared")
    c = tr.train(x)
    km = vlq.GpuKMeans(d // M, 1 << nbits, niter=3)
    want = km.train(x.reshape(n * M, d // M))
    for m in range(M):
        assert knn_ref.same_bits(c[m], want) and np.array_equal(tr.obj[m], km.obj)


@pytest.mark.parametrize("by_residual", [True, False])
def test_ivfpq_train_is_its_composition(by_residual):
    d, nlist, M, nbits, n, mp = 32, 16, 4, 8, 3000, 4
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, d)).astype(F32)
    q = rng.standard_normal((50, d)).astype(F32)
    coarse = vlq.kmeans(x, nlist)
    xs = x[kmeans_ref.rand_perm(n, 1234)[:mp << nbits]]
    if by_residual:
        flat = vlq.GpuFlat(d)
        flat.add(coarse)
        xs = xs - coarse[flat.search(xs, 1)[1][:, 0]]
    pq = vlq.train_pq(xs, M, nbits, max_points_per_centroid=mp, niter=3)
    rows = []
    for trained in (True, False):
        g = vlq.GpuIVFPQ(d, nlist, M, nbits)
        g.set_search_options(by_residual=by_residual, use_precomputed_table=0)
        if trained:
            g.train(x, max_points_per_centroid=mp, niter=3)
        else:
            g.set_coarse_centroids(coarse)
            g.set_pq_centroids(pq)
        g.add(x)
        rows.append(g.search(q, 4, 10))
    assert knn_ref.same_bits(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1])


def test_pq_train_installs_train_pq():
    d, M, nbits = 16, 4, 4
    x = np.random.default_rng(13).standard_normal((1000, d)).astype(F32)
    a, b = vlq.GpuPQ(d, M, nbits), vlq.GpuPQ(d, M, nbits)
    a.train(x, niter=3)
    b.set_centroids(vlq.train_pq(x, M, nbits, niter=3))
    assert np.array_equal(a.encode(x), b.encode(x))


ERRORS = {
    "n < ksub": (dict(), 10, None, 1),
    "a NaN in x": (dict(), 100, "nan", 1),
    "a hypercube train type": (dict(train_type="hypercube"), 100, None, 3),
    "nredo=2 with init": (dict(nredo=2), 100, "init", 1),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_errors(name):
    kw, n, what, code = ERRORS[name]
    x = np.random.default_rng(1).standard_normal((n, 8)).astype(F32)
    if what == "nan":
        x[7, 3] = np.nan
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuPQTrainer(8, 2, 4, **kw).train(x, init=np.zeros((2, 16, 4), F32) if what == "init" else None)
    assert e.value.code == code
