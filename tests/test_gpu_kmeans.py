"""k-means on the device (vlq.GpuKMeans) against its restatement (kmeans_ref.py), bit for bit."""
import numpy as np
import pytest

import kmeans_ref as ref
import vector_line_quantization_amd as vlq

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def labels(rng, what, k, n):
    if what == "perm":                  # every cluster exactly one row
        return rng.permutation(k).astype(np.int64)
    if what == "230":                   # 26 of 256 clusters empty
        return rng.choice(rng.permutation(k)[:230], n).astype(np.int64)
    a = rng.integers(0, k, n).astype(np.int64)
    if what == "half7":                 # a 1500-row chain, and every cluster from 150 on empty
        a = rng.integers(0, 150, n).astype(np.int64)
        a[rng.permutation(n)[:n // 2]] = 7
    return a


UPDATE_CASES = [(1, 1, 1, "any"), (3, 2, 5, "any"), (4, 1000, 1000, "perm"), (8, 256, 4096, "230"), (64, 37, 5000, "any"),
                (65, 37, 5000, "any"), (128, 300, 3000, "half7"), (200, 5, 700, "any")]


@pytest.mark.parametrize("d,k,n,what", UPDATE_CASES)
def test_update_step_bits(d, k, n, what):
    rng = np.random.default_rng(d * 100000 + k * 10 + n)
    x = (100 * rng.standard_normal((n, d))).astype(F32)
    a = labels(rng, what, k, n)
    want_c, want_count, want_nsplit = ref.update(x, a, k)
    km = vlq.GpuKMeans(d, k)
    c, count, nsplit = km.update(x, a)
    print(km.last_info(), "nsplit", nsplit, want_nsplit)
    assert nsplit == want_nsplit
    assert np.array_equal(count, want_count)
    assert bits_equal(c, want_c)
    if what == "230":
        assert nsplit == 26
    if what == "half7":
        assert np.bincount(a, minlength=k)[7] >= 1500 and nsplit >= 150


@pytest.mark.parametrize("label", [5, -1])
def test_bad_label_is_an_error(label):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 6)).astype(F32)
    a = rng.integers(0, 5, 40).astype(np.int64)
    a[17] = label
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuKMeans(6, 5).update(x, a)
    assert e.value.code == 1 and "label" in str(e.value)


def composed_run(x, k, niter, spherical, start):
    """one run of the loop out of its parts: GpuFlat for the assignment, the restatement for the update"""
    c, objs = ref.renorm(start) if spherical else start, []
    for _ in range(niter):
        flat = vlq.GpuFlat(x.shape[1])
        flat.add(c)
        D, I = flat.search(x, 1)
        flat.close()
        objs.append(D.astype(np.float64).sum())
        c = ref.update(x, I[:, 0], k)[0]
        c = ref.renorm(c) if spherical else c
    return c, objs


TRAIN_CASES = {
    "plain": dict(d=16, k=20, n=2000, niter=4),
    "subsampled": dict(d=128, k=64, n=19200, niter=3),        # above 64 * 256: 16 384 rows are gathered
    "spherical": dict(d=24, k=10, n=1500, niter=3, spherical=True),
    "nredo": dict(d=16, k=20, n=2000, niter=3, nredo=2),
    "init": dict(d=16, k=20, n=2000, niter=3, init=True),
}


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_train_is_its_composition(name):
    case = dict(TRAIN_CASES[name])
    d, k, n, niter = case.pop("d"), case.pop("k"), case.pop("n"), case.pop("niter")
    spherical, nredo, seed = case.get("spherical", False), case.get("nredo", 1), 1234
    rng = np.random.default_rng(k * 1000 + d)
    x = (rng.standard_normal((n, d)) + 3 * rng.standard_normal((k, d))[rng.integers(0, k, n)]).astype(F32)
    init = x[rng.permutation(n)[:k]].copy() if case.get("init") else None
    xs = x[ref.rand_perm(n, seed)[:k * 256]] if n > k * 256 else x
    runs = []
    for redo in range(nredo):
        start = init if init is not None else xs[ref.rand_perm(xs.shape[0], seed + 1 + redo * 15486557)[:k]]
        runs.append(composed_run(xs, k, niter, spherical, start))
    want_c = min(runs, key=lambda r: r[1][-1])[0]
    want_obj = np.array([o for r in runs for o in r[1]])

    km = vlq.GpuKMeans(d, k, niter=niter, nredo=nredo, spherical=spherical, seed=seed)
    c = km.train(x, init=init)
    print(name, km.last_info(), "obj", km.obj, want_obj)
    assert bits_equal(c, want_c) and bits_equal(km.centroids, want_c)
    assert km.obj.shape == (niter * nredo,)
    np.testing.assert_allclose(km.obj, want_obj, rtol=1e-6)
    if nredo > 1:
        assert runs[0][1][-1] != runs[1][1][-1]
    assert bits_equal(km.train(x, init=init), c)        # a second run: the same bits
    D, I = km.assign(xs)
    assert np.array_equal(I, composed_assign(xs, want_c))


def composed_assign(x, c):
    flat = vlq.GpuFlat(x.shape[1])
    flat.add(c)
    return flat.search(x, 1)[1][:, 0]
