"""k-means on the device at the edges of its update plan (csrc/kmeans_plan.h; tests/test_train_plans.py holds the same shapes against
the header on the CPU): chain lengths around the id batch (256) and the unroll (8) in both update kernels, widths around the
64-component slice and the four-wave workgroup, the sort key's bit counts, and the objective kernels' second strided trip.
GpuKMeans.update against its restatement (kmeans_ref.py), bit for bit."""
import numpy as np
import pytest

import kmeans_ref as ref
import knn_ref
import vector_line_quantization_amd as vlq
from test_gpu_pca_train import on_device
from test_gpu_pq_train import composed

pytestmark = pytest.mark.gpu
F32 = np.float32
# rows of cluster c: nothing, one, around the unroll, around one id batch (and its unroll remainder), around two batches
COUNTS = [0, 1, 7, 8, 9, 255, 256, 257, 263, 264, 512, 513]


def info_of(h):
    return dict(kv.split("=", 1) for kv in h.last_info().split())


def labels(rng, what, k, n):
    if what == "counts":                # the rows of a cluster spread over a permutation: ascending row order is the sort's doing
        assert k == len(COUNTS) and n == sum(COUNTS)
        return np.repeat(np.arange(k), COUNTS)[rng.permutation(n)].astype(np.int64)
    return rng.integers(0, k, n).astype(np.int64)


N_COUNTS = sum(COUNTS)                  # 2345
# (d, k, n, labels): kernel, waves, slices, key_bits
UPDATE_CASES = [
    ((5, 12, N_COUNTS, "counts"), ("kmeans_update_packed_kernel", 4, 0, 16)),
    ((63, 12, N_COUNTS, "counts"), ("kmeans_update_packed_kernel", 4, 0, 16)),
    ((64, 12, N_COUNTS, "counts"), ("kmeans_update_kernel", 1, 1, 16)),
    ((130, 12, N_COUNTS, "counts"), ("kmeans_update_kernel", 3, 3, 16)),
    ((63, 9, 700, "any"), ("kmeans_update_packed_kernel", 4, 0, 14)),
    ((256, 9, 700, "any"), ("kmeans_update_kernel", 4, 4, 14)),
    ((257, 9, 700, "any"), ("kmeans_update_kernel", 4, 5, 14)),           # grid.y = 2: one live lane in the second workgroup
    ((300, 9, 700, "any"), ("kmeans_update_kernel", 4, 5, 14)),
    ((4, 256, 1024, "any"), ("kmeans_update_packed_kernel", 4, 0, 18)),   # 10 row bits + 8
    ((4, 257, 1025, "any"), ("kmeans_update_packed_kernel", 4, 0, 20)),   # 11 row bits + 9
    ((8, 1, 1000, "any"), ("kmeans_update_packed_kernel", 4, 0, 10)),     # one cluster: no centroid bits in the key
    ((3, 2, 2, "any"), ("kmeans_update_packed_kernel", 4, 0, 2)),         # n - 1 = 1
]


def case_data(d, k, n, what):
    rng = np.random.default_rng(d * 100000 + k * 10 + n)
    return (100 * rng.standard_normal((n, d))).astype(F32), labels(rng, what, k, n)


@pytest.mark.parametrize("shape,plan", UPDATE_CASES)
def test_update_step_bits(shape, plan):
    d, k, n, what = shape
    x, a = case_data(d, k, n, what)
    want_c, want_count, want_nsplit = ref.update(x, a, k)
    km = vlq.GpuKMeans(d, k)
    c, count, nsplit = km.update(x, a)
    info = info_of(km)
    print(info, "nsplit", nsplit, want_nsplit)
    assert (info["kernel"], int(info["waves"]), int(info["slices"]), int(info["key_bits"])) == plan and int(info["n"]) == n
    assert nsplit == want_nsplit
    assert np.array_equal(count, want_count)
    assert knn_ref.same_bits(c, want_c)
    if what == "counts":
        assert np.array_equal(np.bincount(a, minlength=k), COUNTS) and nsplit == 1


def test_update_of_device_rows_and_labels():
    d, k, n, what = 130, 12, N_COUNTS, "counts"
    x, a = case_data(d, k, n, what)
    km = vlq.GpuKMeans(d, k)
    c, count, nsplit = km.update(x, a)
    cd, countd, nsplitd = km.update(on_device(x), on_device(a))
    assert info_of(km)["kernel"] == "kmeans_update_kernel"                 # (synchronises the stream)
    assert cd.is_cuda and countd.is_cuda and nsplitd == nsplit
    assert knn_ref.same_bits(cd.cpu().numpy(), c) and np.array_equal(countd.cpu().numpy(), count)


@pytest.fixture(scope="module")
def many_rows():
    """more rows than one trip of the objective kernels' 128 x 256 strided chains, few enough that nothing is subsampled"""
    n = 33000
    assert 128 * 256 < n <= 130 * 256
    return (np.random.default_rng(33).standard_normal((n, 8)) * 2 + 1).astype(F32)


def test_objective_second_trip(many_rows):
    x = np.ascontiguousarray(many_rows[:, :4])
    n, k = x.shape[0], 130
    init = x[np.random.default_rng(34).permutation(n)[:k]].copy()
    km = vlq.GpuKMeans(4, k, niter=1)
    km.train(x, init=init)
    assert int(info_of(km)["n"]) == n                   # no subsample
    flat = vlq.GpuFlat(4)
    flat.add(init)
    want = flat.search(x, 1)[0].astype(np.float64).sum()
    # non-negative terms in a fixed order the test does not know: the bound of any double summation order, for both sums
    print(km.obj[0], want, abs(km.obj[0] - want) / want)
    assert km.obj.shape == (1,) and abs(km.obj[0] - want) <= n * 2.0 ** -52 * want


def test_batched_objective_second_trip(many_rows):
    """kmeans_objective_batch_kernel: a slice's objective is its GpuKMeans run's, exactly.  ksub 128 subsamples above 128 * 256 =
    32 768 rows at the default 256 points per centroid, so both sides take 512: all 33 000 rows are trained on."""
    x = many_rows
    n = x.shape[0]
    kw = dict(niter=1, max_points_per_centroid=512)
    tr = vlq.GpuPQTrainer(8, 2, 7, **kw)
    c = tr.train(x)
    info = tr.last_info()
    print(info)
    assert " n=%d " % n in info and " route=batched " in " " + info and " grid=258x1 " in info
    want_c, want_obj = composed(x, 2, 7, **kw)
    assert tr.obj.shape == (2, 1) and np.array_equal(tr.obj, want_obj) and knn_ref.same_bits(c, want_c)
