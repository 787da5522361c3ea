"""Product-quantizer training on the device at every branch of its plan (csrc/pq_train_plan.h; tests/test_train_plans.py holds the
same shapes against the header on the CPU): ragged and halved slice groups, every column-tile count, both loop-route reasons, the
row-tile walk, the update kernels over the in-place view.  The assignment against the flat search's restatement (knn_ref.py) per
slice, the training against M GpuKMeans runs over contiguous slice copies; everything bit for bit.  Every case asserts the
last_info() fields that prove its branch, so a later change to the plan cannot move it off the branch unnoticed.

`rest == 3` in pq_assign_kernel is unreachable (cols / 32 is 1, 2, 4 or 8) and has no case."""
import numpy as np
import pytest

import knn_ref
import vector_line_quantization_amd as vlq
from test_gpu_pca_train import on_device
from test_gpu_pq_train import composed, few_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
WHY_LDS = "why=one slice's codebook does not fit 160 KB of LDS beside the row tile"


def has(info, expect):
    for key in expect:
        assert (" " + key + " ") in (" " + info + " "), (key, info)


def check_rows(x, cb, D, I):
    """(D [M][n], I [n][M]) is the flat search of every slice; a row without a distance below FLT_MAX is labelled -1"""
    (n, _d), (M, ksub, dsub) = x.shape, cb.shape
    for m in range(M):
        Dm, Im = knn_ref.search(x[:, m * dsub:(m + 1) * dsub], cb[m], 1, "l2", nq_call=n)
        assert np.array_equal(I[:, m], np.where(Im[:, 0] < 0, -1, Im[:, 0] + m * ksub)), m
        assert knn_ref.same_bits(D[m], Dm[:, 0]), m


def check_assign(x, cb, nbits, expect_route="batched", expect=()):
    tr = vlq.GpuPQTrainer(x.shape[1], cb.shape[0], nbits)
    tr.set_centroids(cb)
    D, I = tr.assign(x)
    info = tr.last_info()
    print(info)
    has(info, ("route=" + expect_route,) + tuple(expect))
    check_rows(x, cb, D, I)
    tr.close()
    return D, I


def data(d, M, nbits, n):
    rng = np.random.default_rng(d * 1000 + M * 10 + nbits)
    x = (rng.standard_normal((n, d)) * 3 + 1).astype(F32)
    cb = (rng.standard_normal((M, 1 << nbits, d // M)) * 3 + 1).astype(F32)
    return rng, x, cb


ASSIGN_SHAPES = {                       # (d, M, nbits, n), the route, the plan fields that prove the branch
    "ragged group, vector loads": ((48, 6, 4, 300), "batched", ("group=4", "ngroups=2", "vec=1", "lds=23040", "grid=3x2")),
    "ragged group, scalar loads": ((48, 8, 3, 200), "batched", ("group=6", "ngroups=2", "vec=0", "lds=34560", "grid=2x2")),
    "dsub 1: group 32 -> 16 -> 8": ((32, 32, 8, 300), "batched", ("group=8", "ngroups=4", "kq=1", "lds=110592", "grid=3x4")),
    "dsub 2: group 16 -> 8": ((32, 16, 8, 300), "batched", ("group=8", "ngroups=2", "kq=1", "lds=110592", "grid=3x2")),
    "one column tile": ((32, 4, 5, 300), "batched", ("cols=32", "group=4", "ngroups=1", "lds=23040")),
    "two column tiles": ((32, 4, 6, 300), "batched", ("cols=64", "group=4", "ngroups=1", "lds=27648")),
    "four column tiles": ((32, 4, 7, 300), "batched", ("cols=128", "group=4", "ngroups=1", "lds=36864")),
    "the largest batched codebook": ((104, 1, 8, 300), "batched", ("kq=13", "stride=52", "lds=161280", "grid=3x1")),
    "LDS loop route, M = 1": ((105, 1, 8, 300), "loop", ("kq=14", "stride=60", "ngroups=1", "lds=0")),
    "LDS loop route, M = 2": ((224, 2, 8, 300), "loop", ("kq=14", "stride=60", "ngroups=2", "lds=0")),
    # 17 row tiles under 8 walkers: walker 0 takes tiles 0, 8 and 16, and tile 16 holds one row
    "row tiles walked": ((2048, 64, 2, 2049), "batched", ("group=1", "ngroups=64", "lds=26240", "grid=8x64")),
}


@pytest.mark.parametrize("edge", sorted(ASSIGN_SHAPES))
def test_assign_at_every_plan_branch(edge):
    (d, M, nbits, n), route, expect = ASSIGN_SHAPES[edge]
    _rng, x, cb = data(d, M, nbits, n)
    if route == "loop":
        expect += (WHY_LDS,)
    if edge == "row tiles walked":
        walkers = int([e for e in expect if e.startswith("grid=")][0][5:].split("x")[0])
        assert (n + 127) // 128 == 17 > walkers and n % 128 == 1
    check_assign(x, cb, nbits, route, expect)


def test_assign_rows_that_are_codebook_rows():
    """(|x|^2 + |c|^2) - 2 ip lands on zero or a few ulps either side of it: negative keys and -0 order as the flat search's"""
    d, M, nbits, n = 32, 4, 4, 300
    rng, _x, cb = data(d, M, nbits, n)
    cb *= F32(1000)
    x = np.concatenate([cb[m][rng.integers(0, 1 << nbits, n)] for m in range(M)], axis=1)
    D, _I = check_assign(x, cb, nbits)
    norms = np.stack([(x[:, m * 8:(m + 1) * 8].astype(np.float64) ** 2).sum(1) for m in range(M)])
    print("negative", int((D < 0).sum()), "zero", int((D == 0).sum()), "positive", int((D > 0).sum()))
    assert np.all(np.abs(D) <= 1e-5 * norms)            # every winner is a copy (up to the rounding of the three terms)
    assert (D <= 0).any()


@pytest.fixture(scope="module")
def overflowing():
    """a finite row whose slice norms overflow: no distance of it is below FLT_MAX"""
    _rng, x, cb = data(32, 4, 4, 300)
    bad = x.copy()
    bad[137] = 3e19
    return x, bad, cb


def test_assign_row_without_a_distance_below_flt_max(overflowing):
    x, bad, cb = overflowing
    D0, I0 = check_assign(x, cb, 4)
    D, I = check_assign(bad, cb, 4)                     # (knn_ref models the row: the heap admits nothing, FLT_MAX / -1)
    assert np.all(I[137] == -1) and np.all(D[:, 137] == FLT_MAX)
    keep = np.arange(300) != 137
    assert np.array_equal(I[keep], I0[keep]) and knn_ref.same_bits(D[:, keep], D0[:, keep])
    # ... and the flat index itself says the same of that row
    flat = vlq.GpuFlat(8)
    flat.add(cb[0])
    Df, If = flat.search(np.ascontiguousarray(bad[137:138, :8]), 1)
    assert If[0, 0] == -1 and Df[0, 0] == FLT_MAX


def test_assign_row_without_a_distance_on_the_loop_route():
    _rng, x, cb = data(105, 1, 8, 300)
    x[137] = 3e19
    D, I = check_assign(x, cb, 8, "loop", (WHY_LDS,))
    assert I[137, 0] == -1 and D[0, 137] == FLT_MAX and (I[np.arange(300) != 137] >= 0).all()


def test_train_row_without_a_distance_is_an_error(overflowing):
    _x, bad, _cb = overflowing
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuPQTrainer(32, 4, 4, niter=3).train(bad)
    assert e.value.code == 1 and "FLT_MAX" in str(e.value)


def test_assign_unaligned_device_rows():
    """rows that start 4 bytes past a 16-byte boundary take the 4-byte loads: the same D and I as the aligned copy"""
    import torch
    d, M, nbits, n = 32, 4, 4, 300
    _rng, x, cb = data(d, M, nbits, n)
    xa = on_device(x)
    buf = torch.empty(n * d + 4, dtype=torch.float32, device=xa.device)
    xu = buf[1:1 + n * d].view(n, d)
    xu.copy_(xa)
    torch.cuda.synchronize()
    assert xa.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    tr = vlq.GpuPQTrainer(d, M, nbits)
    tr.set_centroids(cb)
    out = []
    for rows in (xa, xu):
        D, I = tr.assign(rows)
        has(tr.last_info(), ("route=batched", "vec=1", "group=4"))       # (synchronises the stream)
        out.append((D.cpu().numpy(), I.cpu().numpy()))
    assert knn_ref.same_bits(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    check_rows(x, cb, *out[1])


TRAIN_CASES = {                         # (d, M, nbits, n), the route, the fields that prove the branch, the data
    "dsub 64: wide update, one wave": ((128, 2, 4, 600), "batched", ("update=kmeans_update_kernel", "lds=46720", "grid=5x2"), ""),
    "dsub 96: two slices": ((192, 2, 3, 300), "batched", ("update=kmeans_update_kernel", "lds=67200", "grid=3x2"), ""),
    "dsub 248: the widest batched": ((496, 2, 3, 200), "batched", ("update=kmeans_update_kernel", "kq=31", "lds=159360", "grid=2x2"), ""),
    "dsub 10: scalar loads, packed update": ((40, 4, 4, 500), "batched", ("update=kmeans_update_packed_kernel", "vec=0", "group=4", "lds=64000"), ""),
    "ragged group with splits": ((48, 6, 4, 400), "batched", ("update=kmeans_update_packed_kernel", "group=4", "ngroups=2", "grid=4x2"), "few rows"),
    "LDS loop route": ((105, 1, 8, 600), "loop", ("kq=14", "lds=0", WHY_LDS), ""),
}


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_train_at_every_plan_branch(name):
    (d, M, nbits, n), route, expect, what = TRAIN_CASES[name]
    rng = np.random.default_rng(d * 100 + n)
    x = few_rows(rng, n, d, (1 << nbits) // 2) if what == "few rows" else rng.standard_normal((n, d)).astype(F32)
    tr = vlq.GpuPQTrainer(d, M, nbits, niter=3)
    c = tr.train(x)
    info = tr.last_info()
    print(name, info)
    has(info, ("route=" + route,) + expect)
    want_c, want_obj = composed(x, M, nbits, niter=3)
    assert knn_ref.same_bits(c, want_c) and np.array_equal(tr.obj, want_obj)
    if what == "few rows":
        assert int(info.split("nsplit=")[1].split()[0]) > 0
