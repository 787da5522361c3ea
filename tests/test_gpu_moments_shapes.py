"""GpuMoments and train_pca at the edges of the moments plan (csrc/moments_plan.h; tests/test_train_plans.py holds the same shapes
against the header on the CPU): tile grids that are not square, every strip height and forced slice counts, rows that do not start
on 16 bytes, host rows page by page.  Every result against numpy in float64 under the rounding bound test_gpu_pca_train.py derives
(check_moments), every call twice for the same bits."""
import numpy as np
import pytest

import kmeans_ref
import vector_line_quantization_amd as vlq
from test_gpu_pca_train import check_moments, gamma, on_device
from test_gpu_pca_train import spectrum  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def rows(n, dx, dy, seed=0):
    rng = np.random.default_rng(n + dx + seed)
    x = (rng.standard_normal((n, dx)) + 100).astype(F32)
    return x, None if dy is None else (rng.standard_normal((n, dy)) + 100).astype(F32)


def host(a):
    return None if a is None else a if isinstance(a, np.ndarray) else a.cpu().numpy()


def same_bits(a, b):
    return all(u is None or np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def run(x, y, center=True, split=None, xin=None, yin=None, expect=()):
    """two computes of one handle, checked against float64; (mean_x, mean_y, C) on the host and last_info's fields.  xin / yin:
    what is handed to the library in place of device copies of x / y"""
    mom = vlq.GpuMoments(x.shape[1], 0 if y is None else y.shape[1])
    if split is not None:
        mom.set_split(*split)
    xin = on_device(x) if xin is None else xin
    yin = (None if y is None else on_device(y)) if yin is None else yin
    out = [mom.compute(xin, yin, center=center) for _ in range(2)]
    info = dict(kv.split("=", 1) for kv in mom.last_info().split())       # (synchronises the stream)
    res, again = [[host(o) for o in r] for r in out]
    print(info)
    check_moments(x, y, center, *res)
    assert same_bits(res, again) and info["kernel"] == "moment_kernel" and int(info["n"]) == x.shape[0]
    for key, value in expect:
        assert info[key] == str(value), (key, value, info)
    mom.close()
    return res, info


# (n, dx, dy): pairs, S, slice_len.  Tiles 1 x 3 and 3 x 1 tell ta = block / tiles_y from its transpose; 129 and 127 columns: a
# second tile of one column beside a tile one column short
TWO_OPERAND = [((300, 100, 300), (3, 2, 160)), ((300, 300, 100), (3, 2, 160)), ((200, 129, 127), (2, 1, 224))]
# (n, d): six pairs (three tiles a side) | the second tile holds one column | one full tile, one slice | exactly one strip
SYMMETRIC = [((300, 300), (6, 2, 160)), ((200, 129), (3, 1, 224)), ((128, 128), (1, 1, 128)), ((32, 7), (1, 1, 32))]


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("shape,plan", TWO_OPERAND)
def test_two_operand_tile_grids(shape, plan, center):
    x, y = rows(*shape)
    (mx, my, C), _info = run(x, y, center, expect=zip(("pairs", "S", "slice_len", "kr"), plan + (32,)))
    assert C.shape == (shape[1], shape[2]) and mx.shape == (shape[1],) and my.shape == (shape[2],)


@pytest.mark.parametrize("shape,plan", SYMMETRIC)
def test_symmetric_tile_grids(shape, plan):
    x, _none = rows(shape[0], shape[1], None)
    run(x, None, expect=zip(("pairs", "S", "slice_len", "kr"), plan + (32,)))


# set_split(kr, slices) at n = 1000: (S, slice_len); S is recomputed from the slice length rounded up to kr
SPLITS = {(16, 0): (13, 80), (16, 1): (1, 1008), (16, 7): (7, 144), (16, 9): (9, 112),
          (64, 0): (3, 384), (64, 1): (1, 1024), (64, 7): (6, 192), (64, 9): (8, 128)}


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("split", sorted(SPLITS))
def test_set_split(split, symmetric):
    x, y = rows(1000, 130, None if symmetric else 130)
    S, slice_len = SPLITS[split]
    expect = dict(kr=split[0], S=S, slice_len=slice_len, pairs=3 if symmetric else 4, lds=4 * split[0] * 128 * 4)
    run(x, y, split=split, expect=expect.items())


def test_set_split_more_slices_than_strips_and_back():
    x, _none = rows(100, 40, None)
    xd = on_device(x)
    mom = vlq.GpuMoments(40)

    def compute(plan):
        out = mom.compute(xd)
        assert plan in mom.last_info()                  # (synchronises the stream: the device outputs are there)
        res = [host(o) for o in out]
        check_moments(x, None, True, *res)
        return res
    plain = compute("S=1 slice_len=128 kr=32")
    mom.set_split(32, 50)
    compute("S=4 slice_len=32 kr=32")
    mom.set_split(0, 0)                 # the default plan again: its bits
    back = compute("S=1 slice_len=128 kr=32")
    assert same_bits(plain, back)
    for kr, slices in ((8, 0), (32, 5000), (32, -1)):
        with pytest.raises(vlq.VlqError) as e:
            mom.set_split(kr, slices)
        assert e.value.code == 1


def unaligned(a):
    """a device copy of a whose base is 4 bytes past a 16-byte boundary"""
    import torch
    n, d = a.shape
    buf = torch.empty(n * d + 4, dtype=torch.float32, device=torch.device("cuda", 0))
    t = buf[1:1 + n * d].view(n, d)
    t.copy_(on_device(a))
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


@pytest.mark.parametrize("symmetric", [True, False])
def test_unaligned_device_base(symmetric):
    """d % 4 == 0 rows that do not start on 16 bytes take the scalar loads.  The load width changes neither the centring (one
    subtraction per component) nor the order of the MFMA chain, so the bits are those of the aligned call."""
    x, y = rows(257, 64, None if symmetric else 64)
    expect = dict(pairs=1, S=2, slice_len=160)
    aligned, _i = run(x, y, expect=expect.items())
    if symmetric:
        moved, _i = run(x, None, xin=unaligned(x), expect=expect.items())
    else:                               # only y unaligned
        moved, _i = run(x, y, yin=unaligned(y), expect=expect.items())
    assert same_bits(aligned, moved)


@pytest.mark.parametrize("y_on", ["host", "device"])
def test_two_operand_host_rows_cross_a_page(y_on):
    """both operands paged from the host; and host x beside device y, which for_pages and stage_in serve too: x is staged page by
    page, y is read in place at the page's offset.  Outputs follow x."""
    n, dx, dy = 32768 + 5, 20, 36
    x, y = rows(n, dx, dy)
    (mx, my, C), _info = run(x, y, xin=x, yin=y if y_on == "host" else on_device(y),
                             expect=dict(pages=2, S=256, slice_len=128, col_slices=128).items())
    assert C.shape == (dx, dy)


@pytest.mark.parametrize("n,pages", [(32768, 1), (32769, 2)])
def test_symmetric_host_rows_at_the_page_edge(n, pages):
    x, _none = rows(n, 20, None)        # 32 769: a last page of one row
    run(x, None, xin=x, expect=dict(pages=pages, S=256, slice_len=128).items())


def test_host_rows_with_strips_of_64():
    x, _none = rows(40000, 20, None)
    run(x, None, split=(64, 0), xin=x, expect=dict(pages=2, kr=64, S=128, slice_len=256).items())


def test_train_pca_subsample(spectrum):  # noqa: F811
    x = spectrum[0]
    n, d = x.shape
    assert n > 50 * d
    sub = vlq.train_pca(x, 16, max_points_per_d=50)
    want = vlq.train_pca(np.ascontiguousarray(x[kmeans_ref.rand_perm(n, 1234)[:50 * d]]), 16)
    for name in ("A", "b", "mean", "eigenvalues"):
        got, ref = getattr(sub, name), getattr(want, name)
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name
    assert not np.array_equal(sub.mean, spectrum[1].mean)


def test_train_pca_without_bias(spectrum):  # noqa: F811
    x = spectrum[0]
    n, d = x.shape
    pca = vlq.train_pca(x, d, have_bias=False)
    assert not pca.mean.any() and not pca.b.any() and pca.mean.shape == (d,) and pca.b.shape == (d,)
    x64 = x.astype(F64)
    C64, E = x64.T @ x64, gamma(n) * np.linalg.norm(np.abs(x64).T @ np.abs(x64))         # the uncentred rows
    w = np.linalg.eigh(C64)[0][::-1]
    lam = pca.eigenvalues.astype(F64)
    assert np.all(np.abs(lam - w) <= E + 1e-9 * w[0])                     # Weyl
    resid = np.linalg.norm(pca.PCAMat.astype(F64) @ C64 - lam[:, None] * pca.PCAMat, axis=1)
    assert np.all(resid <= E + 1e-5 * w[0]), resid.max()
