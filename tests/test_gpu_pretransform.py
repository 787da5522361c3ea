"""The vector transforms and GpuPreTransform on the device against their restatement (transform_ref.py), bit for bit."""
import numpy as np
import pytest

import transform_ref as tr
import vector_line_quantization_amd as vlq

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def info(t):
    return dict(kv.split("=", 1) for kv in t.last_info().split() if "=" in kv)


def plan():
    """the strip height, the small-batch threshold and the residency limit, read from a transform's plan of a full page"""
    i = info(vlq.GpuLinearTransform(8, 8, np.eye(8, dtype=F32)))
    return int(i["rows"]), int(i["small_n"]), int(i["max_resident_d"])


def on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def to_host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def draw(rng, shape, ints):
    if ints:        # small integers times a power of two: every product and sum is exact, a wrong element is a wrong value
        return (rng.integers(-8, 9, shape) * 0.125).astype(F32)
    return rng.standard_normal(shape).astype(F32)


SHAPES = [(1, 1), (3, 5), (7, 64), (64, 7), (33, 31), (128, 128), (128, 64), (96, 160), (130, 40), ("K+4", 33)]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_linear_apply_bits(shape, bias):
    strip, small_n, max_res = plan()
    d_in, d_out = (max_res + 4 if shape[0] == "K+4" else shape[0]), shape[1]
    ints = shape == (33, 31)
    rng = np.random.default_rng(d_in * 1000 + d_out)
    ns = [1, 3, small_n, small_n + 1, 31, 33, strip - 1, strip + 1, 2 * strip + 5]
    x, A = draw(rng, (max(ns), d_in), ints), draw(rng, (d_out, d_in), ints)
    b = draw(rng, (d_out,), ints) if bias else None
    if ints:
        x[2] = 0        # a zero row under a bias of -0.0f: the chain keeps the sign of its start
        if bias:
            b[0] = F32(-0.0)
    want = tr.linear(x, A, b)
    # the definition itself against the float64 product, within d_in rounding steps of the absolute sum
    exact = x.astype(np.float64) @ A.astype(np.float64).T + (0 if b is None else b.astype(np.float64))
    bound = d_in * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(A).astype(np.float64).T + (0 if b is None else np.abs(b)))
    assert (np.abs(want - exact) <= bound).all()
    t = vlq.GpuLinearTransform(d_in, d_out, A, b)
    x_d = on_device(x)
    kernels = set()
    for n in ns:
        assert bits_equal(t.apply(x[:n]), want[:n]), "host rows, n=%d" % n
        kernels.add(info(t)["kernel"])
        assert bits_equal(to_host(t.apply(x_d[:n])), want[:n]), "device rows, n=%d" % n
    strip_kernel = "linear_strip_kernel<%s>" % ("true" if d_in <= max_res else "false")
    assert kernels == {"linear_rows_kernel", strip_kernel}


def test_linear_apply_beyond_a_page():
    rng = np.random.default_rng(7)
    n = 32768 + 1
    x, A, b = draw(rng, (n, 8), False), draw(rng, (8, 8), False), draw(rng, (8,), False)
    assert bits_equal(vlq.GpuLinearTransform(8, 8, A, b).apply(x), tr.linear(x, A, b))


def test_rows_that_arrive_late_on_the_transforms_stream():
    """stream-ordered use: the rows are still being written on a non-blocking stream when apply is called on that stream"""
    import torch
    rng = np.random.default_rng(8)
    n = 20000
    x, A = draw(rng, (n, 64), False), draw(rng, (48, 64), False)
    t = vlq.GpuLinearTransform(64, 48, A)
    s = torch.cuda.Stream()
    t.set_stream(s.cuda_stream)
    x_pinned = torch.from_numpy(x).pin_memory()
    with torch.cuda.stream(s):
        x_d = torch.zeros((n, 64), dtype=torch.float32, device="cuda")
        for _ in range(20):         # work ahead of the rows on the same stream
            x_d.add_(1.0)
        x_d.copy_(x_pinned, non_blocking=True)
        out = t.apply(x_d)
    s.synchronize()
    assert bits_equal(out.cpu().numpy(), tr.linear(x, A))


@pytest.mark.parametrize("d_in,d_out,bias", [(48, 48, False), (40, 24, True)])
def test_linear_reverse_bits(d_in, d_out, bias):
    strip, small_n, _ = plan()
    rng = np.random.default_rng(d_out)
    A = vlq.random_rotation(d_in, d_out, seed=3)
    b = draw(rng, (d_out,), False) if bias else None
    y = draw(rng, (strip + 9, d_out), False)
    t = vlq.GpuLinearTransform(d_in, d_out, A, b, is_orthonormal=True)
    want = tr.linear_reverse(y, A, b)
    for n in (1, small_n + 1, strip + 9):
        assert bits_equal(t.reverse(y[:n]), want[:n])
        assert bits_equal(to_host(t.reverse(on_device(y[:n]))), want[:n])
    with pytest.raises(vlq.VlqError):
        vlq.GpuLinearTransform(d_in, d_out, A, b).reverse(y)


@pytest.mark.parametrize("d_in,d_out", [(5, 9), (9, 4)])
def test_remap(d_in, d_out):
    rng = np.random.default_rng(d_in)
    m = rng.integers(-1, d_in, d_out).astype(np.int32)
    m[0], m[-1] = -1, d_in - 1
    x, xt = draw(rng, (70, d_in), False), draw(rng, (70, d_out), False)
    t = vlq.GpuRemapDimensions(d_in, d_out, m)
    assert bits_equal(t.apply(x), tr.remap(x, m))
    assert bits_equal(to_host(t.reverse(on_device(xt))), tr.remap_reverse(xt, m, d_in))
    with pytest.raises(vlq.VlqError):
        vlq.GpuRemapDimensions(d_in, d_out, np.full(d_out, d_in, np.int32))


@pytest.mark.parametrize("d", [64, 30, 3])
def test_l2norm(d):
    x = draw(np.random.default_rng(d), (67, d), False)
    x[5] = 0
    t = vlq.GpuNormalization(d)
    assert bits_equal(t.apply(x), tr.l2norm(x))
    assert bits_equal(to_host(t.apply(on_device(x))), tr.l2norm(x))
    assert bits_equal(t.reverse(x), x)


def make_base(kind, d, xb):
    if kind == "flat":
        return vlq.GpuFlat(d)
    rng = np.random.default_rng(11)
    g = vlq.GpuIVFPQ(d, 16, 4, 8)
    g.set_coarse_centroids(np.ascontiguousarray(xb[:16]))
    g.set_pq_centroids(rng.standard_normal((4, 256, d // 4)).astype(F32))
    return vlq.GpuRefineFlat(g) if kind == "refine" else g


def make_chain(which, rng):
    """(transforms, their restatement, d of the rows that go in)"""
    if which == "rotation":
        A, b = vlq.random_rotation(32, 32, seed=9), draw(rng, (32,), False)
        return [vlq.GpuLinearTransform(32, 32, A, b, is_orthonormal=True)], (lambda x: tr.linear(x, A, b)), 32
    A, b = (draw(rng, (32, 64), False) * F32(0.125)), draw(rng, (32,), False)
    return [vlq.GpuLinearTransform(64, 32, A, b), vlq.GpuNormalization(32)], (lambda x: tr.l2norm(tr.linear(x, A, b))), 64


@pytest.mark.parametrize("which", ["rotation", "pca_l2norm"])
@pytest.mark.parametrize("kind", ["flat", "ivfpq", "refine"])
def test_pretransform_search(kind, which):
    rng = np.random.default_rng(5)
    chain, restated, d = make_chain(which, rng)
    xb, xq = draw(rng, (300, d), False), draw(rng, (40, d), False)
    xb_t, xq_t = restated(xb), restated(xq)
    bare, p = make_base(kind, 32, xb_t), vlq.GpuPreTransform(chain, make_base(kind, 32, xb_t))
    assert p.d == d
    bare.add(xb_t)
    p.add(xb)
    assert p.ntotal == 300
    for nq in (1, 40):
        if kind == "flat":
            D0, I0 = bare.search(xq_t[:nq], 5)
        elif kind == "ivfpq":
            D0, I0 = bare.search(xq_t[:nq], 4, 5)
        else:
            D0, I0 = bare.search(xq_t[:nq], 5, 4)
        D, I = p.search(xq[:nq], 5, nprobe=4)
        assert bits_equal(D, D0) and np.array_equal(I, I0)
        Dd, Id = p.search(on_device(xq[:nq]), 5, nprobe=4)
        assert Dd.is_cuda and bits_equal(to_host(Dd), D0) and np.array_equal(to_host(Id), I0)


def test_pretransform_reconstruct_and_chain_errors():
    rng = np.random.default_rng(6)
    A = vlq.random_rotation(32, 32, seed=2)
    rot = vlq.GpuLinearTransform(32, 32, A, is_orthonormal=True)
    p = vlq.GpuPreTransform([rot], vlq.GpuFlat(32))
    xb = draw(rng, (150, 32), False)
    p.add(xb)
    assert bits_equal(p.reconstruct_n(3, 140), tr.linear_reverse(tr.linear(xb, A)[3:143], A))
    p.reset()
    assert p.ntotal == 0
    base = vlq.GpuFlat(32)
    assert vlq.GpuPreTransform([], base) is base
    with pytest.raises(ValueError):
        vlq.GpuPreTransform([rot], vlq.GpuFlat(16))
    with pytest.raises(ValueError):
        vlq.GpuPreTransform([vlq.GpuNormalization(16), rot], vlq.GpuFlat(32))
