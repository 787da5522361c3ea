"""GpuMoments and train_pca on the device against numpy in float64.  The tolerance is derived, not tuned: for any summation
order of fp32 products, fused or not, |fl(sum a_i b_i) - sum a_i b_i| <= gamma * sum |a_i| |b_i| with
gamma = (n + 2) u / (1 - (n + 2) u), u = 2^-24; the double-precision join of the slices' partials only tightens it."""
import numpy as np
import pytest

import vector_line_quantization_amd as vlq

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def gamma(n):
    return (n + 2) * 2.0 ** -24 / (1 - (n + 2) * 2.0 ** -24)


def on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def check_moments(x, y, center, mean_x, mean_y, C):
    """the bounds of the module docstring; the centring rounding is shared: Xc is formed in fp32 from the device's mean"""
    n = x.shape[0]
    ops = []
    for v, mean in ((x, mean_x),) + (() if y is None else ((y, mean_y),)):
        assert np.all(np.abs(mean.astype(F64) - v.astype(F64).mean(0)) <= gamma(n) * np.abs(v).astype(F64).mean(0))
        ops.append(((v - mean) if center else v).astype(F32).astype(F64))
    xc, yc = ops[0], ops[-1]
    err, bound = np.abs(C.astype(F64) - xc.T @ yc), gamma(n) * (np.abs(xc).T @ np.abs(yc))
    assert np.all(err <= bound), "worst element misses its bound by a factor %g" % np.max(err / np.maximum(bound, 1e-300))
    if y is None:
        assert np.array_equal(C, C.T)


# (n, dx, dy): one row | d % 4 != 0, one partial strip | a full tile against a half tile | two column tiles a side, off-diagonal
# pairs and the mirror, ragged last tile and strip | S >= 3 with a short last slice
SHAPES = [(1, 4, 4), (33, 30, 30), (1000, 128, 64), (4099, 200, 130), (70001, 130, 130)]


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n,dx,dy", SHAPES)
def test_moments(n, dx, dy, symmetric, center):
    rng = np.random.default_rng(n + dx)
    x = (rng.standard_normal((n, dx)) + 100).astype(F32)
    y = None if symmetric else (rng.standard_normal((n, dy)) + 100).astype(F32)
    mom = vlq.GpuMoments(dx, 0 if symmetric else dy)
    xd, yd = on_device(x), None if symmetric else on_device(y)
    out = [mom.compute(xd, yd, center=center) for _ in range(2)]
    info = dict(kv.split("=", 1) for kv in mom.last_info().split())       # (synchronises the stream)
    (mx, my, C), again = [[None if o is None else o.cpu().numpy() for o in res] for res in out]
    check_moments(x, y, center, mx, my, C)
    assert C.shape == (dx, dx if symmetric else dy) and info["kernel"] == "moment_kernel"
    if n == 70001:
        S, slice_len = int(info["S"]), int(info["slice_len"])
        assert S >= 3 and 0 < n - (S - 1) * slice_len < slice_len
    for a, b in zip((mx, my, C), again):          # two calls, the same bits
        assert a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_moments_host_rows_cross_a_page():
    n, d = 70001, 130                  # three pages of 32 768 rows: the partials are carried across them
    x = (np.random.default_rng(5).standard_normal((n, d)) + 100).astype(F32)
    mom = vlq.GpuMoments(d)
    mx, my, C = mom.compute(x)
    assert my is None and isinstance(C, np.ndarray) and "pages=3" in mom.last_info()
    check_moments(x, None, True, mx, None, C)


@pytest.fixture(scope="module")
def spectrum():
    """x = z diag(s) Q + 10 with a separated spectrum, and its float64 covariance of the rows centred in fp32"""
    rng = np.random.default_rng(40)
    n, d = 5000, 40
    q, _r = np.linalg.qr(rng.standard_normal((d, d)))
    x = ((rng.standard_normal((n, d)) * 2.0 ** (-np.arange(d) / 4)) @ q + 10).astype(F32)
    pca = vlq.train_pca(x, d)
    xc = (x - pca.mean).astype(F32).astype(F64)
    return x, pca, xc.T @ xc, gamma(n) * np.linalg.norm(np.abs(xc).T @ np.abs(xc))


def test_train_pca_spectrum(spectrum):
    x, pca, C64, E = spectrum
    w = np.linalg.eigh(C64)[0][::-1]
    lam = pca.eigenvalues.astype(F64)
    assert np.all(np.abs(lam - w) <= E + 1e-9 * w[0])                     # Weyl
    resid = np.linalg.norm(pca.PCAMat.astype(F64) @ C64 - lam[:, None] * pca.PCAMat, axis=1)
    assert np.all(resid <= E + 1e-5 * w[0]), resid.max()


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("eigen_power", [0.0, -0.5])
def test_train_pca_A_and_b(spectrum, eigen_power, rotate):
    x, full, _C64, _E = spectrum
    n, d_in = x.shape
    pca = vlq.train_pca(x, 16, eigen_power=eigen_power, random_rotation=rotate)
    A = pca.A.astype(F64)
    assert A.shape == (16, d_in) and np.array_equal(pca.eigenvalues, full.eigenvalues)
    assert np.all(np.abs(pca.b + A @ pca.mean) <= gamma(d_in) * (np.abs(A) @ np.abs(pca.mean)))
    if eigen_power == 0:
        assert pca.is_orthonormal and np.all(np.abs(A @ A.T - np.eye(16)) <= d_in * 2.0 ** -23)
    else:                              # whitening: the eigenvalues are sums, so every output component has variance 1 / n
        assert np.allclose(n * pca.apply(x).astype(F64).var(axis=0), 1.0, rtol=1e-3, atol=0)


def test_train_pca_balanced_bins(spectrum):
    x, _full, _C64, _E = spectrum
    plain, bal = vlq.train_pca(x, 16), vlq.train_pca(x, 16, balanced_bins=4)
    accu, counter, order = np.zeros(4, F32), [0] * 4, [None] * 16
    for i in range(16):                # the reference's greedy loop (VectorTransform.cpp:500-515)
        j = min((b for b in range(4) if counter[b] < 4), key=lambda b: accu[b])
        order[j * 4 + counter[j]] = i
        accu[j] += plain.eigenvalues[i]
        counter[j] += 1
    assert sorted(order) != order and np.array_equal(bal.A, plain.A[order])


def test_pretransform_over_trained_pca(spectrum):
    x = spectrum[0]
    pca = vlq.train_pca(x, 16)
    pre, flat = vlq.GpuPreTransform([pca], vlq.GpuFlat(16)), vlq.GpuFlat(16)
    pre.add(x)
    flat.add(pca.apply(x))
    (D, I), (Dr, Ir) = pre.search(x[:100], 5), flat.search(pca.apply(x[:100]), 5)
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)) and np.array_equal(I, Ir)


def test_train_pca_needs_d_in_rows():
    with pytest.raises(ValueError, match="at least d_in"):
        vlq.train_pca(np.zeros((10, 16), F32), 4)
