"""Numpy restatement of k-means' update step and the parts of Clustering::train around it, as include/vlq_ivfpq.h (vlq_kmeans_*)
specifies them.  TEST INFRASTRUCTURE ONLY.

  update     np.add.at on float32 is the sequential loop c[assign[i]] += x[i], i ascending; then c /= float32(count)
  split      the LCG s = (s * 1103515245 + 12345) & 0x7fffffff seeded 1234 on every call, p in the reference's types
  rand_perm  identity, then perm[i] <-> perm[i + rand_int() % (n - i)] for i = 0 .. n-2
  renorm     fvec_renorm_L2: x *= float32(1.0 / sqrtf(fvec_norm_L2sqr(x))) where the norm is > 0
"""
import numpy as np

from ip_ref import ip_sse

F32 = np.float32


class Lcg:
    def __init__(self, seed):
        self.s = (seed & 0xFFFFFFFF) or 1

    def rand_int(self):
        self.s = (self.s * 1103515245 + 12345) & 0x7FFFFFFF
        return self.s

    def rand_float(self):
        return F32(self.rand_int()) / F32(2.0 ** 31)


def rand_perm(n, seed):
    perm = list(range(n))
    rng = Lcg(seed)
    for i in range(n - 1):
        i2 = i + rng.rand_int() % (n - i)
        perm[i], perm[i2] = perm[i2], perm[i]
    return np.array(perm, np.int64)


def update(x, assign, k):
    """km_update_centroids: (centroids [k][d] float32, counts [k] after the splits, nsplit)"""
    n, d = x.shape
    c = np.zeros((k, d), F32)
    np.add.at(c, assign, x)
    count = np.bincount(assign, minlength=k).astype(np.int64)
    full = count > 0
    c[full] = c[full] / count[full].astype(F32)[:, None]
    rng = Lcg(1234)
    eps = 1 / 1024.
    even = np.arange(d) % 2 == 0
    nsplit = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for ci in range(k):
            if count[ci] != 0:
                continue
            cj = 0
            while True:
                p = F32((np.float64(count[cj]) - 1.0) / np.float64(F32(n - k)))
                if rng.rand_float() < p:
                    break
                cj = (cj + 1) % k
            row = c[cj].astype(np.float64)
            c[ci] = (row * np.where(even, 1 + eps, 1 - eps)).astype(F32)
            c[cj] = (row * np.where(even, 1 - eps, 1 + eps)).astype(F32)
            count[ci] = count[cj] // 2
            count[cj] -= count[ci]
            nsplit += 1
    return c, count, nsplit


def renorm(c):
    nr = ip_sse(c, c)
    out = c.copy()
    pos = nr > 0
    inv = (1.0 / np.sqrt(nr[pos]).astype(F32).astype(np.float64)).astype(F32)
    out[pos] = c[pos] * inv[:, None]
    return out
