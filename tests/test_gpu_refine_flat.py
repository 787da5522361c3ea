"""GPU: IndexRefineFlat on the device (csrc/refine_flat.hip; include/vlq_ivfpq.h: vlq_flat_compute_distance_subset,
vlq_flat_refine; vlq.GpuRefineFlat).

  seam against the reference     every fixture of tests/golden/refineflat (the reference's IndexRefineFlat over its own base
                                 index): refine on the reference's shortlist equals its D / I by assert_same_topk, no query
                                 left out; compute_distance_subset equals sub_D bit for bit, skipped entries untouched
  seam against the restatement   random data at the shapes where the kernel can go wrong (tests/refineflat_ref.py): every bit and
                                 every label, since the order (distance, shortlist position) is the defined one
  whole search                   GpuRefineFlat over GpuIVFPQ and GpuIVFFlat built from the fixture's index
  errors                         a label == ntotal is never dereferenced: VLQ_ERR_INVALID, and the next call is clean
"""
import glob
import os

import numpy as np
import pytest

import refineflat_ref as rr
import vector_line_quantization_amd as vlq
from util import GOLDEN, assert_same_topk

pytestmark = pytest.mark.gpu

DIR = os.path.join(GOLDEN, "refineflat")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))
WHOLE = [n for n in ("l2_ivfpq_d32", "ip_ivfflat_d32", "padded", "padded_ip", "kfactor_1") if n in FIXTURES]
METRIC = {0: "ip", 1: "l2"}
VLQ_ERR_INVALID, VLQ_ERR_UNSUPPORTED = 1, 3

K_BASES = (1, 2, 63, 64, 65, 128, 255, 256, 257, 1024)
DIMS = (1, 3, 4, 5, 28, 31, 32, 33, 36, 128, 132, 200)
NB = 300          # stored vectors of the random cases
NROW = 33


def load(name):
    z = np.load(os.path.join(DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def flat_of(xb, metric):
    g = vlq.GpuFlat(xb.shape[1], metric=metric)
    g.add(xb)
    return g


def test_fixtures_exist():
    want = {"l2_ivfpq_d32", "ip_ivfflat_d32", "tail_d3_l2", "tail_d3_ip", "tail_d5_l2", "tail_d5_ip", "tail_d30_l2", "tail_d30_ip",
            "wide_d200_l2", "kbase_1024", "kfactor_1", "padded", "padded_ip", "ties"}
    assert want <= set(FIXTURES), sorted(want - set(FIXTURES))


# ------------------------------------------------------------------------------------------------------------------------------
# seam against the reference
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_seam_against_reference(name):
    z = load(name)
    metric = METRIC[int(z["metric"])]
    k = int(z["k"])
    g = flat_of(z["xb"], metric)
    D, I = g.refine(z["xq"], z["base_D"], z["base_I"], k)
    loose = assert_same_topk(D, I, z["D"], z["I"], name)
    if name != "ties":
        assert loose == 0
    sub = z["base_D"].copy()
    g.compute_distance_subset(z["xq"], z["base_I"], sub)
    assert rr.same_bits(sub, z["sub_D"]), "compute_distance_subset differs from the reference"
    skipped = z["base_I"] < 0
    assert rr.same_bits(sub[skipped], z["base_D"][skipped])
    if name in ("padded", "padded_ip"):
        assert skipped.any()
    if name == "kfactor_1":         # the in-place form
        D2, I2 = z["base_D"].copy(), z["base_I"].copy()
        g.refine(z["xq"], D2, I2, k, D2, I2)
        assert_same_topk(D2, I2, z["D"], z["I"], name + " in place")


# ------------------------------------------------------------------------------------------------------------------------------
# seam against the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def shortlist(rng, k_base, nb=NB, nrow=NROW):
    """[nrow][k_base] labels and incoming distances; row r follows pattern r % 5:
    0 labels 0 and ntotal - 1 in front; 1 the same label twice in a row (everywhere); 2 -1 entries interleaved with live ones;
    3 a row that is entirely -1; 4 plain random.  Every entry carries an arbitrary finite incoming distance."""
    lab = rng.integers(0, nb, (nrow, k_base)).astype(np.int64)
    for r in range(nrow):
        p = r % 5
        if p == 0:
            lab[r, 0] = 0
            lab[r, -1] = nb - 1
        elif p == 1:
            lab[r, 1::2] = lab[r, 0:k_base - 1:2][:lab[r, 1::2].size]
        elif p == 2:
            lab[r, rng.random(k_base) < 0.4] = -1
            lab[r, 0] = -1
        elif p == 3:
            lab[r] = -1
    dis = (rng.standard_normal((nrow, k_base)) * 10).astype(np.float32)
    return lab, dis


def rows_of(nq):
    """which rows of the 33 a call of nq queries takes: one query sees the interleaved row, two the all -1 row and a plain one"""
    return {1: slice(2, 3), 2: slice(3, 5), 33: slice(0, 33)}[nq]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("d", DIMS)
def test_seam_against_restatement(d, metric):
    rng = np.random.default_rng(1000 + d)
    xb = rng.standard_normal((NB, d)).astype(np.float32)
    xq = rng.standard_normal((NROW, d)).astype(np.float32)
    g = flat_of(xb, metric)
    for k_base in K_BASES:
        lab, dis = shortlist(rng, k_base)
        sub = rr.compute_distance_subset(xb, xq, lab, dis, metric)
        for nq in (1, 2, 33):
            rows = rows_of(nq)
            got = dis[rows].copy()
            g.compute_distance_subset(xq[rows], lab[rows], got)
            assert rr.same_bits(got, sub[rows]), (d, metric, k_base, nq, "subset")
            for k in sorted({1, k_base // 2 + 1, k_base}):
                Dw, Iw = rr.reorder(sub[rows], lab[rows], k, metric)
                D, I = g.refine(xq[rows], dis[rows], lab[rows], k)
                assert rr.same_bits(D, Dw), (d, metric, k_base, nq, k)
                assert np.array_equal(I, Iw), (d, metric, k_base, nq, k)
        assert "slots=%d" % max(64, 1 << (k_base - 1).bit_length()) in g.last_refine_info()
    assert ("read=tile128" if d % 4 == 0 else "read=dword") in g.last_refine_info()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_device_rows_and_in_place(metric):
    import torch
    d, k_base = 36, 130
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((NB, d)).astype(np.float32)
    xq = rng.standard_normal((NROW, d)).astype(np.float32)
    lab, dis = shortlist(rng, k_base)
    g = flat_of(xb, metric)
    Dw, Iw = rr.refine(xb, xq, dis, lab, k_base, metric)
    dev = torch.device("cuda", 0)
    xq_d, D_d, I_d = torch.from_numpy(xq).to(dev), torch.from_numpy(dis).to(dev), torch.from_numpy(lab).to(dev)
    torch.cuda.synchronize()
    D, I = g.refine(xq_d, D_d, I_d, 7)
    assert D.is_cuda and I.is_cuda
    assert rr.same_bits(D.cpu().numpy(), Dw[:, :7]) and np.array_equal(I.cpu().numpy(), Iw[:, :7])
    g.refine(xq_d, D_d, I_d, k_base, D_d, I_d)          # k == k_base: D / I are base_D / base_I
    assert rr.same_bits(D_d.cpu().numpy(), Dw) and np.array_equal(I_d.cpu().numpy(), Iw)
    Dh, Ih = dis.copy(), lab.copy()
    g.refine(xq, Dh, Ih, k_base, Dh, Ih)
    assert rr.same_bits(Dh, Dw) and np.array_equal(Ih, Iw)
    sub_d = torch.from_numpy(dis).to(dev)
    torch.cuda.synchronize()
    g.compute_distance_subset(xq_d, torch.from_numpy(lab).to(dev), sub_d)
    assert rr.same_bits(sub_d.cpu().numpy(), rr.compute_distance_subset(xb, xq, lab, dis, metric))


def test_crosses_a_query_page():
    nq, k_base, d = 32769, 2, 4
    rng = np.random.default_rng(9)
    xb = rng.standard_normal((NB, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    lab = rng.integers(0, NB, (nq, k_base)).astype(np.int64)
    lab[::7, 0] = -1
    dis = (rng.standard_normal((nq, k_base)) * 3).astype(np.float32)
    g = flat_of(xb, "l2")
    for k in (1, 2):
        D, I = g.refine(xq, dis, lab, k)
        Dw, Iw = rr.refine(xb, xq, dis, lab, k, "l2")
        assert rr.same_bits(D, Dw) and np.array_equal(I, Iw)
    assert "page=32768" in g.last_refine_info()


def test_empty_store_all_skipped():
    g = vlq.GpuFlat(8, metric="l2")
    lab = np.full((3, 5), -1, np.int64)
    dis = np.arange(15, dtype=np.float32).reshape(3, 5)[:, ::-1].copy()
    D, I = g.refine(np.zeros((3, 8), np.float32), dis, lab, 2)
    assert np.array_equal(D, np.sort(dis, axis=1)[:, :2]) and (I == -1).all()


# ------------------------------------------------------------------------------------------------------------------------------
# whole search
# ------------------------------------------------------------------------------------------------------------------------------
def base_of(z, empty=False):
    metric = METRIC[int(z["metric"])]
    d, nlist = int(z["xb"].shape[1]), int(z["nlist"])
    if int(z["base_kind"]) == 0:
        g = vlq.GpuIVFPQ(d, nlist, int(z["M"]), int(z["nbits"]), metric=metric)
        g.set_coarse_centroids(z["coarse_centroids"])
        g.set_pq_centroids(z["pq_centroids"])
        g.set_search_options(by_residual=True, use_precomputed_table=min(int(z["table_mode"][0]), 1))
        if not empty:
            g.set_lists(z["codes"], z["ids"], z["list_offsets"])
    else:
        g = vlq.GpuIVFFlat(d, nlist, metric=metric)
        g.set_coarse_centroids(z["coarse_centroids"])
        if not empty:
            g.set_lists(z["vecs"], z["ids"], z["list_offsets"])
    return g


@pytest.mark.parametrize("name", WHOLE)
def test_whole_search(name):
    import torch
    z = load(name)
    metric = METRIC[int(z["metric"])]
    k, nprobe, xq, xb = int(z["k"]), int(z["nprobe"]), z["xq"], z["xb"]
    r = vlq.GpuRefineFlat(base_of(z))
    with pytest.raises(ValueError, match="store"):
        r.search(xq, k, nprobe)                 # lists set, no matching store yet: labels are not store positions
    r.set_store(xb)
    r.k_factor = float(z["k_factor"])
    kb = rr.k_base(k, r.k_factor)
    assert kb == z["base_I"].shape[1]
    D, I = r.search(xq, k, nprobe)
    # rows whose shortlist does not depend on the base's heap history: the reference's rows
    free = z["boundary_tie"] == 0
    assert free.sum() * 4 >= 3 * free.size
    assert_same_topk(D[free], I[free], z["D"][free], z["I"][free], name)
    # every row: the restatement fed the device's own first stage
    bD, bI = r.base.search(xq, nprobe, kb)
    Dw, Iw = rr.refine(xb, xq, bD, bI, k, metric)
    assert rr.same_bits(D, Dw) and np.array_equal(I, Iw)
    # device inputs
    xq_d = torch.from_numpy(xq).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    Dd, Id = r.search(xq_d, k, nprobe)
    assert Dd.is_cuda and rr.same_bits(Dd.cpu().numpy(), D) and np.array_equal(Id.cpu().numpy(), I)
    # add on the device, then the same search
    r2 = vlq.GpuRefineFlat(base_of(z, empty=True))
    r2.k_factor = r.k_factor
    half = xb.shape[0] // 2
    r2.add(xb[:half])
    r2.add(xb[half:], np.arange(half, xb.shape[0], dtype=np.int64))
    assert r2.ntotal == xb.shape[0] == r2.base.ntotal
    D2, I2 = r2.search(xq, k, nprobe)
    assert_same_topk(D2, I2, D, I, name + " after add")
    with pytest.raises(ValueError, match="sequential"):
        r2.add(xb[:2], np.array([5, 6], np.int64))
    r2.reset()
    assert r2.ntotal == 0 and r2.base.ntotal == 0


def test_refine_over_flat_and_pq_bases():
    rng = np.random.default_rng(3)
    xb = rng.standard_normal((500, 16)).astype(np.float32)
    xq = rng.standard_normal((25, 16)).astype(np.float32)
    r = vlq.GpuRefineFlat(vlq.GpuFlat(16, metric="l2"))
    r.k_factor = 3.0
    r.add(xb)
    D, I = r.search(xq, 5)
    bD, bI = r.base.search(xq, 15)
    Dw, Iw = rr.refine(xb, xq, bD, bI, 5, "l2")
    assert rr.same_bits(D, Dw) and np.array_equal(I, Iw)
    # ... and over a GpuPQ: a shortlist of approximate distances, re-ranked by the exact ones
    base = vlq.GpuPQ(16, 4, 8)
    base.set_centroids((0.6 * rng.standard_normal((4, 256, 4))).astype(np.float32))
    r = vlq.GpuRefineFlat(base)
    r.k_factor = 3.0
    r.add(xb[:300])
    r.add(xb[300:])
    assert r.ntotal == 500 == base.ntotal
    D, I = r.search(xq, 5)
    bD, bI = base.search(xq, 15)
    assert not np.array_equal(bI[:, :5], I), "the PQ order is not the exact order: the re-ranking shows"
    Dw, Iw = rr.refine(xb, xq, bD, bI, 5, "l2")
    assert rr.same_bits(D, Dw) and np.array_equal(I, Iw)
    exact = vlq.GpuFlat(16)
    exact.add(xb)
    De, Ie = exact.search(xq, 5)
    assert (I[:, 0] == Ie[:, 0]).mean() >= 0.5, "the best of 15 PQ candidates is the true neighbour for most queries"


# ------------------------------------------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    rng = np.random.default_rng(4)
    xb = rng.standard_normal((40, 8)).astype(np.float32)
    xq = rng.standard_normal((3, 8)).astype(np.float32)
    g = flat_of(xb, "l2")
    lab = rng.integers(0, 40, (3, 6)).astype(np.int64)
    dis = np.zeros((3, 6), np.float32)
    bad = lab.copy()
    bad[1, 4] = 40                                  # == ntotal: never dereferenced
    with pytest.raises(vlq.VlqError) as e:
        g.refine(xq, dis, bad, 3)
    assert e.value.code == VLQ_ERR_INVALID
    with pytest.raises(vlq.VlqError) as e:
        g.compute_distance_subset(xq, bad, dis.copy())
    assert e.value.code == VLQ_ERR_INVALID
    D, I = g.refine(xq, dis, lab, 3)                # a following valid call succeeds
    Dw, Iw = rr.refine(xb, xq, dis, lab, 3, "l2")
    assert rr.same_bits(D, Dw) and np.array_equal(I, Iw)
    with pytest.raises(vlq.VlqError) as e:          # k > k_base
        g.refine(xq, dis, lab, 7)
    assert e.value.code == VLQ_ERR_INVALID
    with pytest.raises(vlq.VlqError) as e:          # k_base > VLQ_MAX_K
        g.refine(xq, np.zeros((3, 1025), np.float32), np.zeros((3, 1025), np.int64), 3)
    assert e.value.code == VLQ_ERR_INVALID
    with pytest.raises(vlq.VlqError) as e:          # aliased outputs with k < k_base
        g.refine(xq, dis, lab, 3, dis, lab)
    assert e.value.code == VLQ_ERR_INVALID
    r = vlq.GpuRefineFlat(vlq.GpuFlat(8, metric="l2"))
    r.add(xb)
    r.k_factor = 0.5
    with pytest.raises(ValueError, match="k_factor"):
        r.search(xq, 4)
    r.k_factor = 300.0
    with pytest.raises(ValueError, match="k_base"):
        r.search(xq, 4)
    with pytest.raises(ValueError, match="store_pairs"):
        r.search(xq, 4, store_pairs=True)
    with pytest.raises(TypeError):
        vlq.GpuRefineFlat(object())
