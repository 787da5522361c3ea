"""GPU, BASELINE config-1 sizes (1M codes, nlist=4096, M=16x8bit, nprobe=32, k=10,
10 000 queries): size-independent properties of the hot path plus an oracle check on
a sample.  Index content is synthetic (random centroids / codes): the properties hold
for any content."""
import numpy as np
import pytest

import vector_line_quantization_amd as vlq
from oracle import pyoracle
from util import FULLSIZE, FULLSIZE_REFERENCE, bits, fullsize_inputs, inputs_sha

pytestmark = pytest.mark.gpu

D_, NLIST, M, NB, NQ, NPROBE, K = (FULLSIZE[n] for n in ("d", "nlist", "M", "nb", "nq", "nprobe", "k"))


@pytest.fixture(scope="module")
def world():
    coarse, pq, codes, ids, off, xq = fullsize_inputs()
    g = vlq.GpuIVFPQ(D_, NLIST, M, 8)
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.set_lists(codes, ids, off)
    ox = pyoracle.OracleIndex(D_, NLIST, M, 8, coarse, pq, codes=codes, ids=ids, list_offsets=off)
    Dg, Ig = g.search(xq, NPROBE, K)
    return dict(g=g, ox=ox, xq=xq, D=Dg, I=Ig, off=off, ids=ids)


def test_sample_matches_oracle_bit_exact(world):
    sel = np.arange(0, NQ, 41)[:200]
    Do, Io = world["ox"].search(world["xq"][sel], NPROBE, K, canonical=True)
    assert np.array_equal(bits(world["D"][sel]), bits(Do))
    assert np.array_equal(world["I"][sel], Io)


def test_full_batch_vs_compiled_reference(world):
    """All 10 000 queries against the reference's own CPU IndexIVFPQ (oracle/_ref, built from the
    reference's sources), whose answer for these inputs is stored in tests/golden/reference/: same
    probe sets up to the BLAS coarse stage's rounding, and wherever the label agrees the distance
    agrees to 1e-4 relative (north-star tolerance) -- in practice bit for bit."""
    z = np.load(FULLSIZE_REFERENCE)
    ox = world["ox"]
    assert np.array_equal(z["inputs_sha256"], inputs_sha(ox.coarse_centroids, ox.pq_centroids, ox.codes, ox.ids,
                                                         ox.list_offsets, world["xq"])), \
        "the stored reference answer belongs to other inputs: python tests/golden/make_golden.py fullsize_c1"
    Dr, Ir, meta = z["D"], z["I"], z["meta"]
    D, I = world["D"], world["I"]
    assert meta[0] == 1
    from util import label_agreement
    # the BLAS coarse stage (MKL sgemm) may round a probe boundary differently from the k-ordered MFMA
    # chain (unpinned by construction): rows whose probe sets agree -- decided by the
    # row's distances agreeing bit for bit -- must agree in EVERY slot; the others are counted and bounded
    row_eq = (D.view(np.uint32) == Dr.view(np.uint32)).all(axis=1)
    print("rows bit-equal to the compiled reference in every distance: %d of %d (%.5f)" % (row_eq.sum(), row_eq.shape[0], row_eq.mean()))
    assert row_eq.mean() >= 0.999, row_eq.mean()
    assert label_agreement(D[row_eq], I[row_eq], Dr[row_eq], Ir[row_eq]) == 1.0
    same = I == Ir
    rel = np.abs(D[same] - Dr[same]) / np.maximum(np.abs(Dr[same]), 1e-20)
    assert rel.max() <= 1e-4                                        # north-star tolerance where labels agree


def test_host_buffers_device_buffers_and_schedules_agree(world):
    """The same 10 000 queries through host buffers (numpy in / out), through device buffers, and under
    the list-owned schedule: one answer."""
    import torch
    g, xq = world["g"], world["xq"]
    xd = torch.from_numpy(xq).cuda()
    Dd, Id = g.search(xd, NPROBE, K)
    torch.cuda.synchronize()
    assert np.array_equal(bits(Dd.cpu().numpy()), bits(world["D"])) and np.array_equal(Id.cpu().numpy(), world["I"])
    g.set_scan_schedule(2)
    try:
        Do, Io = g.search(xq, NPROBE, K)
        Dod, Iod = g.search(xd, NPROBE, 100)
        g.set_scan_schedule(1)
        Dq, Iq = g.search(xd, NPROBE, 100)
        torch.cuda.synchronize()
    finally:
        g.set_scan_schedule(0)
    assert np.array_equal(bits(Do), bits(world["D"])) and np.array_equal(Io, world["I"])
    assert torch.equal(Dod, Dq) and torch.equal(Iod, Iq)


def test_ncode_counter_matches_list_lengths(world):
    g = world["g"]
    g.stats(reset=True)
    cd, keys = g.coarse_search(world["xq"], NPROBE)
    g.search_preassigned(world["xq"], keys, cd, K)
    nq, ncode = g.stats(reset=True)
    lens = np.diff(world["off"])
    assert ncode == int(lens[keys].sum()) and nq == NQ


def test_results_do_not_depend_on_batch_composition(world):
    """Query order / batch split / paging change which queries share a workgroup
    neighbourhood and the sort order of the batch -- never a result."""
    g, xq = world["g"], world["xq"]
    perm = np.random.default_rng(1).permutation(NQ)
    Dp, Ip = g.search(xq[perm], NPROBE, K)
    assert np.array_equal(bits(Dp), bits(world["D"][perm])) and np.array_equal(Ip, world["I"][perm])
    for lo, hi in ((0, 1), (5, 24), (100, 1100), (1100, 4000)):          # 1 / <20 (direct coarse: see below) / <1024 / >=1024
        Ds, Is = g.search(xq[lo:hi], NPROBE, K)
        if hi - lo >= 20:
            assert np.array_equal(bits(Ds), bits(world["D"][lo:hi])) and np.array_equal(Is, world["I"][lo:hi])
        else:   # the reference's small-batch coarse path rounds differently (utils.cpp:935-946): labels agree
            assert (Is == world["I"][lo:hi]).mean() > 0.95


def test_smaller_k_is_a_prefix(world):
    g, xq = world["g"], world["xq"]
    D5, I5 = g.search(xq[:3000], NPROBE, 5)
    assert np.array_equal(bits(D5), bits(world["D"][:3000, :5])) and np.array_equal(I5, world["I"][:3000, :5])
    D1, I1 = g.search(xq[:3000], NPROBE, 1)
    assert np.array_equal(I1[:, 0], world["I"][:3000, 0])


def test_store_pairs_decode_to_the_same_ids(world):
    g, xq = world["g"], world["xq"][:2000]
    cd, keys = g.coarse_search(xq, NPROBE)
    D, I = g.search_preassigned(xq, keys, cd, K)
    Dp, Ip = g.search_preassigned(xq, keys, cd, K, store_pairs=True)
    assert np.array_equal(bits(D), bits(Dp))
    lst, o = Ip >> 32, Ip & 0xFFFFFFFF
    assert np.array_equal(world["ids"][world["off"][lst] + o], I)


def test_more_probes_never_hurt(world):
    g, xq = world["g"], world["xq"][:2000]
    D64, _ = g.search(xq, 64, K)
    assert (D64 <= world["D"][:2000]).all()


def test_many_lists_deep1b_shape():
    """The Deep1B driver's shape scaled down (BASELINE configs[3]: d=96 -> dsub=6, nlist 2^15 here
    instead of 2^17, M=16, nprobe=128): many short lists, per-query tables from the table kernel
    (no fused d=128 path), 32 k-row term2, select over 32 k columns, device-side add."""
    d, nlist, nb, nq, nprobe, k = 96, 32768, 300000, 1500, 128, 10
    rng = np.random.default_rng(9)
    coarse = rng.random((nlist, d), dtype=np.float32)
    pq = (rng.random((16, 256, d // 16), dtype=np.float32) - 0.5) * 0.2
    xb = (coarse[rng.integers(0, nlist, nb)] + 0.05 * rng.standard_normal((nb, d))).astype(np.float32)
    xq = (coarse[rng.integers(0, nlist, nq)] + 0.05 * rng.standard_normal((nq, d))).astype(np.float32)
    g = vlq.GpuIVFPQ(d, nlist, 16, 8)
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.add(xb[:200000])
    g.add(xb[200000:])
    assert g.ntotal == nb
    D, I = g.search(xq, nprobe, k)
    # the lists, bulk-read through the ABI, into the oracle
    lens = np.array([g.list_length(i) for i in range(nlist)], np.int64)
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    codes = np.empty((nb, 16), np.uint8)
    ids = np.empty((nb,), np.int64)
    for i in np.flatnonzero(lens):
        c, ii = g.get_list(int(i))
        codes[off[i]:off[i + 1]] = c
        ids[off[i]:off[i + 1]] = ii
    assert np.array_equal(np.sort(ids), np.arange(nb))
    ox = pyoracle.OracleIndex(d, nlist, 16, 8, coarse, pq, codes=codes, ids=ids, list_offsets=off)
    sel = np.arange(0, nq, 50)
    Do, Io = ox.search(xq[sel], nprobe, k, canonical=True)
    assert np.array_equal(bits(D[sel]), bits(Do))
    assert np.array_equal(I[sel], Io)
    # and a vector finds itself
    Ds, Is = g.search(xb[:64], nprobe, 1)
    assert (Is[:, 0] == np.arange(64)).mean() > 0.9


@pytest.mark.parametrize("k", [10, 100, 200])
def test_long_lists_wide_rows_vs_oracle(k):
    """Deep1B-like proportions at a size the oracle finishes in seconds: 16 384 lists (two-level coarse
    select from tile minima, 1-NN assignment without a matrix), lists of ~3000 codes (pipelined loop for
    every selection class), d = 96 (dsub = 6), 2 M codes with runs of identical codes (exact ties across
    chunks and waves).  Distances and labels equal to the oracle's canonical order on a query sample."""
    rng = np.random.default_rng(99 + k)
    d, nlist, M_, nb, nq, nprobe = 96, 16384, 16, 2000000, 2000, 24
    coarse = rng.random((nlist, d), dtype=np.float32)
    pq = (rng.random((M_, 256, d // M_), dtype=np.float32) - 0.5) * 0.2
    hot = rng.choice(nlist, 640, replace=False)                       # the codes sit in 640 lists
    lens = np.zeros(nlist, np.int64)
    lens[hot] = rng.multinomial(nb, np.full(640, 1.0 / 640))
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    codes = rng.integers(0, 256, (nb, M_), dtype=np.uint8)
    codes[5000:5600] = codes[5000]
    ids = rng.permutation(nb).astype(np.int64)
    xq = (coarse[rng.choice(hot, nq)] + 0.02 * rng.standard_normal((nq, d))).astype(np.float32)
    g = vlq.GpuIVFPQ(d, nlist, M_, 8)
    g.set_coarse_centroids(coarse)
    g.set_pq_centroids(pq)
    g.set_lists(codes, ids, off)
    assert g.ntotal >= 1024 * 640
    D, I = g.search(xq, nprobe, k)
    sel = np.arange(0, nq, 67)
    ox = pyoracle.OracleIndex(d, nlist, M_, 8, coarse, pq, codes=codes, ids=ids, list_offsets=off)
    Do, Io = ox.search(xq[sel], nprobe, k, canonical=True)
    assert np.array_equal(bits(D[sel]), bits(Do))
    assert np.array_equal(I[sel], Io)
    # the assignment path (no distance matrix) agrees with the first probe of the search path
    assign, _c = g.encode(xq[:400])
    _cd, keys = g.coarse_search(xq[:400], nprobe)
    assert np.array_equal(assign, keys[:, 0])
