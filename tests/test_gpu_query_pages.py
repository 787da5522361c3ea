"""GPU: searches of more than one 32 768-query page.  Every entry point cuts a call into pages (scan_stage.hip, coarse_stage.hip,
refine_api.hip, line_api.hip); per page the host offsets the queries, probes and output rows, plans the scan again with the
page's own size and re-reserves the workspaces, so the last page of a call usually runs another kernel than the first.  Every
case here makes ONE call of 32 768 + r queries and compares EVERY row, distances as bits, with the reference of the same
operation over the same batch, and the counters with the reference's for the whole call.

The reference is the C++ oracle (canonical tie order) for the L2 IVFPQ and VLQ searches, over all-distinct queries.  The
numpy restatements (ip_ref, polysemous_ref, ivfflat_ref, refine_ref) work per query: they are evaluated once on a pool of 512
distinct queries, the batch is pool[idx] with a seeded idx and the expectation ref[idx] (a row does not depend on the batch it
is in); idx[i] != idx[i - 32768] on the last page, so a row written one page off cannot land on its own value.

tests/golden/scan_plan.txt (tail_page_*) pins, without a GPU, which plan the last page of the 16-byte cases gets."""
import functools

import numpy as np
import pytest

import ip_ref
import ivfflat_ref as fr
import vector_line_quantization_amd as vlq
from oracle.pyoracle import OracleIndex
from polysemous_ref import labels_to_ids, oracle_filtered, oracle_scan
from refine_ref import refine_ref
from test_vlq_oracle import make_vlq
from util import bits

pytestmark = pytest.mark.gpu
PAGE = 32768
POOL = 512
F32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------
# shared helpers
# ----------------------------------------------------------------------------------------------------------------------
def host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def assert_whole_call(got, want, what=""):
    """Every row of every output array of one call of more than a page equals the reference's: float32 arrays as bits, the
    others as they are.  Names the first differing row and the page it lies in."""
    assert len(got) == len(want)
    n = want[0].shape[0]
    assert n > PAGE, "not a call of more than one page"
    for j, (g, w) in enumerate(zip(got, want)):
        g = host(g)
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: output %d is %s %s, expected %s %s" % (what, j, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype == np.float32:
            g, w = bits(g), bits(w)
        bad = np.nonzero((g.reshape(n, -1) != w.reshape(n, -1)).any(axis=1))[0]
        assert bad.size == 0, "%s: output %d differs in %d of %d rows, first row %d (page %d, row %d of it)" % (
            what, j, bad.size, n, bad[0], bad[0] // PAGE, bad[0] % PAGE)


def pool_rows(seed, n, npool=POOL):
    """idx [n] into a pool of distinct queries; no row of the last page repeats the row one page before it"""
    idx = np.random.default_rng(seed).integers(0, npool, n)
    tail = np.arange(PAGE, n)
    clash = tail[idx[tail] == idx[tail - PAGE]]
    idx[clash] = (idx[clash] + 1) % npool
    assert (idx[PAGE:] != idx[:n - PAGE]).all()
    return idx


def probed_codes(keys, list_offsets):
    """codes a query scans without a max_codes cut: the lengths of its lists, keys < 0 skipped [n]"""
    lens = np.diff(list_offsets)
    return np.where(keys >= 0, lens[np.maximum(keys, 0)], 0).sum(axis=1)


class World:
    """host arrays of a small IVFPQ index + its oracle + distinct queries; gpu() loads a fresh handle"""

    def __init__(self, seed, d, nlist, M, nbits, nb, nq, nprobe, by_residual=True, table=1, imi_nbits=0, descriptors=False):
        rng = np.random.default_rng(seed)
        self.d, self.nlist, self.M, self.nbits, self.nprobe = d, nlist, M, nbits, nprobe
        self.by_residual, self.table, self.imi_nbits = by_residual, table, imi_nbits
        self.coarse = self.imi = None
        if descriptors:          # normalised descriptors: term 2 stays inside the half range (float16 tables)
            centres = rng.standard_normal((300, d)).astype(F32)

            def gen(n):
                x = centres[rng.integers(0, 300, n)] + 0.35 * rng.standard_normal((n, d)).astype(F32)
                return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
            self.coarse = gen(nlist)
            self.pq = (0.08 * rng.standard_normal((M, 1 << nbits, d // M))).astype(F32)
        else:
            if imi_nbits:
                kc = 1 << imi_nbits
                assert nlist == kc * kc
                self.imi = rng.standard_normal((2, kc, d // 2)).astype(F32)
                centres = np.concatenate([self.imi[0][rng.integers(0, kc, 400)], self.imi[1][rng.integers(0, kc, 400)]], axis=1)
            else:
                self.coarse = rng.standard_normal((nlist, d)).astype(F32)
                centres = self.coarse

            def gen(n):
                return (centres[rng.integers(0, centres.shape[0], n)] + 0.6 * rng.standard_normal((n, d))).astype(F32)
            self.pq = (0.3 * rng.standard_normal((M, 1 << nbits, d // M))).astype(F32)
        xb = gen(nb)
        xb[nb // 2:nb // 2 + 40] = xb[7]               # identical vectors: exact distance ties inside a list
        self.ox = OracleIndex(d, nlist, M, nbits, self.coarse, self.pq, by_residual=by_residual, use_precomputed_table=table,
                              imi_centroids=self.imi, imi_nbits=imi_nbits)
        self.ox.add(xb, canonical=True)
        self.xq = gen(nq)
        self._memo = {}

    def gpu(self, metric="l2"):
        g = vlq.GpuIVFPQ(self.d, self.nlist, self.M, self.nbits, metric=metric)
        if self.imi_nbits:
            g.set_imi_centroids(self.imi_nbits, self.imi)
        else:
            g.set_coarse_centroids(self.coarse)
        g.set_pq_centroids(self.pq)
        if not (self.by_residual and self.table == 1):
            g.set_search_options(self.by_residual, self.table, 0)
        g.set_lists(self.ox.codes, self.ox.ids, self.ox.list_offsets)
        return g

    def expect(self, n, k, fp16=False):
        """the oracle's search of the first n queries: D, I, keys, coarse_dis, ncode (computed once per argument set)"""
        key = (n, k, fp16)
        if key not in self._memo:
            self.ox.float16_tables = fp16
            try:
                D, I, keys, cdis = self.ox.search(self.xq[:n], self.nprobe, k, canonical=True, return_coarse=True)
            finally:
                self.ox.float16_tables = False
            for a in (D, I, keys, cdis):
                a.setflags(write=False)
            self._memo[key] = (D, I, keys, cdis, self.ox.last_ncode)
        return self._memo[key]


def search_whole_call(w, g, r, k, what):
    """g.search of 32 768 + r queries == the oracle's search of them, counters included"""
    n = PAGE + r
    De, Ie, _keys, _cd, ncode = w.expect(n, k)
    g.stats(reset=True)
    D, I = g.search(w.xq[:n], w.nprobe, k)
    assert_whole_call((D, I), (De, Ie), what)
    assert g.stats() == (n, ncode), what


# ----------------------------------------------------------------------------------------------------------------------
# L2 IVFPQ, 16-byte codes
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world16():
    # 64 lists of ~62 codes: neither short (< 24 a list) nor long (>= 1024 a list)
    return World(16, 128, 64, 16, 8, 4000, PAGE + 3100, 32, descriptors=True)


# the last page's plan by scan_plan.h (tests/golden/scan_plan.txt: tail_page_*): split + merge (1, 7, 100), four-wave ordered
# scan16 (1100), scan16_tail (1500), two-wave scan16 (3100).  The name tells 1100 and 3100 from the rest.
LAST_PAGE_KERNEL = {1100: "kernel=scan16_kernel<1, 4, 1, false", 3100: "kernel=scan16_kernel<1, 2, 1, false"}


@pytest.mark.parametrize("r", [1, 7, 100, 1100, 1500, 3100])
def test_tail_pages(r):
    w = world16()
    g = w.gpu()
    search_whole_call(w, g, r, 10, "r=%d" % r)
    if r in LAST_PAGE_KERNEL:
        assert LAST_PAGE_KERNEL[r] in g.last_scan_info()


@pytest.mark.parametrize("how", ["plain", "store_pairs", "max_codes"])
def test_search_preassigned(how):
    w = world16()
    n = PAGE + 1500
    _D, _I, keys, cd, _nc = w.expect(n, 10)
    probed = int(probed_codes(keys, w.ox.list_offsets).min())
    g = w.gpu()
    sp = how == "store_pairs"
    w.ox.max_codes = probed // 2 if how == "max_codes" else 0       # below what every query probes: every row is cut
    try:
        if w.ox.max_codes:
            g.set_search_options(True, 1, w.ox.max_codes)
        De, Ie = w.ox.search_preassigned(w.xq[:n], keys, cd, 10, store_pairs=sp, canonical=True)
        ncode = w.ox.last_ncode
    finally:
        w.ox.max_codes = 0
    if how == "max_codes":
        assert ncode < int(probed_codes(keys, w.ox.list_offsets).sum())
    g.stats(reset=True)
    D, I = g.search_preassigned(w.xq[:n], keys, cd, 10, store_pairs=sp)
    assert_whole_call((D, I), (De, Ie), how)
    assert g.stats() == (n, ncode)


@pytest.mark.parametrize("buffers", ["numpy", "device", "pinned"])
def test_buffers(buffers):
    w = world16()
    n, k = PAGE + 1500, 10
    De, Ie, keys, cd, ncode = w.expect(n, k)
    g = w.gpu()
    x = w.xq[:n]
    if buffers == "numpy":
        D, I = np.full((n, k), -1, F32), np.full((n, k), -7, np.int64)
        g.search(x, w.nprobe, k, D=D, I=I)
        Dp, Ip = g.search_preassigned(x, keys, cd, k)
    elif buffers == "device":
        import torch
        xd, kd, cdd = (torch.from_numpy(np.array(a)).cuda() for a in (x, keys, cd))
        torch.cuda.synchronize()
        D, I = g.search(xd, w.nprobe, k)
        Dp, Ip = g.search_preassigned(xd, kd, cdd, k)
        g.stats()                                   # synchronises the index's stream
    else:
        # page-locked inputs AND outputs: the library is documented to hand such output rows to the scan kernel itself, at the
        # page's offset (include/vlq_ivfpq.h).  Nothing in the ABI tells a zero-copy write from a staged one, so this case
        # checks the rows that arrive in the caller's memory (prefilled with sentinels), not how they got there.
        import torch
        xp, kp, cp = (torch.from_numpy(np.array(a)).pin_memory() for a in (x, keys, cd))
        Dt, It = torch.full((n, k), -1.0, dtype=torch.float32).pin_memory(), torch.full((n, k), -7, dtype=torch.int64).pin_memory()
        D, I = g.search(xp.numpy(), w.nprobe, k, D=Dt.numpy(), I=It.numpy())
        D, I = D.copy(), I.copy()
        Dt.fill_(-1.0)
        It.fill_(-7)
        Dp, Ip = g.search_preassigned(xp.numpy(), kp.numpy(), cp.numpy(), k, D=Dt.numpy(), I=It.numpy())
    assert_whole_call((D, I), (De, Ie), buffers + " search")
    assert_whole_call((Dp, Ip), (De, Ie), buffers + " search_preassigned")
    assert g.stats() == (2 * n, 2 * ncode)


@pytest.mark.parametrize("k", [130, 300])
def test_selection_sizes(k):
    """scan16_bigk on both pages: one selection per workgroup, list capacity 256 and 512"""
    w = world16()
    search_whole_call(w, w.gpu(), 1500, k, "k=%d" % k)


@pytest.mark.parametrize("r", [100, 1500])
def test_float16_tables(r):
    w = world16()
    n = PAGE + r
    De, Ie, _keys, _cd, ncode = w.expect(n, 10, fp16=True)
    assert not np.array_equal(bits(De), bits(w.expect(n, 10)[0])), "the float16 tables are another arithmetic"
    g = w.gpu()
    g.set_float16_tables(True)
    D, I = g.search(w.xq[:n], w.nprobe, 10)
    assert_whole_call((D, I), (De, Ie), "fp16 r=%d" % r)
    assert g.stats() == (n, ncode)


@pytest.mark.parametrize("r", [100, 1500])
@pytest.mark.parametrize("schedule", [2, 3, 4])
def test_scan_schedules(schedule, r):
    """list-owned schedules on the first page; at r = 100 the last page is query-major again (below kOrderBatch)"""
    w = world16()
    g = w.gpu()
    g.set_scan_schedule(schedule)
    search_whole_call(w, g, r, 10, "schedule %d r=%d" % (schedule, r))


@functools.lru_cache(maxsize=None)
def coarse_world():
    """256 centroids in 128 dimensions: the smallest quantizer the float16 screen and the arg-min kernels serve
    (coarse_screen_shape_ok, coarse_screen_nn_shape_ok, coarse_argmin_ok: nlist >= 256, d % 4 == 0, d <= 128)"""
    rng = np.random.default_rng(256)
    d, nlist, n = 128, 256, PAGE + 1500
    coarse = rng.standard_normal((nlist, d)).astype(F32)
    x = (coarse[rng.integers(0, nlist, n)] + 0.6 * rng.standard_normal((n, d))).astype(F32)
    return coarse, x, OracleIndex(d, nlist, 4, 8, coarse, np.zeros((4, 256, d // 4), F32))


@pytest.mark.parametrize("r", [7, 1500])
@pytest.mark.parametrize("nprobe", [1, 8])
@pytest.mark.parametrize("screen", [1, 0])
def test_coarse_search(screen, nprobe, r):
    """The coarse stage alone, by coarse_page's conditions (coarse_stage.hip).  Screen on: the page of 32 768 rows goes through
    the float16 screen (nprobe 1: launch_coarse_screened_nn, nprobe 8: launch_coarse_screened), the last page (< 2048 rows) does
    not: arg-min over tile minima at nprobe 1, distance matrix + select at nprobe 8.  Screen off: both pages take the arg-min
    kernels at nprobe 1 and the matrix at nprobe 8.  The screen's own row counter says which pages it saw."""
    coarse, x, ox = coarse_world()
    n = PAGE + r
    cde, keyse = ox.coarse_search(x[:n], nprobe, canonical=True)
    g = vlq.GpuIVFPQ(128, 256, 4, 8)
    g.set_coarse_centroids(coarse)
    g.set_coarse_screen(screen)
    assert g.coarse_screen_state() == (bool(screen), 0, 0)
    cd, keys = g.coarse_search(x[:n], nprobe)
    assert_whole_call((keys, cd), (keyse, cde), "coarse screen=%d nprobe=%d r=%d" % (screen, nprobe, r))
    enabled, rows, undecided = g.coarse_screen_state()
    # the first page's rows were screened, the last page's were not; the screen was not defeated (it decides all but 0.5 % of the rows)
    assert (enabled, rows) == (bool(screen), PAGE if screen else 0) and undecided * 200 <= PAGE


# ---- data far from the origin: |x|^2 + |y|^2 - 2 <x, y> of the matrix formulation cancels, the direct (x - y)^2 of the
# reference's small batches (knn_L2sqr, n < 20) does not, so the two give different neighbours
def offset_data(seed, nlist, d, n):
    rng = np.random.default_rng(seed)
    return (50 + rng.random((nlist, d))).astype(F32), (50 + rng.random((n, d))).astype(F32)


def test_coarse_search_tail_rows_are_matrix_rows():
    """seven queries at the end of a big call are rows of the call's matrix formulation, not a small batch"""
    d, nlist, nprobe, n = 16, 1024, 4, PAGE + 7
    coarse, x = offset_data(41, nlist, d, n)
    ox = OracleIndex(d, nlist, 4, 8, coarse, np.zeros((4, 256, d // 4), F32))
    _c1, k1 = ox.coarse_search(x[PAGE:], nprobe, canonical=True, force_path=1)
    _c2, k2 = ox.coarse_search(x[PAGE:], nprobe, canonical=True, force_path=2)
    assert (k1 != k2).any(axis=1).sum() >= 3, "the two formulations agree on this data: the test could not tell them apart"
    cde, keyse = ox.coarse_search(x, nprobe, canonical=True, force_path=2)
    assert np.array_equal(keyse[PAGE:], k2)
    g = vlq.GpuIVFPQ(d, nlist, 4, 8)
    g.set_coarse_centroids(coarse)
    cd, keys = g.coarse_search(x, nprobe)
    assert_whole_call((keys, cd), (keyse, cde), "offset data")


def test_bad_and_skipped_keys():
    w = world16()
    n = PAGE + 100
    _D, _I, keys, cd, _nc = w.expect(n, 10)
    g = w.gpu()
    bad = keys.copy()
    bad[PAGE + 5, 3] = w.nlist                       # a row of the second page
    with pytest.raises(ValueError):                  # the reference aborts the search (IndexIVFPQ.cpp:1008-1011), and so does the oracle
        w.ox.search_preassigned(w.xq[:n], bad, cd, 10, canonical=True)
    with pytest.raises(vlq.VlqError) as e:
        g.search_preassigned(w.xq[:n], bad, cd, 10)
    assert e.value.code == 1 and "key" in str(e.value)
    g.stats()                                        # the flag was consumed by the error
    holes = keys.copy()
    holes[PAGE - 1, 0] = holes[PAGE - 1, 5] = -1     # the last row of the first page
    holes[PAGE, 0] = holes[PAGE, 31] = -1            # the first row of the second
    holes[n - 1] = -1                                # and a row with no probe at all
    De, Ie = w.ox.search_preassigned(w.xq[:n], holes, cd, 10, canonical=True)
    assert (Ie[n - 1] == -1).all() and not np.array_equal(Ie[PAGE], w.expect(n, 10)[1][PAGE])
    g.stats(reset=True)
    D, I = g.search_preassigned(w.xq[:n], holes, cd, 10)
    assert_whole_call((D, I), (De, Ie), "skipped keys")
    assert g.stats() == (n, w.ox.last_ncode)


# ----------------------------------------------------------------------------------------------------------------------
# the other scan organisations of the L2 search, against the C++ oracle
# ----------------------------------------------------------------------------------------------------------------------
NQ = PAGE + 1500
NQ_M8 = PAGE + 3100
OTHER = {   # name: (world arguments, the kernel of the last page by scan_plan.h)
    "scanm": (dict(seed=1, d=32, nlist=64, M=8, nbits=8, nb=4000, nq=NQ_M8, nprobe=8), "kernel=scanm_kernel<8>"),
    "scanm_table0": (dict(seed=2, d=64, nlist=64, M=16, nbits=8, nb=4000, nq=NQ, nprobe=8, table=0), "kernel=scanm_kernel<16>"),
    "generic_m5_6bit": (dict(seed=3, d=40, nlist=64, M=5, nbits=6, nb=4000, nq=NQ, nprobe=8), "kernel=scan_kernel "),
    "generic_not_by_residual": (dict(seed=4, d=32, nlist=64, M=8, nbits=8, nb=4000, nq=NQ, nprobe=8, by_residual=False),
                                "kernel=scan_kernel "),
    "scan16_short": (dict(seed=5, d=128, nlist=256, M=16, nbits=8, nb=3000, nq=NQ, nprobe=16), "kernel=scan16_short_kernel "),
    "scanm_short": (dict(seed=6, d=32, nlist=256, M=8, nbits=8, nb=3000, nq=NQ, nprobe=16), "kernel=scanm_short_kernel<8>"),
    # 4^4 = 256 cells, 25 codes a cell: the multi-index instantiation of the ordinary 16-byte kernel
    "multi_index": (dict(seed=7, d=128, nlist=256, M=16, nbits=8, nb=6400, nq=NQ, nprobe=16, imi_nbits=4), "true, false>"),
}


@functools.lru_cache(maxsize=None)
def other_world(name):
    return World(**OTHER[name][0])


@pytest.mark.parametrize("r", [7, 1500])
@pytest.mark.parametrize("name", sorted(OTHER))
def test_other_scan_organisations(name, r):
    w = other_world(name)
    g = w.gpu()
    search_whole_call(w, g, r, 10, "%s r=%d" % (name, r))
    assert OTHER[name][1] in g.last_scan_info(), g.last_scan_info()


def test_scanm_two_wave_tail():
    """8-byte codes with a last page of 3000 queries or more: scanm's two-wave instantiation (tail_page_3100_m8 of
    tests/golden/scan_plan.txt; the name in last_scan_info does not tell the waves)"""
    w = other_world("scanm")
    g = w.gpu()
    search_whole_call(w, g, 3100, 10, "scanm r=3100")
    assert OTHER["scanm"][1] in g.last_scan_info()


def test_multi_index_runs_of_probes():
    """more probes than one launch takes (scan_runs_dev): 1100 = a run of 1024 and a ragged one of 76, joined per page"""
    w = World(seed=8, d=128, nlist=4096, M=16, nbits=8, nb=6000, nq=PAGE + 300, nprobe=1100, imi_nbits=6)
    n = PAGE + 300
    cd, keys = w.ox.coarse_search(w.xq, w.nprobe)
    De, Ie = w.ox.search_preassigned(w.xq, keys, cd, 10, canonical=True)
    g = w.gpu()
    for call in (lambda: g.search_preassigned(w.xq, keys, cd, 10), lambda: g.search(w.xq, w.nprobe, 10)):
        g.stats(reset=True)
        D, I = call()
        assert_whole_call((D, I), (De, Ie), "runs of probes")
        assert g.stats() == (n, w.ox.last_ncode)


# ----------------------------------------------------------------------------------------------------------------------
# the scans whose reference is a numpy restatement: a pool of distinct queries, the batch drawn from it
# ----------------------------------------------------------------------------------------------------------------------
def small_lists(rng, nlist, nb):
    lens = rng.multinomial(nb, rng.dirichlet(np.full(nlist, 0.8)))
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, rng.permutation(nb).astype(np.int64) * 5 - 7


@functools.lru_cache(maxsize=None)
def ip_world(M, d):
    """inner-product IVFPQ over 64 lists and the restatement's rows of the pool, from its own coarse stage"""
    rng = np.random.default_rng(600 + M)
    nlist, nb, nprobe, k = 64, 3000, 8, 10
    coarse = rng.standard_normal((nlist, d)).astype(F32)
    pq = (0.5 * rng.standard_normal((M, 256, d // M))).astype(F32)
    off, ids = small_lists(rng, nlist, nb)
    codes = rng.integers(0, 256, (nb, M), dtype=np.uint8)
    pool = rng.standard_normal((POOL, d)).astype(F32)
    z = dict(coarse_centroids=coarse, pq_centroids=pq, codes=codes, ids=ids, list_offsets=off, by_residual=1, max_codes=0)
    keys, cdis = ip_ref.coarse_search(coarse, pool, nprobe)
    D, I, nc = ip_ref.search_preassigned(z, pool, keys, k)
    return dict(z=z, d=d, M=M, nlist=nlist, nprobe=nprobe, k=k, pool=pool, keys=keys, cdis=cdis, D=D, I=I, nc=nc)


@pytest.mark.parametrize("r", [7, 1500])
@pytest.mark.parametrize("M,d", [(16, 64), (5, 20)])
def test_inner_product(M, d, r):
    w = ip_world(M, d)
    z, n, k = w["z"], PAGE + r, w["k"]
    idx = pool_rows(M * 10 + r, n)
    x = np.ascontiguousarray(w["pool"][idx])
    g = vlq.GpuIVFPQ(d, w["nlist"], M, 8, metric="ip")
    g.set_coarse_centroids(z["coarse_centroids"])
    g.set_pq_centroids(z["pq_centroids"])
    g.set_lists(z["codes"], z["ids"], z["list_offsets"])
    g.stats(reset=True)
    D, I = g.search_preassigned(x, w["keys"][idx], w["cdis"][idx], k)
    assert_whole_call((D, I), (w["D"][idx], w["I"][idx]), "ip search_preassigned")
    assert g.stats() == (n, int(w["nc"][idx].sum()))
    # Its own coarse stage.  The device's inner products are the reference's only to rounding (another summation order), so
    # the expected coarse rows are the DEVICE's, from one page of the pool: this part checks that paging changes nothing
    # (offsets of x, keys and coarse_dis on the second page); it does not tie the rows to an independent reference beyond
    # the 99 % agreement of the probe sets with ip_ref below.
    cdp, keysp = g.coarse_search(w["pool"], w["nprobe"])
    assert (np.sort(keysp, axis=1) == np.sort(w["keys"], axis=1)).all(axis=1).mean() >= 0.99      # (near-ties may swap)
    cd, keys = g.coarse_search(x, w["nprobe"])
    assert_whole_call((keys, cd), (keysp[idx], cdp[idx]), "ip coarse")
    # the restatement's rows from the device's probes: the pool's own rows where the probes are ip_ref's, the others anew
    De, Ie, nc = w["D"].copy(), w["I"].copy(), w["nc"].copy()
    other = np.nonzero((keysp != w["keys"]).any(axis=1))[0]
    if other.size:
        De[other], Ie[other], nc[other] = ip_ref.search_preassigned(z, w["pool"][other], keysp[other], k)
    g.stats(reset=True)
    D, I = g.search(x, w["nprobe"], k)
    assert_whole_call((D, I), (De[idx], Ie[idx]), "ip search")
    assert g.stats() == (n, int(nc[idx].sum()))


@functools.lru_cache(maxsize=None)
def poly_world():
    rng = np.random.default_rng(700)
    d, nlist, M, nb, nprobe, k = 64, 64, 16, 3000, 8, 10
    coarse = rng.standard_normal((nlist, d)).astype(F32)
    pq = (0.5 * rng.standard_normal((M, 256, d // M))).astype(F32)
    off, ids = small_lists(rng, nlist, nb)
    codes = rng.integers(0, 256, (nb, M), dtype=np.uint8)
    pool = (coarse[rng.integers(0, nlist, POOL)] + rng.standard_normal((POOL, d))).astype(F32)
    ox = OracleIndex(d, nlist, M, 8, coarse, pq, codes=codes, ids=ids, list_offsets=off)
    cdis, keys = ox.coarse_search(pool, nprobe, canonical=True)
    scan = oracle_scan(ox, pool, keys, cdis)
    hd = np.sort(np.concatenate(scan["hd"]))
    ht = int(hd[hd.size // 2]) + 1                  # about half of the scanned codes pass
    D, P, npass, ncode = oracle_filtered(scan, ht, k)
    return dict(ox=ox, pool=pool, keys=keys, cdis=cdis, qcodes=scan["qcodes"], ht=ht, D=D, I=labels_to_ids(off, ids, P),
                npass=npass, ncode=ncode, nprobe=nprobe, k=k)


@pytest.mark.parametrize("r", [7, 1500])
def test_polysemous(r):
    w = poly_world()
    ox, n, k = w["ox"], PAGE + r, w["k"]
    idx = pool_rows(70 + r, n)
    x = np.ascontiguousarray(w["pool"][idx])
    keys, cdis = w["keys"][idx], w["cdis"][idx]
    g = vlq.GpuIVFPQ(ox.d, ox.nlist, ox.M, 8)
    g.set_coarse_centroids(ox.coarse_centroids)
    g.set_pq_centroids(ox.pq_centroids)
    g.set_lists(ox.codes, ox.ids, ox.list_offsets)
    # the q_code of every (query, probe) of the whole batch: written at qcodes + i0 * nprobe * M
    assert_whole_call((g.query_codes(x, keys),), (w["qcodes"][idx],), "query_codes")
    g.set_polysemous_ht(w["ht"])
    want = (w["D"][idx], w["I"][idx])
    counters = (n, int(w["ncode"][idx].sum()))
    for call in (lambda: g.search_preassigned(x, keys, cdis, k), lambda: g.search(x, w["nprobe"], k)):
        g.stats(reset=True)
        g.polysemous_stats(reset=True)
        D, I = call()
        assert_whole_call((D, I), want, "polysemous")
        assert g.stats() == counters and g.polysemous_stats() == int(w["npass"][idx].sum())
    assert "kernel=scan_poly_kernel<4>" in g.last_scan_info()


@functools.lru_cache(maxsize=None)
def flat_world(metric):
    rng = np.random.default_rng(800 + len(metric))
    d, nlist, nb, nprobe, k = 32, 64, 3000, 8, 10
    coarse = rng.standard_normal((nlist, d)).astype(F32)
    off, ids = small_lists(rng, nlist, nb)
    vecs = rng.standard_normal((nb, d)).astype(F32)
    pool = rng.standard_normal((POOL, d)).astype(F32)
    return dict(d=d, nlist=nlist, nprobe=nprobe, k=k, coarse=coarse, pool=pool, z=dict(vecs=vecs, ids=ids, list_offsets=off))


@pytest.mark.parametrize("r", [7, 1500])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivfflat(metric, r):
    """the coarse stage pages, the scan does not"""
    w = flat_world(metric)
    z, n, k, nprobe = w["z"], PAGE + r, w["k"], w["nprobe"]
    idx = pool_rows(80 + r, n)
    x = np.ascontiguousarray(w["pool"][idx])
    g = vlq.GpuIVFFlat(w["d"], w["nlist"], metric=metric)
    g.set_coarse_centroids(w["coarse"])
    g.set_lists(z["vecs"], z["ids"], z["list_offsets"])
    if metric == "l2":      # the C++ oracle's quantizer (the matrix formulation: 512 queries)
        ox = OracleIndex(w["d"], w["nlist"], 4, 8, w["coarse"], np.zeros((4, 256, w["d"] // 4), F32))
        cdp, keysp = ox.coarse_search(w["pool"], nprobe, canonical=True)
    else:                   # the DEVICE's probes of the pool, in one page: as in test_inner_product this checks that paging
                            # changes nothing, not the coarse rows against an independent reference (near-ties may swap)
        cdp, keysp = g.coarse_search(w["pool"], nprobe)
        keysr, _dis = ip_ref.coarse_search(w["coarse"], w["pool"], nprobe)
        assert (np.sort(keysp, axis=1) == np.sort(keysr, axis=1)).all(axis=1).mean() >= 0.99
    cd, keys = g.coarse_search(x, nprobe)
    assert_whole_call((keys, cd), (keysp[idx], cdp[idx]), "ivfflat coarse")
    De, Ie, nv, nd = fr.search_preassigned(z, w["pool"], keysp, k, metric)
    for call in (lambda: g.search(x, nprobe, k), lambda: g.search_preassigned(x, keysp[idx], k)):
        g.stats(reset=True)
        D, I = call()
        assert_whole_call((D, I), (De[idx], Ie[idx]), "ivfflat " + metric)
        assert g.stats() == (n, int(nv[idx].sum()), int(nd[idx].sum()))


# ----------------------------------------------------------------------------------------------------------------------
# IVFPQR: the refine stage and the two-stage searches, against refine_ref over the oracle's first stage
# ----------------------------------------------------------------------------------------------------------------------
class RefineWorld:
    """IVFPQR over random codes; per pool query the oracle's first stage at k_coarse (store_pairs) and the restatement's
    rows from it.  force_path: the formulation of the oracle's coarse stage (0: by the batch size, 1 direct, 2 matrix)."""

    def __init__(self, seed, d, nlist, M, Mr, nb, nprobe, k, k_factor, offset=False):
        rng = np.random.default_rng(seed)
        self.d, self.nlist, self.M, self.Mr, self.nprobe, self.k, self.kf = d, nlist, M, Mr, nprobe, k, k_factor
        self.kc = int(F32(k) * F32(k_factor))
        if offset:
            self.coarse = (50 + rng.random((nlist, d))).astype(F32)
            self.pool = (50 + rng.random((POOL, d))).astype(F32)
        else:
            self.coarse = (3 * rng.standard_normal((nlist, d))).astype(F32)
            self.pool = (self.coarse[rng.integers(0, nlist, POOL)] + rng.standard_normal((POOL, d))).astype(F32)
        self.pq = rng.standard_normal((M, 256, d // M)).astype(F32)
        self.rpq = (0.3 * rng.standard_normal((Mr, 256, d // Mr))).astype(F32)
        self.off, self.ids = small_lists(rng, nlist, nb)
        self.codes = rng.integers(0, 256, (nb, M), dtype=np.uint8)
        self.rcodes = rng.integers(0, 256, (nb, Mr), dtype=np.uint8)
        self.ox = OracleIndex(d, nlist, M, 8, self.coarse, self.pq, codes=self.codes, ids=self.ids, list_offsets=self.off)

    def gpu(self):
        g = vlq.GpuIVFPQ(self.d, self.nlist, self.M, 8)
        g.set_coarse_centroids(self.coarse)
        g.set_pq_centroids(self.pq)
        g.set_refine_pq(self.Mr, 8, self.rpq)
        g.set_lists(self.codes, self.ids, self.off)
        g.set_refine_codes(self.rcodes)
        return g

    def stages(self, force_path):
        """keys, coarse_dis, shortlist, D, I, ncode per query of the pool"""
        cdis, keys = self.ox.coarse_search(self.pool, self.nprobe, canonical=True, force_path=force_path)
        _Ds, sl = self.ox.search_preassigned(self.pool, keys, cdis, self.kc, store_pairs=True, canonical=True)
        ncode = probed_codes(keys, self.off)
        assert int(ncode.sum()) == self.ox.last_ncode
        D, I = refine_ref(self.pool, sl, self.k, self.coarse, self.pq, self.codes, self.rpq, self.rcodes, self.ids, self.off)
        return keys, cdis, sl, D, I, ncode


@functools.lru_cache(maxsize=None)
def refine_world():
    w = RefineWorld(900, 64, 64, 8, 16, 3000, 8, 10, 4.0)
    return w, w.stages(0)


@pytest.mark.parametrize("r", [7, 1500])
def test_refine(r):
    w, (keys, cdis, sl, De, Ie, ncode) = refine_world()
    n = PAGE + r
    idx = pool_rows(90 + r, n)
    x = np.ascontiguousarray(w.pool[idx])
    want = (De[idx], Ie[idx])
    g = w.gpu()
    assert_whole_call(g.refine(x, sl[idx], w.k), want, "refine")
    g.stats(reset=True)
    assert_whole_call(g.search_refined_preassigned(x, keys[idx], cdis[idx], w.k, w.kf), want, "search_refined_preassigned")
    assert g.stats() == (n, int(ncode[idx].sum()))
    g.stats(reset=True)
    assert_whole_call(g.search_refined(x, w.nprobe, w.k, w.kf), want, "search_refined")
    assert g.stats() == (n, int(ncode[idx].sum()))


def test_search_refined_takes_the_coarse_formulation_from_the_call():
    """IndexIVFPQR::search hands the quantizer the whole batch (IndexIVFPQ.cpp:1371): the 7 queries of the last page get the
    matrix formulation of a 32 775-query call, not the direct distances of a 7-query batch.  On data far from the origin
    the two find other lists."""
    w = RefineWorld(913, 16, 1024, 4, 8, 6000, 4, 10, 4.0, offset=True)
    n = PAGE + 7
    idx = pool_rows(913, n)
    _k1, _c1, _s1, D1, I1, _n1 = w.stages(1)
    _k2, _c2, _s2, D2, I2, ncode = w.stages(2)
    tail = idx[PAGE:]
    differ = (bits(D1[tail]) != bits(D2[tail])).any(axis=1) | (I1[tail] != I2[tail]).any(axis=1)
    assert differ.sum() >= 1, "both formulations give the same rows for the last page: the test could not tell them apart"
    g = w.gpu()
    g.stats(reset=True)
    D, I = g.search_refined(np.ascontiguousarray(w.pool[idx]), w.nprobe, w.k, w.kf)
    assert_whole_call((D, I), (D2[idx], I2[idx]), "search_refined on offset data")
    assert g.stats() == (n, int(ncode[idx].sum()))


# ----------------------------------------------------------------------------------------------------------------------
# VLQ
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vlq_world():
    """the 16-byte shape (row modes 1 / 2 / 3 are its three scan kernels) over 32 centroids, 32 768 + 40 distinct queries"""
    v, xb, _xq = make_vlq(seed=5, d=128, nlist=32, M=16, nbits=8, nedge=8, nlambda=64, nb=4000)
    rng = np.random.default_rng(55)
    n = PAGE + 40
    xq = (xb[rng.integers(0, xb.shape[0], n)] + 0.05 * rng.standard_normal((n, xb.shape[1]))).astype(F32)
    memo = {}

    def expect(fp16):
        if fp16 not in memo:
            memo[fp16] = v.search(xq, 8, 32, 10, return_lines=True, fp16=fp16) + (v.last_ncode,)
        return memo[fp16]
    return v, xq, expect


def vlq_gpu(v):
    g = vlq.GpuVLQ(v.d, v.nlist, v.M, v.nbits, v.nedge, v.nlambda)
    g.set_coarse_centroids(v.coarse)
    g.set_graph(v.edge_info, v.edge_dist)
    g.set_lambda_codebook(v.lambda_info)
    g.set_pq_centroids(v.pq_centroids)
    g.set_lists(v.codes, v.lambdas, v.ids, v.line_off)
    return g


@pytest.mark.parametrize("rows,parts,fp16", [(1, 1, False), (1, 3, False), (2, 1, False), (2, 3, False), (3, 1, False), (3, 3, False),
                                             (3, 1, True)])
def test_vlq_search(rows, parts, fp16):
    v, xq, expect = vlq_world()
    De, Ie, le, ncode = expect(fp16)
    g = vlq_gpu(v)
    g.set_row_mode(rows)
    g.set_scan_parts(parts)
    g.set_float16_tables(fp16)
    D, I, lines = g.search(xq, 8, 32, 10, return_lines=True)
    assert_whole_call((lines, D, I), (le, De, Ie), "vlq rows=%d parts=%d fp16=%d" % (rows, parts, fp16))
    assert g.stats() == ncode
