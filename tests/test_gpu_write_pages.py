"""GPU: ONE call of 32 768 + r rows through every write entry point -- add, add_preassigned, encode, encode_preassigned, assign,
residuals, apply -- compared in full (write_cases.whole_call: every row of every output, float32 as bits; same_lists: every
list's rows, side bytes, ids and order) with a CPU reference of the same operation over the same batch.

The 1-NN assignment behind these calls is cut into pages of 32 768 rows (coarse_dev_of_call, assign_dev, ivf_assign); the
encoders and the list append run once over all rows and read the paged results.  r = 7 is a tail below the reference's 20-row
dispatch boundary (it must stay a row of the call's GEMM formulation: test_tail_rows_take_the_calls_formulation has data on
which the two differ), r = 1500 a tail that is not screened behind a screened first page, r = 2048 the shortest tail that is.
Which assignment path a page takes follows from the predicates of coarse_stage.hip for the worlds of write_cases.py:

  world                        first page (32 768 rows)                   last page (7 / 1500 rows)
  ivfpq_l2, screen on          float16-screened 1-NN                      tile arg-min (2048 rows: screened 1-NN)
  ivfpq_l2, screen off         tile arg-min                               tile arg-min
  ivfpq_matrix (d 6, 250)      distance matrix + select                   distance matrix + select
  ivfpq_imi (2 x 4 bits)       two half tables (matrix), pair select      the same
  ivfpq_ip, ivfflat_ip         tile arg-min over -2 <x, c>                the same
  ivfpqr, ivfflat_l2, ivfsq    float16-screened 1-NN                      tile arg-min
  vlq                          float16-screened 1-NN (coarse_page)        tile arg-min
  offset_tail                  float16-screened 1-NN                      tile arg-min, 7 rows: NOT the direct small-batch kernel

The references: the C++ oracle in canonical order on the whole batch of all-distinct rows (IVFPQ L2, multi-index, IVFFlat and
IVFSQ assignment, VLQ); ip_ref / pq_ref / refine_ref / ivfsq_ref / lsh_ref restatements, the per-row ones on a pool of 512 rows
(write_cases.pool_rows).  The inner-product worlds are integer-valued, so ip_ref.coarse_search is an independent reference in
any summation order: no expectation here is derived from the device."""
import numpy as np
import pytest

import ivfsq_ref
import lsh_ref
import pq_ref
import vector_line_quantization_amd as vlq
import write_cases as wc
from write_cases import F32, PAGE, TAILS, bits, expected_lists, read_lists, same_lists, whole_call

pytestmark = pytest.mark.gpu
NQ, NPROBE, K = 64, 8, 10


# ----------------------------------------------------------------------------------------------------------------------
# IVFPQ
# ----------------------------------------------------------------------------------------------------------------------
def gpu_ivfpq(w, by_residual=True, metric="l2", refine=False):
    g = vlq.GpuIVFPQ(w.d, w.nlist, w.M, w.nbits, metric=metric)
    if getattr(w, "imi_nbits", 0):
        g.set_imi_centroids(w.imi_nbits, w.imi)
    else:
        g.set_coarse_centroids(w.coarse)
    g.set_pq_centroids(w.pq)
    if not by_residual:
        g.set_search_options(False, 0, 0)
    if refine:
        g.set_refine_pq(w.Mr, w.nbits_r, w.rpq)
    return g


def check_ivfpq_lists(g, want, what, refine=False):
    """get_list (and the refine codes) of every list against the expected lists"""
    def get(i):
        codes, ids = g.get_list(i)
        return (codes, g.get_list_refine_codes(i), ids) if refine else (codes, ids)
    same_lists(read_lists(want.nlist, get), want, what)


def search_like_fresh(g, fresh, want, xq, what):
    """a search of g equals, as bits, the search of a fresh handle given the expected lists through set_lists"""
    flat, ids = want.flat()
    fresh.set_lists(flat[0], ids, want.offsets())
    D, I = g.search(xq[:NQ], NPROBE, K)
    Df, If = fresh.search(xq[:NQ], NPROBE, K)
    assert (If[:, K - 1] >= 0).all(), what
    assert np.array_equal(bits(D), bits(Df)) and np.array_equal(I, If), what


@pytest.mark.parametrize("r", TAILS + (wc.R_MAX,))
@pytest.mark.parametrize("screen", [1, 0])
def test_ivfpq_encode(screen, r):
    w = wc.ivfpq_l2()
    n = PAGE + r
    g = gpu_ivfpq(w)
    g.set_coarse_screen(screen)
    assign, codes = g.encode(w.x[:n])
    whole_call((assign, codes), wc.oracle_encode("ivfpq_l2", n), "encode screen=%d r=%d" % (screen, r))
    enabled, rows, _undecided = g.coarse_screen_state()
    # the screen's own row counter: the first page went through it, a tail of fewer than 2048 rows did not
    assert (enabled, rows) == (bool(screen), (PAGE + (r if r >= 2048 else 0)) if screen else 0)


def test_ivfpq_encode_without_residual():
    w = wc.ivfpq_l2()
    n = PAGE + TAILS[1]
    g = gpu_ivfpq(w, by_residual=False)
    whole_call(g.encode(w.x[:n]), wc.oracle_encode("ivfpq_l2", n, by_residual=False), "encode, by_residual off")


def test_ivfpq_encode_preassigned():
    """the oracle's assignment with a seeded tenth of the rows at -1: those are encoded as a zero residual"""
    w = wc.ivfpq_l2()
    n = PAGE + TAILS[1]
    a, c = wc.oracle_encode("ivfpq_l2", n)
    assign = a.copy()
    assign[np.random.default_rng(21).random(n) < 0.1] = -1
    assign[PAGE + 3] = -1
    want = wc.residual_codes(w, w.x[:n], assign, lambda res: wc.oracle_flat_codes(w, res))
    assert np.array_equal(want[assign >= 0], c[assign >= 0]) and np.unique(want[assign < 0], axis=0).shape[0] == 1
    g = gpu_ivfpq(w)
    whole_call((g.encode_preassigned(w.x[:n], assign),), (want,), "encode_preassigned")


@pytest.mark.parametrize("r", TAILS)
def test_ivfpq_add(r):
    """add of the whole batch with given ids, then a second add of 32 768 + 7 rows that grows lists that are already long"""
    w = wc.ivfpq_l2()
    n = PAGE + r
    g = gpu_ivfpq(w)
    g.add(w.x[:n], w.ids[:n])
    a, c = wc.oracle_encode("ivfpq_l2", n)
    want = expected_lists(a, c, w.ids[:n], w.nlist)
    assert g.ntotal == n == want.ntotal
    check_ivfpq_lists(g, want, "add r=%d" % r)
    search_like_fresh(g, gpu_ivfpq(w), want, w.xq, "search after add r=%d" % r)
    a2, c2 = wc.oracle_encode("ivfpq_l2", batch="x2")
    want2 = expected_lists(a2, c2, w.ids2, w.nlist, base=want)
    assert want.lens.min() > 32 and (want2.lens > want.lens + want.lens // 4).any(), "long lists overflow their slack"
    g.add(w.x2, w.ids2)
    assert g.ntotal == n + w.x2.shape[0] == want2.ntotal
    check_ivfpq_lists(g, want2, "second add r=%d" % r)
    search_like_fresh(g, gpu_ivfpq(w), want2, w.xq, "search after the second add r=%d" % r)


@pytest.mark.parametrize("r", TAILS)
def test_ivfpq_matrix_path(r):
    """d = 6, nlist = 250, M = 3: neither arg-min nor screen, every page through the distance matrix"""
    w = wc.ivfpq_matrix()
    n = PAGE + r
    g = gpu_ivfpq(w)
    a, c = wc.oracle_encode("ivfpq_matrix", n)
    whole_call(g.encode(w.x[:n]), (a, c), "matrix path encode r=%d" % r)
    assert g.coarse_screen_state()[1] == 0
    g.add(w.x[:n], w.ids[:n])
    want = expected_lists(a, c, w.ids[:n], w.nlist)
    assert g.ntotal == n
    check_ivfpq_lists(g, want, "matrix path add r=%d" % r)
    search_like_fresh(g, gpu_ivfpq(w), want, w.xq, "matrix path search r=%d" % r)


@pytest.mark.parametrize("r", TAILS)
def test_ivfpq_multi_index(r):
    w = wc.ivfpq_imi()
    n = PAGE + r
    g = gpu_ivfpq(w)
    a, c = wc.oracle_encode("ivfpq_imi", n)
    whole_call(g.encode(w.x[:n]), (a, c), "multi-index encode r=%d" % r)
    g.add(w.x[:n], w.ids[:n])
    assert g.ntotal == n
    check_ivfpq_lists(g, expected_lists(a, c, w.ids[:n], w.nlist), "multi-index add r=%d" % r)


@pytest.mark.parametrize("r", TAILS)
def test_ivfpq_inner_product(r):
    """integer data: the assignment against ip_ref.coarse_search (the first maximum, exact in any order), the codes against
    pq_ref.compute_codes of the residuals, then add"""
    w = wc.ivfpq_ip()
    n = PAGE + r
    x = w.pool[w.idx[:n]]
    a, c = w.pool_assign[w.idx[:n]], w.pool_codes[w.idx[:n]]
    g = gpu_ivfpq(w, metric="ip")
    whole_call(g.encode(x), (a, c), "inner-product encode r=%d" % r)
    g.add(x, w.ids[:n])
    want = expected_lists(a, c, w.ids[:n], w.nlist)
    assert g.ntotal == n
    check_ivfpq_lists(g, want, "inner-product add r=%d" % r)
    search_like_fresh(g, gpu_ivfpq(w, metric="ip"), want, w.pool, "inner-product search r=%d" % r)


@pytest.mark.parametrize("r", TAILS)
def test_ivfpqr_add(r):
    """the refine codes an add stores: the first-minimum code of (x - coarse[a]) - pq_decode(code) under the refine quantizer"""
    w = wc.ivfpqr()
    n = PAGE + r
    idx = w.idx[:n]
    g = gpu_ivfpq(w, refine=True)
    g.add(w.pool[idx], w.ids[:n])
    want = expected_lists(w.pool_assign[idx], (w.pool_codes[idx], w.pool_rcodes[idx]), w.ids[:n], w.nlist)
    assert g.ntotal == n
    check_ivfpq_lists(g, want, "IVFPQR add r=%d" % r, refine=True)


# ----------------------------------------------------------------------------------------------------------------------
# IVFFlat, IVFSQ
# ----------------------------------------------------------------------------------------------------------------------
def flat_batch(metric, n):
    if metric == "l2":
        w = wc.ivfflat_l2()
        return w, w.x[:n], w.assign[:n]
    w = wc.ivfflat_ip()
    return w, w.pool[w.idx[:n]], w.pool_assign[w.idx[:n]]


def gpu_flat(w, metric):
    g = vlq.GpuIVFFlat(w.d, w.nlist, metric=metric)
    g.set_coarse_centroids(w.coarse)
    return g


@pytest.mark.parametrize("r", TAILS)
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivfflat_add(metric, r):
    n = PAGE + r
    w, x, a = flat_batch(metric, n)
    g = gpu_flat(w, metric)
    g.add(x, w.ids[:n])
    want = expected_lists(a, x, w.ids[:n], w.nlist)
    assert g.ntotal == n
    same_lists(read_lists(w.nlist, g.get_list), want, "IVFFlat %s add r=%d" % (metric, r))
    xq = x[PAGE - 30:PAGE + 7]                    # stored rows as queries: each finds itself
    fresh = gpu_flat(w, metric)
    fresh.set_lists(want.flat()[0][0], want.flat()[1], want.offsets())
    D, I = g.search(xq, NPROBE, K)
    Df, If = fresh.search(xq, NPROBE, K)
    assert np.array_equal(bits(D), bits(Df)) and np.array_equal(I, If)


@pytest.fixture(scope="module")
def torch():
    """torch with its device context up: the start-up of the first device tensor (about ten seconds) is this fixture's set-up,
    not part of the time of whichever test happens to come first"""
    import torch
    torch.zeros(1).cuda()
    torch.cuda.synchronize()
    return torch


@pytest.mark.parametrize("buffers", ["numpy", "device"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivfflat_add_preassigned(metric, buffers, torch):
    """assignments < 0 and >= nlist are dropped: ntotal is the placed count"""
    n = PAGE + TAILS[1]
    w, x, a = flat_batch(metric, n)
    assign = wc.holes(31, a, w.nlist)
    ids = w.ids[:n]
    g = gpu_flat(w, metric)
    if buffers == "device":
        xd, ad, idd = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (x, assign, ids))
        torch.cuda.synchronize()
        g.add_preassigned(xd, ad, idd)
    else:
        g.add_preassigned(x, assign, ids)
    want = expected_lists(assign, x, ids, w.nlist)
    assert g.ntotal == want.ntotal == int(((assign >= 0) & (assign < w.nlist)).sum()) < n
    same_lists(read_lists(w.nlist, g.get_list), want, "IVFFlat %s add_preassigned %s" % (metric, buffers))


def test_ivfflat_add_device_tensors(torch):
    n = PAGE + TAILS[0]
    w, x, a = flat_batch("l2", n)
    g = gpu_flat(w, "l2")
    xd, idd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(w.ids[:n].copy()).cuda()
    torch.cuda.synchronize()
    g.add(xd, idd)
    assert g.ntotal == n
    same_lists(read_lists(w.nlist, g.get_list), expected_lists(a, x, w.ids[:n], w.nlist), "IVFFlat add of device tensors")


def gpu_sq(w):
    g = vlq.GpuIVFSQ(w.d, w.nlist, w.qtype)
    g.set_coarse_centroids(w.coarse)
    g.set_trained(w.trained)
    return g


@pytest.mark.parametrize("r", TAILS)
@pytest.mark.parametrize("qtype", ["8bit", "4bit"])
def test_ivfsq_encode(qtype, r):
    w = wc.ivfsq(qtype)
    n = PAGE + r
    codes, assign = gpu_sq(w).encode(w.x[:n])
    whole_call((codes, assign), (w.codes[:n], w.assign[:n]), "IVFSQ %s encode r=%d" % (qtype, r))


@pytest.mark.parametrize("qtype", ["8bit", "4bit"])
def test_ivfsq_add(qtype):
    w = wc.ivfsq(qtype)
    n = PAGE + TAILS[1]
    g = gpu_sq(w)
    g.add(w.x[:n], w.ids[:n])
    want = expected_lists(w.assign[:n], w.codes[:n], w.ids[:n], w.nlist)
    assert g.ntotal == n
    same_lists(read_lists(w.nlist, g.get_list), want, "IVFSQ %s add" % qtype)
    fresh = gpu_sq(w)
    fresh.set_lists(want.flat()[0][0], want.flat()[1], want.offsets())
    D, I = g.search(w.xq, NPROBE, K)
    Df, If = fresh.search(w.xq, NPROBE, K)
    assert (If[:, K - 1] >= 0).all() and np.array_equal(bits(D), bits(Df)) and np.array_equal(I, If)


@pytest.mark.parametrize("qtype", ["8bit", "4bit"])
def test_ivfsq_add_preassigned(qtype):
    """the codes are those of the residual to the GIVEN list: the rows are sent to the list after their nearest one"""
    w = wc.ivfsq(qtype)
    n = PAGE + TAILS[1]
    assign = wc.holes(32, (w.assign[:n] + 1) % w.nlist, w.nlist)
    ok = (assign >= 0) & (assign < w.nlist)
    res = (w.x[:n] - w.coarse[np.where(ok, assign, 0)]).astype(F32)
    want = expected_lists(assign, ivfsq_ref.encode(res, w.qt, w.trained), w.ids[:n], w.nlist)
    g = gpu_sq(w)
    g.add_preassigned(w.x[:n], assign, w.ids[:n])
    assert g.ntotal == want.ntotal == int(ok.sum()) < n
    same_lists(read_lists(w.nlist, g.get_list), want, "IVFSQ %s add_preassigned" % qtype)


def test_tail_rows_take_the_calls_formulation():
    """Seven rows behind a full page, on data where the GEMM formulation and the direct small-batch one assign every one of
    them to different lists: they are rows of the call (32 775 rows), so the GEMM formulation's lists are the right ones."""
    w = wc.offset_tail()
    for g in (vlq.GpuIVFFlat(w.d, w.nlist), vlq.GpuIVFPQ(w.d, w.nlist, 4, 8)):
        g.set_coarse_centroids(w.coarse)
        _cd, keys = g.coarse_search(w.x, 1)
        whole_call((keys[:, 0].copy(),), (w.assign,), "1-NN of %s" % type(g).__name__)
    ids = wc.given_ids(40, w.x.shape[0])
    g = vlq.GpuIVFFlat(w.d, w.nlist)
    g.set_coarse_centroids(w.coarse)
    g.add(w.x, ids)
    same_lists(read_lists(w.nlist, g.get_list), expected_lists(w.assign, w.x, ids, w.nlist), "offset data add")
    # and the same seven rows as a call of their own take the direct formulation (the reference's dispatch for n < 20)
    _cd, keys = g.coarse_search(w.x[PAGE:], 1)
    assert np.array_equal(keys[:, 0], w.direct)


# ----------------------------------------------------------------------------------------------------------------------
# VLQ
# ----------------------------------------------------------------------------------------------------------------------
def gpu_vlq(v):
    g = vlq.GpuVLQ(v.d, v.nlist, v.M, v.nbits, v.nedge, v.nlambda)
    g.set_coarse_centroids(v.coarse)
    g.set_graph(v.edge_info, v.edge_dist)
    g.set_lambda_codebook(v.lambda_info)
    g.set_pq_centroids(v.pq_centroids)
    return g


@pytest.mark.parametrize("r", TAILS)
def test_vlq(r):
    """assign, residuals, encode and add of one batch against the VLQ oracle; 512 lines"""
    w = wc.vlq_world()
    v, n = w.v, PAGE + r
    x = w.x[:n]
    g = gpu_vlq(v)
    line, lam = v.assign(x)
    whole_call(g.assign(x), (line, lam), "VLQ assign r=%d" % r)
    lb = v.quantize_lambda(lam)
    whole_call((g.residuals(x),), (v.residuals(x, line, lb),), "VLQ residuals r=%d" % r)
    fresh = wc.fresh_vlq(v)
    line2, lb2, codes = fresh.add(x, w.ids[:n])
    assert np.array_equal(line2, line) and np.array_equal(lb2, lb)
    whole_call(g.encode(x), (line, lb, codes), "VLQ encode r=%d" % r)
    g.add(x, w.ids[:n])
    want = expected_lists(line, (codes, lb.reshape(n, 1)), w.ids[:n], w.nlines)
    assert np.array_equal(want.offsets(), fresh.line_off) and np.array_equal(want.flat()[1], fresh.ids)      # (the oracle's own append)
    assert g.ntotal == want.ntotal

    def get(i):
        c, l, ids = g.get_list(i)
        return c, l.reshape(-1, 1), ids
    same_lists(read_lists(w.nlines, get), want, "VLQ add r=%d" % r)
    D, I = g.search(w.xq, 8, 16, K)
    De, Ie = fresh.search(w.xq, 8, 16, K)
    assert np.array_equal(bits(D), bits(De)) and np.array_equal(I, Ie)


# ----------------------------------------------------------------------------------------------------------------------
# the single-list kinds: no pages, but the encoders' grids and row offsets come from n and the append is the shared one
# ----------------------------------------------------------------------------------------------------------------------
N1 = PAGE + TAILS[0]


def test_pq_single_list():
    w = wc.ivfpq_l2()
    idx = wc.pool_rows(52, N1)                   # (pq_ref works per row: a pool of the world's first 512 rows)
    x = w.x[:wc.POOL][idx]
    want = pq_ref.compute_codes(w.x[:wc.POOL], w.pq)[idx]
    g = vlq.GpuPQ(w.d, w.M, w.nbits)
    g.set_centroids(w.pq)
    whole_call((g.encode(x),), (want,), "GpuPQ.encode")
    g.add(x[:5])
    g.add(x[5:])
    assert g.ntotal == N1
    whole_call((g.codes(),), (want,), "GpuPQ.add + codes")


@pytest.mark.parametrize("qtype", ["8bit", "4bit"])
def test_sq_single_list(qtype):
    w = wc.ivfsq(qtype)
    x = w.res[:N1]                               # (rows that reach both clamps of the trained range)
    want = ivfsq_ref.encode(x, w.qt, w.trained)
    g = vlq.GpuSQ(w.d, qtype)
    g.set_trained(w.trained)
    whole_call((g.encode(x),), (want,), "GpuSQ.encode")
    g.add(x[:3])
    g.add(x[3:])
    assert g.ntotal == N1
    whole_call((g.codes(),), (want,), "GpuSQ.add + codes")
    whole_call((g.reconstruct_n(),), (ivfsq_ref.decode_scalar(want, w.d, w.qt, w.trained),), "GpuSQ.reconstruct_n")


def test_lsh_single_list():
    """30 bits out of 16 dimensions, with a rotation, a bias and thresholds; pooled (lsh_ref's fmaf chain runs per row)"""
    rng = np.random.default_rng(50)
    d, nbits = 16, 30
    pool = rng.standard_normal((wc.POOL, d)).astype(F32)
    A = vlq.random_rotation(d, nbits, seed=11)
    b, thr = (0.1 * rng.standard_normal(nbits)).astype(F32), (0.1 * rng.standard_normal(nbits)).astype(F32)
    idx = wc.pool_rows(51, N1)
    x = pool[idx]
    g = vlq.GpuLSH(d, nbits, rotate_data=True, train_thresholds=True)
    g.set_rotation(A, b)
    g.set_thresholds(thr)
    whole_call((g.apply(x),), (lsh_ref.apply(pool, nbits, A, b, thr)[idx],), "GpuLSH.apply")
    want = lsh_ref.encode(pool, nbits, A, b, thr)[idx]
    assert np.unique(want, axis=0).shape[0] > 400
    whole_call((g.encode(x),), (want,), "GpuLSH.encode")
    g.add(x[:9])
    g.add(x[9:])
    assert g.ntotal == N1
    whole_call((g.get_codes(),), (want,), "GpuLSH.add + get_codes")


def test_flat_single_list():
    w = wc.ivfflat_l2()
    x = w.x[:N1].copy()
    x[PAGE + 1, 0], x[5, 1] = -0.0, np.float32(np.nan)          # stored as bits
    g = vlq.GpuFlat(w.d)
    g.add(x[:PAGE + 2])
    g.add(x[PAGE + 2:])
    assert g.ntotal == N1
    whole_call((g.reconstruct_n(),), (x,), "GpuFlat.add + reconstruct_n")


def test_refine_flat_add(torch):
    """GpuRefineFlat.add with the sequential ids it takes: the base's lists and the store's rows"""
    w = wc.ivfflat_l2()
    x, a = w.x[:N1], w.assign[:N1]
    rf = vlq.GpuRefineFlat(gpu_flat(w, "l2"))
    ids = np.arange(N1, dtype=np.int64)
    rf.add(x, ids)
    assert rf.ntotal == rf.base.ntotal == N1
    same_lists(read_lists(w.nlist, rf.base.get_list), expected_lists(a, x, ids, w.nlist), "GpuRefineFlat.add: the base")
    whole_call((rf.store.reconstruct_n(),), (x,), "GpuRefineFlat.add: the store")
    with pytest.raises(ValueError):
        rf.add(x[:4], w.ids[:4])                  # not the sequential ids
    xq = x[PAGE - 3:PAGE + 4]
    rf.k_factor = 2.0
    D, I = rf.search(xq, 1, nprobe=4)
    assert np.array_equal(I[:, 0], np.arange(PAGE - 3, PAGE + 4)), D
