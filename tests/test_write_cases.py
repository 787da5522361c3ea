"""CPU: the helpers and worlds of the write-path tests (tests/write_cases.py) keep their promises -- the page worlds spread
their last page over many lists and never repeat the list of the row one page earlier, the growth plan overflows what it says
it overflows, the two PQ encoders' references agree, the planted ties are ties -- and the comparison helpers FAIL on the
mistakes they exist to catch (an expectation rolled by a page, two rows swapped, two rows of a list exchanged, one id changed).
That sensitivity is checked here, on wrong expectations; no wrong kernel ever runs on a device."""
import numpy as np
import pytest

import ivfsq_ref
import lsh_ref
import pq_ref
import write_cases as wc
from write_cases import PAGE, TAILS


def last_page_is_spread(assign, what):
    """rows of the last page go to at least 8 lists, the first seven of them (the tail of r = 7) to seven; no row of the last
    page goes where the row one page earlier went"""
    a = np.asarray(assign)
    assert np.unique(a[PAGE:]).size >= 8, what
    assert np.unique(a[PAGE:PAGE + 7]).size == 7, what
    assert (a[PAGE:] != a[:a.shape[0] - PAGE]).all(), what


def test_page_worlds_oracle():
    for name, w in (("ivfpq_l2", wc.ivfpq_l2()), ("ivfpq_matrix", wc.ivfpq_matrix()), ("ivfpq_imi", wc.ivfpq_imi())):
        a, _c = wc.oracle_encode(name)
        assert a.shape[0] == w.x.shape[0] and (a >= 0).all() and a.max() < w.nlist
        last_page_is_spread(a, name)
        for r in TAILS:       # the shorter calls see the same lists: a row's assignment does not depend on the batch behind it
            ar, _cr = wc.oracle_encode(name, PAGE + r)
            assert np.array_equal(ar, a[:PAGE + r]), (name, r)
    w = wc.ivfpq_l2()
    a2, _c2 = wc.oracle_encode("ivfpq_l2", batch="x2")
    assert a2.shape[0] == w.x2.shape[0] and np.unique(a2[PAGE:]).size == 7
    assert np.unique(np.concatenate([w.ids, w.ids2])).size == w.ids.size + w.ids2.size
    # by_residual off: other codes on the same lists
    an, cn = wc.oracle_encode("ivfpq_l2", PAGE + 7, by_residual=False)
    ar, cr = wc.oracle_encode("ivfpq_l2", PAGE + 7)
    assert np.array_equal(an, ar) and (cn != cr).any(axis=1).mean() > 0.9


def test_page_worlds_flat_and_sq():
    last_page_is_spread(wc.ivfflat_l2().assign, "ivfflat_l2")
    for qtype in ("8bit", "4bit"):
        w = wc.ivfsq(qtype)
        last_page_is_spread(w.assign, qtype)
        vmin, vdiff = ivfsq_ref.ranges(w.trained, w.d, w.qt)
        for rows in (w.res[:PAGE], w.res[PAGE:PAGE + TAILS[0]], w.res[PAGE:]):       # both clamps on both pages
            if rows.shape[0] > 7:
                assert (rows < vmin).any() and (rows > vmin + vdiff).any(), qtype
        assert w.codes.shape == (w.x.shape[0], ivfsq_ref.code_size(w.d, w.qt))
    a = wc.holes(3, wc.ivfflat_l2().assign, 256)
    assert (a[PAGE:] < 0).any() and (a[PAGE:] >= 256).any() and 0.8 < ((a >= 0) & (a < 256)).mean() < 0.9


def test_page_worlds_pooled():
    for name, w in (("ivfpq_ip", wc.ivfpq_ip()), ("ivfpqr", wc.ivfpqr()), ("ivfflat_ip", wc.ivfflat_ip())):
        assert np.unique(w.pool, axis=0).shape[0] == wc.POOL, name
        assert (w.idx[PAGE:] != w.idx[:w.idx.shape[0] - PAGE]).all(), name
        last_page_is_spread(w.pool_assign[w.idx], name)
    for w in (wc.ivfpq_ip(), wc.ivfflat_ip()):
        # integer data: every inner product is an exact integer, whatever the order of the sum; ties exist and go to the lower list
        ip = w.pool.astype(np.float64) @ w.coarse.astype(np.float64).T
        assert np.array_equal(ip, np.round(ip)) and np.abs(ip).max() < 2 ** 20
        assert np.array_equal(w.pool_assign, np.argmax(ip, axis=1))         # (argmax returns the first maximum)
        assert ((ip == ip.max(axis=1, keepdims=True)).sum(axis=1) > 1).any()
    w = wc.ivfpqr()
    assert w.d // w.Mr < 16 and np.unique(w.pool_rcodes, axis=0).shape[0] > 100


def test_vlq_world():
    w = wc.vlq_world()
    line, _lam = w.v.assign(w.x)
    assert w.nlines >= 256 and (line >= 0).all()
    last_page_is_spread(line, "vlq")


def test_offset_tail():
    w = wc.offset_tail()
    assert w.x.shape[0] == PAGE + 7
    assert (w.direct != w.gemm).all(), "the two formulations must disagree on every row of the tail"
    assert np.array_equal(w.assign[PAGE:], w.gemm), "the rows of a big call are rows of its GEMM formulation"


def test_growth_plan():
    lens = wc.growth_lens()
    assert lens.shape == (wc.GROWTH_NLIST,) and wc.GROWTH_NLIST > 256
    for n in (0, 1, 31, 32, 33, 40, 255, 256, 257, 1000):
        assert (lens[:256] == n).any(), "a list of %d rows in the first workgroup" % n
    first = lens[:256]
    long_at = np.nonzero(first > wc.GROWTH_SHORT)[0]
    assert all((first[i - 1] <= wc.GROWTH_SHORT) and (first[i + 1] <= wc.GROWTH_SHORT) for i in long_at), "long lists between short ones"
    assert (lens[256:] > wc.GROWTH_SHORT).any() and (lens[256:] == 0).any(), "a long and an empty list in the second workgroup"
    # with reclaim_memory (every kind but VLQ): packed again behind the first step, so the second overflows too
    steps, relayouts = wc.growth_run(reclaims=True)
    assert [s["overflows"] for s in steps] == [True, True, False, True, True]
    assert [s["reclaimed"] is not None for s in steps] == [True, False, True, False, True]
    # without (VLQ): the second batch fits the slack of the first
    steps_v, relayouts_v = wc.growth_run(reclaims=False)
    assert [s["overflows"] for s in steps_v] == [True, False, False, True, True] and all(s["reclaimed"] is None for s in steps_v)
    for run in (steps, steps_v):
        s0, s2, s3, s4 = run[0], run[2], run[3], run[4]
        assert s0["lens_before"][wc.GROWTH_LONG] > wc.GROWTH_SHORT and (s0["cap"] == s0["lens"] + s0["lens"] // 4).all()
        assert np.array_equal(s2["cap"], s2["cap_before"]) and (s2["lens"] <= s2["cap"]).all() and s2["counts"].sum() > 0
        assert s3["lens_before"][wc.GROWTH_SHORT_TO_LONG] <= wc.GROWTH_SHORT < s3["lens"][wc.GROWTH_SHORT_TO_LONG]
        assert s3["lens_before"][wc.GROWTH_SHORT_TO_LONG] + s3["counts"][wc.GROWTH_SHORT_TO_LONG] > s3["cap_before"][wc.GROWTH_SHORT_TO_LONG]
        assert s4["lens_before"][wc.GROWTH_SHORT_TO_LONG] > wc.GROWTH_SHORT, "the list that became long is moved as a long one"
        assert s4["lens"].max() < 1024, "no line beyond the VLQ scan's cap"
    # the slack the reclaims give back is the growth's own: it is not uniform, and lists of both workgroups carry some
    for s in (steps[0], steps[2], steps[4]):
        slack = s["cap"] - s["lens"]
        assert s["reclaimed"] == slack.sum() > 0 and np.unique(slack).size > 5 and slack[:256].sum() > 0 and slack[256:].sum() > 0
    # behind the batch that fits, the capacities are still those of the growth before it: a relayout there would show
    assert np.array_equal(steps[2]["cap"], steps[1]["cap"]) and steps[2]["reclaimed"] != (steps[2]["lens"] // 4).sum()


@pytest.mark.parametrize("case", sorted(wc.GROWTH_ROW_BYTES))
def test_growth_plan_copy_paths(case):
    """which copy path of the relayout kernel the lists of a row width take follows from the model's offsets: every width
    copies short lists per thread and long lists at unaligned offsets (16-byte rows: never) and at aligned ones, with a byte
    tail behind the 16-byte words unless the row is 16 bytes"""
    b = wc.GROWTH_ROW_BYTES[case]
    _steps, relayouts = wc.growth_run(reclaims=case != "vlq")
    n = wc.relayout_paths(relayouts, b)
    assert len(relayouts) == (3 if case == "vlq" else 9)
    assert n["short"] > 100 and n["aligned"] >= len(relayouts)
    if b == 16:
        assert n["unaligned"] == 0 and n["tail"] == 0
    else:
        assert n["unaligned"] >= len(relayouts) and n["tail"] >= len(relayouts)


@pytest.mark.parametrize("d,M,nbits", wc.PQ_SHAPES)
def test_pq_shapes(d, M, nbits):
    """pq_ref.compute_codes == the oracle's encode with by_residual off, byte for byte; rows planted on a duplicated centroid
    are at distance 0 of both copies and get the lower one"""
    w = wc.pq_shape(d, M, nbits)
    want = pq_ref.compute_codes(w.x_flat, w.pq)
    assert np.array_equal(wc.oracle_flat_codes(w, w.x_flat), want)
    assert (w.dup[:, 0] < w.dup[:, 1]).all() and np.array_equal(w.pq[np.arange(M), w.dup[:, 0]], w.pq[np.arange(M), w.dup[:, 1]])
    assert np.array_equal(want[:64], np.broadcast_to(w.dup[:, 0].astype(np.uint8), (64, M)))
    res = (w.x_res - w.coarse[w.cells]).astype(np.float32)
    assert np.array_equal(res[:64], w.x_flat[:64]), "the planted residuals are exact"
    assert np.array_equal(wc.residual_codes(w, w.x_res, w.cells, lambda r: pq_ref.compute_codes(r, w.pq))[:64], want[:64])
    dsub = d // M
    assert dsub in (1, 2, 3, 4, 6, 8)


def test_pq_shapes_cover_the_sweep():
    assert {d // M for d, M, _b in wc.PQ_SHAPES} == {1, 2, 3, 4, 6, 8}
    assert {b for _d, _M, b in wc.PQ_SHAPES} == {4, 5, 6, 7, 8}
    ds = [d for d, _M, _b in wc.PQ_SHAPES]
    assert min(ds) == 4 and max(ds) > 64 and max(ds) % 64 != 0
    assert any(1 << b < 64 for _d, _M, b in wc.PQ_SHAPES), "fewer centroids than lanes"
    assert {b for _d, M, b in wc.PQ_SHAPES if M % 8 == 0} == {4, 5, 6, 7, 8}, "the table arg-min kernel at every nbits"


@pytest.mark.parametrize("qt", range(4))
@pytest.mark.parametrize("d", wc.SQ_DIMS)
def test_sq_shapes(d, qt):
    w = wc.sq_shape(d, qt)
    vmin, vdiff = ivfsq_ref.ranges(w.trained, d, qt)
    top = 255 if ivfsq_ref.bits_of(qt) == 8 else 15
    comp = ivfsq_ref.components(ivfsq_ref.encode(w.res, qt, w.trained), d, qt)
    assert (comp[0] == 0).all() and (comp[1] == top).all(), "the end rows"
    assert (w.res < vmin).any() and (w.res > vmin + vdiff).any() and 0 < (comp == 0).mean() < 0.5 and 0 < (comp == top).mean() < 0.5
    # the residual the index takes from x is the planted one for the end rows, and the planted cell is the nearest by far
    assert np.array_equal((w.x - w.coarse[w.cells]).astype(np.float32)[:w.nends], w.res[:w.nends])
    assert np.array_equal(wc.l2_assign(w, w.x), w.cells)


def test_lsh_shapes():
    for nbits in wc.LSH_BITS:
        for rotate in (False, True):
            w = wc.lsh_shape(nbits, rotate)
            codes = lsh_ref.encode(w.x, nbits, w.A, None)
            assert codes.shape == (w.x.shape[0], (nbits + 7) // 8)
            if nbits % 8:
                assert (codes[:, -1] >> (nbits % 8) == 0).all(), "pad bits are zero"
            if rotate:
                assert (codes[:8] == lsh_ref.bits(np.zeros((8, nbits), np.float32))).all(), "0.0 and -0.0 set every bit"
            else:
                z = w.x[:, :nbits]
                assert ((z == 0) & ~np.signbit(z)).any() and ((z == 0) & np.signbit(z)).any()


# --- the helpers fail when they should -----------------------------------------------------------------------------------
def test_whole_call_sensitivity():
    w = wc.ivfpq_l2()
    n = PAGE + TAILS[0]
    a, c = wc.oracle_encode("ivfpq_l2", n)
    wc.whole_call((a.copy(), c.copy()), (a, c), "equal")
    with pytest.raises(AssertionError, match=r"page 0, row 0 of it"):
        wc.whole_call((np.roll(a, PAGE), c), (a, c), "rolled by a page")
    with pytest.raises(AssertionError, match=r"output 1 .* \(page 1, row 0 of it\)"):
        wc.whole_call((a, np.concatenate([c[:PAGE], c[:TAILS[0]]])), (a, c), "the first page's rows again on the last")
    swapped = a.copy()
    swapped[[PAGE + 2, PAGE + 5]] = swapped[[PAGE + 5, PAGE + 2]]
    with pytest.raises(AssertionError, match=r"differs in 2 of %d rows, first row %d \(page 1, row 2 of it\)" % (n, PAGE + 2)):
        wc.whole_call((swapped, c), (a, c), "two rows of the last page swapped")
    f = np.zeros((n, 2), np.float32)
    with pytest.raises(AssertionError):
        wc.whole_call((-f,), (f,), "-0.0 is not 0.0: float32 goes as bits")
    with pytest.raises(AssertionError, match="not a call of more than one page"):
        wc.whole_call((a[:100],), (a[:100],), "short")
    # a pooled batch rolled by a page differs in every row of the last page
    p = wc.ivfpq_ip()
    ap = p.pool_assign[p.idx]
    with pytest.raises(AssertionError):
        wc.whole_call((np.concatenate([ap[:PAGE], ap[:ap.shape[0] - PAGE]]),), (ap,), "pooled")


def test_list_comparison_sensitivity():
    w = wc.ivfflat_l2()
    n = PAGE + TAILS[0]
    a = wc.holes(5, w.assign[:n], w.nlist)
    side = (np.arange(n) % 251).astype(np.uint8).reshape(n, 1)
    want = wc.expected_lists(a, (w.x[:n], side), w.ids[:n], w.nlist)
    placed = (a >= 0) & (a < w.nlist)
    assert want.ntotal == placed.sum() < n and np.array_equal(want.lens, np.bincount(a[placed], minlength=w.nlist))
    for i in (0, 100, 255):          # input order inside a list
        rows = np.nonzero(a == i)[0]
        assert np.array_equal(want.ids[i], w.ids[rows]) and np.array_equal(want.parts[i][0], w.x[rows]) and np.array_equal(want.parts[i][1], side[rows])
    again = wc.read_lists(w.nlist, lambda i: (want.parts[i][0].copy(), want.parts[i][1].copy(), want.ids[i].copy()))
    wc.same_lists(again, want, "equal")
    flat, ids = want.flat()
    assert flat[0].shape == (want.ntotal, w.d) and ids.shape == (want.ntotal,) and want.offsets()[-1] == want.ntotal
    big = int(np.argmax(want.lens))
    assert want.lens[big] >= 2
    # two rows of one list exchanged (rows and side bytes travel together, the ids stay): the rows differ
    again.parts[big] = tuple(np.concatenate([p[1:2], p[0:1], p[2:]]) for p in again.parts[big])
    with pytest.raises(AssertionError, match="list %d part 0 differs in 2 rows, first row 0" % big):
        wc.same_lists(again, want, "exchanged")
    again.parts[big] = want.parts[big]
    again.ids[big] = np.concatenate([want.ids[big][1:2], want.ids[big][0:1], want.ids[big][2:]])
    with pytest.raises(AssertionError, match="list %d, row 0: id" % big):
        wc.same_lists(again, want, "ids exchanged")
    again.ids[big] = want.ids[big].copy()
    again.ids[big][-1] += 1
    with pytest.raises(AssertionError, match="list %d, row %d: id" % (big, want.lens[big] - 1)):
        wc.same_lists(again, want, "one id changed")
    again.ids[big] = want.ids[big][:-1]
    with pytest.raises(AssertionError, match="holds %d rows" % (want.lens[big] - 1)):
        wc.same_lists(again, want, "a row short")
    # a second batch goes behind the first
    more = wc.expected_lists(a[:50], (w.x[:50], side[:50]), w.ids[:50] + 10 ** 6, w.nlist, base=want)
    i = int(a[np.nonzero(placed[:50])[0][0]])
    assert np.array_equal(more.ids[i][:want.lens[i]], want.ids[i]) and more.ids[i][want.lens[i]] >= 10 ** 6
    assert more.ntotal == want.ntotal + placed[:50].sum()


def test_pool_rows():
    idx = wc.pool_rows(1, PAGE + 1500)
    assert idx.shape == (PAGE + 1500,) and idx.min() >= 0 and idx.max() < wc.POOL and np.unique(idx).size == wc.POOL
    assert (idx[PAGE:] != idx[:1500]).all()
    lab = np.arange(wc.POOL) % 5
    idx = wc.pool_rows(1, PAGE + 1500, labels=lab)
    assert (lab[idx[PAGE:]] != lab[idx[:1500]]).all()
