"""GPU: the encoders at small, awkward shapes, every byte against a CPU reference (the worlds are write_cases.py's, held to
their promises by tests/test_write_cases.py).

  encode_kernel           IVFPQ encode / encode_preassigned (oracle) and GpuPQ.encode (pq_ref.compute_codes): nbits 4 .. 8 --
                          below 6 bits lanes without a centroid take part in the wave reduction --, dsub 1, 2, 3, 4, 6, 8, d from
                          4 to 72, n in 1, 3, 4, 5, 257 (four vectors per workgroup), by_residual on and off; two centroids of
                          every sub-quantizer are duplicates and 64 rows lie exactly on them: the lower index must win
  pq_table_argmin_kernel  GpuPQ.query_codes under the polysemous search type (GpuPQ.encode goes through encode_kernel): the
                          type needs M % 8 == 0 -- five of the shapes, nbits 4 .. 8, so lanes beyond ksub < 64 are reached too
  sq_encode_kernel        GpuIVFSQ.encode, sqflat_encode_kernel: GpuSQ.encode, sqflat_decode_kernel: GpuSQ.reconstruct_n
                          (ivfsq_ref): four qtypes, d in 1, 3, 5, 33, 64, 65, 129, both clamps and both ends of the range
  lsh_encode_kernel       GpuLSH.apply / encode (lsh_ref): nbits in 1, 7, 8, 9, 60, 64, 65, 128, 130, with and without rotation,
                          bias and thresholds, components that are 0.0 and -0.0
  line_assign, lambda_quantize, line_residual, encode_kernel   GpuVLQ.encode (VLQ oracle): nlambda 2, 16, 256, nedge 1, 2, 8

No constructor refused a shape of these sweeps when they were written; a refusal fails the test (nothing is skipped)."""
import numpy as np
import pytest

import ivfsq_ref
import lsh_ref
import pq_ref
import vector_line_quantization_amd as vlq
import write_cases as wc
from test_vlq_oracle import make_vlq
from write_cases import bits

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------------------------
# product quantizer
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_residual", [True, False])
@pytest.mark.parametrize("d,M,nbits", wc.PQ_SHAPES)
def test_ivfpq_encode(d, M, nbits, by_residual):
    w = wc.pq_shape(d, M, nbits)
    g = vlq.GpuIVFPQ(d, w.nlist, M, nbits)
    g.set_coarse_centroids(w.coarse)
    g.set_pq_centroids(w.pq)
    if not by_residual:
        g.set_search_options(False, 0, 0)
    ox = wc.oracle_of(w, by_residual)
    x = w.x_res if by_residual else w.x_flat
    for n in wc.PQ_ROWS:        # (below 20 rows and d % 4 == 0 the reference assigns by the direct formulation: so do both sides)
        assign, codes = g.encode(x[:n])
        ae, ce = ox.encode(x[:n], canonical=True)
        assert np.array_equal(assign, ae), (n, np.nonzero(assign != ae)[0][:5])
        assert np.array_equal(codes, ce), (n, np.nonzero((codes != ce).any(axis=1))[0][:5])
    if not by_residual:
        assert np.array_equal(codes[:64], np.broadcast_to(w.dup[:, 0].astype(np.uint8), (64, M))), "the lower duplicate wins"
        return
    # the residual to a GIVEN list: the planted rows lie exactly on a duplicated centroid, a row without a list is a zero residual
    cells = w.cells.copy()
    cells[70:80] = -1
    want = wc.residual_codes(w, x, cells, lambda res: pq_ref.compute_codes(res, w.pq))
    assert np.array_equal(want, wc.residual_codes(w, x, cells, lambda res: wc.oracle_flat_codes(w, res)))
    for n in wc.PQ_ROWS:
        got = g.encode_preassigned(x[:n], cells[:n])
        assert np.array_equal(got, want[:n]), (n, np.nonzero((got != want[:n]).any(axis=1))[0][:5])
    assert np.array_equal(got[:64], np.broadcast_to(w.dup[:, 0].astype(np.uint8), (64, M))), "the lower duplicate wins"


@pytest.mark.parametrize("d,M,nbits", wc.PQ_SHAPES)
def test_pq_encode(d, M, nbits):
    w = wc.pq_shape(d, M, nbits)
    want = pq_ref.compute_codes(w.x_flat, w.pq)
    g = vlq.GpuPQ(d, M, nbits)
    g.set_centroids(w.pq)
    for n in wc.PQ_ROWS:
        got = g.encode(w.x_flat[:n])
        assert np.array_equal(got, want[:n]), (n, np.nonzero((got != want[:n]).any(axis=1))[0][:5])
    assert np.array_equal(got[:64], np.broadcast_to(w.dup[:, 0].astype(np.uint8), (64, M))), "the lower duplicate wins"
    for n in wc.PQ_ROWS[:-1]:
        g.add(w.x_flat[g.ntotal:g.ntotal + n])
    assert np.array_equal(g.codes(), want[:sum(wc.PQ_ROWS[:-1])])
    if M % 8 == 0:          # the first minimum of the query's own table (pq_table_argmin_kernel)
        g.search_type = "polysemous"
        for n in wc.PQ_ROWS:
            assert np.array_equal(g.query_codes(w.x_flat[:n]), want[:n]), n


# ----------------------------------------------------------------------------------------------------------------------
# scalar quantizer
# ----------------------------------------------------------------------------------------------------------------------
QTYPE_NAMES = sorted(ivfsq_ref.QTYPES, key=ivfsq_ref.QTYPES.get)


@pytest.mark.parametrize("qtype", QTYPE_NAMES)
@pytest.mark.parametrize("d", wc.SQ_DIMS)
def test_ivfsq_encode(d, qtype):
    """the residual of every row to its nearest centroid (the planted one, 64 apart from the next): rows on both ends of the
    range, beyond both clamps, inside"""
    qt = ivfsq_ref.QTYPES[qtype]
    w = wc.sq_shape(d, qt)
    g = vlq.GpuIVFSQ(d, w.nlist, qtype)
    g.set_coarse_centroids(w.coarse)
    g.set_trained(w.trained)
    assert g.code_size == ivfsq_ref.code_size(d, qt)
    want = ivfsq_ref.encode((w.x - w.coarse[w.cells]).astype(np.float32), qt, w.trained)
    top = 255 if g.bits == 8 else 15
    comp = ivfsq_ref.components(want, d, qt)
    assert (comp[0] == 0).all() and (comp[1] == top).all()
    for n in (1, 3, 4, 5, w.x.shape[0]):
        codes, assign = g.encode(w.x[:n])
        assert np.array_equal(assign, w.cells[:n]), n
        assert np.array_equal(codes, want[:n]), (n, np.nonzero((codes != want[:n]).any(axis=1))[0][:5])


@pytest.mark.parametrize("qtype", QTYPE_NAMES)
@pytest.mark.parametrize("d", wc.SQ_DIMS)
def test_sq_encode_and_reconstruct(d, qtype):
    qt = ivfsq_ref.QTYPES[qtype]
    w = wc.sq_shape(d, qt)
    g = vlq.GpuSQ(d, qtype)
    g.set_trained(w.trained)
    want = ivfsq_ref.encode(w.res, qt, w.trained)
    for n in (1, 3, 4, 5, w.res.shape[0]):
        codes = g.encode(w.res[:n])
        assert np.array_equal(codes, want[:n]), (n, np.nonzero((codes != want[:n]).any(axis=1))[0][:5])
    g.add(w.res[:5])
    g.add(w.res[5:])
    assert np.array_equal(g.codes(), want)
    rec = ivfsq_ref.decode_scalar(want, d, qt, w.trained)
    assert np.array_equal(bits(g.reconstruct_n()), bits(rec))
    assert np.array_equal(bits(g.reconstruct_n(3, 7)), bits(rec[3:10]))


# ----------------------------------------------------------------------------------------------------------------------
# LSH
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresholds", [False, True])
@pytest.mark.parametrize("rotate", ["no", "rotation", "rotation+bias"])
@pytest.mark.parametrize("nbits", wc.LSH_BITS)
def test_lsh_encode(nbits, rotate, thresholds):
    w = wc.lsh_shape(nbits, rotate != "no")
    g = vlq.GpuLSH(w.d, nbits, rotate_data=rotate != "no", train_thresholds=thresholds)
    b = w.b if rotate == "rotation+bias" else None
    if rotate != "no":
        g.set_rotation(w.A, b)
    thr = w.thr if thresholds else None
    if thresholds:
        g.set_thresholds(thr)
    assert g.bytes_per_vec == (nbits + 7) // 8
    xt = lsh_ref.apply(w.x, nbits, w.A, b, thr)
    want = lsh_ref.bits(xt)
    for n in (1, 3, 4, 5, w.x.shape[0]):
        assert np.array_equal(bits(g.apply(w.x[:n])), bits(xt[:n])), n
        codes = g.encode(w.x[:n])
        assert np.array_equal(codes, want[:n]), (n, np.nonzero((codes != want[:n]).any(axis=1))[0][:5])
    g.add(w.x[:3])
    g.add(w.x[3:])
    assert np.array_equal(g.get_codes(), want)


# ----------------------------------------------------------------------------------------------------------------------
# VLQ
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nedge", [1, 2, 8])
@pytest.mark.parametrize("nlambda", [2, 16, 256])
def test_vlq_encode(nlambda, nedge):
    v, xb, _xq = make_vlq(seed=100 * nlambda + nedge, d=8, nlist=12, M=2, nbits=5, nedge=nedge, nlambda=nlambda, nb=257)
    g = vlq.GpuVLQ(v.d, v.nlist, v.M, v.nbits, v.nedge, v.nlambda)
    g.set_coarse_centroids(v.coarse)
    g.set_graph(v.edge_info, v.edge_dist)
    g.set_lambda_codebook(v.lambda_info)
    g.set_pq_centroids(v.pq_centroids)
    for n in (1, 3, 4, 5, 257):
        x = xb[:n]
        line, lam = v.assign(x)
        gl, glam = g.assign(x)
        assert np.array_equal(gl, line) and np.array_equal(bits(glam), bits(lam)), n
        lb = v.quantize_lambda(lam)
        assert np.array_equal(bits(g.residuals(x)), bits(v.residuals(x, line, lb))), n
        l2, lb2, codes = g.encode(x)
        lo, lbo, co = v.encode(x)
        assert np.array_equal(l2, lo) and np.array_equal(lb2, lbo) and np.array_equal(codes, co), n
    assert np.unique(lbo).size >= 2 and (nedge == 1 or np.unique(lo % nedge).size >= 2), "more than one lambda and one edge in use"
