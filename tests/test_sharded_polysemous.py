"""sharded.set_polysemous_ht: every rank sets IndexIVFPQ::polysemous_ht on its own handle, no collective involved.  On the CPU
with a stand-in that records the call (no process group exists: the helper must not need one); on the GPU with a real handle,
whose next search is then the filtered one."""
import pytest

from vector_line_quantization_amd import sharded


class _Recorder:
    def __init__(self):
        self.calls = []

    def set_polysemous_ht(self, ht):
        self.calls.append(ht)


def test_helper_sets_the_threshold_on_the_rank_s_index():
    idx = _Recorder()
    sharded.set_polysemous_ht(idx, 17)
    sharded.set_polysemous_ht(idx, 0)
    assert idx.calls == [17, 0]


@pytest.mark.gpu
def test_helper_sets_the_threshold_on_a_handle():
    import vector_line_quantization_amd as vlq
    from util import Case
    case = Case("poly_table1")
    g = vlq.GpuIVFPQ(case.d, case.nlist, case.M, case.nbits, device=0)
    g.set_coarse_centroids(case["coarse_centroids"])
    g.set_pq_centroids(case["pq_centroids"])
    g.set_lists(case["codes"], case["ids"], case["list_offsets"])
    ht = int(case["poly_hts"][2])
    sharded.set_polysemous_ht(g, ht)
    assert g.polysemous_ht == ht
    g.polysemous_stats(reset=True)
    g.stats(reset=True)
    g.search_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k)
    assert "scan_poly" in g.last_scan_info()
    assert 0 < g.polysemous_stats() < g.stats()[1]
    with pytest.raises(vlq.VlqError):
        sharded.set_polysemous_ht(g, -1)
    sharded.set_polysemous_ht(g, 0)
    g.search_preassigned(case.xq, case["keys"], case["coarse_dis"], case.k)
    assert "scan_poly" not in g.last_scan_info()
    g.close()
