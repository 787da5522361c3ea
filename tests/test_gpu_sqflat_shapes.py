"""GPU: the flat scalar-quantizer scan (csrc/scan_sqflat.hip) under every split of its grid -- query tiles of 1, 2 and 4,
slices whose edges lie off every 64 / 256 boundary, the tail of a tile -- and at every edge of the selection's k."""
import numpy as np
import pytest

import sqflat_ref as fr
import vector_line_quantization_amd as vlq
from sqflat_cases import METRIC, bits, distances, load

pytestmark = pytest.mark.gpu

SPLIT_CASES = ["sqf_8bit_l2_d32", "sqf_8bit_ip_d32", "sqf_4bit_l2_d32", "sqf_4bit_ip_d32", "sqf_8bit_l2_d33", "sqf_4bit_ip_d33", "sqf_8bit_l2_d40"]


def index_of(z):
    g = vlq.GpuSQ(int(z["d"]), int(z["qtype"]), metric=METRIC[int(z["metric"])])
    g.set_trained(z["trained"])
    g.set_codes(z["codes"])
    return g


@pytest.mark.parametrize("name", SPLIT_CASES)
def test_rows_do_not_depend_on_the_split(name):
    z = load(name)
    g = index_of(z)
    k = int(z["k"])
    D0, I0 = g.search(z["xq"], k)
    for Q in (1, 2, 4):
        for S in (1, 2, 3, 7):
            g.set_scan_split(Q, S)
            D, I = g.search(z["xq"], k)
            info = g.last_scan_info()
            assert "Q=%d S=%d " % (Q, S) in info
            assert np.array_equal(bits(D), bits(D0)) and np.array_equal(I, I0), (name, info)
    # the tail of a tile: 1 and 5 queries in tiles of 4
    g.set_scan_split(4, 0)
    for nq in (1, 5):
        D, I = g.search(z["xq"][:nq], k)
        assert "Q=4 " in g.last_scan_info()
        assert np.array_equal(bits(D), bits(D0[:nq])) and np.array_equal(I, I0[:nq]), (name, nq)
    g.close()


@pytest.mark.parametrize("name", ["sqf_8bit_l2_d32", "sqf_4bit_ip_d32"])
def test_every_edge_of_k_against_the_restatement(name):
    z = load(name)
    metric = METRIC[int(z["metric"])]
    dis = distances(name)
    g = index_of(z)
    for k in (1, 64, 65, 256, 257, 1024):
        Dn, In = fr.rows_of(dis, k, metric)
        for Q, S in ((0, 0), (4, 3), (2, 1)):
            g.set_scan_split(Q, S)
            D, I = g.search(z["xq"], k)
            info = g.last_scan_info()
            assert "kernel=scan_sqflat_kernel<%d, %d," % (1 if k > 256 else (Q or 4), 1 if k <= 64 else 4 if k <= 256 else 16) in info
            assert np.array_equal(bits(D), bits(Dn)) and np.array_equal(I, In), (name, k, info)
    g.close()
