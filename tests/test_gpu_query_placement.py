"""GPU: the key that sorts the queries of a batch onto the XCDs (csrc/placement_key.h: the probes vote for one of the eight
partitions of neighbouring lists) is a schedule, not arithmetic.  A key the histogram and the placement disagree on breaks the
permutation -- queries are lost or scanned twice -- so every row of every case must equal the oracle's, bit for bit, in the
library's own order and under VLQ_WALK_FIRST=-1 (the reference's walking order).  The library reads its switches once per
process, so each setting runs in a fresh process that checks itself."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CODE = r'''
import sys, json, numpy as np
sys.path.insert(0, "tests")
import test_gpu_code_sizes as t
import vector_line_quantization_amd as vlq
from oracle.pyoracle import OracleIndex
from util import bits
out = {}
def same(tag, D, I, Do, Io):
    assert D.shape == Do.shape and np.array_equal(bits(D), bits(Do)), tag
    assert np.array_equal(I, Io), tag
    out[tag] = [int(bits(D).astype(np.uint64).sum()), int(I.sum())]
# d = 32, 64 lists, M = 16, ~310 vectors per list; 1024 = the smallest ordered batch, 1031 a ragged last chunk (one workgroup
# sorts), 2056 the histogram in the coarse stage's last kernel + the placement kernel
rng, ox, g, gen = t.make(16, 2, 64, 20000, 4711)
for nq in (1024, 1031, 2056):
    xq = gen(nq)
    D, I = g.search(xq, 16, 10)
    Do, Io = ox.search(xq, 16, 10, canonical=True)
    same("search_%d" % nq, D, I, Do, Io)
    assert "placement=vote" in g.last_scan_info(), g.last_scan_info()
# invalid and padded probe keys: holes, rows whose nearest key is invalid, a row without any probe (the caller's keys: the
# histogram kernel counts them)
for nq in (1031, 2056):
    xq = gen(nq)
    cd, keys = g.coarse_search(xq, 16)
    keys = keys.copy()
    keys[rng.random(keys.shape) < 0.2] = -1
    keys[::7, 0] = -1
    keys[::5, 9:] = -1
    keys[3] = -1
    D, I = g.search_preassigned(xq, keys, cd, 10)
    Do, Io = ox.search_preassigned(xq, keys, cd, 10, canonical=True)
    same("invalid_%d" % nq, D, I, Do, Io)
g.close()
# 256 lists, every query next to one centroid: all vote for one partition, and its XCD chunk overflows into the neighbours
rng, ox, g, gen = t.make(16, 2, 256, 20000, 4712)
for nq in (1031, 2056):
    xq = (ox.coarse_centroids[17] + 0.02 * rng.standard_normal((nq, 32))).astype(np.float32)
    D, I = g.search(xq, 16, 10)
    Do, Io = ox.search(xq, 16, 10, canonical=True)
    same("clustered_%d" % nq, D, I, Do, Io)
g.close()
# a multi-index handle (2 x 3 bits = 64 cells): no list_rank, the key is the id of the nearest cell as before
rng = np.random.default_rng(4713)
cent = rng.random((16, 32)).astype(np.float32)
draw = lambda n: (cent[rng.integers(0, 16, n)] + 0.08 * rng.standard_normal((n, 32))).astype(np.float32)
xb, xq = draw(20000), draw(1031)
imi = np.stack([xb[rng.choice(20000, 8, replace=False), :16], xb[rng.choice(20000, 8, replace=False), 16:]]).astype(np.float32)
pq = (0.15 * rng.standard_normal((16, 256, 2))).astype(np.float32)
g = vlq.GpuIVFPQ(32, 64, 16, 8)
g.set_imi_centroids(3, imi)
g.set_pq_centroids(pq)
g.set_search_options(by_residual=True, use_precomputed_table=1)
g.add(xb)
ox = OracleIndex(32, 64, 16, 8, None, pq, imi_centroids=imi, imi_nbits=3, by_residual=1, use_precomputed_table=2)
ox.add(xb, canonical=True)
D, I = g.search(xq, 16, 10)
Do, Io = ox.search(xq, 16, 10, canonical=True)
same("multi_index_1031", D, I, Do, Io)
assert "placement=nearest-id" in g.last_scan_info(), g.last_scan_info()
print(json.dumps(out))
'''

CASES = ["search_1024", "search_1031", "search_2056", "invalid_1031", "invalid_2056", "clustered_1031", "clustered_2056",
         "multi_index_1031"]


@pytest.fixture(scope="module")
def runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for name, extra in (("library", {}), ("reference_order", {"VLQ_WALK_FIRST": "-1"})):
        env = dict(os.environ)
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", CODE], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (name, p.stderr[-3000:])
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
    return res


@pytest.mark.parametrize("setting", ["library", "reference_order"])
def test_every_query_returns_the_oracles_row(runs, setting):
    assert sorted(runs[setting]) == sorted(CASES)        # each process asserted every row against the oracle


def test_placement_does_not_depend_on_the_walking_order(runs):
    assert runs["library"] == runs["reference_order"]
