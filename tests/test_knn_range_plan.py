"""CPU: path, row tile, slices, page, LDS and scratch of the flat index's range search are one pure host function
(csrc/knn_range_plan.h: plan_knn_range).  tests/cpp/knn_range_plan_dump.cpp -- host compiler only -- prints the plan of the
shapes below; the expected values are written by hand from the header's rules and the kernels' layouts:

  path     direct when the call's nq < 20 and d % 4 == 0 (utils.cpp:1239-1262), gemm otherwise
  rows     gemm: 128 from 2048 queries of a page on, 64 from 512, else 32; direct: 1, 4 or 19 queries in LDS, fewer where d is large
  S        as many slices as give 512 workgroups, of 2048 columns at least, 1024 at most, and at most 32 MiB / 12 / nq (so that the
           counts never hold a term in nq x ntotal); forced: at most ntotal / 128 (gemm) resp. ntotal / 256 (direct) and 64
  lds      gemm: 2 (rows + 128) 36 floats of staged tiles, rows x 16 bytes of hit masks, rows x 8 of counts and norms;
           direct: roundup16(4 rows d) of queries, 36864 of row tiles, 32 rows of trip counts; at most 160 KiB
  scratch  12 (nq S + 1) bytes of counts and slots, 4 nq of query norms on the gemm path
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")
TILES = 4 * 64 * 36 * 4
PAGE = 32768


def gemm_lds(rows):
    return 2 * (rows + 128) * 36 * 4 + rows * 16 + rows * 8


def direct_lds(rows, d):
    return (rows * d * 4 + 15) // 16 * 16 + TILES + 2 * 4 * rows * 4


def line(nq, ntotal, d, fr, fs, path, rows, S):
    lds = gemm_lds(rows) if path == "gemm" else direct_lds(rows, d)
    scratch = 12 * (nq * S + 1) + (4 * nq if path == "gemm" else 0)
    return "nq=%d ntotal=%d d=%d force=%d,%d: path=%s rows=%d S=%d slice=%d page=%d lds=%d scratch=%d" % (
        nq, ntotal, d, fr, fs, path, rows, S, -(-ntotal // S) if ntotal else 0, PAGE, lds, scratch)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knn_range_plan") / "knn_range_plan_dump")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "knn_range_plan.mk", "OUT=" + exe])

    def run(shapes):
        p = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()
    return run


def test_dispatch(dump):
    """19 against 20 queries, d % 4, and the call's nq beyond a page"""
    cases = [
        ((19, 1000000, 128, 0, 0), ("direct", 19, 488)),        # 512 groups wanted, 1000000 // 2048 slices at most
        ((20, 1000000, 128, 0, 0), ("gemm", 32, 488)),
        ((19, 1000000, 30, 0, 0), ("gemm", 32, 488)),           # d % 4 != 0
        ((1, 1000000, 130, 0, 0), ("gemm", 32, 488)),
        ((1, 1000000, 128, 0, 0), ("direct", 1, 488)),
        ((4, 1000000, 128, 0, 0), ("direct", 4, 488)),
        ((5, 1000000, 128, 0, 0), ("direct", 19, 488)),
        ((5, 300, 8, 0, 0), ("direct", 19, 1)),
        ((511, 100000, 64, 0, 0), ("gemm", 32, 32)),            # 16 row tiles -> 32 slices
        ((512, 100000, 64, 0, 0), ("gemm", 64, 48)),            # 8 row tiles -> 64 slices, 100000 // 2048 = 48
        ((2048, 1000000, 64, 0, 0), ("gemm", 128, 32)),
        ((10000, 1000000, 128, 0, 0), ("gemm", 128, 7)),
        ((33000, 300, 8, 0, 0), ("gemm", 128, 1)),
        ((5, 0, 8, 0, 0), ("direct", 19, 1)),
    ]
    got = dump([c[0] for c in cases])
    assert got == [line(*a, *b) for a, b in cases]
    assert got[1] == "nq=20 ntotal=1000000 d=128 force=0,0: path=gemm rows=32 S=488 slice=2050 page=32768 lds=46848 scratch=117212"


def test_bounds_at_scale(dump):
    """10^8 vectors, a full page of queries and beyond: scratch has no term in nq x ntotal, LDS stays within 160 KiB"""
    got = dump([(32768, 10 ** 8, 128, 0, 0), (32768, 10 ** 8, 128, 32, 64), (10 ** 6, 10 ** 8, 128, 0, 0), (10 ** 7, 10 ** 8, 128, 0, 64)])
    assert got[0] == line(32768, 10 ** 8, 128, 0, 0, "gemm", 128, 2)
    assert got[1] == line(32768, 10 ** 8, 128, 32, 64, "gemm", 32, 64)
    assert got[2] == line(10 ** 6, 10 ** 8, 128, 0, 0, "gemm", 128, 2)          # (32 MiB / 12) // 10^6 = 2
    assert got[3] == line(10 ** 7, 10 ** 8, 128, 0, 64, "gemm", 128, 1)         # (32 MiB / 12) // 10^7 = 0: one slice, forced or not
    for g in got:
        nq = int(g.split()[0][3:])
        assert int(g.rsplit("scratch=", 1)[1]) <= (32 << 20) + 16 * nq
        assert int(g.split("lds=")[1].split()[0]) <= 160 * 1024
    assert gemm_lds(128) == 76800


def test_forced_splits(dump):
    cases = [
        ((150, 8200, 8, 32, 1), ("gemm", 32, 1)),
        ((150, 8200, 8, 64, 3), ("gemm", 64, 3)),
        ((150, 8200, 8, 128, 64), ("gemm", 128, 64)),
        ((150, 300, 8, 128, 64), ("gemm", 128, 2)),             # never below one 128-column tile
        ((150, 100, 8, 0, 64), ("gemm", 32, 1)),
        ((19, 8200, 8, 128, 3), ("direct", 19, 3)),             # the row tile means nothing on the direct path
        ((19, 8200, 8, 0, 64), ("direct", 19, 32)),             # never below one 256-row trip
    ]
    got = dump([c[0] for c in cases])
    assert got == [line(*a, *b) for a, b in cases]


def test_limits(dump):
    got = dump([(0, 10, 8, 0, 0), (5, 10, 0, 0, 0), (5, 1 << 32, 8, 0, 0), (5, 10, 8, 48, 0), (5, 10, 8, 0, 65), (5, 10, 8, 0, -1)])
    assert all(": invalid (" in g for g in got), got
    # the direct path keeps the k-NN's limit: one query in LDS beside the row tiles; the GEMM path takes any d
    dmax = (160 * 1024 - TILES - 32) // 16 * 4
    got = dump([(1, 1000, dmax, 0, 0), (1, 1000, dmax + 4, 0, 0), (19, 1000, dmax, 0, 0), (1, 1000, dmax + 5, 0, 0), (20, 1000, 10 ** 6, 0, 0)])
    assert got[0] == line(1, 1000, dmax, 0, 0, "direct", 1, 1)
    assert ": unsupported (" in got[1]
    assert got[2] == line(19, 1000, dmax, 0, 0, "direct", 1, 1)          # 19 queries of this d: one at a time
    assert got[3] == line(1, 1000, dmax + 5, 0, 0, "gemm", 32, 1)
    assert got[4] == line(20, 1000, 10 ** 6, 0, 0, "gemm", 32, 1)
    # between: 19 queries, then 4, then 1 as d grows
    got = dump([(19, 1000, 1000, 0, 0), (19, 1000, 2000, 0, 0), (19, 1000, 8000, 0, 0)])
    assert [g.split("rows=")[1].split()[0] for g in got] == ["19", "4", "1"]


def test_plan_header_needs_no_hip():
    with open(os.path.join(CSRC, "knn_range_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
    assert '#include "knn_plan.h"' in text
    for const in ("kKnnDirectBelow", "kKnnColTile", "kKnnKC"):
        assert const in text and "constexpr int " + const not in text        # reused, not restated
