"""CPU: path, route, row tile, slices, chunk, page, LDS and scratch of the flat exact k-NN scan are one pure host function
(csrc/knn_plan.h: plan_knn).  tests/cpp/knn_plan_dump.cpp -- host compiler only -- prints the plan of the shapes below; the
expected values follow from the rules of the header:

  path     direct when nq < 20 and d % 4 == 0 (the whole call's nq), gemm otherwise
  route    fused for gemm with k <= 256; matrix for gemm with larger k and for direct
  rows     fused: forced, else 128 from 2048 queries on, 64 from 512, else 32; halved until the LDS fits (k > 64: 32)
           direct: 1, 4 or 19 queries in LDS, the smallest that holds the call, fewer while 4 * rows * d + 36864 passes 160 KiB
  S        fused: forced (never below one 128-column tile), else ceil(512 / row tiles), at most ntotal / 2048, 64; at least 1
  lds      fused: roundup16(max(2 * (rows + 128) * 36 * 4, rows * 129 * 4)) + rows * 64 * kpl * 8 + rows * 8 + 2048
  scratch  no term in nq * ntotal: at most 256 MiB whatever the shape
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")
LDS_LIMIT = 160 * 1024
SCRATCH_LIMIT = 256 << 20


def fused_lds(rows, kpl):
    return (max(2 * (rows + 128) * 36 * 4, rows * 129 * 4) + 15) // 16 * 16 + rows * 64 * kpl * 8 + rows * 8 + 2048


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knn_plan") / "knn_plan_dump")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "knn_plan.mk", "OUT=" + exe])

    def run(shapes):
        out = []
        for i in range(0, len(shapes), 512):        # (the command line is finite)
            p = subprocess.run([exe] + [str(v) for s in shapes[i:i + 512] for v in s], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, p.stderr
            out += p.stdout.splitlines()
        assert len(out) == len(shapes)
        return [dict(re.findall(r"(\w+)=(\S+)", ln.split(": ", 1)[1])) if ": unsupported" not in ln else None for ln in out]
    return run


def test_dispatch_boundary(dump):
    """20 queries and d % 4, nothing else, decide the path"""
    shapes = [(19, 1000, 128, 10, 0, 0), (20, 1000, 128, 10, 0, 0), (19, 1000, 30, 10, 0, 0), (1, 1000, 4, 10, 0, 0), (1, 1000, 3, 10, 0, 0),
              (19, 1000, 128, 1024, 0, 0), (20, 1000, 128, 256, 0, 0), (20, 1000, 128, 257, 0, 0), (40000, 1000, 8, 5, 0, 0)]
    want = [("direct", "matrix"), ("gemm", "fused"), ("gemm", "fused"), ("direct", "matrix"), ("gemm", "fused"), ("direct", "matrix"),
            ("gemm", "fused"), ("gemm", "matrix"), ("gemm", "fused")]
    for p, (path, route) in zip(dump(shapes), want):
        assert (p["path"], p["route"]) == (path, route)


def test_plan_of_chosen_shapes(dump):
    got = dump([(64, 1000000, 128, 10, 0, 0), (10000, 1000000, 128, 10, 0, 0), (1000, 1000000, 128, 100, 0, 0), (300, 4999, 128, 10, 128, 7),
                (300, 4999, 128, 65, 128, 7), (1, 1000000, 128, 10, 0, 0), (16, 1000000, 128, 10, 0, 0), (19, 1000, 2048, 10, 0, 0)])
    assert (got[0]["rows"], got[0]["S"], got[0]["kpl"], got[0]["slice"], got[0]["lds"]) == ("32", "64", "1", "15625", str(fused_lds(32, 1)))
    assert (got[1]["rows"], got[1]["S"], got[1]["slice"], got[1]["page"], got[1]["lds"]) == ("128", "7", "142858", "32768", str(fused_lds(128, 1)))
    assert (got[2]["rows"], got[2]["S"], got[2]["kpl"], got[2]["lds"]) == ("32", "16", "4", str(fused_lds(32, 4)))
    assert (got[3]["rows"], got[3]["S"], got[3]["slice"], got[3]["join"]) == ("128", "7", "715", "1")
    assert (got[4]["rows"], got[4]["S"], got[4]["kpl"]) == ("32", "7", "4")          # a forced tile that does not fit shrinks
    assert (got[5]["rows"], got[5]["chunk"]) == ("1", "1000000")
    assert (got[6]["rows"], got[6]["S"]) == ("19", "64")
    assert got[7]["rows"] == "4"                                                     # 19 queries of d = 2048 do not fit beside the tiles


def test_lds_within_160k(dump):
    shapes = [(nq, 100000, d, k, fr, 0) for d in (1, 128, 2048) for k in range(1, 1025) for nq, fr in ((19, 0), (20, 0), (5000, 128))]
    for s, p in zip(shapes, dump(shapes)):
        assert p is not None, s
        assert int(p["lds"]) <= LDS_LIMIT, (s, p)
        if p["route"] == "fused":
            assert int(p["lds"]) == fused_lds(int(p["rows"]), int(p["kpl"]))


def test_scratch_is_bounded(dump):
    """no term in nq * ntotal: the largest shapes stay under 256 MiB by paging the queries and chunking the columns"""
    shapes = [(32768, 10 ** 8, d, k, fr, fs) for d in (8, 128, 130) for k in (1, 64, 256, 257, 1024) for fr, fs in ((0, 0), (32, 64), (128, 64))]
    shapes += [(19, 10 ** 8, 128, k, 0, fs) for k in (1, 1024) for fs in (0, 64)]
    shapes += [(1, (1 << 32) - 1, 4, 1024, 0, 0), (20, (1 << 32) - 1, 4, 1024, 0, 0)]
    for s, p in zip(shapes, dump(shapes)):
        assert p is not None, s
        assert int(p["scratch"]) <= SCRATCH_LIMIT, (s, p)
        assert 1 <= int(p["page"]) <= 32768
        nq, ntotal = s[0], s[1]
        assert int(p["scratch"]) < nq * ntotal            # (and far from it)


def test_slices_never_below_a_column_tile(dump):
    shapes = [(300, nt, 128, k, 0, fs) for nt in (1, 100, 127, 128, 129, 300, 1000, 4999) for k in (10, 1024) for fs in (0, 2, 7, 64)]
    shapes += [(5, nt, 128, 10, 0, fs) for nt in (1, 100, 300, 4999) for fs in (0, 7, 64)]
    for s, p in zip(shapes, dump(shapes)):
        S, slc = int(p["S"]), int(p["slice"])
        assert S >= 1
        if S > 1:
            assert slc >= 128, (s, p)
        width = int(p["chunk"]) if p["route"] == "matrix" else s[1]
        assert S * slc >= width                           # the slices cover the columns


def test_limits(dump):
    bad = [(0, 1000, 8, 10, 0, 0), (5, 1000, 0, 10, 0, 0), (5, 1000, 8, 0, 0, 0), (5, 1000, 8, 1025, 0, 0), (5, 1 << 32, 8, 10, 0, 0),
           (5, 1000, 8, 10, 48, 0), (5, 1000, 8, 10, 0, 65), (19, 1000, 40000, 10, 0, 0)]
    assert all(p is None for p in dump(bad))


def test_plan_header_needs_no_hip():
    with open(os.path.join(CSRC, "knn_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
