"""CPU: which query tile, how many code slices, which summation order, filter, load width, selection width and LDS size serve a
shape of the flat PQ scan is one pure host function (csrc/pq_plan.h: plan_pq_scan).  tests/cpp/pq_plan_dump.cpp -- host compiler
only -- prints the plan of the shapes below; the expected values are written by hand from the rules of the header:

  kpl     1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
  order   ST_PQ: 0 (M == 4), 1 (M % 4 == 0), 2 (any other M); every other search type: 2 (from 0, left to right)
  filter  0, 1 (ST_polysemous), 2 (ST_polysemous_generalize); both need M % 8 == 0
  load    16 (M % 16 == 0 under the grouped order or the Hamming filter), else 4 (M % 4 == 0), else 1
  Q       forced, else 1 for k > 256 and for the filtered types, else 2 from two queries on; halved until the LDS fits
  S       forced, else ceil(512 / tiles) with tiles = ceil(min(nq, 32768) / Q), at most ntotal / 4096, at most 64, at least 1
  slice   ceil(ntotal / S); join = S > 1
  page    32768 queries, fewer where page * S * k * 8 bytes of partial rows would pass 256 MiB
  lds     roundup16(max(Q * M * ksub * 4, Q * 4 * k * 8)) + 4 * Q * 64 * 8 + (filter: 4 * Q * 128 * 4 + Q * 64) + 16; at most 160 KiB
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")
PQ, HE, SDC, POLY, POLYGEN = 0, 1, 3, 4, 5


def lds(Q, M, ksub, k, flt):
    return (max(Q * M * ksub * 4, Q * 4 * k * 8) + 15) // 16 * 16 + 4 * Q * 64 * 8 + ((4 * Q * 128 * 4 + Q * 64) if flt else 0) + 16


# (nq, ntotal, M, ksub, k, search type, force_q, force_s): Q, S, kpl, order, filter, load, slice, page
SHAPES = [
    ((1, 1000000, 16, 256, 10, PQ, 0, 0), (1, 64, 1, 1, 0, 16, 15625, 32768)),           # one query: cut along the codes only
    ((64, 1000000, 16, 256, 10, PQ, 0, 0), (2, 16, 1, 1, 0, 16, 62500, 32768)),
    ((1000, 1000000, 16, 256, 100, PQ, 0, 0), (2, 2, 4, 1, 0, 16, 500000, 32768)),
    ((10000, 1000000, 16, 256, 10, PQ, 0, 0), (2, 1, 1, 1, 0, 16, 1000000, 32768)),      # a batch that fills the chip: no slices
    ((10000, 1000000, 16, 256, 1024, PQ, 0, 0), (1, 1, 16, 1, 0, 16, 1000000, 32768)),
    ((10000, 1000000, 16, 256, 10, POLY, 0, 0), (1, 1, 1, 2, 1, 16, 1000000, 32768)),
    ((64, 1000000, 16, 256, 10, POLY, 0, 0), (1, 8, 1, 2, 1, 16, 125000, 32768)),
    ((64, 1000000, 16, 256, 10, POLYGEN, 0, 0), (1, 8, 1, 2, 2, 4, 125000, 32768)),
    ((64, 1000000, 8, 256, 10, POLY, 0, 0), (1, 8, 1, 2, 1, 4, 125000, 32768)),
    ((64, 1000000, 16, 256, 10, SDC, 0, 0), (2, 16, 1, 2, 0, 4, 62500, 32768)),
    ((5, 2000, 4, 256, 10, PQ, 0, 0), (2, 1, 1, 0, 0, 4, 2000, 32768)),                   # M == 4; too few codes for a slice
    ((5, 2000, 6, 256, 10, PQ, 0, 0), (2, 1, 1, 2, 0, 1, 2000, 32768)),                   # M % 4 != 0: bytes, left to right
    ((5, 2000, 20, 64, 65, PQ, 0, 0), (2, 1, 4, 1, 0, 4, 2000, 32768)),
    ((5, 2000, 64, 256, 256, PQ, 4, 0), (2, 1, 4, 1, 0, 16, 2000, 32768)),                # four tables of 64 KB do not fit: halved
    ((5, 2000, 16, 256, 257, PQ, 4, 7), (1, 7, 16, 1, 0, 16, 286, 18651)),                # k > 256: one query whatever is asked; 2^28 / (7 * 257 * 8)
    ((5, 2000, 16, 256, 10, PQ, 4, 7), (4, 7, 1, 1, 0, 16, 286, 32768)),
    ((5, 0, 16, 256, 10, PQ, 0, 0), (2, 1, 1, 1, 0, 16, 0, 32768)),                       # an empty index
    ((40000, 100000, 16, 256, 1024, PQ, 1, 64), (1, 64, 16, 1, 0, 16, 1563, 512)),        # the scratch bound pages the queries
]
UNSUPPORTED = [(5, 2000, 16, 256, 10, HE, 0, 0), (5, 2000, 16, 256, 10, 2, 0, 0), (5, 2000, 12, 256, 10, POLY, 0, 0), (5, 2000, 65, 256, 10, PQ, 0, 0),
               (5, 2000, 16, 256, 1025, PQ, 0, 0), (5, 2000, 16, 256, 0, PQ, 0, 0), (5, 2000, 16, 512, 10, PQ, 0, 0), (5, 1 << 32, 16, 256, 10, PQ, 0, 0),
               (5, 2000, 16, 256, 10, PQ, 3, 0), (5, 2000, 16, 256, 10, PQ, 0, 65), (0, 2000, 16, 256, 10, PQ, 0, 0)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pq_plan") / "pq_plan_dump")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(CPP, "pq_plan_dump.cpp"),
                           "-o", exe])

    def run(shapes):
        p = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()
    return run


def test_plan_of_every_shape(dump):
    got = dump([s for s, _w in SHAPES])
    assert len(got) == len(SHAPES)
    for line, ((nq, nt, M, ksub, k, st, fq, fs), (Q, S, kpl, order, flt, load, slc, page)) in zip(got, SHAPES):
        want = "nq=%d ntotal=%d M=%d ksub=%d k=%d st=%d fq=%d fs=%d: Q=%d S=%d waves=4 kpl=%d order=%d filter=%d load=%d join=%d slice=%d page=%d lds=%d" % (
            nq, nt, M, ksub, k, st, fq, fs, Q, S, kpl, order, flt, load, S > 1, slc, page, lds(Q, M, ksub, k, flt))
        assert line == want


def test_limits(dump):
    for line in dump(UNSUPPORTED):
        assert ": unsupported (" in line, line
    # the LDS bound: M = 64 tables of one query are 64 KB, a k = 1024 merge area 32 KB: served at Q = 1
    got = dump([(5, 2000, 64, 256, 1024, PQ, 0, 0)])
    assert "Q=1 " in got[0] and "lds=%d" % lds(1, 64, 256, 1024, 0) in got[0] and lds(1, 64, 256, 1024, 0) <= 160 * 1024


def test_plan_header_needs_no_hip():
    with open(os.path.join(CSRC, "pq_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
