"""CPU: which query tile, how many code slices, which load width, selection width and LDS layout serve a shape of the exhaustive
Hamming scan is one pure host function (csrc/hamming_plan.h: plan_hamming_scan).  tests/cpp/hamming_plan_dump.cpp -- host
compiler only -- prints the plan of the shapes below; the expected values are written by hand from the rules of the header:

  width   served: 4 bytes, or a multiple of 8 up to 128 (hamming.cpp:482-505)
  kpl     1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
  load    16 (code_size % 16 == 0), else 8 (code_size % 8 == 0), else 4
  S(Q)    forced, else ceil(512 / tiles) with tiles = ceil(min(nq, 32768) / Q), at most the join cap, at most ntotal / 4096, at most
          64, at least 1.  The join cap: isqrt(ntotal * (16 + code_size) / (512 * k)) -- the divisor doubled for k > 256 -- held
          inside 8 .. 64
  Q       forced, else 4 from four queries on where a slice of S(4) holds at least 2 MiB of codes, else 2 from two queries on;
          always 1 for k > 256
  slice   ceil(ntotal / S); join = S > 1
  page    32768 queries, fewer where page * S * k * 8 bytes of partial rows would pass 256 MiB
  lds     merge area roundup16(Q * 4 * k * 8) at 0, then the queues 4 * Q * 64 * 8, then the query codes Q * 128; at most 160 KiB
"""
import itertools
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")


def layout(Q, k):
    selq = (Q * 4 * k * 8 + 15) // 16 * 16
    qcode = selq + 4 * Q * 64 * 8
    return selq, qcode, qcode + Q * 128


# (nq, ntotal, code_size, k, force_q, force_s): Q, S, kpl, load, slice, page
SHAPES = [
    ((1, 1000000, 8, 10, 0, 0), (1, 64, 1, 8, 15625, 32768)),              # one query: cut along the codes only
    ((64, 1000000, 32, 10, 0, 0), (2, 16, 1, 16, 62500, 32768)),
    ((1000, 1000000, 16, 100, 0, 0), (4, 3, 4, 16, 333334, 32768)),        # 5.3 MB of codes per slice: four queries per workgroup
    ((10000, 1000000, 128, 10, 0, 0), (4, 1, 1, 16, 1000000, 32768)),      # a batch that fills the chip: no slices
    ((64, 10000000, 8, 10, 0, 0), (4, 32, 1, 8, 312500, 32768)),           # 2.5 MB per slice at Q = 4
    ((1, 1000000, 8, 100, 0, 0), (1, 21, 4, 8, 47620, 15978)),             # the join cap: isqrt(1e6 * 24 / 51200) = 21
    ((1, 1000000, 8, 1024, 0, 0), (1, 8, 16, 8, 125000, 4096)),            # ... isqrt(1e6 * 24 / 1048576) = 4: never below 8
    ((10000, 10000000, 8, 1024, 0, 0), (1, 1, 16, 8, 10000000, 32768)),
    ((64, 100000, 4, 10, 0, 0), (2, 16, 1, 4, 6250, 32768)),
    ((64, 100000, 24, 10, 0, 0), (2, 16, 1, 8, 6250, 32768)),              # 24 = 8 * 3: pieces of 8
    ((64, 100000, 40, 65, 0, 0), (2, 12, 4, 8, 8334, 32768)),              # the join cap: isqrt(1e5 * 56 / 33280) = 12
    ((5, 2000, 8, 10, 0, 0), (2, 1, 1, 8, 2000, 32768)),                   # too few codes for a slice
    ((5, 2000, 8, 256, 4, 0), (4, 1, 4, 8, 2000, 32768)),
    ((5, 2000, 8, 257, 4, 7), (1, 7, 16, 8, 286, 18651)),                  # k > 256: one query whatever is asked; 2^28 / (7 * 257 * 8)
    ((5, 2000, 8, 10, 4, 7), (4, 7, 1, 8, 286, 32768)),
    ((5, 1, 8, 10, 1, 64), (1, 64, 1, 8, 1, 32768)),                       # more slices than codes: the others are empty
    ((5, 0, 8, 10, 0, 0), (2, 1, 1, 8, 0, 32768)),                         # an empty index
    ((40000, 100000, 64, 1024, 1, 64), (1, 64, 16, 16, 1563, 512)),        # the scratch bound pages the queries
]
REFUSED = [
    ((5, 2000, 13, 10, 0, 0), "code width not served"),
    ((5, 2000, 12, 10, 0, 0), "code width not served"),
    ((5, 2000, 136, 10, 0, 0), "code width not served"),
    ((5, 2000, 0, 10, 0, 0), "code width not served"),
    ((5, 2000, 8, 1025, 0, 0), "k outside 1..1024"),
    ((5, 2000, 8, 0, 0, 0), "k outside 1..1024"),
    ((5, 1 << 32, 8, 10, 0, 0), "ntotal beyond the key's 32-bit position"),
    ((5, -1, 8, 10, 0, 0), "ntotal beyond the key's 32-bit position"),
    ((0, 2000, 8, 10, 0, 0), "no queries"),
    ((5, 2000, 8, 10, 3, 0), "query tile must be 1, 2 or 4"),
    ((5, 2000, 8, 10, 0, 65), "slices outside 1..64"),
]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hamming_plan") / "hamming_plan_dump")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "hamming_plan.mk", "OUT=" + exe])

    def run(shapes):
        p = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()
    return run


def test_plan_of_every_shape(dump):
    got = dump([s for s, _w in SHAPES])
    assert len(got) == len(SHAPES)
    for line, ((nq, nt, cs, k, fq, fs), (Q, S, kpl, load, slc, page)) in zip(got, SHAPES):
        selq, qcode, lds = layout(Q, k)
        want = "nq=%d ntotal=%d cs=%d k=%d fq=%d fs=%d: Q=%d S=%d waves=4 kpl=%d load=%d join=%d slice=%d page=%d selq=%d qcode=%d lds=%d" % (
            nq, nt, cs, k, fq, fs, Q, S, kpl, load, S > 1, slc, page, selq, qcode, lds)
        assert line == want


def test_refusals(dump):
    got = dump([s for s, _w in REFUSED])
    assert len(got) == len(REFUSED)
    for line, (_s, why) in zip(got, REFUSED):
        assert ": unsupported (" + why in line, line


def test_grid(dump):
    """over a grid of shapes: the rules of the docstring, the LDS layout under 160 KB, the slices covering ntotal exactly"""
    grid = list(itertools.product((1, 2, 700, 32768 + 5), (0, 1, 4097, 100000, 10 ** 7), (4, 8, 16, 24, 32, 40, 64, 128),
                                  (1, 64, 65, 256, 257, 1024), (0, 1, 2, 4), (0, 3, 64)))
    got = dump(grid)
    assert len(got) == len(grid)
    pat = re.compile(r"Q=(\d+) S=(\d+) waves=4 kpl=(\d+) load=(\d+) join=(\d) slice=(\d+) page=(\d+) selq=(\d+) qcode=(\d+) lds=(\d+)$")
    for line, (nq, nt, cs, k, fq, fs) in zip(got, grid):
        m = pat.search(line)
        assert m, line
        Q, S, kpl, load, join, slc, page, selq, qcode, lds = (int(v) for v in m.groups())
        assert kpl == (1 if k <= 64 else 4 if k <= 256 else 16)
        assert load == (16 if cs % 16 == 0 else 8 if cs % 8 == 0 else 4) and cs % load == 0

        def slices(q):
            if fs:
                return fs
            tiles = (min(nq, 32768) + q - 1) // q
            cap = max(8, min(64, math.isqrt(nt * (16 + cs) // (512 * k * (2 if kpl == 16 else 1)))))
            return max(1, min((512 + tiles - 1) // tiles, cap, nt // 4096, 64))
        wide = nq >= 4 and (nt + slices(4) - 1) // slices(4) * cs >= 2 << 20
        assert Q == (1 if kpl == 16 else fq if fq else 4 if wide else 2 if nq >= 2 else 1)
        assert S == slices(Q)
        assert join == (S > 1) and slc == ((nt + S - 1) // S if nt else 0)
        assert sum(min(slc, max(0, nt - s * slc)) for s in range(S)) == nt, line
        assert page == (max(1, min(32768, (256 << 20) // (S * k * 8))) if S > 1 else 32768)
        assert (selq, qcode, lds) == layout(Q, k) and lds <= 160 * 1024 and selq % 16 == 0 and qcode % 16 == 0


def test_plan_header_needs_no_hip():
    with open(os.path.join(CSRC, "hamming_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
