"""CPU: which query tile, how many code slices, which operation order, read path, selection width and LDS layout serve a shape of
the flat scalar-quantizer scan is one pure host function (csrc/sqflat_plan.h: plan_sqflat_scan).  tests/cpp/sqflat_plan_dump.cpp
-- host compiler only -- prints the plan of the shapes below; the expected values are written by hand from the rules of the
header:

  kpl     1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
  codec   bits 8 / 4 and uniform from the quantizer type; code_size d at 8 bits, (d + 1) / 2 at 4; order8 = d % 8 == 0
  read    tile128 when order8 and code_size % 16 == 0, else lane (the rule of sq_plan.h)
  Q       forced, else 4 from four queries on, 2 from two on; always 1 for k > 256; halved until the layout fits 160 KB
  S       forced, else ceil(512 / tiles) with tiles = ceil(min(nq, 32768) / Q), at most ntotal / 4096, at most 64, at least 1
  slice   ceil(ntotal / S); join = S > 1
  page    32768 queries, fewer where page * S * k * 8 bytes of partial rows would pass 256 MiB
  lds     max(4 * 64 * 144 bytes of turn tiles, the merge area Q * 4 * k * 8) at 0, then the queues 4 * Q * 64 * 8, the queries
          roundup16(d * Q * 4), and for the non-uniform types vmin and vdiff of roundup16(d * 4) each
"""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")
WHY_LDS = "the query, the range and the tiles do not fit 160 KB of LDS"


def r16(n):
    return (n + 15) // 16 * 16


def layout(Q, d, k, uniform):
    selq = r16(max(4 * 64 * 144, Q * 4 * k * 8))
    sq = selq + 4 * Q * 64 * 8
    vmin = sq + r16(d * Q * 4)
    vdiff = vmin + (0 if uniform else r16(d * 4))
    return selq, sq, vmin, vdiff, vdiff + (0 if uniform else r16(d * 4))


# (nq, ntotal, d, qtype, k, force_q, force_s): Q, S, kpl, order8, read, bits, uniform, code_size, slice, page
SHAPES = [
    ((1, 1000000, 128, 0, 10, 0, 0), (1, 64, 1, 1, "tile128", 8, 0, 128, 15625, 32768)),         # one query: cut along the codes only
    ((64, 1000000, 128, 0, 10, 0, 0), (4, 32, 1, 1, "tile128", 8, 0, 128, 31250, 32768)),
    ((1000, 1000000, 128, 1, 100, 0, 0), (4, 3, 4, 1, "tile128", 4, 0, 64, 333334, 32768)),
    ((10000, 1000000, 128, 2, 10, 0, 0), (4, 1, 1, 1, "tile128", 8, 1, 128, 1000000, 32768)),    # a batch that fills the chip: no slices
    ((10000, 1000000, 128, 0, 1024, 0, 0), (1, 1, 16, 1, "tile128", 8, 0, 128, 1000000, 32768)),
    ((1, 1000000, 128, 0, 1024, 0, 0), (1, 64, 16, 1, "tile128", 8, 0, 128, 15625, 512)),         # 2^28 / (64 * 1024 * 8)
    ((3, 100000, 40, 0, 10, 0, 0), (2, 24, 1, 1, "lane", 8, 0, 40, 4167, 32768)),                 # rows of 40 bytes: not 16-byte aligned
    ((3, 100000, 48, 1, 10, 0, 0), (2, 24, 1, 1, "lane", 4, 0, 24, 4167, 32768)),
    ((3, 100000, 32, 3, 10, 0, 0), (2, 24, 1, 1, "tile128", 4, 1, 16, 4167, 32768)),              # one 16-byte unit per row
    ((5, 2000, 33, 1, 10, 0, 0), (4, 1, 1, 0, "lane", 4, 0, 17, 2000, 32768)),                    # scalar order; too few codes for a slice
    ((5, 2000, 30, 0, 257, 4, 7), (1, 7, 16, 0, "lane", 8, 0, 30, 286, 18651)),                   # k > 256: one query whatever is asked
    ((5, 2000, 8, 0, 256, 4, 7), (4, 7, 4, 1, "lane", 8, 0, 8, 286, 18724)),                       # 2^28 / (7 * 256 * 8)
    ((5, 1, 5, 0, 10, 1, 64), (1, 64, 1, 0, "lane", 8, 0, 5, 1, 32768)),                          # more slices than codes: the others are empty
    ((5, 0, 32, 0, 10, 0, 0), (4, 1, 1, 1, "tile128", 8, 0, 32, 0, 32768)),                       # an empty index
    ((40000, 100000, 64, 0, 1024, 1, 64), (1, 64, 16, 1, "tile128", 8, 0, 64, 1563, 512)),        # the scratch bound pages the queries
    ((100, 100000, 4000, 0, 10, 0, 0), (4, 21, 1, 1, "tile128", 8, 0, 4000, 4762, 32768)),       # 36864 + 8192 + 64000 + 32000 bytes
    ((100, 100000, 5000, 0, 10, 0, 0), (2, 11, 1, 1, "lane", 8, 0, 5000, 9091, 32768)),           # 165 056 bytes at four queries: two
    ((100, 100000, 6000, 0, 10, 0, 0), (2, 11, 1, 1, "tile128", 8, 0, 6000, 9091, 32768)),
    ((100, 100000, 8000, 0, 10, 0, 0), (1, 6, 1, 1, "tile128", 8, 0, 8000, 16667, 32768)),        # 168 960 bytes at two queries: one
    ((100, 100000, 16000, 2, 10, 0, 0), (1, 6, 1, 1, "tile128", 8, 1, 16000, 16667, 32768)),      # ... one
]
REFUSED = [
    ((5, 2000, 32, 0, 1025, 0, 0), "k outside 1..1024"),
    ((5, 2000, 32, 0, 0, 0, 0), "k outside 1..1024"),
    ((5, 1 << 32, 32, 0, 10, 0, 0), "ntotal beyond the key's 32-bit position"),
    ((5, -1, 32, 0, 10, 0, 0), "ntotal beyond the key's 32-bit position"),
    ((5, 2000, 32, 4, 10, 0, 0), "d or the quantizer type outside the kernel's limits"),
    ((5, 2000, 0, 0, 10, 0, 0), "d or the quantizer type outside the kernel's limits"),
    ((5, 2000, 32, 0, 10, 3, 0), "query tile must be 1, 2 or 4"),
    ((5, 2000, 32, 0, 10, 0, 65), "slices outside 1..64"),
    ((5, 2000, 20000, 0, 10, 0, 0), WHY_LDS),            # 36864 + 2048 + 3 * 80000
    ((5, 2000, 50000, 2, 10, 0, 0), WHY_LDS),
]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sqflat_plan") / "sqflat_plan_dump")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "sqflat_plan.mk", "OUT=" + exe])

    def run(shapes):
        p = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()
    return run


def test_plan_of_every_shape(dump):
    got = dump([s for s, _w in SHAPES])
    assert len(got) == len(SHAPES)
    for line, ((nq, nt, d, qt, k, fq, fs), (Q, S, kpl, o8, read, nbits, uni, cs, slc, page)) in zip(got, SHAPES):
        want = ("nq=%d ntotal=%d d=%d qtype=%d k=%d fq=%d fs=%d: Q=%d S=%d kpl=%d order8=%d read=%s bits=%d uniform=%d code_size=%d join=%d "
                "slice=%d page=%d selq=%d sq=%d vmin=%d vdiff=%d lds=%d" % ((nq, nt, d, qt, k, fq, fs, Q, S, kpl, o8, read, nbits, uni, cs, S > 1, slc, page)
                                                                         + layout(Q, d, k, uni)))
        assert line == want


def test_refusals(dump):
    got = dump([s for s, _w in REFUSED])
    assert len(got) == len(REFUSED)
    for line, (_s, why) in zip(got, REFUSED):
        assert ": unsupported (" + why in line, line


def test_grid(dump):
    """over a grid of shapes: the rules of the docstring, the LDS layout under 160 KB, the slices covering ntotal exactly"""
    grid = list(itertools.product((1, 3, 700, 32768 + 5), (0, 4097, 10 ** 7), (5, 8, 40, 128, 9000), (0, 1, 2, 3),
                                  (1, 64, 65, 256, 257, 1024), (0, 2, 4), (0, 3)))
    got = dump(grid)
    assert len(got) == len(grid)
    pat = re.compile(r"Q=(\d+) S=(\d+) kpl=(\d+) order8=(\d) read=(\w+) bits=(\d) uniform=(\d) code_size=(\d+) join=(\d) slice=(\d+) page=(\d+) "
                     r"selq=(\d+) sq=(\d+) vmin=(\d+) vdiff=(\d+) lds=(\d+)$")
    for line, (nq, nt, d, qt, k, fq, fs) in zip(got, grid):
        m = pat.search(line)
        assert m, line
        Q, S, kpl, o8 = (int(v) for v in m.groups()[:4])
        read = m.group(5)
        nbits, uni, cs, join, slc, page, selq, sq, vmin, vdiff, lds = (int(v) for v in m.groups()[5:])
        assert kpl == (1 if k <= 64 else 4 if k <= 256 else 16)
        assert (nbits, uni) == ((8, 4)[qt & 1], qt >> 1) and cs == (d if nbits == 8 else (d + 1) // 2) and o8 == (d % 8 == 0)
        assert read == ("tile128" if o8 and cs % 16 == 0 else "lane")
        want_q = 1 if kpl == 16 else fq if fq else 4 if nq >= 4 else 2 if nq >= 2 else 1
        while want_q > 1 and layout(want_q, d, k, uni)[4] > 160 * 1024:
            want_q //= 2
        assert Q == want_q
        tiles = (min(nq, 32768) + Q - 1) // Q
        assert S == (fs if fs else max(1, min((512 + tiles - 1) // tiles, nt // 4096, 64)))
        assert join == (S > 1) and slc == ((nt + S - 1) // S if nt else 0)
        assert sum(min(slc, max(0, nt - s * slc)) for s in range(S)) == nt, line
        assert page == (max(1, min(32768, (256 << 20) // (S * k * 8))) if S > 1 else 32768)
        assert (selq, sq, vmin, vdiff, lds) == layout(Q, d, k, uni) and lds <= 160 * 1024
        assert selq % 16 == 0 and sq % 16 == 0 and vmin % 16 == 0 and vdiff % 16 == 0


def test_plan_header_needs_no_hip():
    with open(os.path.join(CSRC, "sqflat_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
