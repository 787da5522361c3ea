"""CPU: which read path, operation order, selection width and LDS size serve a shape of the IVF scalar-quantizer scan is one pure
host function (csrc/sq_plan.h: plan_sq_scan).  tests/cpp/sq_plan_dump.cpp -- host compiler only -- prints the plan of the shapes
below; the expected values are written by hand from the rules of the header and the kernel's layout:

  order8     d % 8 == 0 (the reference takes its AVX quantizer classes exactly then)
  read       tile128 when order8 and code_size % 16 == 0, lane otherwise
  code_size  d at 8 bits, (d + 1) / 2 at 4 bits
  kpl        1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
  lds        max(4 * 64 * 144 tile bytes, 4 * k * 8 merge bytes) + 2048 (queues) + roundup16(24 * nprobe + 8) + 16
             + 4 * roundup16(4 * d)          (the query, vmin, vdiff, the probe's residual); at most 160 KiB
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")
Q8, Q4, Q8U, Q4U = 0, 1, 2, 3


def r16(x):
    return (x + 15) // 16 * 16


def lds(d, nprobe, k):
    return r16(max(4 * 64 * 144, 4 * k * 8)) + 2048 + r16(24 * nprobe + 8) + 16 + 4 * r16(4 * d)


# (d, qtype, nprobe, k): kpl, bits, uniform, order8, code_size, read
SHAPES = [
    ((128, Q8, 32, 10), (1, 8, 0, 1, 128, "tile128")),        # the headline shape
    ((128, Q4, 32, 10), (1, 4, 0, 1, 64, "tile128")),
    ((32, Q8U, 5, 10), (1, 8, 1, 1, 32, "tile128")),
    ((32, Q4U, 5, 100), (4, 4, 1, 1, 16, "tile128")),
    ((16, Q8, 5, 10), (1, 8, 0, 1, 16, "tile128")),
    ((16, Q4, 5, 10), (1, 4, 0, 1, 8, "lane")),               # 8-byte rows
    ((40, Q8, 4, 10), (1, 8, 0, 1, 40, "lane")),              # AVX order, rows not 16-byte aligned
    ((48, Q4, 4, 10), (1, 4, 0, 1, 24, "lane")),
    ((136, Q8, 4, 10), (1, 8, 0, 1, 136, "lane")),
    ((8, Q8, 3, 10), (1, 8, 0, 1, 8, "lane")),
    ((30, Q8, 3, 10), (1, 8, 0, 0, 30, "lane")),              # scalar order
    ((33, Q4, 3, 10), (1, 4, 0, 0, 17, "lane")),
    ((31, Q4, 3, 10), (1, 4, 0, 0, 16, "lane")),              # 16-byte rows, but the scalar order: no tiles
    ((5, Q8, 3, 1024), (16, 8, 0, 0, 5, "lane")),
    ((32, Q8, 1024, 1024), (16, 8, 0, 1, 32, "tile128")),
    ((32, Q8, 3, 64), (1, 8, 0, 1, 32, "tile128")),           # the edges of the selection widths
    ((32, Q8, 3, 65), (4, 8, 0, 1, 32, "tile128")),
    ((32, Q8, 3, 256), (4, 8, 0, 1, 32, "tile128")),
    ((32, Q8, 3, 257), (16, 8, 0, 1, 32, "tile128")),
]
UNSUPPORTED = [(32, Q8, 1025, 10), (32, Q8, 5, 1025), (32, 4, 5, 10), (0, Q8, 5, 10), (32, Q8, 0, 10), (12000, Q8, 5, 10)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sq_plan") / "sq_plan_dump")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(CPP, "sq_plan_dump.cpp"),
                           "-o", exe])

    def run(shapes):
        p = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()
    return run


def test_plan_of_every_shape(dump):
    got = dump([s for s, _w in SHAPES])
    assert len(got) == len(SHAPES)
    for line, ((d, qt, nprobe, k), (kpl, nbits, uni, o8, cs, read)) in zip(got, SHAPES):
        want = "d=%d qtype=%d nprobe=%d k=%d: kpl=%d bits=%d uniform=%d order8=%d code_size=%d read=%s lds=%d" % (
            d, qt, nprobe, k, kpl, nbits, uni, o8, cs, read, lds(d, nprobe, k))
        assert line == want


def test_limits(dump):
    for line in dump(UNSUPPORTED):
        assert line.endswith(": unsupported"), line
    # the LDS bound on d: the largest d that fits with one probe, and the next
    dmax = max(d for d in range(7000, 9000, 4) if lds(d, 1, 1) <= 160 * 1024)
    got = dump([(dmax, Q8, 1, 1), (dmax + 4, Q8, 1, 1)])
    assert "lds=%d" % lds(dmax, 1, 1) in got[0] and got[1].endswith(": unsupported")


def test_plan_header_needs_no_hip():
    with open(os.path.join(CSRC, "sq_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
