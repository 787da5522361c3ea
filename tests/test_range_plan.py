"""CPU: which read path and how much LDS serve a shape of the IVFFlat range scan is one pure host function
(csrc/range_plan.h: plan_flat_range).  tests/cpp/range_plan_dump.cpp -- host compiler only -- prints the plan of the shapes
below; the expected values are written by hand from the kernel's layout:

  read   tile128 when d % 4 == 0 (rows are 16-byte aligned), dword otherwise
  lds    4 waves x 64 rows x 36 floats of tiles (36864 bytes: the k-NN scan's, without its merge area), 32 bytes for the two
         sets of four per-trip hit counts, roundup16(24 * nprobe + 8) of probe metadata, roundup16(4 * d) for the query;
         no selection queues; at most 160 KiB
  limits 1 <= nprobe <= 1024 (VLQ_MAX_NPROBE), d >= 1
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")
TILES = 4 * 64 * 36 * 4


def r16(x):
    return (x + 15) // 16 * 16


def line(d, nprobe):
    meta = TILES + 32
    sq = meta + r16(24 * nprobe + 8)
    return "d=%d nprobe=%d: read=%s xch=%d meta=%d sq=%d lds=%d" % (d, nprobe, "tile128" if d % 4 == 0 else "dword", TILES, meta, sq,
                                                                    sq + r16(4 * d))


SHAPES = [(32, 5), (128, 6), (128, 32), (30, 3), (5, 3), (3, 3), (36, 6), (100, 6), (16, 4), (4, 1), (1, 1), (128, 1024), (20000, 32)]
UNSUPPORTED = [(32, 1025), (32, 0), (0, 5), (-4, 5), (40000, 5)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("range_plan") / "range_plan_dump")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "range_plan.mk", "OUT=" + exe])

    def run(shapes):
        p = subprocess.run([exe] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()
    return run


def test_plan_of_every_shape(dump):
    got = dump(SHAPES)
    assert got == [line(d, nprobe) for d, nprobe in SHAPES]
    assert got[0] == "d=32 nprobe=5: read=tile128 xch=36864 meta=36896 sq=37024 lds=37152"      # (one written out in full)


def test_limits(dump):
    for got in dump(UNSUPPORTED):
        assert got.endswith(": unsupported"), got
    # the LDS bound on d: the largest d that fits with one probe, and the next; and with every probe
    for nprobe in (1, 1024):
        room = 160 * 1024 - TILES - 32 - r16(24 * nprobe + 8)
        dmax = room // 4
        got = dump([(dmax, nprobe), (dmax + 1, nprobe)])
        assert got[0] == line(dmax, nprobe) and got[0].endswith("lds=%d" % (160 * 1024)) and got[1].endswith(": unsupported")


def test_plan_header_needs_no_hip():
    """range_plan.h is plain C++ over flat_plan.h's constants, and lays out no selection queues"""
    with open(os.path.join(CSRC, "range_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
    assert '#include "flat_plan.h"' in text and "selq" not in text
