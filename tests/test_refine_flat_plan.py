"""CPU: read path, trips, sorted slots, waves, page and LDS of the flat re-ranking kernel are one pure host function
(csrc/refine_flat_plan.h: plan_refine_flat).  tests/cpp/refine_flat_plan_dump.cpp -- host compiler only -- prints the plan of
the shapes below; the expected values follow from the rules of the header:

  read     tile128 when d % 4 == 0 (gathered 64 x 128 B tiles), dword otherwise
  trips    ceil(k_base / 64)
  slots    the next power of two at or above k_base, 64 at least
  waves    1 for one trip, 2 for two or three, 4 from four trips on
  lds      waves * 64 * 36 * 4 (the row tiles) + 16 * slots (keys and labels; none without the selection) + roundup16(4 d)
  limits   1 <= k <= k_base <= 1024 and d >= 1, else invalid; a query row that does not fit 160 KiB: unsupported
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")
LDS_LIMIT = 160 * 1024


def want_plan(d, k_base, select=True):
    trips = (k_base + 63) // 64
    slots = 64
    while slots < k_base:
        slots *= 2
    waves = 4 if trips >= 4 else 2 if trips >= 2 else 1
    lds = waves * 64 * 36 * 4 + (16 * slots if select else 0) + (4 * d + 15) // 16 * 16
    return dict(read="tile128" if d % 4 == 0 else "dword", trips=trips, slots=slots, waves=waves, lds=lds)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("refine_flat_plan") / "refine_flat_plan_dump")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "refine_flat_plan.mk", "OUT=" + exe])

    def run(shapes):
        out = []
        for i in range(0, len(shapes), 512):        # (the command line is finite)
            p = subprocess.run([exe] + [str(v) for s in shapes[i:i + 512] for v in s], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, p.stderr
            out += p.stdout.splitlines()
        assert len(out) == len(shapes)
        res = []
        for ln in out:
            body = ln.split(": ", 1)[1]
            res.append(body.split(" ", 1)[0] if body.startswith(("invalid", "unsupported")) else dict(re.findall(r"(\w+)=(\S+)", body)))
        return res
    return run


def test_every_k_base_and_lds_within_160k(dump):
    shapes = [(d, kb, k, 1) for d in (1, 128, 2048) for kb in range(1, 1025) for k in sorted({1, kb // 2 + 1, kb})]
    for s, p in zip(shapes, dump(shapes)):
        assert isinstance(p, dict), (s, p)
        w = want_plan(s[0], s[1])
        assert (p["read"], int(p["trips"]), int(p["slots"]), int(p["waves"]), int(p["lds"])) == \
            (w["read"], w["trips"], w["slots"], w["waves"], w["lds"]), (s, p)
        assert int(p["lds"]) <= LDS_LIMIT
        assert int(p["page"]) == 32768
        # the areas follow each other without overlap: tiles, keys [slots], labels [slots], the query row
        assert int(p["keys"]) == int(p["waves"]) * 9216 and int(p["labels"]) == int(p["keys"]) + 8 * int(p["slots"])
        assert int(p["sq"]) == int(p["labels"]) + 8 * int(p["slots"]) and int(p["sq"]) % 16 == 0
        assert int(p["slots"]) >= s[1] and int(p["trips"]) * 64 >= s[1] and int(p["slots"]) >= int(p["trips"]) * 64


def test_subset_plan_keeps_no_keys(dump):
    shapes = [(d, kb, kb, 0) for d in (1, 128, 2048) for kb in (1, 64, 65, 128, 129, 256, 257, 1024)]
    for s, p in zip(shapes, dump(shapes)):
        w = want_plan(s[0], s[1], select=False)
        assert (int(p["waves"]), int(p["lds"])) == (w["waves"], w["lds"]), (s, p)
        assert int(p["keys"]) == int(p["labels"]) == int(p["sq"])


def test_wave_thresholds(dump):
    kbs = [1, 64, 65, 128, 129, 192, 193, 256, 257, 1024]
    got = dump([(128, kb, 1, 1) for kb in kbs])
    assert [int(p["waves"]) for p in got] == [1, 1, 2, 2, 2, 2, 4, 4, 4, 4]
    assert [int(p["slots"]) for p in got] == [64, 64, 128, 128, 256, 256, 256, 256, 512, 1024]


def test_limits(dump):
    invalid = [(0, 10, 5, 1), (8, 0, 0, 1), (8, 10, 0, 1), (8, 10, 11, 1), (8, 1025, 10, 1), (8, 1025, 1025, 0), (-4, 10, 5, 1)]
    assert dump(invalid) == ["invalid"] * len(invalid)
    # one query row beside the tiles and the keys: 4 d <= 160 KiB - 4 * 9216 - 16 * 1024 at k_base 1024
    edge = (LDS_LIMIT - 4 * 9216 - 16 * 1024) // 4
    got = dump([(edge, 1024, 10, 1), (edge + 4, 1024, 10, 1), (40000, 10, 5, 1), (1 << 20, 1, 1, 0)])
    assert isinstance(got[0], dict) and int(got[0]["lds"]) == LDS_LIMIT
    assert got[1:] == ["unsupported"] * 3


def test_plan_header_needs_no_hip():
    with open(os.path.join(CSRC, "refine_flat_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
