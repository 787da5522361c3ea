"""CPU: which scan kernel serves a page, in which instantiation and with how much LDS, is one pure host function
(csrc/scan_plan.h: plan_scan).  tests/cpp/scan_plan_dump.cpp -- host compiler only, neither the library nor the HIP runtime --
prints the plan of a list of named shapes; tests/golden/scan_plan.txt holds the expected lines, written by hand from the
conditions of scan_dev and the launchers as they were before the plan existed (not dumped from plan_scan)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")


def plan_lines(tmp_path):
    exe = str(tmp_path / "scan_plan_dump")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-I" + CSRC,
                           os.path.join(CPP, "scan_plan_dump.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()


def test_plan_of_every_named_shape(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "scan_plan.txt")) as fh:
        want = fh.read().splitlines()
    got = plan_lines(tmp_path)
    assert [l.split(":")[0] for l in got] == [l.split(":")[0] for l in want]
    for g, w in zip(got, want):
        assert g == w


def test_plan_header_needs_no_hip():
    """scan_plan.h is plain C++: it includes nothing of HIP, so a host compiler builds it alone."""
    with open(os.path.join(CSRC, "scan_plan.h")) as fh:
        text = fh.read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text


def test_thresholds_are_written_once():
    """The list-length classes and the probe metadata's size have one definition under csrc/."""
    hits = {"nlist * 24": 0, "nlist * 1024": 0, "nprobe * 24": 0, "nlist * kShortListCodes": 0, "nlist * kLongListCodes": 0}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".cuh")):
            with open(os.path.join(CSRC, f)) as fh:
                text = fh.read()
            for key in hits:
                hits[key] += text.count(key)
    assert hits == {"nlist * 24": 0, "nlist * 1024": 0, "nprobe * 24": 1, "nlist * kShortListCodes": 1, "nlist * kLongListCodes": 1}, hits
