"""CPU: the rounding bound of the 16-byte scan's stored-sums loop (csrc/scan_sum_bound.h) holds.  tests/cpp/scan_sum_bound_check.cpp
-- a stand-alone program, host compiler only, built here with the address and undefined-behaviour sanitizers -- draws term-2 rows,
per-query tables and codes (magnitudes 1e-4 .. 1e6, mixed signs, heavy cancellation, offset data), forms the screened value A and
the reference's value D in fp32 as the kernel does and asserts |A - D| <= eps(B) for every code; a non-finite input must give a
non-finite eps."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")


def test_bound_holds_on_random_tables(tmp_path):
    exe = str(tmp_path / "scan_sum_bound_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(CPP, "scan_sum_bound_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.startswith("OK "), p.stdout


def test_bound_header_needs_no_hip():
    """scan_sum_bound.h is plain C++ for host and device, like placement_key.h."""
    with open(os.path.join(CSRC, "scan_sum_bound.h")) as fh:
        text = fh.read()
    assert "#include" not in text
