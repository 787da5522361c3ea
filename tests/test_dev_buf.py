"""The ownership rules of the device buffer (csrc/dev_buf.h) on the host: growth and its two allocation attempts, the
destructor, moves, std::swap, no copies.  tests/cpp/test_dev_buf.cpp instantiates the template over a counting allocator and
is a stand-alone program built with -fsanitize=address,undefined (tests/cpp/dev_buf.mk); no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_dev_buf_ownership_on_the_host():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "dev_buf.mk"])
    p = subprocess.run([os.path.join(CPP, "test_dev_buf")], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
