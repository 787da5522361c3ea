"""The key that sorts queries onto the XCDs (csrc/placement_key.h) on the host: a vote with a clear majority, a tie that goes
to the nearest probe, invalid keys, and no list_part (the key as it was).  tests/cpp/test_placement_key.cpp is a stand-alone
program built with -fsanitize=address,undefined (tests/cpp/placement_key.mk); no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_placement_key_on_the_host():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "placement_key.mk"])
    p = subprocess.run([os.path.join(CPP, "test_placement_key")], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
