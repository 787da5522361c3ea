"""The offset check every list loader shares (csrc/list_offsets.h) on the host: offsets that start at 0 and never drop, the
noun and the index in the messages, the 2^31 limit of the IVF kinds and its absence for the line index.
tests/cpp/test_list_offsets.cpp is a stand-alone program built with -fsanitize=address,undefined
(tests/cpp/list_offsets.mk); no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_list_offsets_check_on_the_host():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "list_offsets.mk"])
    p = subprocess.run([os.path.join(CPP, "test_list_offsets")], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
