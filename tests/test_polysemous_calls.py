"""GPU: tests/cpp/polysemous_calls.cpp -- the reference's own faiss::IndexIVFPQ with polysemous_ht set, through the interposer
(integration/reference_interposer.cpp), against the same member of the reference's library reached through dlsym: served on
the device and bit-equal where the code of the query is the reference's (not by_residual, multi-index type 2), left to the
reference's own path for a by-residual index over a flat quantizer.  Runs from what build() left in tests/cpp/ref_drivers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RD = os.path.join(ROOT, "tests", "cpp", "ref_drivers")


def _env(extra):
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.join(ROOT, "oracle/_ref/mkl") + ":" + e.get("LD_LIBRARY_PATH", "")
    e["OMP_NUM_THREADS"] = "8"
    e["OMP_WAIT_POLICY"] = "passive"
    e.update(extra)
    return e


@pytest.mark.gpu
def test_polysemous_calls_of_a_user_program():
    exe = os.path.join(RD, "polysemous_calls")
    if not (os.path.exists(exe) and os.path.exists(os.path.join(ROOT, "oracle/_ref/libfaiss_ref.so"))):
        pytest.skip("tests/cpp/ref_drivers was not prebuilt (needs the reference tree at build time)")
    p = subprocess.run([exe], env=_env({"VLQ_INTERPOSE": "on"}), capture_output=True, text=True, timeout=900)
    print(p.stdout[-4000:], p.stderr[-600:])
    assert p.returncode == 0 and "polysemous_calls: PASSED" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"cpu_fallbacks=(\d+)", p.stderr)
    # the by-residual flat index: its 10 calls (5 thresholds x store_pairs off / on) took the reference's own path, the other 20 the device
    assert m and int(m.group(1)) == 10, p.stderr[-600:]
    m = re.search(r"searches=(\d+)", p.stderr)
    assert m and int(m.group(1)) == 20, p.stderr[-600:]
    # ... with the same rows as a run that never touches the device
    q = subprocess.run([exe], env=_env({"VLQ_INTERPOSE": "off"}), capture_output=True, text=True, timeout=900)
    rows = lambda out: [l for l in out.splitlines() if l.startswith("by_residual flat")]
    assert q.returncode == 0 and rows(q.stdout) == rows(p.stdout) and len(rows(p.stdout)) == 10
