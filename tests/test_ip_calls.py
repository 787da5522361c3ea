"""GPU: tests/cpp/ip_calls.cpp -- the reference's own faiss::IndexIVFPQ with METRIC_INNER_PRODUCT over an IndexFlatIP, through the
interposer (integration/reference_interposer.cpp), against the same member of the reference's library reached through dlsym:
search_knn_with_key and search are served on the device and bit-equal; polysemous_ht > 0 under the metric is left to the
reference's own path.  Runs from what build() left in tests/cpp/ref_drivers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RD = os.path.join(ROOT, "tests", "cpp", "ref_drivers")


@pytest.mark.gpu
def test_inner_product_calls_of_a_user_program():
    exe = os.path.join(RD, "ip_calls")
    if not (os.path.exists(exe) and os.path.exists(os.path.join(ROOT, "oracle/_ref/libfaiss_ref.so"))):
        pytest.skip("tests/cpp/ref_drivers was not prebuilt (needs the reference tree at build time)")
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.join(ROOT, "oracle/_ref/mkl") + ":" + e.get("LD_LIBRARY_PATH", "")
    e.update({"OMP_NUM_THREADS": "8", "OMP_WAIT_POLICY": "passive", "VLQ_INTERPOSE": "on"})
    p = subprocess.run([exe], env=e, capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-600:])
    assert p.returncode == 0 and "ip_calls: PASSED" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
    # three compare() rounds on the device: 2 search_knn_with_key each, a whole search in two of them.  Fallbacks: the polysemous round's 2 calls
    # and the one the reference's own search makes, and the add of the not-by-residual index
    m = re.search(r"device searches=(\d+)", p.stderr)
    assert m and int(m.group(1)) == 8, p.stderr[-600:]
    m = re.search(r"whole_searches=(\d+)", p.stderr)
    assert m and int(m.group(1)) == 2, p.stderr[-600:]
    m = re.search(r"cpu_fallbacks=(\d+)", p.stderr)
    assert m and int(m.group(1)) == 4, p.stderr[-600:]
    m = re.search(r"adds=(\d+) vectors=(\d+)", p.stderr)
    assert m and int(m.group(1)) == 1 and int(m.group(2)) == 30000, p.stderr[-600:]   # by_residual add on the device
