"""faiss::IndexPQ of the C++ shell (include/faiss_amd/IndexPQ.h): on CPU the class surface, the defaults and the throws, and
the "IxPq" record the reference wrote is read, compared field by field and written again byte for byte ("IxPQ" / "IxPo" are
read too); on the GPU box tests/cpp/test_indexpq_shell builds the index from a fixture's codes or vectors, searches and
compares with the reference's rows and indexPQ_stats."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pq")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "indexpq_shell.mk"])
    return os.path.join(CPP, "test_indexpq_shell")


def export_case(name, d, run=0):
    """the fixture's arrays as raw files (what the binary reads); run: which of the recorded searches"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    ht = int(z["hts"][run]) if "hts" in z.files else 0
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d %d %d\n" % (z["d"], z["M"], z["nbits"], z["codes"].shape[0], z["xq"].shape[0], z["k"], z["metric"],
                                                 z["search_type"], ht))
    for fn, a, dt in (("cent.f32", z["centroids"], np.float32), ("xq.f32", z["xq"], np.float32), ("D.f32", z["D%d" % run], np.float32),
                      ("I.i64", z["I%d" % run], np.int64), ("stats.i64", z["stats%d" % run], np.int64), ("codes.u8", z["codes"], np.uint8)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, fn))
    if "xb" in z.files:
        np.ascontiguousarray(z["xb"], dtype=np.float32).tofile(os.path.join(d, "xb.f32"))
    if "index_bytes" in z.files:
        z["index_bytes"].tofile(os.path.join(d, "index.bin"))


def test_class_surface_and_ixpq_record(tmp_path):
    export_case("pq_m4_d16", str(tmp_path))
    p = subprocess.run([_build(), "cpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name,run", [("pq_m4_d16", 0), ("pq_m16_d64_ip", 0), ("pq_m6_d30", 0), ("pq_poly_m16", 0), ("pq_sdc_m8", 0)])
def test_indexpq_shell_on_gpu(name, run, tmp_path):
    exe = _build()
    export_case(name, str(tmp_path), run)
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
