"""faiss::IndexIVFFlat / faiss::gpu::GpuIndexIVFFlat of the C++ shell (include/faiss_amd/): on CPU the "IvFl" record the
reference wrote is read, compared field by field and written again byte for byte, and float16 list storage is refused; on
the GPU box tests/cpp/test_ivfflat_shell builds the index from a fixture's lists, searches and compares with the reference's
rows, and round-trips through GpuIndexIVFFlat (copyFrom, search, copyTo, add)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ivfflat")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "ivfflat_shell.mk"])
    return os.path.join(CPP, "test_ivfflat_shell")


def export_case(name, d):
    """the fixture's arrays as raw files (what the binary reads)"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d\n" % (z["d"], z["nlist"], z["ids"].shape[0], z["xq"].shape[0], z["nprobe"], z["k"], z["metric"]))
    for fn, a, dt in (("coarse.f32", z["coarse_centroids"], np.float32), ("vecs.f32", z["vecs"], np.float32),
                      ("xq.f32", z["xq"], np.float32), ("D.f32", z["D"], np.float32), ("I.i64", z["I"], np.int64),
                      ("keys.i64", z["keys"], np.int64), ("ids.i64", z["ids"], np.int64), ("off.i64", z["list_offsets"], np.int64)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, fn))
    if "index_bytes" in z.files:
        z["index_bytes"].tofile(os.path.join(d, "index.bin"))


def test_ivfl_record_roundtrip_and_float16_refusal(tmp_path):
    export_case("flat_tail_d5_l2", str(tmp_path))
    p = subprocess.run([_build(), "cpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat_l2_d32", "flat_ip_d32", "flat_tail_d30_ip"])
def test_ivfflat_shell_on_gpu(name, tmp_path):
    exe = _build()
    export_case(name, str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
