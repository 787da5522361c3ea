"""faiss::IndexFlatIP / faiss::IndexIVFPQ with METRIC_INNER_PRODUCT of the C++ shell (include/faiss_amd/): compiles, links,
round-trips through index_io and refuses a multi-index quantizer on CPU; on the GPU box tests/cpp/test_ivfpq_ip builds the
index from a fixture's trained parts, adds, searches and compares with the reference's rows."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN_IP = os.path.join(ROOT, "tests", "golden", "ip")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "vector_line_quantization_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "ip_shell.mk"])
    return os.path.join(CPP, "test_ivfpq_ip")


def export_case(name, d):
    """the fixture's arrays as raw files (what the binary reads)"""
    z = np.load(os.path.join(GOLDEN_IP, name + ".npz"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d %d %d %d\n" % (z["d"], z["nlist"], z["M"], z["nbits"], z["xb"].shape[0], z["xq"].shape[0],
                                                   z["nprobe"], z["k"], z["by_residual"], z["max_codes"]))
    for fn, a, dt in (("coarse.f32", z["coarse_centroids"], np.float32), ("pq.f32", z["pq_centroids"], np.float32),
                      ("xb.f32", z["xb"], np.float32), ("xq.f32", z["xq"], np.float32), ("D.f32", z["D"], np.float32),
                      ("cdis.f32", z["coarse_dis"], np.float32), ("I.i64", z["I"], np.int64), ("P.i64", z["I_pairs"], np.int64),
                      ("keys.i64", z["keys"], np.int64), ("ids.i64", z["ids"], np.int64), ("off.i64", z["list_offsets"], np.int64),
                      ("codes.u8", z["codes"], np.uint8)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, fn))


def test_ip_shell_io_roundtrip_and_refusals():
    p = subprocess.run([_build(), "cpu"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ip_residual", "ip_nonresidual", "ip_padding_ties"])
def test_ip_shell_on_gpu(name, tmp_path):
    exe = _build()
    export_case(name, str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
