"""faiss::ScalarQuantizer / faiss::IndexIVFScalarQuantizer of the C++ shell (include/faiss_amd/IndexScalarQuantizer.h): on CPU
the shell's host parts are held to the reference's fixtures with no device -- ScalarQuantizer::train gives the range bit for
bit, compute_codes the stored codes byte for byte, decode the vectors sq.decode of the reference gave -- and the "IvSQ" record
the reference wrote is read, compared field by field and written again byte for byte; on the GPU box tests/cpp/test_ivfsq_shell
trains and fills the index through the shell and compares its search with the reference's rows."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ivfsq")
WITH_BYTES = ["sq_8bit_l2_d5", "sq_4bit_l2_d33", "sq_4bit_uniform_ip_d32"]      # fixtures that hold index_bytes and decoded


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "ivfsq_shell.mk"])
    return os.path.join(CPP, "test_ivfsq_shell")


def export_case(name, d):
    """the fixture's arrays as raw files (what the binary reads)"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d %d %d\n" % (z["d"], z["nlist"], z["ids"].shape[0], z["xq"].shape[0], z["nprobe"], z["k"], z["metric"],
                                                  z["qtype"], z["nt"]))
    for fn, a, dt in (("coarse.f32", z["coarse_centroids"], np.float32), ("xb.f32", z["xb"], np.float32), ("xq.f32", z["xq"], np.float32),
                      ("D.f32", z["D"], np.float32), ("I.i64", z["I"], np.int64), ("trained.f32", z["trained"], np.float32),
                      ("codes.u8", z["codes"], np.uint8), ("ids.i64", z["ids"], np.int64), ("off.i64", z["list_offsets"], np.int64),
                      ("decoded.f32", z["decoded"] if "decoded" in z.files else np.zeros(0), np.float32)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, fn))
    if "index_bytes" in z.files:
        z["index_bytes"].tofile(os.path.join(d, "index.bin"))


@pytest.mark.parametrize("name", WITH_BYTES)
def test_host_parts_and_ivsq_record(name, tmp_path):
    export_case(name, str(tmp_path))
    p = subprocess.run([_build(), "cpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sq_coarse_int_l2", "sq_coarse_int_ip"])
def test_ivfsq_shell_on_gpu(name, tmp_path):
    exe = _build()
    export_case(name, str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
