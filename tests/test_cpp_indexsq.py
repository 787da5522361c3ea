"""faiss::IndexScalarQuantizer of the C++ shell (include/faiss_amd/IndexScalarQuantizer.h): on CPU the class surface, the throws
and the host parts are held to the reference's fixtures with no device -- train gives the range bit for bit, add the stored
codes byte for byte, reconstruct_n the vectors the reference gave -- and the "IxSQ" record the reference wrote is read,
compared field by field and written again byte for byte, by an index read and by one built through the shell; on the GPU box
tests/cpp/test_indexsq_shell trains and fills the index through the shell and compares its search with the reference's rows,
sorted."""
import os
import subprocess

import numpy as np
import pytest

import sqflat_ref as fr
from sqflat_cases import METRIC, WITH_BYTES, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "indexsq_shell.mk"])
    return os.path.join(CPP, "test_indexsq_shell")


def export_case(name, d):
    """the fixture's arrays as raw files (what the binary reads); D / I sorted by (distance, label), as the library returns them"""
    z = load(name)
    Ds, Is = fr.sorted_rows(z["D"], z["I"], METRIC[int(z["metric"])])
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d\n" % (z["d"], z["xb"].shape[0], z["xq"].shape[0], z["k"], z["metric"], z["qtype"], z["nt"]))
    for fn, a, dt in (("xb.f32", z["xb"], np.float32), ("xq.f32", z["xq"], np.float32), ("D.f32", Ds, np.float32), ("I.i64", Is, np.int64),
                      ("trained.f32", z["trained"], np.float32), ("codes.u8", z["codes"], np.uint8), ("decoded.f32", z["decoded"], np.float32)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, fn))
    if "index_bytes" in z:
        z["index_bytes"].tofile(os.path.join(d, "index.bin"))


@pytest.mark.parametrize("name", WITH_BYTES)
def test_host_parts_and_ixsq_record(name, tmp_path):
    export_case(name, str(tmp_path))
    p = subprocess.run([_build(), "cpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sqf_8bit_l2_d32", "sqf_4bit_ip_d33", "sqf_4bit_uniform_ip_d32", "sqf_8bit_l2_d5"])
def test_indexsq_shell_on_gpu(name, tmp_path):
    exe = _build()
    export_case(name, str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
