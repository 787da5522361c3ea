"""faiss::IndexLSH of the C++ shell (include/faiss_amd/IndexLSH.h, VectorTransform.h): on CPU the class surface, the defaults and
the throws, the host transform in the stated fmaf order, train against the fixture's thresholds, and the "IxHe" record (with its
"rrot") the reference wrote is read, compared field by field and written again byte for byte ("IxHE" is read too); on the GPU
box tests/cpp/test_indexlsh_shell builds the index with the fixture's matrix, trains, adds and searches, and compares with the
reference's codes and rows."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lsh")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "indexlsh_shell.mk"])
    return os.path.join(CPP, "test_indexlsh_shell")


def export_case(name, d):
    """the fixture's arrays as raw files (what the binary reads)"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    nt = z["xt"].shape[0] if "xt" in z.files else 0
    exact = int(str(z["kind"]) in ("thresh", "rot_int"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d %d %d\n" % (z["d"], z["nbits"], z["xb"].shape[0], z["xq"].shape[0], z["k"], z["rotate"], z["thresh"], nt, exact))
    for fn, key, dt in (("xb.f32", "xb", np.float32), ("xq.f32", "xq", np.float32), ("xt.f32", "xt", np.float32), ("A.f32", "A", np.float32),
                        ("thr.f32", "thresholds", np.float32), ("D.f32", "D", np.float32), ("I.i64", "I", np.int64),
                        ("codes.u8", "codes", np.uint8), ("qcodes.u8", "qcodes", np.uint8), ("index.bin", "index_bytes", np.uint8)):
        if key in z.files:
            np.ascontiguousarray(z[key], dtype=dt).tofile(os.path.join(d, fn))


@pytest.mark.parametrize("name", ["rot_thresh_16_64", "rot_int", "thresh_even", "thresh_odd", "prefix", "width_60"])
def test_class_surface_and_ixhe_record(name, tmp_path):
    export_case(name, str(tmp_path))
    p = subprocess.run([_build(), "cpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rot_int", "rot_thresh_64_32", "thresh_odd", "plain", "width_192", "kwide"])
def test_indexlsh_shell_on_gpu(name, tmp_path):
    exe = _build()
    export_case(name, str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
