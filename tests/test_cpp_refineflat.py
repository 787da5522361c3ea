"""faiss::IndexRefineFlat of the C++ shell (include/faiss_amd/IndexFlat.h, index_io.h): on CPU both constructors, the
defaults, k_factor, the throws and an "IxRF" write / read round trip with the bytes compared field by field; on the GPU box
tests/cpp/test_refineflat_shell puts the shell's IndexRefineFlat over the shell's IndexIVFPQ built from the l2_ivfpq_d32
fixture, adds on the device, searches and compares with the reference's rows (the rows without a boundary tie)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "refineflat")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "refineflat_shell.mk"])
    return os.path.join(CPP, "test_refineflat_shell")


def export_case(name, d):
    """the fixture's arrays as raw files (what the binary reads)"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert int(z["base_kind"]) == 0 and int(z["metric"]) == 1
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d %d %r %d\n" % (z["xb"].shape[1], z["nlist"], z["M"], z["nbits"], z["xb"].shape[0], z["xq"].shape[0],
                                                     z["nprobe"], z["k"], float(z["k_factor"]), z["table_mode"][0]))
    for fn, a, dt in (("coarse.f32", z["coarse_centroids"], np.float32), ("pq.f32", z["pq_centroids"], np.float32),
                      ("xb.f32", z["xb"], np.float32), ("xq.f32", z["xq"], np.float32), ("D.f32", z["D"], np.float32),
                      ("I.i64", z["I"], np.int64), ("tie.u8", z["boundary_tie"], np.uint8)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, fn))
    return z


def test_class_surface_and_ixrf_record(tmp_path):
    p = subprocess.run([_build(), "cpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_refineflat_shell_on_gpu(tmp_path):
    exe = _build()
    z = export_case("l2_ivfpq_d32", str(tmp_path))
    assert (z["boundary_tie"] == 0).sum() * 4 >= 3 * z["boundary_tie"].size
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
