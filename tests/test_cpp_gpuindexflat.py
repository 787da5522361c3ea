"""faiss::gpu::GpuIndexFlat / GpuIndexFlatL2 / GpuIndexFlatIP of the C++ shell (include/faiss_amd/gpu/GpuIndexFlat.h): on the GPU
box tests/cpp/test_gpuindexflat_shell builds each class empty and from a faiss::IndexFlat, copies it back, searches and
compares with faiss::IndexFlat::search of the shell (the present route) and with the reference's rows of a tests/golden/flatknn/
fixture: an integer-valued set and a general-float set at 25 queries, and a small batch, where the inner product takes the
reference's fvec_inner_product order, which the present route does not.  On CPU: the headers still go together."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "flatknn")
KIND = {"int": 0, "blas": 1, "small": 2}


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "gpuindexflat_shell.mk"])
    return os.path.join(CPP, "test_gpuindexflat_shell")


def export_case(name, nq, d):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert nq <= z["xq"].shape[0]
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d\n" % (z["d"], z["xb"].shape[0], nq, z["k"], KIND[str(z["kind"])]))
    for fn, a, dt in (("xb.f32", z["xb"], np.float32), ("xq.f32", z["xq"][:nq], np.float32), ("D_l2.f32", z["D_l2"][:nq], np.float32),
                      ("I_l2.i64", z["I_l2"][:nq], np.int64), ("D_ip.f32", z["D_ip"][:nq], np.float32), ("I_ip.i64", z["I_ip"][:nq], np.int64)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, fn))


def test_shell_builds_and_config_moved():
    """host compiler only: the test program compiles against the in-tree headers; GpuIndexFlatConfig lives in the new header"""
    assert os.path.exists(_build())
    new = open(os.path.join(ROOT, "include", "faiss_amd", "gpu", "GpuIndexFlat.h")).read()
    old = open(os.path.join(ROOT, "include", "faiss_amd", "gpu", "GpuIndexIVFPQ.h")).read()
    assert "struct GpuIndexFlatConfig" in new and "struct GpuIndexFlatConfig" not in old and '#include "GpuIndexFlat.h"' in old


@pytest.mark.gpu
@pytest.mark.parametrize("name,nq", [("int_d64_nq40", 25), ("int_d30_nq40", 25), ("blas_d128_nq150", 25), ("blas_d30_nq150", 25), ("small_d32_nq19", 19),
                                     ("small_d128_nq1", 1)])
def test_gpuindexflat_shell_on_gpu(name, nq, tmp_path):
    exe = _build()
    export_case(name, nq, str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
