"""faiss::IndexFlat::range_search of the C++ shell (include/faiss_amd/IndexFlat.h): on CPU the argument check in front of any
device call; on the GPU box tests/cpp/test_flat_range fills the index from a flat k-NN fixture's vectors -- in two adds with a
call between them, after a reset, and through xb directly -- and compares range_search at the fixture's radii with the
reference's arrays (tests/golden/flatrange/): one fixture of the SSE path, element for element, and one of the GEMM path, whose
labels and limits are the reference's (its distances are held to the reference's by tests/test_gpu_flat_range.py's bound)."""
import os
import subprocess

import numpy as np
import pytest

from test_knn_range_ref import LIMS_ONLY, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "flat_range.mk"])
    return os.path.join(CPP, "test_flat_range")


def export_case(name, metric, d):
    """the source fixture's vectors and the range fixture's results as raw files (what the binary reads)"""
    z = load(name)
    names = [nm for nm in z["names"] if nm not in LIMS_ONLY]
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d\n" % (z["d"], z["xb"].shape[0], z["xq"].shape[0], 0 if metric == "ip" else 1, len(names),
                                         int(z["kind"] != "blas")))
    radii = np.array([z["radii_" + metric][z["names"].index(nm)] for nm in names], np.float32)
    for fn, a in (("xb.f32", z["xb"]), ("xq.f32", z["xq"]), ("radii.f32", radii)):
        np.ascontiguousarray(a, dtype=np.float32).tofile(os.path.join(d, fn))
    for i, nm in enumerate(names):
        z["lims_%s_%s" % (metric, nm)].astype(np.int64).tofile(os.path.join(d, "lims_%d.i64" % i))
        z["D_%s_%s" % (metric, nm)].astype(np.float32).tofile(os.path.join(d, "D_%d.f32" % i))
        z["I_%s_%s" % (metric, nm)].astype(np.int64).tofile(os.path.join(d, "I_%d.i64" % i))


def test_result_object_is_checked_first():
    p = subprocess.run([_build(), "cpu"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("name", ["small_d32_nq19", "blas_d128_nq150"])
def test_range_search_shell_on_gpu(name, metric, tmp_path):
    exe = _build()
    export_case(name, metric, str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
