"""faiss::RangeSearchResult and faiss::IndexIVFFlat::range_search of the C++ shell (include/faiss_amd/): on CPU the result
object as constructed and do_allocation on given counts; on the GPU box tests/cpp/test_ivfflat_range builds the index from a
fixture's lists and compares range_search at every stored radius with the reference's arrays, element for element."""
import os
import subprocess

import numpy as np
import pytest

import range_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "ivfflat_range.mk"])
    return os.path.join(CPP, "test_ivfflat_range")


def export_case(name, d):
    """the source fixture's arrays and the range fixture's results as raw files (what the binary reads)"""
    z, r, prefix, metric, keys = rr.load_case(name)
    names = rr.radius_names(r)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d\n" % (z["d"], z["nlist"], z["ids"].shape[0], z["xq"].shape[0], keys.shape[1], z["metric"], len(names)))
    for fn, a, dt in (("coarse.f32", z["coarse_centroids"], np.float32), ("vecs.f32", z["vecs"], np.float32), ("xq.f32", z["xq"], np.float32),
                      ("radii.f32", r["radii"], np.float32), ("keys.i64", keys, np.int64), ("ids.i64", z["ids"], np.int64),
                      ("off.i64", z["list_offsets"], np.int64)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, fn))
    for i, rn in enumerate(names):
        r["lims_" + rn].astype(np.int64).tofile(os.path.join(d, "lims_%d.i64" % i))
        r["D_" + rn].astype(np.float32).tofile(os.path.join(d, "D_%d.f32" % i))
        r["I_" + rn].astype(np.int64).tofile(os.path.join(d, "I_%d.i64" % i))


def test_range_search_result():
    p = subprocess.run([_build(), "cpu"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat_l2_d32", "flat_ip_d32", "flat_tail_d30_ip"])
def test_range_search_shell_on_gpu(name, tmp_path):
    exe = _build()
    export_case(name, str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
