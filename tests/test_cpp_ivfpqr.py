"""faiss::IndexIVFPQR of the C++ shell (include/faiss_amd/IndexIVFPQ.h): compiles and links on CPU; on the GPU box
tests/cpp/test_ivfpqr_shell builds the index from a refine_* fixture's trained parts, adds, searches and compares with
the reference's IndexIVFPQR."""
import os
import subprocess

import numpy as np
import pytest

from util import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "vector_line_quantization_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "ivfpqr.mk"])
    return os.path.join(CPP, "test_ivfpqr_shell")


def export_case(case, d):
    """the fixture's arrays as raw files (what the binary reads)"""
    Mr, nbits_r, _kc = (int(v) for v in case["refine_cfg"])
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %d %d %d %d %r\n" % (case.d, case.nlist, case.M, case.nbits, Mr, nbits_r, len(case.xb), case.nq,
                                                        case.nprobe, case.k, float(case["k_factor"][0])))
    by_id = np.zeros((len(case.xb), Mr), np.uint8)
    by_id[case["ids"]] = case["refine_codes"]
    for name, a, dt in (("coarse.f32", case["coarse_centroids"], np.float32), ("pq.f32", case["pq_centroids"], np.float32),
                        ("rpq.f32", case["refine_centroids"], np.float32), ("xb.f32", case.xb, np.float32), ("xq.f32", case.xq, np.float32),
                        ("D.f32", case["refine_D"], np.float32), ("I.i64", case["refine_I"], np.int64), ("ids.i64", case["ids"], np.int64),
                        ("off.i64", case["list_offsets"], np.int64), ("codes.u8", case["codes"], np.uint8), ("rcodes_by_id.u8", by_id, np.uint8),
                        ("tie.u8", case["boundary_tie"], np.uint8)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, name))


def test_ivfpqr_shell_compiles_and_links():
    assert os.access(_build(), os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["refine_c1_small", "refine_tail", "refine_duplicates"])
def test_ivfpqr_shell_on_gpu(name, tmp_path):
    exe = _build()
    export_case(Case(name), str(tmp_path))
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout
