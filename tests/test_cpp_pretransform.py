"""faiss::IndexPreTransform of the C++ shell (include/faiss_amd/VectorTransform.h, index_io.h): on CPU the host transforms,
set_is_orthonormal and the "IxPT" record over "LTra" + "IxF2" (and over every other transform record) written, read back and
written again byte for byte; on the GPU box search against IndexFlatL2::search on the host chain's rows and reconstruct against
the host transform_transpose (tests/cpp/test_pretransform_shell.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "pretransform_shell.mk"])
    return os.path.join(CPP, "test_pretransform_shell")


def test_host_transforms_and_ixpt_record(tmp_path):
    p = subprocess.run([_build(), "cpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_pretransform_shell_on_gpu(tmp_path):
    p = subprocess.run([_build(), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "all ok" in p.stdout, p.stdout + p.stderr
