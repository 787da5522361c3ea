"""CPU: the storage option of vlq.GpuIVFFlat is checked before the library is asked for anything, and a float16 index has no
path without a device either."""
import pytest

import vector_line_quantization_amd as vlq


def test_unknown_storage_is_a_value_error():
    with pytest.raises(ValueError):
        vlq.GpuIVFFlat(8, 4, storage="bf16")


def test_f16_fails_loudly_without_gpu():
    if vlq.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(vlq.VlqError) as e:
        vlq.GpuIVFFlat(8, 4, storage="f16")
    assert "no HIP device" in str(e.value)
