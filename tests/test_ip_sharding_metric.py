"""CPU: sharded.py under the inner-product metric.  List-range sharding merges ascending and refuses the metric, whether the
caller names it or the index that `local_search` is a bound method of carries it; query sharding pads its unused slots with
-FLT_MAX there."""
import numpy as np
import pytest
import torch

from vector_line_quantization_amd import sharded


class FakeIndex:
    """stands for GpuIVFPQ: a `metric` attribute and a search method"""

    def __init__(self, metric):
        self.metric = metric
        self.calls = 0

    def search(self, x, nprobe, k):
        self.calls += 1
        n = x.shape[0]
        D = torch.arange(n * k, dtype=torch.float32).reshape(n, k)
        if self.metric == "ip":
            D = -D
        return D, torch.arange(n * k, dtype=torch.int64).reshape(n, k)


def plain(x, nprobe, k):
    return FakeIndex("l2").search(x, nprobe, k)


def test_metric_is_read_from_the_index():
    assert sharded._metric_of(FakeIndex("ip").search, None) == "ip"
    assert sharded._metric_of(FakeIndex("l2").search, None) == "l2"
    assert sharded._metric_of(plain, None) == "l2"
    assert sharded._metric_of(plain, "ip") == "ip"
    assert sharded._metric_of(FakeIndex("l2").search, "ip") == "ip"      # the caller's word wins
    with pytest.raises(ValueError):
        sharded._metric_of(plain, "cosine")


def test_list_range_sharding_refuses_inner_product():
    x = torch.zeros((3, 4))
    ix = FakeIndex("ip")
    with pytest.raises(NotImplementedError, match="inner-product"):
        sharded.list_sharded_search(ix.search, x, 2, 5)                  # default argument, metric on the index
    with pytest.raises(NotImplementedError, match="inner-product"):
        sharded.list_sharded_search(plain, x, 2, 5, metric="ip")
    assert ix.calls == 0                                                  # refused before any search
    D, I = sharded.list_sharded_search(FakeIndex("l2").search, x, 2, 5)  # L2, one process: the local rows
    assert D.shape == (3, 5) and np.array_equal(I.numpy(), np.arange(15).reshape(3, 5))


def test_query_sharding_pads_with_the_metrics_neutral():
    """an unused slot of the gather: FLT_MAX under L2, -FLT_MAX under inner product (what the scan itself pads with)"""
    flt_max = float(np.finfo(np.float32).max)
    assert sharded.pad_distance("l2") == flt_max
    assert sharded.pad_distance("ip") == -flt_max
    assert sharded.pad_distance(sharded._metric_of(FakeIndex("ip").search, None)) == -flt_max
