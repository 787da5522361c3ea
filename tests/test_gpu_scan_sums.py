"""GPU: the stored-sums loop of the 16-byte scan (csrc/scan16.hip, csrc/scan_sum_bound.h) returns, bit for bit, what the
stored-rows loop and the oracle return -- on the shapes it serves (two and four waves, k 1 / 10 / 32, both visiting orders),
on ties at the k-th distance, on data that defeat its bound (every query undecided, the handle drops the loop), with non-finite
and huge queries, after everything that makes the stored sums stale, and through search_preassigned.  The cases live in
tests/scan_sums_cases.py; each runs in a process of its own."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(case, extra=None):
    env = dict(os.environ)
    env.update(extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scan_sums_cases.py"), case], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (case, extra, p.stdout[-2000:], p.stderr[-3000:])


@pytest.mark.parametrize("walk_first", ["-1", "1"])
def test_shapes_and_both_visiting_orders(walk_first):
    run_case("shapes", {"VLQ_WALK_FIRST": walk_first})


def test_ties_at_the_kth_distance():
    run_case("ties")


def test_data_that_defeat_the_bound_drop_the_loop():
    run_case("defeat")


def test_non_finite_and_huge_queries():
    run_case("nonfinite")


def test_stale_sums_are_rebuilt():
    run_case("stale")


def test_search_preassigned():
    run_case("preassigned")
