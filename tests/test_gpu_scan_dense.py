"""GPU: the dense stream of the stored-sums loop (csrc/scan16.hip: a query's live probes scanned as one index space, 64 codes
at a time across list boundaries) returns, bit for bit, what the oracle and the stored-rows loop return, and counts the codes
the oracle counts -- with many boundaries in one block, boundaries on and next to block edges, totals on and next to
multiples of the trip size, dead and empty probes, exact ties across a boundary, 1 to 128 probes, max_codes and store_pairs,
on the two-wave and the four-wave shape, k 1 / 10 / 32, in both visiting orders.  The cases live in tests/scan_dense_cases.py;
each runs in a process of its own."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(case, walk_first):
    env = dict(os.environ)
    env["VLQ_WALK_FIRST"] = walk_first
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scan_dense_cases.py"), case], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (case, walk_first, p.stdout[-2000:], p.stderr[-3000:])


@pytest.mark.parametrize("walk_first", ["-1", "1"])
def test_boundaries_inside_and_on_the_edges_of_a_block(walk_first):
    run_case("stream", walk_first)


@pytest.mark.parametrize("walk_first", ["-1", "1"])
def test_one_and_seven_probes(walk_first):
    run_case("narrow", walk_first)


@pytest.mark.parametrize("walk_first", ["-1", "1"])
def test_more_than_64_probes(walk_first):
    run_case("wide", walk_first)


@pytest.mark.parametrize("walk_first", ["-1", "1"])
def test_max_codes_and_store_pairs(walk_first):
    run_case("options", walk_first)
