"""GPU: growth of the inverted lists at the boundaries of the relayout kernel (lists.hip: relayout_kernel), with the host model
of tests/test_gpu_list_store.py at 300 lists -- two workgroups of the kernel, 256 + 44 lists.

The lists are loaded through set_lists with the lengths of write_cases.growth_lens(): 0, 1, 31, 32, 33, 40, 255, 256, 257 and
1000 rows among lists of 0 .. 4, every long list between short ones, a list of 500 rows, an empty one and one of 33 in the second
workgroup.  Then the batches of write_cases.GROWTH_STEPS are added, every row of a batch aimed at one list: a long list
overflows and every list moves (25 % slack); a batch fits the slack and nothing moves; a list of 31 rows overflows and becomes
long; another overflow moves it as a long list.  After every step the rows, side bytes, ids and order of EVERY list are those
of the model, a search equals, as bits, the search of a fresh handle loaded from the model, and the step grew, or did not
grow, what write_cases.growth_run() plans on the host.

Capacities.  The one place a capacity shows is reclaim_memory's byte count.  It is asserted straight behind the first overflow,
behind the batch that fits and behind the last step, while the capacities are the ones the growth kernels made: need + need // 4
per list at the last overflow, unchanged by the batch that fits -- a wrong slack, a wrong capacity in the second workgroup or
a relayout in the step that moves nothing changes that count (test_write_cases.py: the three counts are those of the planned
capacities, and the second is not what a fresh growth would leave).  After a reclaim the lists are packed, so the next batch
overflows again.  A separate round of reserve_memory and reclaim_memory follows.
A VLQ handle has neither call: its capacities are observed only through what they cause -- the second batch fits the slack of
the first there -- not as numbers.

Copy paths of the kernel (a list of at most 32 rows: its own thread; a longer one: the whole workgroup, in 16-byte words plus a
byte tail when its old and new byte offsets are both multiples of 16, else in bytes).  tests/test_write_cases.py
(test_growth_plan_copy_paths) derives from the model's offsets that every case below copies short lists, long lists at aligned
offsets (list 0 always is) with a byte tail, and long lists at unaligned offsets -- except the 16-byte rows, always aligned and
without a tail:

  ivfpq-M16    16-byte rows: the uint4 special case per thread
  ivfpq-M8     8-byte rows            ivfpq-M5     5-byte rows
  ivfpqr       2-byte rows + 2 side bytes (the refine codes) copied beside them on both paths
  ivfflat-d3   12-byte rows           ivfflat-d4   16-byte rows (uint4 case)
  ivfsq-4bit   d = 5: 3-byte rows
  vlq          2-byte rows + the lambda byte; 150 cells x 2 edges = 300 lines; growth relayouts only
"""
import numpy as np
import pytest

import write_cases as wc
from test_gpu_list_store import Geometry, Model, check_search, make, near, stored_as

pytestmark = pytest.mark.gpu

CASES = {
    "ivfpq-M16": ("ivfpq", dict(d=16, M=16)),
    "ivfpq-M8": ("ivfpq", dict(d=8, M=8)),
    "ivfpq-M5": ("ivfpq", dict(d=5, M=5)),
    "ivfpqr": ("ivfpqr", dict(d=8, M=2, mr=2, nbits_r=4)),
    "ivfflat-d3": ("ivfflat", dict(d=3)),
    "ivfflat-d4": ("ivfflat", dict(d=4)),
    "ivfsq-4bit": ("ivfsq", dict(d=5, qtype="4bit")),
    "vlq": ("vlq", dict(d=8, M=2, nedge=2, nlist=wc.GROWTH_NLIST // 2)),
}
assert set(CASES) == set(wc.GROWTH_ROW_BYTES)


def aimed(kind, g, geo, rng, counts):
    """rows that the index itself sends to the given lists, counts[list] of them each: candidates beside the list's coarse
    centroid, kept where the index's own assignment is that list (of a VLQ cell's two lines either may take a candidate)"""
    per_cell = 2 if kind == "vlq" else 1
    out = []
    for target in np.nonzero(counts)[0]:
        cand = near(rng, [target // per_cell] * (6 * int(counts[target]) + 64), geo)
        assign = stored_as("ivfpq" if kind == "ivfpqr" else kind, g, cand, geo)[0]
        hit = cand[assign == target]
        assert len(hit) >= counts[target], "too few candidates land in list %d" % target
        out.append(hit[:counts[target]])
    x = np.concatenate(out)
    return x[rng.permutation(len(x))]


@pytest.mark.parametrize("case", sorted(CASES))
def test_list_growth(case):
    kind, shape = CASES[case]
    has_reclaim = kind != "vlq"
    geo = Geometry(**dict(dict(nlist=wc.GROWTH_NLIST, seed=300), **shape))
    geo.world()
    rng = np.random.RandomState(6)
    g = make(kind, geo)
    model = Model(kind, geo)
    assert model.nlists == wc.GROWTH_NLIST and model.row_bytes == wc.GROWTH_ROW_BYTES[case] + 8 + model.side
    plan, _relayouts = wc.growth_run(reclaims=has_reclaim)

    # 1. loading
    model.load(rng, list(wc.growth_lens()))
    model.load_into(g)
    model.check(g, "load")
    check_search(kind, g, model, "search after load")

    # 2. the planned batches
    for step in plan:
        what, counts = step["what"], step["counts"]
        x = aimed(kind, g, geo, rng, counts)
        assign, rows, sides = stored_as(kind, g, x, geo)
        assert np.array_equal(np.bincount(assign, minlength=model.nlists), counts), what
        assert np.array_equal(model.lens, step["lens_before"]) and np.array_equal(model.cap, step["cap_before"]), what
        grown = model.grown
        g.add(x)
        model.add(assign, rows, sides)
        assert model.grown == grown + int(step["overflows"]), what
        assert np.array_equal(model.lens, step["lens"]) and np.array_equal(model.cap, step["cap"]), what
        model.check(g, what)
        check_search(kind, g, model, "search after: " + what)       # (VLQ: the constants of the rows appended in place, too)
        if step["reclaimed"] is not None:
            # the capacities the growth left, as bytes: asserted before anything else evens them out
            assert g.reclaim_memory() == model.reclaim() == step["reclaimed"] * model.row_bytes > 0, "reclaim_memory after: " + what
            assert g.reclaim_memory() == 0, "second reclaim_memory"
            model.check(g, "reclaim_memory after: " + what)
            check_search(kind, g, model, "search after reclaim_memory after: " + what)
    assert model.lens[wc.GROWTH_SHORT_TO_LONG] > wc.GROWTH_SHORT and model.lens.max() < 1024

    # 3. a round of reserving and reclaiming, where the kind has them: two more relayouts of every list
    if has_reclaim:
        room = int(model.cap.max() + 3) * model.nlists
        g.reserve_memory(room)
        model.reserve(room)
        assert (model.cap == model.cap.max()).all()
        model.check(g, "reserve_memory")
        assert g.reclaim_memory() == model.reclaim() > 0, "reclaim_memory"
        assert g.reclaim_memory() == 0, "second reclaim_memory"
        model.check(g, "last reclaim_memory")
        check_search(kind, g, model, "search after the last reclaim_memory")
