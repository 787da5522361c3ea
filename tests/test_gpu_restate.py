"""GPU: handles that are retrained, re-moded or reloaded AFTER a search.  Every handle caches state derived from what its setters
were given (csrc/handle.h: term 2 in both precisions, stored table sums, the coarse screen, list ranks, the SDC table, the stored
norms, line16c's per-code constants ...); a setter that forgets to drop one of them leaves a handle that answers plausibly and
wrongly.  One live handle per kind walks the steps of tests/restate_cases.py (tests/test_restate_cases.py shows on the CPU that
every step moves at least half of the rows and that the comparisons reject the stale answer).  After every step the live search is

  * equal, D as bits and I in every slot, to a FRESH handle of the same state built in canonical order (constructor, trained
    state, options, set_lists / set_codes of what the live handle's get_list / codes() returns): same library, same state;
  * equal to the kind's CPU reference by the rule the kind's own test_gpu_*.py uses.

What the live handle stores is first compared with the walk's host-side state (a reset that cleared nothing, or an add that
appended the wrong rows, would otherwise make all three agree).

A step in the middle of every walk moves the handle onto torch's current stream and a later one onto a stream of its own; in
between the queries and the rows are device tensors, copied out asynchronously.  Steps that must be refused are refused by the host
before any launch, with their code, and are followed by a clean search."""
import numpy as np
import pytest

import restate_cases as rc
import vector_line_quantization_amd as vlq

pytestmark = pytest.mark.gpu


def search_rows(kind, g, state, xq):
    """the rows of one search as host arrays; on torch's stream: device tensors in and out, copied out without a wait in between"""
    if state["stream"] != "torch":
        D, I = kind.search(g, state, xq)
        return rc.host(D), rc.host(I)
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(xq)).cuda()
    D, I = kind.search(g, state, xd)
    assert D.is_cuda and I.is_cuda
    Dh = torch.empty(D.shape, dtype=D.dtype, pin_memory=True)
    Ih = torch.empty(I.shape, dtype=I.dtype, pin_memory=True)
    Dh.copy_(D, non_blocking=True)
    Ih.copy_(I, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return Dh.numpy().copy(), Ih.numpy().copy()


def check_step(kind, g, step, what):
    stored = kind.read(g)
    kind.check_stored(step.state, stored, what)
    state = kind.with_stored(step.state, stored)
    xq = kind.queries(state)
    got = search_rows(kind, g, state, xq)
    kind.ran(g, state)
    f = kind.fresh(state)
    try:
        rc.exact(got, tuple(rc.host(a) for a in kind.search(f, state, xq)), what + ": live handle against a fresh one of the same state")
    finally:
        kind.close(f)
    kind.rule(state)(got, kind.reference(state, xq, kind.coarse(g, state, xq)), what + ": against the CPU reference")
    for name, a, b in kind.extras(g, state):
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s" % (what, name)
    return got


@pytest.mark.parametrize("name", [k.name for k in rc.KINDS])
def test_walk(name):
    kind, steps = rc.walk_of(name)
    g = kind.start(steps[0].state)
    try:
        last = check_step(kind, g, steps[0], name + ": A")
        for step in steps[1:]:
            what = "%s: %s" % (name, step.label)
            for fn in step.pre:
                fn(g)
            if step.refuse is not None:
                with pytest.raises(vlq.VlqError) as e:
                    step.fn(g)
                assert e.value.code == step.refuse, (what, str(e.value))
                continue
            step.fn(g)
            got = check_step(kind, g, step, what)
            if step.noop:
                rc.exact(got, last, what + ": a toggle that must not change a row")
            last = got
    finally:
        kind.close(g)
