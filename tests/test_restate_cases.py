"""CPU: tests/restate_cases.py held to its promises with the references alone (no device).

  sensitivity   for every step of every walk the reference rows of the state after the step differ, in the bits of D or in I, in
                at least half of the query rows from the rows of the same state with the changed component left at its old value
                (reset + add of other vectors: from the old vectors) -- a stale buffer behind that step cannot hide at these
                shapes.  The toggles that must not change a row are no-ops on the reference side.
  comparisons   the comparison rule a kind uses fails when it is fed those stale rows in place of the right ones
  recipes       the fresh-handle recipe is a function of the state alone: step history, stream and speed-only toggles do not show
"""
import functools

import numpy as np
import pytest

import restate_cases as rc

NAMES = [k.name for k in rc.KINDS]
SILENT = ("history",) + rc.NOOP_COMPONENTS


@functools.lru_cache(maxsize=None)
def rows(name, i, stale):
    kind, steps = rc.walk_of(name)
    state = steps[i].stale if stale else steps[i].state
    return kind.reference(state, kind.queries(state))


def moving(steps):
    """indices of the steps that change what the handle must answer"""
    return [i for i, s in enumerate(steps) if i and s.refuse is None and not s.noop and not s.resize]


@pytest.mark.parametrize("name", NAMES)
def test_walk_shape(name):
    kind, steps = rc.walk_of(name)
    assert steps[0].label == "A" and steps[0].fn is None
    labels = [s.label for s in steps]
    assert len(set(labels)) == len(labels), "labels name the steps"
    streams = [s.state["stream"] for s in steps]
    on = streams.index("torch")
    back = on + streams[on:].index("own")
    assert 0 < on < back and any(i in moving(steps) for i in range(on + 1, back)), "a moving step runs on torch's stream"
    for s in steps:
        if s.refuse is not None:
            assert s.refuse in (rc.ERR_STATE, rc.ERR_UNSUPPORTED)
            nxt = steps[steps.index(s) + 1]
            assert nxt.refuse is None, "a refusal is followed by a clean search"
    assert moving(steps), name


@pytest.mark.parametrize("name", NAMES)
def test_every_step_moves_the_answer(name):
    kind, steps = rc.walk_of(name)
    for i in moving(steps):
        share = float(rc.rows_differ(rows(name, i, False), rows(name, i, True)).mean())
        assert share >= 0.5, (name, steps[i].label, share)
    for i, s in enumerate(steps):
        if s.noop:
            rc.exact(rows(name, i, False), rows(name, i, True), "%s: %s is no toggle of results" % (name, s.label))
        if s.resize:
            keep = dict(s.state, nq=steps[i - 1].state["nq"], k=steps[i - 1].state.get("k"), history=None)
            assert kind.recipe_key(keep) == kind.recipe_key(dict(steps[i - 1].state, history=None)), "only the batch changes"


@pytest.mark.parametrize("name", NAMES)
def test_comparison_rejects_the_stale_rows(name):
    kind, steps = rc.walk_of(name)
    for i in moving(steps):
        right, stale = rows(name, i, False), rows(name, i, True)
        rule = kind.rule(steps[i].state)
        rule(right, right, "the right rows pass")
        with pytest.raises(AssertionError):
            rule(stale, right, steps[i].label)
        with pytest.raises(AssertionError):          # the comparison with the fresh handle
            rc.exact(stale, right, steps[i].label)


def components(state):
    return {c: v for c, v in state.items() if c not in SILENT}


def same_value(a, b):
    if isinstance(a, tuple) and isinstance(b, tuple):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("name", NAMES)
def test_recipe_is_a_function_of_the_state(name):
    kind, steps = rc.walk_of(name)
    twins = 0
    for i, s in enumerate(steps):
        key = kind.recipe_key(s.state)
        assert key == kind.recipe_key(dict(s.state)), "the same state twice"
        other = dict(s.state, history=("another", "way", "here"), stream="torch" if s.state["stream"] == "own" else "own")
        assert key == kind.recipe_key(other), (name, s.label)
        for t in steps[:i]:
            a, b = components(s.state), components(t.state)
            if a.keys() == b.keys() and all(same_value(a[c], b[c]) for c in a):
                assert key == kind.recipe_key(t.state), (name, t.label, s.label)
                twins += 1
            else:
                differs = [c for c in a if c not in ("nq", "k") and not same_value(a[c], b.get(c))]
                if differs and differs != ["range"]:          # ("range": whether the GPU test also runs a range search here)
                    assert key != kind.recipe_key(t.state), (name, t.label, s.label, differs)
    assert twins > 0, "every walk comes back to a state it has been in (at least by a set_stream)"


def test_kinds_cover_the_handles():
    heads = {n.split("-")[0] for n in NAMES}
    assert heads == {"flat", "lsh", "sq", "pq", "ivfflat", "ivfsq", "ivfpq", "ivfpqr", "vlq", "refineflat"}
    assert len(set(NAMES)) == len(NAMES)


def test_smallest_share():
    """the smallest share of differing rows over all moving steps of all walks: the figure of the commit message"""
    low = min((float(rc.rows_differ(rows(name, i, False), rows(name, i, True)).mean()), name, rc.walk_of(name)[1][i].label)
              for name in NAMES for i in moving(rc.walk_of(name)[1]))
    print("smallest differing-row share: %.3f (%s: %s)" % low)
    assert low[0] >= 0.5, low
