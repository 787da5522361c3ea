"""No GPU: tests/async_cases.py against the headers.  The table of tests/test_gpu_async_streams.py must name every handle that
has a set_stream, must classify every entry point as the header's own words do, and every decoy it hands to a device must be a
valid input of its call."""
import numpy as np
import pytest

import async_cases as ac
import vector_line_quantization_amd._lib as vlib


def test_every_handle_with_a_set_stream_is_in_the_table():
    kinds = ac.set_stream_kinds()
    assert kinds, "no vlq_<kind>_set_stream found in the headers"
    assert set(kinds) == set(ac.TABLE), "handles with a set_stream %s, kinds of the table %s" % (kinds, sorted(ac.TABLE))
    covered = {a.prefix for a in ac.KINDS}
    assert covered == set(ac.TABLE) | set(ac.PYTHON_ONLY), "kinds without a case in the GPU file: %s" % sorted((set(ac.TABLE) | set(ac.PYTHON_ONLY)) - covered)


def test_set_stream_scan_sees_a_new_handle():
    text = ac.header_text() + "\nint vlq_newkind_set_stream(vlq_newkind_t h, void* hip_stream);\n"
    assert "newkind" in ac.set_stream_kinds(text)


@pytest.mark.parametrize("prefix", sorted(ac.TABLE))
def test_classes_are_the_headers_words(prefix):
    docs = ac.entry_comments()
    row = ac.TABLE[prefix]
    assert "vlq_%s_set_stream" % prefix in docs
    for name in row["A"]:
        assert name in docs and name in vlib.SYMBOLS, name
        assert docs[name].strip(), "%s has no comment" % name
        assert not ac.says_synchronises(docs[name]), "%s is class A in the table, its comment says it synchronises the stream" % name
    for name in row["B"]:
        assert name in docs and name in vlib.SYMBOLS, name
        assert ac.says_synchronises(docs[name]), "%s is class B in the table, its comment has no \"Synchronises the stream\"" % name
    assert not set(row["A"]) & set(row["B"])


def test_comment_parser():
    text = "/* one.  Synchronises the stream. */\nint vlq_a_f(int x);\nint vlq_a_g(int y);\n/* two */\nint vlq_a_h(void);\ntypedef int t;\nint vlq_a_i(void);\n"
    docs = ac.entry_comments(text)
    assert ac.says_synchronises(docs["vlq_a_f"]) and ac.says_synchronises(docs["vlq_a_g"])
    assert docs["vlq_a_h"].strip() == "two" and docs["vlq_a_i"] == ""
    assert ac.says_synchronises("the call\n * synchronises the  stream once") and not ac.says_synchronises("the call synchronises and returns")


def test_every_call_names_an_entry_point_of_its_kind():
    for a in ac.KINDS:
        row = dict(ac.TABLE, **ac.PYTHON_ONLY)[a.prefix]
        for c in ac.all_calls(a):
            assert c.klass in ("A", "B")
            assert c.entry in row.get(c.klass, ()), "%s: %s is not a class %s entry point of %s" % (c.what, c.entry, c.klass, a.prefix)
    called = {c.entry for a in ac.KINDS for c in ac.all_calls(a)}
    # stats, last_scan_info, add and encode take no Call: the GPU file has a scenario of its own for each
    own = ("_stats", "_polysemous_stats", "_last_scan_info", "_add", "_encode")
    for prefix, row in ac.TABLE.items():
        for name in row["A"] + row["B"]:
            assert name in called or name.endswith(own), "%s is in the table and no case calls it" % name


@pytest.mark.parametrize("name", [a.name for a in ac.KINDS])
def test_decoys_are_valid_inputs(name):
    a = ac.BY_NAME[name]
    calls = ac.all_calls(a)
    assert calls
    for c in calls:
        ac.check_decoys(c)
        for n_ in c.inout:
            assert n_ in c.ins
        assert not set(c.outs) & set(c.ins)
    two = a.two_searches()
    assert two.ins["x2"].shape[0] <= two.ins["x"].shape[0]          # nothing regrows between the two


def test_check_decoys_rejects():
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    keys = np.array([[0, 1], [2, -1]], np.int64)
    ok = ac.Call("ok", "e", "A", None, dict(x=x, keys=keys), dict(x=ac.other_rows(x), keys=ac.other_keys(keys, 3)), limits=dict(keys=(0, 3)))
    ac.check_decoys(ok)
    assert (ok.decoys["keys"] == np.array([[1, 2], [0, -1]])).all()
    for bad in (ac.Call("same", "e", "A", None, dict(x=x), dict(x=x.copy())),
                ac.Call("range", "e", "A", None, dict(keys=keys), dict(keys=keys + 1), limits=dict(keys=(0, 3))),
                ac.Call("no limits", "e", "A", None, dict(keys=keys), dict(keys=ac.other_keys(keys, 3)))):
        with pytest.raises(AssertionError):
            ac.check_decoys(bad)
    for names in (ac.COUNTED, ac.BAD_KEYS, ac.ADDS, ac.ENCODES):
        assert set(names) <= set(ac.BY_NAME)
