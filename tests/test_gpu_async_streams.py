"""GPU: stream-ordered use of every handle that has a set_stream.  include/vlq_ivfpq.h promises that all work is issued on the
index's stream, that a call whose buffers are all device-resident is asynchronous on it, and that inputs produced earlier ON that
stream need no host synchronisation; some calls instead say "Synchronises the stream" and are complete on return.  This is how a
device-resident caller uses an index -- queries written by a kernel, rows read by the next one -- and what the other GPU tests
never do: they hand over inputs that are complete, on the null stream, under a device-wide synchronise.

The late-input harness (tests/async_cases.py has the calls, the decoys and the table of classes):

  1. every tensor is allocated first, on torch's default stream -- device inputs filled with a DECOY (a different but valid input),
     outputs filled with a sentinel, page-locked mirrors -- and kept to the end of the test;
  2. the handle moves to a non-blocking stream s and is warmed with the same call on host arrays: `want`, compared with the kind's
     CPU reference by the kind's own rule; then with the decoy on host arrays: `want_decoy` (and the handle's workspaces now hold
     what the decoy left there);
  3. on s: a delay kernel of about 50 ms, the copies that bring the real inputs, THE CALL, copies of the outputs to page-locked
     memory, and the decoy over every input again -- no host synchronisation anywhere;
  4. after s.synchronize() the rows are `want` bit for bit.  A library that read an input early, or on another stream, or late,
     computed the decoy's rows; one that did not wait for its second stream read what the decoy's call left in the workspace.

Class A calls (device-resident buffers, no "Synchronises the stream" in the header) must return while the delay is still pending:
`not s.query()`.  Class B calls get the late input and must simply be right.  Two controls, run once per session, show that the
delay really withholds the data and that the null stream is not ordered behind s (the condition under which a legacy-stream
hipMemcpy / hipMemset inside the library is a hazard)."""
import contextlib
import time

import numpy as np
import pytest

import async_cases as ac
import restate_cases as rc
import vector_line_quantization_amd as vlq

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
SENTINEL = 0xA5
HOST_MS = {}          # what -> host milliseconds of the measured call (printed: the delay only has to be long against these)


def T():
    import torch
    return torch


# ----------------------------------------------------------------------------------------------------------------------
# the delay and the controls
# ----------------------------------------------------------------------------------------------------------------------
class Delay:
    def __init__(self, how, arg, ms, enqueue):
        self.how, self.arg, self.ms, self.enqueue = how, arg, ms, enqueue

    def __repr__(self):
        return "Delay(%s, %s, %.1f ms)" % (self.how, self.arg, self.ms)


def stream_ms(fn):
    torch = T()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


@pytest.fixture(scope="session")
def delay():
    """about 50 ms of stream time: torch.cuda._sleep calibrated with two events, or a chain of matrix products of measured length"""
    torch = T()
    torch.cuda.init()
    try:
        stream_ms(lambda: torch.cuda._sleep(1000))
        probe = 2_000_000
        ms = stream_ms(lambda: torch.cuda._sleep(probe))
        if ms > 0.2:
            cycles = int(probe * 50.0 / ms)
            got = stream_ms(lambda: torch.cuda._sleep(cycles))
            if 25.0 <= got <= 250.0:
                d = Delay("torch.cuda._sleep", cycles, got, lambda: torch.cuda._sleep(cycles))
                print("\n[async] delay: torch.cuda._sleep(%d) = %.1f ms" % (cycles, got))
                return d
    except (AttributeError, RuntimeError):
        pass
    a = torch.randn(4096, 4096, device="cuda")
    c = torch.empty_like(a)
    stream_ms(lambda: torch.mm(a, a, out=c))
    one = stream_ms(lambda: torch.mm(a, a, out=c))
    reps = max(1, int(np.ceil(50.0 / one)))

    def chain():
        for _ in range(reps):
            torch.mm(a, a, out=c)
    got = stream_ms(chain)
    assert got >= 25.0, "no usable delay on this machine: %d products take %.1f ms" % (reps, got)
    print("\n[async] delay: %d products of 4096^2 = %.1f ms" % (reps, got))
    return Delay("torch.mm chain", reps, got, chain)


@pytest.fixture(scope="session")
def controls(delay):
    """While the delay is pending on s, a clone of x_dev on a second stream, and one on torch's default (the null) stream, must
    both hold the DECOY: the delay withholds the data, and neither stream is ordered behind s."""
    torch = T()
    real = torch.arange(4096, dtype=torch.float32).pin_memory()
    x = torch.full((4096,), -1.0, device="cuda")
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay.enqueue()
        x.copy_(real, non_blocking=True)
    with torch.cuda.stream(s2):
        other = x.clone()
    legacy = x.clone()          # torch's default stream
    pending = not s.query()
    s2.synchronize()
    torch.cuda.default_stream().synchronize()
    still = not s.query()
    s.synchronize()
    out = dict(pending_on_return=pending, pending_after_clones=still,
               second_stream_saw_decoy=bool((other == -1).all().item()), legacy_stream_saw_decoy=bool((legacy == -1).all().item()),
               data_arrived=bool((x.cpu() == real).all().item()))
    print("\n[async] controls: %s" % out)
    return out


def test_controls(delay, controls):
    assert controls["data_arrived"]
    assert controls["pending_on_return"] and controls["pending_after_clones"], "the delay does not hold the stream: %s, %s" % (delay, controls)
    assert controls["second_stream_saw_decoy"], "a second stream saw the late data: the delay withholds nothing (%s)" % (controls,)
    assert controls["legacy_stream_saw_decoy"], ("the null stream is ordered behind a torch stream on this machine: legacy-stream "
                                                 "copies inside the library are no hazard here and this file proves nothing (%s)" % (controls,))


@pytest.fixture()
def late(delay, controls):
    """the delay, usable only where both controls hold"""
    test_controls(delay, controls)
    return delay


# ----------------------------------------------------------------------------------------------------------------------
# the harness
# ----------------------------------------------------------------------------------------------------------------------
def tuple_of(ret):
    ret = ret if isinstance(ret, tuple) else (ret,)
    return tuple(np.ascontiguousarray(rc.host(a)) for a in ret)


def host_call(g, call, ins):
    """the call on host arrays: synchronous by construction"""
    b = {k: v.copy() for k, v in ins.items()}
    for name, (shape, dt) in call.outs.items():
        b[name] = np.empty(shape, dt)
    ret = call.issue(g, b)
    names = call.result_names()
    return tuple(b[n] for n in names) if names else (tuple_of(ret) if ret is not None else ())


class Run:
    """every buffer of one Call, allocated up front on torch's default stream"""

    def __init__(self, call):
        torch = T()
        self.call, self.ret = call, None
        self.dev, self.pin, self.decoy, self.out, self.out_pin = {}, {}, {}, {}, {}
        for name, real in call.ins.items():
            self.decoy[name] = torch.from_numpy(call.decoys[name].copy()).cuda()
            self.dev[name] = self.decoy[name].clone()
            self.pin[name] = torch.from_numpy(real.copy()).pin_memory()
        for name, (shape, dt) in call.outs.items():
            self.out[name] = torch.from_numpy(np.empty(shape, dt)).cuda()
            self.out[name].view(torch.uint8).fill_(SENTINEL)
        for name in call.result_names():
            src = self.source(name)
            self.out_pin[name] = torch.empty(src.shape, dtype=src.dtype).pin_memory()

    def rearm(self):
        """before the Run is fired again: the sentinel in the outputs once more (the inputs hold the decoy after every fire)"""
        torch = T()
        for t in self.out.values():
            t.view(torch.uint8).fill_(SENTINEL)
        torch.cuda.synchronize()

    def source(self, name):
        return self.dev[name] if name in self.call.inout else self.out[name]

    def buffers(self):
        return dict(self.dev, **self.out)


def fire(g, s, run, delay, around=None):
    """on s: the delay, the real inputs, the call, the outputs to page-locked memory, the decoy over the inputs again.
    Returns (the stream was still busy when the call returned, host seconds of the call)."""
    torch = T()
    call = run.call
    with torch.cuda.stream(s):
        delay.enqueue()
        for name in call.ins:
            run.dev[name].copy_(run.pin[name], non_blocking=True)
        with (around if around is not None else contextlib.nullcontext()):
            t0 = time.perf_counter()
            run.ret = call.issue(g, run.buffers())
            dt = time.perf_counter() - t0
        busy = not s.query()
        for name in call.result_names():
            run.out_pin[name].copy_(run.source(name), non_blocking=True)
        for name in call.ins:
            run.dev[name].copy_(run.decoy[name], non_blocking=True)
    HOST_MS[call.what] = dt * 1e3
    return busy, dt


def collect(s, run):
    s.synchronize()
    names = run.call.result_names()
    if names:
        return tuple(run.out_pin[n].numpy().copy() for n in names)
    return tuple_of(run.ret) if run.ret is not None else ()


def as_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(got, want, what, want_decoy=None):
    """bit for bit: the same handle ran the same kernels on the same inputs"""
    assert len(got) == len(want), what
    for i, (g_, w) in enumerate(zip(got, want)):
        assert g_.shape == w.shape and g_.dtype == w.dtype, "%s: output %d is %s %s, expected %s %s" % (what, i, g_.dtype, g_.shape, w.dtype, w.shape)
        if np.array_equal(as_bytes(g_), as_bytes(w)):
            continue
        why = ""
        if want_decoy is not None and np.array_equal(as_bytes(g_), as_bytes(want_decoy[i])):
            why = " -- these are the DECOY's rows: an input was not read on the handle's stream"
        elif (as_bytes(g_) == SENTINEL).all():
            why = " -- the sentinel: the output was not written on the handle's stream"
        n = g_.shape[0] if g_.ndim else 1
        bad = np.nonzero((as_bytes(g_).reshape(n, -1) != as_bytes(w).reshape(n, -1)).any(axis=1))[0]
        raise AssertionError("%s: output %d differs from the synchronous call in %d of %d rows, first row %d%s" % (what, i, bad.size, n, bad[0], why))


def assert_asynchronous(busy, dt, delay, what):
    if busy:
        return
    if dt * 1e3 < 0.5 * delay.ms:
        raise AssertionError("%s: the delay did not hold -- the stream was idle when the call returned after %.3f ms on the host "
                             "(delay %.1f ms): nothing is proven" % (what, dt * 1e3, delay.ms))
    raise AssertionError("%s: a class A call waited for its stream (%.1f ms on the host, the delay is %.1f ms); its header promises "
                         "a call that is asynchronous on the handle's stream" % (what, dt * 1e3, delay.ms))


def late_call(g, s, call, run, delay, around=None):
    """warm (want, want_decoy), fire, collect, compare; returns want"""
    want = host_call(g, call, call.ins)
    want_decoy = host_call(g, call, call.decoys)
    busy, dt = fire(g, s, run, delay, around)
    got = collect(s, run)
    same(got, want, call.what, want_decoy)
    if call.klass == "A":
        assert_asynchronous(busy, dt, delay, call.what)
    print("[async] %-70s class %s  host %.3f ms  busy on return %s" % (call.what, call.klass, dt * 1e3, busy))
    return want


def prepared(calls):
    torch = T()
    runs = [Run(c) for c in calls]
    torch.cuda.synchronize()
    return runs


# ----------------------------------------------------------------------------------------------------------------------
# every call of every kind, with late inputs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [a.name for a in ac.KINDS])
def test_late_inputs(name, late):
    torch = T()
    a = ac.BY_NAME[name]
    calls = [a.search_call(), a.two_searches()] + a.calls()
    g = a.fresh()
    try:
        runs = prepared(calls)
        s = torch.cuda.Stream()
        g.set_stream(s.cuda_stream)
        for i, (call, run) in enumerate(zip(calls, runs)):
            screened = g.coarse_screen_state()[1] if name == "ivfpq-imi" else 0
            want = late_call(g, s, call, run, late)
            if i == 0:      # the one tie to the kind's CPU reference: the synchronous rows by the kind's own rule
                rule, ref = a.reference(g)
                rule(want, ref, "%s: the synchronous rows against the CPU reference" % name)
            if name == "ivfpq-imi" and "x2" not in call.ins:
                # both halves of the multi-index went through the screen in each of the three calls: the two-stream stage ran
                # (the second of two searches back to back is below the screen's 2 048 rows)
                assert g.coarse_screen_state()[1] - screened == 3 * 2 * call.ins["x"].shape[0], (call.what, g.coarse_screen_state())
    finally:
        a.close(g)


@pytest.mark.parametrize("name", ac.ENCODES)
def test_encode_of_a_late_input(name, late):
    """class B: the header says these synchronise the stream, for device buffers too"""
    torch = T()
    a = ac.BY_NAME[name]
    x = a.xq()
    call = ac.Call("%s: encode" % name, "vlq_%s_encode" % a.prefix, "B", lambda g, b: g.encode(b["x"]), dict(x=x), dict(x=ac.other_rows(x)))
    g = a.fresh()
    try:
        (run,) = prepared([call])
        s = torch.cuda.Stream()
        g.set_stream(s.cuda_stream)
        late_call(g, s, call, run, late)
        assert s.query()
    finally:
        a.close(g)


@pytest.mark.parametrize("name", ac.ADDS)
def test_add_of_a_late_input(name, late):
    """class B: add synchronises the stream; what the handle stores afterwards is what a handle that was given host rows stores"""
    torch = T()
    a = ac.BY_NAME[name]
    x = a.xq()
    call = ac.Call("%s: add" % name, "vlq_%s_add" % a.prefix, "B", lambda g, b: g.add(b["x"]), dict(x=x), dict(x=ac.other_rows(x)))
    g, f = a.fresh(), a.fresh()
    try:
        (run,) = prepared([call])
        s = torch.cuda.Stream()
        g.set_stream(s.cuda_stream)
        fire(g, s, run, late)
        assert g.ntotal == f.ntotal + x.shape[0]
        collect(s, run)
        f.add(x)
        rc.same_stored(a.rk.read(g), a.rk.read(f), True, "%s: the lists after add(late device rows) against add(host rows)" % name)
    finally:
        a.close(g)
        a.close(f)


# ----------------------------------------------------------------------------------------------------------------------
# counters, pending errors, the private stream, set_stream under load, GpuRefineFlat
# ----------------------------------------------------------------------------------------------------------------------
def counts(a, g):
    return g.stats() + ((g.polysemous_stats(),) if a.prefix == "ivfpq" else ())


@pytest.mark.parametrize("name", ac.COUNTED)
def test_counters_around_an_asynchronous_search(name, late):
    """stats(reset=True), at once a delayed asynchronous search, then stats(): the counts of exactly that search -- a clear that
    is not ordered before the search on the handle's stream, or a read that is not ordered behind it, shows here"""
    torch = T()
    a = ac.BY_NAME[name]
    call = a.search_call()
    g = a.fresh()
    try:
        (run,) = prepared([call])
        s = torch.cuda.Stream()
        g.set_stream(s.cuda_stream)
        host_call(g, call, call.decoys)
        g.stats(reset=True)
        if a.prefix == "ivfpq":
            g.polysemous_stats(reset=True)
        want = host_call(g, call, call.ins)
        want_counts = counts(a, g)
        assert want_counts[0] == call.ins["x"].shape[0] and want_counts[1] > 0, want_counts
        if "polysemous" in name:
            assert want_counts[2] > 0, "the Hamming filter passed nothing: %s" % (want_counts,)
        host_call(g, call, call.decoys)
        g.stats(reset=True)
        if a.prefix == "ivfpq":
            g.polysemous_stats(reset=True)
        busy, dt = fire(g, s, run, late)
        assert_asynchronous(busy, dt, late, call.what)
        got_counts = g.stats()
        assert s.query(), "stats() is documented to synchronise the stream"
        got_counts += (g.polysemous_stats(),) if a.prefix == "ivfpq" else ()
        same(collect(s, run), want, call.what)
        assert got_counts == want_counts, "%s: counts %s after the asynchronous search, %s after the synchronous one" % (name, got_counts, want_counts)
    finally:
        a.close(g)


@pytest.mark.parametrize("name", ac.BAD_KEYS)
def test_pending_error_of_a_late_key(name, late):
    """one key >= nlist, arriving late, device outputs: the call returns without error while the stream is busy, the rows are those
    of the same call with that key -1, the error is raised exactly once by the call documented to raise it, and a clean
    asynchronous search follows"""
    torch = T()
    a = ac.BY_NAME[name]
    bad, skip = a.bad_key_calls()
    clean = a.preassigned_call()
    raise_it = lambda g: getattr(g, a.sync)()  # noqa: E731
    g = a.fresh()
    try:
        run_bad, run_clean = prepared([bad, clean])
        s = torch.cuda.Stream()
        g.set_stream(s.cuda_stream)
        want_skip = host_call(g, skip, skip.ins)
        want_clean = host_call(g, clean, clean.ins)
        want_decoy = host_call(g, clean, clean.decoys)
        raise_it(g)
        busy, dt = fire(g, s, run_bad, late)
        assert_asynchronous(busy, dt, late, bad.what)
        same(collect(s, run_bad), want_skip, bad.what, want_decoy)
        with pytest.raises(vlq.VlqError) as e:
            raise_it(g)
        assert e.value.code == ERR_INVALID and "nlist" in str(e.value)
        raise_it(g)          # exactly once
        busy, dt = fire(g, s, run_clean, late)
        assert_asynchronous(busy, dt, late, clean.what)
        same(collect(s, run_clean), want_clean, clean.what, want_decoy)
        raise_it(g)          # and the clear did not eat a flag, nor leave one
    finally:
        a.close(g)


@pytest.mark.parametrize("name", [a.name for a in ac.KINDS])
def test_private_stream_is_drained_by_the_documented_call(name):
    """never set_stream: device inputs that are complete, device outputs, then only the call documented to synchronise the stream
    (stats, or last_scan_info) -- no device-wide synchronise.  The rows must be complete."""
    torch = T()
    a = ac.BY_NAME[name]
    call = a.search_call()
    g = a.fresh()
    try:
        want = host_call(g, call, call.ins)
        run = Run(call)
        for k_ in call.ins:
            run.dev[k_].copy_(run.pin[k_])
        torch.cuda.synchronize()
        call.issue(g, run.buffers())
        if a.sync is not None:
            getattr(g, a.sync)()
        got = tuple(run.out[n].cpu().numpy() for n in call.result_names())
        same(got, want, "%s on its private stream, then %s()" % (name, a.sync))
    finally:
        a.close(g)


@pytest.mark.parametrize("name", [a.name for a in ac.KINDS if a.search_class == "A"])
def test_set_stream_while_work_is_pending(name, late):
    """a delayed asynchronous search on s1, then set_stream(s2), then a search on s2: the setter drains the old stream"""
    torch = T()
    a = ac.BY_NAME[name]
    first, second = a.search_call(), a.search_call(ac.other_rows(a.xq())[:max(2, a.xq().shape[0] - 1)], "search on the second stream")
    g = a.fresh()
    try:
        run1, run2 = prepared([first, second])
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        g.set_stream(s1.cuda_stream)
        want1, want2 = host_call(g, first, first.ins), host_call(g, second, second.ins)
        host_call(g, first, first.decoys)
        for k_ in second.ins:
            run2.dev[k_].copy_(run2.pin[k_])
        torch.cuda.synchronize()
        busy, dt = fire(g, s1, run1, late)
        assert_asynchronous(busy, dt, late, first.what)
        g.set_stream(s2.cuda_stream)
        assert s1.query(), "set_stream returned while the old stream still had the handle's work"
        with torch.cuda.stream(s2):
            second.issue(g, run2.buffers())
            for n in second.result_names():
                run2.out_pin[n].copy_(run2.source(n), non_blocking=True)
        s2.synchronize()
        same(tuple(run1.out_pin[n].numpy() for n in first.result_names()), want1, first.what)
        same(tuple(run2.out_pin[n].numpy() for n in second.result_names()), want2, second.what)
    finally:
        a.close(g)


@pytest.mark.parametrize("k_factor", [1.0, 4.0])
@pytest.mark.parametrize("name", ["refineflat-over-ivfsq", "refineflat-over-pq"])
def test_refine_flat_from_a_third_stream(name, k_factor, late):
    """GpuRefineFlat chains the base search and GpuFlat.refine through device tensors it allocates on torch's CURRENT stream and
    uses on its own.  Device x, D and I with late inputs, issued while torch's current stream is a third stream; k_factor 1 is the
    in-place form, 4 goes through the shortlist, which the second call (another n) replaces."""
    torch = T()
    a = ac.BY_NAME[name]
    x = a.xq()
    calls = [a.search_call(x, "search, k_factor %g" % k_factor), a.search_call(np.ascontiguousarray(x[::-1][:41]), "search of 41 rows, k_factor %g" % k_factor)]
    r = a.fresh()
    try:
        r.k_factor = k_factor
        runs = prepared(calls)
        third = torch.cuda.Stream()
        # Two streams, one after the other: the runtime spreads its streams over a few hardware queues, and a stream the object
        # forgot to move (the store's private one) is serialised behind the delay BY ACCIDENT where it shares a queue with s.
        # Streams created in a row get different queues, so it can hide behind one of the two at the most.
        for s in (torch.cuda.Stream(), torch.cuda.Stream()):
            r.set_stream(s.cuda_stream)
            for call, run in zip(calls, runs):
                run.rearm()
                late_call(r, s, call, run, late, around=torch.cuda.stream(third))
        if k_factor > 1:
            assert r._short[0].shape == (41, r.k_base(a.k))
    finally:
        a.close(r)
