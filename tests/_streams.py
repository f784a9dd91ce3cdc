"""Stream-ordering harness: makes a launch, memset or copy that is not on the caller's stream
give wrong numbers, deterministically, instead of passing by luck.

Every other GPU test runs on the null stream, where everything is serialised.  Here a call runs
on a side stream S (torch creates it non-blocking: no implicit ordering with the null stream)
between two delays:

    read early   the working tensors hold POISON (valid but wrong input).  On S a delay is queued,
                 then device-to-device copies of the true inputs into the working tensors, then the
                 call, then clones of every output and of every tensor the call updates in place.
                 A launch that is not on S runs during the delay and reads poison.
    write late   before the call a longer delay is queued on the null stream.  A launch that lands
                 there is held back past S's clones, which then see the outputs' SENTINEL fill.

Poison is valid input (finite floats, in-range ascending indices, well-formed packed words, norms
of 1): a misordered launch computes wrong numbers, it never faults.

The delays are torch.cuda._sleep(cycles), calibrated once per process against two events.  A
case's delay is four times the host time its call took to enqueue in a warm-up run on S (floor
20 ms, refused above 500 ms); the null-stream delay is twice that, so that it outlasts S's delay,
copies, kernels and clones.  The warm-up is needed anyway: the first call on a new stream
allocates that stream's workspaces.  It runs on the poison, so no workspace holds an intermediate
of the true inputs for a misordered launch to find.

A case is valid only if both delays are still pending when the call returns on the host; run()
asserts that (a wrapper that synchronises the host would make the case vacuous).
"""
import time

import torch

SENTINEL = -7.0  # the suite's: exact in every dtype
FLOOR_MS = 20.0
CEIL_MS = 500.0
_PROBE_CYCLES = 20_000_000

_state = {}
report = {}  # family -> [(case, enqueue ms, delay ms)], printed by the tests (-s)


def side_stream(name="S"):
    """One side stream per name for the whole process, so its workspaces stay warm."""
    s = _state.get(("stream", name))
    if s is None:
        s = _state[("stream", name)] = torch.cuda.Stream()
    return s


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond on this device: one fixed sleep between two events."""
    c = _state.get("cycles_per_ms")
    if c is None:
        torch.cuda._sleep(1000)  # the first launch loads the kernel
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(_PROBE_CYCLES)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.5, f"_sleep({_PROBE_CYCLES}) took {ms} ms: too short to calibrate from"
        c = _state["cycles_per_ms"] = _PROBE_CYCLES / ms
        print(f"\n[streams] calibration: _sleep({_PROBE_CYCLES}) = {ms:.3f} ms -> {c:.0f} cycles/ms")
    return c


def delay(ms, stream):
    """Queue a delay of `ms` on `stream`; returns an event recorded right behind it."""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms()))
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def delay_for(enqueue_ms):
    d = max(FLOOR_MS, 4.0 * enqueue_ms)
    assert d <= CEIL_MS, f"the call takes {enqueue_ms:.1f} ms to enqueue: a {d:.0f} ms delay -- shrink the case"
    return d


def _tensors(obj):
    if obj is None:
        return []
    if torch.is_tensor(obj):
        return [obj]
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in _tensors(v)]
    if isinstance(obj, (list, tuple)):
        return [t for v in obj for t in _tensors(v)]
    return []


def _clone(obj):
    if torch.is_tensor(obj):
        return obj.clone()
    if isinstance(obj, dict):
        return {k: _clone(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_clone(v) for v in obj)
    return obj


def scribble(obj):
    """Fill every tensor of `obj` with SENTINEL (-7 in its own dtype; 0xF9 in bytes)."""
    for t in _tensors(obj):
        t.fill_(0xF9 if t.dtype == torch.uint8 else SENTINEL if t.dtype.is_floating_point else int(SENTINEL))


def run(call, work, true, poison, outs=(), family="misc", case="", stream=None, other=None,
        read_early=True, write_late=True, warm=2, require_pending=True):
    """One call under the harness.

    call()   the call under test (it reads and updates the `work` tensors, writes `outs`); what it
             returns (tensors, or lists / dicts of them) is cloned on the stream with `outs` and `work`
    work     {name: working tensor}; true / poison: {name: tensor} of the same shapes, prepared
             beforehand (a name missing from poison keeps its true value throughout)
    outs     pre-allocated output tensors, SENTINEL-filled before the call
    stream   the caller's stream (default: the shared side stream); other: the stream the
             write-late delay goes on (default: the null stream)
    warm     warm-up calls on the poison: the first allocates the stream's workspaces (and synchronises),
             the last one is timed

    Returns (returned, work, outs) as clones taken on `stream` right behind the call."""
    S = stream if stream is not None else side_stream()
    null = other if other is not None else torch.cuda.default_stream()
    assert S != null
    cycles_per_ms()

    def refill(src):
        for k, t in work.items():
            t.copy_(src.get(k, true[k]))

    enqueue_ms = 0.0
    for _ in range(warm):
        refill(poison)
        scribble(list(outs))
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            t0 = time.perf_counter()
            ret = call()
            enqueue_ms = (time.perf_counter() - t0) * 1e3
            keep = (_clone(ret), _clone(work), _clone(list(outs)))  # warms the allocator for the clones too
        torch.cuda.synchronize()
        # what the call allocated comes back from the allocator for the real run: leave SENTINEL in it
        with torch.cuda.stream(S):
            scribble(ret)
            scribble(keep)
        torch.cuda.synchronize()
        del ret, keep
    d = delay_for(enqueue_ms)
    report.setdefault(family, []).append((case, enqueue_ms, d))

    refill(poison)
    scribble(list(outs))
    torch.cuda.synchronize()
    ev_s = ev_n = None
    with torch.cuda.stream(S):
        if read_early:
            ev_s = delay(d, S)
        for k, t in work.items():
            t.copy_(true[k], non_blocking=True)
        if write_late:
            ev_n = delay(2.0 * d, null)
        ret = call()
        pending = [ev is None or not ev.query() for ev in (ev_s, ev_n)]
        got = (_clone(ret), _clone(work), _clone(list(outs)))
    S.synchronize()
    torch.cuda.synchronize()
    if require_pending:
        assert pending[0], f"{family}/{case}: the call returned after the {d:.0f} ms delay on its own stream had run " \
                           f"out: it synchronises the host (enqueue {enqueue_ms:.2f} ms)"
        assert pending[1], f"{family}/{case}: the call returned after the null-stream delay had run out"
    return got


def run_whole(fn, family="steps", case=""):
    """A runner that builds its own inputs, steps and compares with its own oracle, run wholly on
    the side stream: the write-late direction alone (the read-early direction stays untested for
    what is run this way).  Such a runner uploads its inputs
    (`torch.from_numpy(...).to(device)`) and reads its results back (`.cpu()`), and both wait for
    the stream, so a delay in front of it on its own stream would only be waited out.  The
    null-stream delay is queued once, in front of the whole runner, sized from the runner's warm
    duration on the side stream: a launch that lands on the null stream is held back past the
    runner's read-backs, and the runner's own comparison fails.  Still pending when the runner
    returns, or the case is not valid."""
    S = side_stream()
    cycles_per_ms()
    ms = 0.0
    for _ in range(2):  # the first run allocates this stream's workspaces
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    d = delay_for(ms)
    report.setdefault(family, []).append((case, ms, d))
    ev = delay(d, torch.cuda.default_stream())
    with torch.cuda.stream(S):
        fn()
    pending = not ev.query()
    torch.cuda.synchronize()
    assert pending, f"{family}/{case}: the {d:.0f} ms null-stream delay ran out before the runner returned ({ms:.1f} ms warm)"


def print_report(family=None):
    for fam, rows in report.items():
        if family is not None and fam != family:
            continue
        enq = [r[1] for r in rows]
        dl = [r[2] for r in rows]
        print(f"[streams] {fam}: {len(rows)} cases, enqueue {min(enq):.3f}..{max(enq):.3f} ms, "
              f"delay {min(dl):.0f}..{max(dl):.0f} ms")
