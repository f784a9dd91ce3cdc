"""The launch path (choco_common.h CHOCO_LAUNCH): every launch of a named call site is
counted, with timing on or off and from any host thread; with timing on each launch that
passes the name filter is timed exactly once, and a filtered-out launch is not timed."""
import threading

import pytest
import torch

from chocosgd_amd import codec

pytestmark = pytest.mark.gpu
DEV = "cuda"
THREADS, CALLS, N = 2, 50, 1024


def _gossip_from_threads(streams):
    """One host thread per stream, CALLS gossip steps each."""
    errors = []

    def work(seed):
        try:
            stream = streams[seed]
            with torch.cuda.stream(stream):
                x = torch.full((N,), float(seed), device=DEV)
                mem = torch.ones(N, device=DEV)
                hat = torch.zeros(N, device=DEV)
                for _ in range(CALLS):
                    codec.gossip_step(x, mem, hat, 0.5)
                stream.synchronize()
            if not torch.equal(x, torch.full((N,), seed + 0.5 * CALLS, device=DEV)):
                errors.append(f"thread {seed}: wrong result")
        except Exception as e:  # reported by the caller's assert
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(streams))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_launches_are_counted_and_timed_once_each_from_two_threads():
    total = THREADS * CALLS
    streams = [torch.cuda.Stream(device=DEV) for _ in range(THREADS)]
    try:
        codec.profile_enable(False)
        c0 = codec.launch_count("gossip_step")
        t0 = codec.profile_read("gossip_step")[1]
        _gossip_from_threads(streams)
        assert codec.launch_count("gossip_step") - c0 == total       # counted with timing off
        assert codec.profile_read("gossip_step")[1] == t0            # and not timed

        codec.profile_enable(True)
        _gossip_from_threads(streams)
        assert codec.profile_read("gossip_step")[1] - t0 == total    # one event pair per launch
        assert codec.launch_count("gossip_step") - c0 == 2 * total

        codec.profile_filter("topk_stream")
        _gossip_from_threads(streams)
        assert codec.profile_read("gossip_step")[1] - t0 == total    # filtered out: rises by 0
        assert codec.launch_count("gossip_step") - c0 == 3 * total   # still counted
    finally:
        codec.profile_filter(None)
        codec.profile_enable(False)
