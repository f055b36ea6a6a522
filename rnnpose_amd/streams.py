"""The stream schedule of the engines: helper streams bound to DISTINCT hardware queues, and the only code that forks and joins them.

ROCm multiplexes every HIP stream of a process onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default): a stream gets
its queue when it is first used -- a new queue while fewer than the maximum exist, otherwise the least-referenced existing
one -- and two streams that land on the same queue execute strictly one after the other.  Measured (r02,
tools/loop_overlap.py): the inner loops of the two batch halves took 6.4 ms each and 13.2 ms "concurrently" when their
streams happened to share a queue, i.e. no overlap at all, and whether they did depended on the order in which unrelated
streams (capture streams, warm-up streams) had been touched before.

So the streams that must run concurrently are created once per device and TOUCHED immediately, in a fixed order, right
after the default stream: default = queue 1, chain[0] = queue 2, chain[1] = queue 3, aux = queue 4.  Everything created
later (torch's capture streams, temporary warm-up streams) shares those queues and only ever carries work that does not
need to overlap with ours.

A cross-queue dependency costs ~100 us on this GPU (r02 timeline: the second chain of every inner iteration started 115 us after the
event it waited for), an in-queue one ~1 us: run_interleaved forks ONCE and joins ONCE, however long its jobs are.
"""
from __future__ import annotations

import torch

from . import ops

_sets = {}


class StreamSet:
    def __init__(self, device):
        self.chain = [torch.cuda.Stream(device=device) for _ in range(2)]   # the two batch halves / image sets
        self.aux = torch.cuda.Stream(device=device)                          # side chain of an unsplit (B = 1) step
        self.extra = [torch.cuda.Stream(device=device) for _ in range(2)]    # (experiments with more than two parts)
        for s in self.chain + [self.aux] + self.extra:
            with torch.cuda.stream(s):
                torch.zeros(1, device=device)        # first use: binds the stream to its hardware queue now
            s.synchronize()


def reserve(device) -> StreamSet:
    """The StreamSet of `device` (created and bound on first call -- call it before any other side stream is used)."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st = _sets.get(dev)
    if st is None:
        st = _sets[dev] = StreamSet(dev)
    return st


def helper_stream(device, i):
    """Element i of chain + [aux] + extra.  Update engine: chain k of a captured loop replays on k; eager, chain i >= 1 runs on i and the
    flow-feature / flow-head side chain of an unsplit step on 2.  Encoder: image set / batch part i >= 1 runs on (i - 1) % 3.
    Under ops.profile() everything goes to the caller's stream: each launch is timed ALONE on the chip -- the duration a roofline wants (and
    what rocprofv3's kernel trace, which serialises kernels, reports); next to its twin on another stream it would include the sharing."""
    if ops.profiling():
        return torch.cuda.current_stream()
    ss = reserve(device)
    return (ss.chain + [ss.aux] + ss.extra)[i]


def run_interleaved(jobs, main):
    """jobs: [(generator, stream)].  Every generator's launches go to its stream; the generators are advanced in turn (hipGraphLaunch
    submits in capture order).  Streams other than `main` start after everything already on `main`; `main` waits for them at the end."""
    fork = torch.cuda.Event()
    fork.record(main)
    for _, st in jobs:
        if st is not main:
            st.wait_event(fork)
    active = list(jobs)
    while active:
        for item in list(active):
            g, st = item
            with torch.cuda.stream(st):
                try:
                    next(g)
                except StopIteration:
                    active.remove(item)
    for _, st in jobs:
        if st is not main:
            j = torch.cuda.Event()
            j.record(st)
            main.wait_event(j)


def side_branch(main, side, fn):
    """fn() on `side`, after everything already on `main` -> the event `main` has to wait for before it reads what fn wrote."""
    fork = torch.cuda.Event()
    fork.record(main)
    side.wait_event(fork)
    with torch.cuda.stream(side):
        fn()
        join = torch.cuda.Event()
        join.record(side)
    return join


def warm_up(fn):
    """fn() on a fresh side stream, between the current stream's past and future work (the eager runs in front of a graph capture)."""
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        fn()
    main.wait_stream(side)


def drain(gen):
    """Run a launch generator to its end -> its return value."""
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value
