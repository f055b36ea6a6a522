"""The stream schedule as an operation log: rnnpose_amd.streams is the one place that forks and joins streams, and these tests pin what
it enqueues, in which order, without a GPU -- recording stand-ins for torch.cuda.Event / torch.cuda.stream / the stream objects take
the place of the real ones (tests/host_exec/hostmode.py does the same with inert ones).  Plus the small shared helpers the engines
read their switches and weight-cache rules from."""
import pytest
import torch

from rnnpose_amd import env, ops, streams


class Log(list):
    def __init__(self):
        super().__init__()
        self.current = None
        self.events = 0


class FakeStream:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def wait_event(self, ev):
        self.log.append(("wait", self.name, ev.name))

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.name, other.name))


@pytest.fixture
def cuda(monkeypatch):
    """-> (log, stream factory); `main` is the current stream."""
    log = Log()

    class Event:
        def __init__(self, *a, **k):
            self.name = f"e{log.events}"
            log.events += 1

        def record(self, stream=None):
            log.append(("record", self.name, (stream or log.current).name))

    class StreamContext:
        def __init__(self, st):
            self.st = st

        def __enter__(self):
            self.prev, log.current = log.current, self.st

        def __exit__(self, *exc):
            log.current = self.prev
            return False

    made = []

    def new_stream(*a, **k):
        made.append(FakeStream(log, f"new{len(made)}"))
        return made[-1]

    mk = lambda name: FakeStream(log, name)
    log.current = mk("main")
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "stream", StreamContext)
    monkeypatch.setattr(torch.cuda, "Stream", new_stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: log.current)
    return log, mk


def _job(log, name, steps, value=None):
    for i in range(steps):
        log.append(("launch", f"{name}.{i}", log.current.name))
        yield
    return value


def test_run_interleaved_three_jobs_exact_log(cuda):
    log, mk = cuda
    main, a, b = log.current, mk("a"), mk("b")
    streams.run_interleaved([(_job(log, "j0", 2), main), (_job(log, "j1", 3), a), (_job(log, "j2", 1), b)], main)
    assert list(log) == [
        ("record", "e0", "main"),
        ("wait", "a", "e0"), ("wait", "b", "e0"),
        ("launch", "j0.0", "main"), ("launch", "j1.0", "a"), ("launch", "j2.0", "b"),
        ("launch", "j0.1", "main"), ("launch", "j1.1", "a"),
        ("launch", "j1.2", "a"),
        ("record", "e1", "a"), ("wait", "main", "e1"),
        ("record", "e2", "b"), ("wait", "main", "e2"),
    ]
    assert log.current is main


def test_run_interleaved_single_job_on_main_has_no_waits(cuda):
    log, _ = cuda
    main = log.current
    streams.run_interleaved([(_job(log, "j0", 2), main)], main)
    assert list(log) == [("record", "e0", "main"), ("launch", "j0.0", "main"), ("launch", "j0.1", "main")]


def test_run_interleaved_two_jobs_off_main_both_wait_and_both_join(cuda):
    """The replay of a captured loop: both batch halves on pool streams, none on the caller's."""
    log, mk = cuda
    main, a, b = log.current, mk("a"), mk("b")
    streams.run_interleaved([(_job(log, "j0", 1), a), (_job(log, "j1", 1), b)], main)
    assert list(log) == [
        ("record", "e0", "main"),
        ("wait", "a", "e0"), ("wait", "b", "e0"),
        ("launch", "j0.0", "a"), ("launch", "j1.0", "b"),
        ("record", "e1", "a"), ("wait", "main", "e1"),
        ("record", "e2", "b"), ("wait", "main", "e2"),
    ]


def test_side_branch_log(cuda):
    log, mk = cuda
    main, side = log.current, mk("side")
    join = streams.side_branch(main, side, lambda: streams.drain(_job(log, "f", 2)))
    assert list(log) == [("record", "e0", "main"), ("wait", "side", "e0"), ("launch", "f.0", "side"), ("launch", "f.1", "side"),
                         ("record", "e1", "side")]
    assert join.name == "e1" and log.current is main            # the caller places main.wait_event(join) itself


def test_warm_up_log(cuda):
    log, _ = cuda
    streams.warm_up(lambda: log.append(("launch", "w", log.current.name)))
    assert list(log) == [("wait_stream", "new0", "main"), ("launch", "w", "new0"), ("wait_stream", "main", "new0")]


def test_drain_returns_the_generators_value(cuda):
    log, _ = cuda
    assert streams.drain(_job(log, "g", 3, value="done")) == "done"
    assert [e[1] for e in log] == ["g.0", "g.1", "g.2"]
    assert streams.drain(iter(())) is None


def test_helper_stream_is_the_current_stream_while_profiling(cuda, monkeypatch):
    log, _ = cuda
    monkeypatch.setattr(ops, "profiling", lambda: True)
    monkeypatch.setattr(streams, "reserve", lambda device: pytest.fail("profiling: no helper streams"))
    for i in range(5):
        assert streams.helper_stream("cuda:0", i) is log.current


def test_helper_stream_index_mapping(cuda, monkeypatch):
    class Set:
        chain, aux, extra = ["c0", "c1"], "aux", ["x0", "x1"]
    monkeypatch.setattr(ops, "profiling", lambda: False)
    monkeypatch.setattr(streams, "reserve", lambda device: Set)
    assert [streams.helper_stream("cuda:0", i) for i in range(5)] == ["c0", "c1", "aux", "x0", "x1"]


def test_env_readers(monkeypatch):
    name = "RNNPOSE_TEST_SWITCH"
    monkeypatch.delenv(name, raising=False)
    assert env.flag(name, True) is True and env.flag(name, False) is False and env.flag(name, None) is None
    assert env.number(name, 2) == 2 and env.number(name, None) is None and env.text(name) is None and env.text(name, "") == ""
    for value, want in (("0", False), ("1", True), ("", True), ("off", True)):
        monkeypatch.setenv(name, value)
        assert env.flag(name, True) is want and env.flag(name, False) is want and env.flag(name, None) is want
    monkeypatch.setenv(name, "3")
    assert env.number(name, 2) == 3 and env.text(name) == "3"


@pytest.mark.parametrize("shape, want", [((256, 324, 1, 1), True), ((256, 352, 1, 1), True), ((256, 356, 1, 1), False),
                                         ((256, 322, 1, 1), False), ((128, 324, 1, 1), False), ((256, 128, 3, 3), False)])
def test_packed_conv1x1_fits(shape, want):
    assert ops.PackedConv1x1.fits(torch.empty(shape)) is want


def test_param_key_tracks_version_and_storage():
    conv = torch.nn.Conv2d(4, 4, 1)
    k0 = ops.param_key([conv])
    assert k0 == ops.param_key([conv]) and len(k0) == 1 and len(k0[0]) == 4
    with torch.no_grad():
        conv.bias.add_(1.0)
    assert ops.param_key([conv]) != k0
