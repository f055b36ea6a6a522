"""bench.py --dump-outputs (the arrays of the last timed step as .npy files) and its argument checks, on the host."""
import os
import sys

import numpy as np
import pytest

import bench


def _arrays(scale=1):
    rng = np.random.default_rng(5)
    return {"Ti_pred": rng.standard_normal((2, 1, 4, 4)).astype(np.float32),
            "lm": rng.standard_normal((2, 6)),                                        # float64 stays float64
            "flow_last": rng.standard_normal((2, 2, 96 * scale, 128)).astype(np.float32),
            "weight": rng.random((2, 1, 1, 96 * scale, 128)).astype(np.float32)}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_every_array_whole_when_it_fits(tmp_path):
    a = _arrays()
    info = bench.dump_outputs(a, str(tmp_path / "o"))
    assert sorted(os.listdir(tmp_path / "o")) == sorted(k + ".npy" for k in a)
    for k, v in a.items():
        got = np.load(tmp_path / "o" / (k + ".npy"))
        assert got.dtype == v.dtype and np.array_equal(got, v)
        assert info[k]["sampled"] is None


def test_dump_samples_large_outputs_within_the_limit_and_reproducibly(tmp_path):
    a = _arrays(scale=16)                                   # ~5 MB of arrays against a 2 MB limit
    limit = 2 * 10**6
    i1 = bench.dump_outputs(a, str(tmp_path / "a"), limit=limit)
    i2 = bench.dump_outputs(a, str(tmp_path / "b"), limit=limit)
    assert i1 == i2
    assert _size(tmp_path / "a") <= limit
    for k, v in a.items():
        x, y = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert np.array_equal(x, y)
        if v.nbytes > 2**20:
            assert i1[k]["sampled"] and 0 < x.size < v.size
            assert np.isin(x, v.reshape(-1)).all()          # a sample of the array's own values
        else:
            assert np.array_equal(x, v)


def test_step_outputs_are_float32_or_float64():
    import torch

    class Pose:
        def __init__(self, g):
            self.G = g

    out = {"Ti_pred": Pose(torch.eye(4).reshape(1, 1, 4, 4)), "Tij": Pose(torch.eye(4, dtype=torch.float64).reshape(1, 1, 4, 4)),
           "flow": [torch.zeros(1, 2, 8, 8)], "flow_last": torch.ones(1, 2, 8, 8), "weight": torch.ones(1, 1, 1, 8, 8),
           "vmask": torch.ones(1, 1, 8, 8, dtype=torch.bool), "f16x3_range_events": torch.zeros(1, dtype=torch.int64)}
    got = bench.step_outputs(out)
    assert set(got) == {"Ti_pred", "Tij", "flow_0", "flow_last", "weight", "vmask", "f16x3_range_events"}
    assert {k: str(v.dtype) for k, v in got.items()} == {"Ti_pred": "float32", "Tij": "float64", "flow_0": "float32", "flow_last": "float32",
                                                          "weight": "float32", "vmask": "float32", "f16x3_range_events": "float64"}


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_step_counts_it_cannot_honour(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_steps_argument_is_taken_as_given(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "0", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.dump_outputs) == (3, 0, "d")


def test_bench_leaves_the_cpu_baseline_and_parity_to_full(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "1", "--full"])
    a = bench.parse()
    assert a.full is True and (a.steps, a.warmup) == (3, 1)
