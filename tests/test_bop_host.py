"""The host side of the BOP metrics (rnnpose_amd/evaluator.py: bop_recalls, BOPAccumulator; eval_epoch.run_epoch(bop_fn=...)) on the
CPU: recalls against hand-computed tables, the epoch with a numpy stand-in for HipEpoch.bop_metrics on one process and on 2 gloo
ranks, and the unchanged call shapes of what was there before."""
import os

import numpy as np
import torch

import bop_ref as br
from rnnpose_amd import eval_epoch as ee
from rnnpose_amd import evaluator as ev
from rnnpose_amd.evaluator import LINEMOD_K
from test_eval_epoch import _halfway, _oracle_metrics, _same, _spawn  # noqa: F401  (helpers only)

N_FRAMES, PER_FRAME, BATCH = 5, 3, 4


def _setup():
    models = ee.synthetic_models(("ape", "cat", "glue"), sub=1)
    models["glue"].symmetries = np.stack([np.eye(4), np.diag([-1.0, -1.0, 1.0, 1.0])]).astype(np.float32)
    items = ee.synthetic_scenes(models, N_FRAMES, PER_FRAME, image_size=(32, 40), seed=5, renderer=None)
    return models, items


def _numpy_bop(models):
    """stand-in for HipEpoch.bop_metrics: MSSD / MSPD of tests/bop_ref.py, and -- no renderer here -- a VSD row made from the MSSD"""
    def fn(batch, poses):
        out = []
        for it, T in zip(batch, np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)):
            m = models[it.class_name]
            sy = np.eye(4, dtype=np.float32)[None] if m.symmetries is None else m.symmetries
            sd = br.sym_dist(m.verts, sy[:, :3], T[None, :3], it.pose_gt[None, :3].astype(np.float32), LINEMOD_K)[0]
            vsd = np.minimum(1.0, sd[0] / m.diameter * np.arange(1, 11))
            out.append(ev.bop_recalls(vsd[None], sd[:1], sd[1:], m.diameter, 640)[0])
        return np.stack(out)
    return fn


def test_recalls_against_hand_computed_tables():
    assert ev.BOP_TAUS == br.TAUS and ev.BOP_THETAS_PX == br.THETAS_PX and ev.BOP_DELTA == br.DELTA
    vsd = np.array([[0.0] * 10, [0.05] * 5 + [0.6] * 5, [np.nan] * 10, [1.0] * 10])
    mssd, mspd, d = np.array([0.0, 0.021, np.nan, 1.0]), np.array([0.0, 12.0, np.nan, 51.0]), np.array([0.1, 0.1, 0.1, 0.2])
    r = ev.bop_recalls(vsd, mssd, mspd, d, 640)
    # row 1: 0.05 is below the 9 thetas above it, strictly, for 5 of 10 taus; 0.021 < 0.025 ... 0.05 (6 of 10); 12 px < 15 ... 50 (8 of 10)
    assert np.allclose(r, [[1.0, 1.0, 1.0], [0.45, 0.6, 0.8], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], rtol=0, atol=1e-15)
    assert np.array_equal(r, br.recalls(vsd, mssd, mspd, d, 640))
    assert ev.bop_recalls(vsd[1:2], mssd[1:2], mspd[1:2], 0.1, 320)[0].tolist() == [0.45, 0.6, 0.6]          # thresholds scale with the width
    assert ev.bop_recalls(vsd[1:2], [0.021], [12.0], 0.1, 640, vsd_thetas=(0.06, 0.7), mssd_thetas=(0.2,), mspd_thetas=(12.0, 12.5))[0].tolist() == \
        [0.75, 0.0, 0.5]
    rng = np.random.default_rng(0)
    vs, ms, mp_, dd = rng.random((7, 10)), rng.random(7) * 0.1, rng.random(7) * 60, 0.1 + rng.random(7) * 0.1
    assert np.array_equal(ev.bop_recalls(vs, ms, mp_, dd, 512), br.recalls(vs, ms, mp_, dd, 512))


def test_accumulator_means_and_duplicates():
    acc = ev.BOPAccumulator(("a", "b", "c"))
    acc.update("a", [1.0, 0.5, 0.0])
    acc.update("a", [0.0, 0.5, 1.0])
    acc.update("b", [0.3, 0.6, 0.9])
    acc.update("b", [9.0, 9.0, 9.0], unique=False)              # a wrap-around duplicate of the sampler: not counted
    r = acc.reduce()
    assert r["a"] == {"ar_vsd": 0.5, "ar_mssd": 0.5, "ar_mspd": 0.5, "ar": 0.5, "n": 2}
    assert r["b"]["n"] == 1 and abs(r["b"]["ar"] - 0.6) < 1e-15 and r["c"]["n"] == 0 and np.isnan(r["c"]["ar"])
    assert r["all"]["n"] == 3 and abs(r["all"]["ar_vsd"] - 1.3 / 3) < 1e-15


def test_epoch_without_bop_fn_is_what_it_was_and_with_it_gains_one_entry():
    models, items = _setup()
    plain = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",), group="frame")
    assert sorted(plain) == ["init", "refined"]
    calls = []
    fn = _numpy_bop(models)

    def bop(batch, poses):
        calls.append(len(batch))
        return fn(batch, poses)
    full = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",), group="frame", bop_fn=bop)
    assert sorted(full) == ["bop", "init", "refined"] and {k: full[k] for k in plain} == plain
    assert calls == [PER_FRAME] * (2 * N_FRAMES)                    # one call per frame batch for the initial and for the refined poses
    b = full["bop"]
    for k in ("init", "refined"):
        assert sorted(b[k]) == ["all", "ape", "cat", "glue"] and b[k]["all"]["n"] == len(items) and b[k]["ape"]["n"] == N_FRAMES
        rows = {c: np.stack([fn([it], (it.pose_init if k == "init" else _halfway(None, [it])[0])[None])[0] for it in items if it.class_name == c])
                for c in models}
        for c in models:
            assert np.allclose([b[k][c]["ar_vsd"], b[k][c]["ar_mssd"], b[k][c]["ar_mspd"]], rows[c].mean(0), rtol=0, atol=1e-12)
            assert abs(b[k][c]["ar"] - rows[c].mean()) < 1e-12
        assert abs(b[k]["all"]["ar"] - np.concatenate(list(rows.values())).mean()) < 1e-12
    assert b["refined"]["all"]["ar_mssd"] >= b["init"]["all"]["ar_mssd"]          # halving the translation error cannot hurt
    by_class = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",), bop_fn=fn)
    _same_bop(by_class["bop"], b, 1e-12)


def _same_bop(a, b, tol=0.0):
    for k in ("init", "refined"):
        assert sorted(a[k]) == sorted(b[k])
        for c in a[k]:
            for name, v in a[k][c].items():
                w = b[k][c][name]
                assert v == w or abs(v - w) <= tol or (np.isnan(v) and np.isnan(w)), (k, c, name, v, w)


def _bop_worker(rank, world, port, q):
    torch.cuda.is_available = lambda: False      # a host rank stays off the GPU
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from rnnpose_amd import distributed as D
    D.init_from_env(backend="gloo")
    models, items = _setup()
    res = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), rank=rank, world=world, batch_size=BATCH, symmetric=("glue",),
                       reduce_device="cpu", group="frame", bop_fn=_numpy_bop(models))
    q.put((rank, res))
    torch.distributed.destroy_process_group()


def test_bop_epoch_on_two_gloo_ranks_equals_a_single_process():
    """15 items over 2 ranks: one wrap-around duplicate, masked in the BOP sums as in the LINEMOD ones."""
    models, items = _setup()
    single = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",), group="frame",
                          bop_fn=_numpy_bop(models))
    outs = _spawn(_bop_worker, world=2)
    _same(outs[0], outs[1])
    _same(outs[0], single, 1e-12)
    _same_bop(outs[0]["bop"], outs[1]["bop"])
    _same_bop(outs[0]["bop"], single["bop"], 1e-12)
    assert single["bop"]["refined"]["all"]["n"] == len(items)


def test_old_positional_constructors_still_work():
    m = ee.ClassModel("ape", np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32), np.zeros((3, 3)), None, None, 0.1, None, None, None, None)
    assert m.texture is None and m.symmetries is None
    it = ee.EvalItem("ape", None, np.eye(3), np.eye(4), np.eye(4), None, 3)
    assert it.frame_id == 3 and it.depth is None
    assert ee.EvalItem("ape", None, None, None, None, None).depth is None
    _, items = _setup()
    assert all(it.depth is None for it in items)                     # no renderer, no observed depth
