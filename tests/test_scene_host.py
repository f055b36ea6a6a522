"""Frame batching of the evaluation epoch (rnnpose_amd/eval_epoch.py: frame_batches, run_epoch(group="frame"), synthetic_scenes) on
the CPU: the epoch logic with a closed-form 'refiner' and the metric oracle, single process and on 2 and 3 gloo ranks."""
import os

import numpy as np
import pytest
import torch

from oracle import eval_oracle as eo
from rnnpose_amd import eval_epoch as ee
from rnnpose_amd.distributed import shard_indices
from rnnpose_amd.evaluator import LINEMOD_K
from test_eval_epoch import _free_port, _halfway, _same, _spawn  # noqa: F401  (helpers only)

N_FRAMES, PER_FRAME, BATCH = 5, 3, 4


def _setup():
    models = ee.synthetic_models(("ape", "cat", "glue"), sub=1)
    items = ee.synthetic_scenes(models, N_FRAMES, PER_FRAME, image_size=(32, 40), seed=5, renderer=None)
    return models, items


def _oracle_metrics(models):
    return lambda cls, pred, gt: eo.pose_metrics(models[cls].verts, pred[:, :3], gt[:, :3], LINEMOD_K, cls == "glue")


def test_synthetic_scenes_share_the_frame_tensors():
    models, items = _setup()
    assert len(items) == N_FRAMES * PER_FRAME and [it.frame_id for it in items] == [f for f in range(N_FRAMES) for _ in range(PER_FRAME)]
    for f in range(N_FRAMES):
        frame = items[f * PER_FRAME:(f + 1) * PER_FRAME]
        assert len({it.class_name for it in frame}) == PER_FRAME                      # different classes in one frame
        assert all(it.image is frame[0].image and it.geofea_2d is frame[0].geofea_2d for it in frame)
        t = np.stack([it.pose_gt[:3, 3] for it in frame])
        px = np.stack([(it.K @ it.pose_gt[:3, 3])[:2] / it.pose_gt[2, 3] for it in frame])
        assert (px >= 0).all() and (px[:, 0] < 40).all() and (px[:, 1] < 32).all()    # inside the 32 x 40 image
        gaps = np.abs(px[:, None] - px[None]).max(-1)[~np.eye(PER_FRAME, dtype=bool)]
        assert gaps.min() > 0.25 * 32 / 2                                             # separated: 2 x 2 cells, jitter of a tenth of a cell
        assert len({round(float(z), 4) for z in t[:, 2]}) == PER_FRAME                # and at different depths
    assert ee.EvalItem("ape", None, None, None, None, None).frame_id is None         # trailing field with a default


def test_frame_batches_grouping_overflow_none_ids_and_order():
    models, items = _setup()
    idx, uq = shard_indices(len(items), 0, 1)
    bs = ee.frame_batches(items, idx, uq, BATCH)
    assert [ids for _, ids, _ in bs] == [list(range(3 * f, 3 * f + 3)) for f in range(N_FRAMES)] and all(c is None for c, _, _ in bs)
    # a frame with more objects than batch_size is split into two batches
    bs = ee.frame_batches(items, idx, uq, 2)
    assert [ids for _, ids, _ in bs][:4] == [[0, 1], [2], [3, 4], [5]]
    # items without a frame id fall back to class_batches order; a frame is never merged with them
    loose = ee.synthetic_dataset(models, 5, image_size=(32, 40), seed=5, renderer=None)
    mixed = items[:3] + loose + items[3:6]
    idx, uq = shard_indices(len(mixed), 0, 1)
    bs = ee.frame_batches(mixed, idx, uq, BATCH)
    assert bs[0][0] is None and bs[0][1] == [0, 1, 2] and bs[-1][0] is None and bs[-1][1] == [8, 9, 10]
    assert [(c, ids) for c, ids, _ in bs[1:-1]] == [(c, [i + 3 for i in ids]) for c, ids, _ in
                                                    ee.class_batches(loose, list(range(5)), [True] * 5, BATCH)]
    # shard order kept and wrap-around duplicates still flagged, on 2 and 4 ranks
    for world in (2, 4):
        seen = []
        for r in range(world):
            idx, uq = shard_indices(len(items), r, world)
            bs = ee.frame_batches(items, idx, uq, BATCH)
            assert [i for _, ids, _ in bs for i in ids] == idx
            for _, ids, us in bs:
                assert len(ids) <= BATCH and len({items[i].frame_id for i in ids}) == 1
                seen += [i for i, u in zip(ids, us) if u]
        assert sorted(seen) == list(range(len(items)))


def test_frame_epoch_equals_class_epoch_single_process():
    models, items = _setup()
    calls = []

    def refine(cls, batch):
        calls.append((cls, [it.class_name for it in batch]))
        return _halfway(cls, batch)
    by_class = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",))
    by_frame = ee.run_epoch(items, models, refine, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",), group="frame")
    _same(by_frame, by_class, 1e-12)
    assert len(calls) == N_FRAMES and all(c is None and len(set(names)) == PER_FRAME for c, names in calls)
    assert sum(by_frame["refined"][c]["n"] for c in models) == len(items)
    with pytest.raises(ValueError):
        ee.run_epoch(items, models, _halfway, _oracle_metrics(models), group="scene")


def _frame_worker(rank, world, port, q):
    torch.cuda.is_available = lambda: False      # a host rank stays off the GPU
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from rnnpose_amd import distributed as D
    D.init_from_env(backend="gloo")
    models, items = _setup()
    res = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), rank=rank, world=world, batch_size=BATCH, symmetric=("glue",),
                       reduce_device="cpu", group="frame")
    q.put((rank, res))
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_frame_epoch_on_gloo_ranks_equals_the_class_epoch(world):
    """15 items over 2 ranks (one wrap-around duplicate) and over 3: every rank ends with the same table, and it is the
    single-process class-batched table."""
    models, items = _setup()
    single = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",))
    outs = _spawn(_frame_worker, world=world)
    for r in range(1, world):
        _same(outs[0], outs[r])
    _same(outs[0], single, 1e-12)
    assert sum(outs[0]["refined"][c]["n"] for c in models) == len(items)
