"""The evaluation epoch (rnnpose_amd/eval_epoch.py = tools/eval.py:224-225,305-316,471,516-562 + model/RNNPose.py:157-222 +
utils/eval_metric.py:306-356): rank-strided shards, one-class batches, refinement, per-sample metrics, ONE all_reduce.
CPU tests run the epoch logic with a closed-form 'refiner' and the metric oracle on 1 and on 2 gloo ranks; the GPU test runs
PoseRefiner on the HIP mesh rasteriser with the device evaluator, single process vs two ranks sharing cuda:0."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import eval_oracle as eo
from rnnpose_amd import eval_epoch as ee
from rnnpose_amd.evaluator import LINEMOD_K

N_ITEMS, BATCH = 13, 4          # 13 items over 2 ranks: one wrap-around duplicate; 3 classes -> ragged one-class batches


def _setup():
    models = ee.synthetic_models(("ape", "cat", "glue"), sub=1)
    items = ee.synthetic_dataset(models, N_ITEMS, image_size=(32, 40), seed=5, renderer=None)
    return models, items


def _halfway(cls, batch):
    """closed-form stand-in for the refiner: halves the translation error, keeps the rotation of the initial pose"""
    out = []
    for it in batch:
        T = it.pose_init.copy()
        T[:3, 3] = 0.5 * (it.pose_init[:3, 3] + it.pose_gt[:3, 3])
        out.append(T)
    return np.stack(out)


def _oracle_metrics(models):
    return lambda cls, pred, gt: eo.pose_metrics(models[cls].verts, pred[:, :3], gt[:, :3], LINEMOD_K, cls == "glue")


def test_class_batches_and_duplicate_mask():
    models, items = _setup()
    from rnnpose_amd.distributed import shard_indices
    seen = []
    for r in range(2):
        idx, uq = shard_indices(len(items), r, 2)
        bs = ee.class_batches(items, idx, uq, BATCH)
        for cls, ids, us in bs:
            assert len(ids) <= BATCH and all(items[i].class_name == cls for i in ids)
            seen += [i for i, u in zip(ids, us) if u]
        assert [i for _, ids, _ in bs for i in ids] == idx              # shard order is kept
    assert sorted(seen) == list(range(len(items)))                     # every item exactly once; the duplicate is masked


def test_single_process_epoch_matches_direct_evaluation():
    models, items = _setup()
    res = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",))
    for cls in models:
        sub = [it for it in items if it.class_name == cls]
        gt = np.stack([it.pose_gt for it in sub])
        for key, poses in (("init", np.stack([it.pose_init for it in sub])), ("refined", _halfway(cls, sub))):
            m = eo.pose_metrics(models[cls].verts, poses[:, :3], gt[:, :3], LINEMOD_K, cls == "glue")
            fl = ee.flags_from_metrics(m, models[cls].diameter, cls == "glue")
            assert res[key][cls]["n"] == len(sub)
            for k, name in enumerate(("add", "add2", "add5", "proj2d", "cmd5")):
                assert abs(res[key][cls][name] - fl[:, k].mean()) < 1e-12
    # halving the translation error cannot make ADD worse
    assert all(res["refined"][c]["add"] >= res["init"][c]["add"] for c in models)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cpu_worker(rank, world, port, q):
    torch.cuda.is_available = lambda: False      # a host rank stays off the GPU (init_from_env would bind it to a device on a GPU box)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from rnnpose_amd import distributed as D
    D.init_from_env(backend="gloo")
    models, items = _setup()
    res = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), rank=rank, world=world, batch_size=BATCH, symmetric=("glue",),
                       reduce_device="cpu")
    q.put((rank, res))
    torch.distributed.destroy_process_group()


def _spawn(worker, world=2):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return dict(outs)


def _same(a, b, tol=0.0):
    for key in ("init", "refined"):
        for cls in a[key]:
            for name, v in a[key][cls].items():
                w = b[key][cls][name]
                assert (v == w) or abs(v - w) <= tol or (np.isnan(v) and np.isnan(w)), (key, cls, name, v, w)


def test_two_rank_epoch_equals_single_process():
    models, items = _setup()
    single = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",))
    outs = _spawn(_cpu_worker)
    _same(outs[0], outs[1])                     # every rank holds the reduced result
    _same(outs[0], single, 1e-12)               # and it equals the single-process epoch (wrap-around duplicate masked)
    assert sum(single["refined"][c]["n"] for c in models) == N_ITEMS


def test_eight_rank_epoch_equals_single_process():
    """The driver's scaling run is 8 ranks (one per GPU); no such box is reachable from the build side, so the 8-rank form of the epoch
    -- 13 items over 8 ranks: three wrap-around duplicates, ranks whose shard holds a single class, ragged one-class batches -- runs
    here on gloo.  Every rank must end with the single-process table."""
    models, items = _setup()
    single = ee.run_epoch(items, models, _halfway, _oracle_metrics(models), batch_size=BATCH, symmetric=("glue",))
    outs = _spawn(_cpu_worker, world=8)
    assert sorted(outs) == list(range(8))
    for r in range(1, 8):
        _same(outs[0], outs[r])
    _same(outs[0], single, 1e-12)


# ---- GPU: the real thing ---------------------------------------------------------------------------------------------
def _gpu_epoch(rank, world, reduce_device=None):
    from oracle import rnnpose_oracle as orc
    from rnnpose_amd import synthetic as syn
    from rnnpose_amd.pose_refiner import default_config
    torch.manual_seed(0)
    models = ee.synthetic_models(("ape", "cat", "glue"), sub=3)
    cfg = default_config(RENDER_ITER_COUNT=2, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=(240, 320), zoom_crop_size=(128, 128))
    hip = ee.HipEpoch(models, cfg=cfg)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    hip.refiner.cf_net.update_block.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
    hip.refiner.image_fea_enc.fnet.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
    items = ee.synthetic_dataset(models, 11, image_size=(240, 320), seed=3, renderer=hip.renderer)
    res = ee.run_epoch(items, models, hip.refine, hip.metrics, rank=rank, world=world, batch_size=3, symmetric=("glue",),
                       reduce_device=reduce_device)
    return res, hip, items, models


def _gpu_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from rnnpose_amd import distributed as D
    D.init_from_env(backend="gloo")            # both ranks drive cuda:0 (one GPU on the test box); the reduction itself is the tested path
    res, _, _, _ = _gpu_epoch(rank, world, reduce_device="cpu")
    q.put((rank, res))
    torch.distributed.destroy_process_group()


@pytest.mark.gpu
def test_hip_epoch_single_vs_two_ranks():
    """Synthetic 'dataset' of rendered ellipsoids through PoseRefiner + MeshRenderer + device metrics: the 2-rank epoch (ranks
    share cuda:0, gloo reduction) reproduces the single-process means exactly -- every sample is refined independently of its
    batch neighbours and duplicates are masked -- and the device metrics agree with the CPU oracle."""
    assert torch.cuda.is_available()
    single, hip, items, models = _gpu_epoch(0, 1)
    n = sum(single["refined"][c]["n"] for c in models)
    assert n == 11 and all(np.isfinite(single["refined"][c]["add"]) for c in models if single["refined"][c]["n"])
    # initial-pose statistics need no network: compare them with the CPU oracle directly
    for cls in models:
        sub = [it for it in items if it.class_name == cls]
        m = eo.pose_metrics(models[cls].verts, np.stack([it.pose_init for it in sub])[:, :3], np.stack([it.pose_gt for it in sub])[:, :3],
                            LINEMOD_K, cls == "glue")
        fl = ee.flags_from_metrics(m, models[cls].diameter, cls == "glue")
        for k, name in enumerate(("add", "add2", "add5", "proj2d", "cmd5")):
            assert abs(single["init"][cls][name] - fl[:, k].mean()) < 1e-12
    outs = _spawn(_gpu_worker)
    _same(outs[0], outs[1])
    _same(outs[0], single, 1e-12)
