#!/usr/bin/env python3
"""Object onboarding wall time, device events, medians of 20 runs after 3 warm-ups, one process:

  * ops.point_diameter at P = 5 000 / 20 000 / 100 000 against the CPU route a user has today, numpy brute force in fp64 (row blocks;
    timed up to 20 000 points);
  * ops.farthest_points at the same P with n = 64 / 1024 / 3000 against the fp64 restatement of the reference's fragmentation_fps
    (tests/model_prep_ref.py) -- the CPU side is timed once per shape (torch.set_num_threads(16) / at most 16 threads);
  * model_prep.build_class_model end to end on a 20 000-vertex synthetic mesh (both KPConv networks, 3000 evaluation points);
  * the matcher of tools/scene_bench.py --init (8 objects, 480 x 640, 2562 vertices each) with and without point_subset=1024.

    python tools/model_bench.py [--runs 20] [--warmup 3] [--out profiles/model_prep_bench.json] [--quick]

Nothing is compared against a threshold; the tool is not part of any gate."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import desc3d_fp64 as R  # noqa: E402
import model_prep_ref as mr  # noqa: E402
from rnnpose_amd import eval_epoch as ee, model_prep, ops  # noqa: E402
from rnnpose_amd.descriptor3d import KPSuperpoint3Dv2  # noqa: E402
from rnnpose_amd.pose_init import DescriptorPoseInitializer  # noqa: E402
from rnnpose_amd.rasterizer import MeshRenderer  # noqa: E402

NAMES = ("ape", "can", "cat", "driller", "duck", "eggbox", "glue", "holepuncher")


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(e))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def cpu_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def numpy_diameter(p32, block=256):
    """fp64 brute force in row blocks (a P x P matrix of 100 000 points does not fit)"""
    p = p32.astype(np.float64)
    best = 0.0
    for a in range(0, len(p), block):
        d = p[a:a + block, None, :] - p[None, a:, :]
        best = max(best, float(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max()))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="P = 5000 only and no CPU side at n = 3000")
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev), "runs": a.runs, "warmup": a.warmup, "diameter": [], "fps": []}
    for P in ((5000,) if a.quick else (5000, 20000, 100000)):
        p32 = (np.random.default_rng(P).standard_normal((P, 3)) * np.array([0.06, 0.045, 0.035])).astype(np.float32)
        pts = torch.from_numpy(p32).to(dev)
        row = {"points": P, "hip": timed(lambda: ops.point_diameter(pts), a.runs, a.warmup)}
        got = float(ops.point_diameter(pts)[0][0])
        if P <= 20000:                                     # (at 100 000 points the numpy route takes many minutes: not timed)
            want = []
            row["numpy_fp64_ms"] = cpu_ms(lambda: want.append(numpy_diameter(p32)))
            row["equal"] = got == want[0]
            row["speedup"] = row["numpy_fp64_ms"] / row["hip"]["median_ms"]
        res["diameter"].append(row)
        print(json.dumps(row), flush=True)
        for n in (64, 1024, 3000):
            frow = {"points": P, "n": n, "hip": timed(lambda: ops.farthest_points(pts, n), a.runs, a.warmup)}
            if not (a.quick and n == 3000):
                ref = []
                frow["numpy_fp64_ms"] = cpu_ms(lambda: ref.append(mr.fps(p32, n)))
                idx, d2 = ops.farthest_points(pts, n)
                frow["equal"] = bool(np.array_equal(idx[0].cpu().numpy(), ref[0][0]) and np.array_equal(d2[0].cpu().numpy(), ref[0][1]))
                frow["speedup"] = frow["numpy_fp64_ms"] / frow["hip"]["median_ms"]
            res["fps"].append(frow)
            print(json.dumps(frow), flush=True)

    # build_class_model end to end: a 20 000-vertex ellipsoid cloud with a token face list (the builder does not walk the faces)
    nets = {}
    for name, cfg in (("desc", R.DESC), ("ctx", R.CTX)):
        net = KPSuperpoint3Dv2(dict(cfg))
        w = R.make_weights({k: tuple(v.shape) for k, v in net.state_dict().items()}, cfg, R.SEEDS[name])
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()})
        nets[name] = net.to(dev).eval()
    cloud = R.ellipsoid_cloud("model_bench", 5000 if a.quick else 20000, axes=(0.5, 0.4, 0.3)).astype(np.float32)
    mesh = dict(verts=cloud, faces=np.array([[0, 1, 2]], np.int32))
    with torch.no_grad():
        build = lambda: model_prep.build_class_model("bench", mesh, nets["desc"], nets["ctx"], [40, 40, 40, 40], n_eval_points=3000)
        res["build_class_model"] = dict(vertices=len(cloud), n_eval_points=3000, **timed(build, a.runs, a.warmup))
        bare = lambda: model_prep.build_class_model("bench", mesh, n_eval_points=3000)
        res["build_class_model_without_networks"] = dict(vertices=len(cloud), n_eval_points=3000, **timed(bare, a.runs, a.warmup))
    print(json.dumps({k: res[k] for k in ("build_class_model", "build_class_model_without_networks")}), flush=True)

    # the matcher on the frame of tools/scene_bench.py --init
    H, W = 480, 640
    models = ee.synthetic_models(NAMES, sub=4)
    renderer = MeshRenderer({n: dict(verts=m.verts, faces=m.faces, colors=m.colors) for n, m in models.items()}, device="cuda")
    items = ee.synthetic_scenes(models, 1, len(NAMES), image_size=(H, W), seed=3, renderer=renderer)
    names = [it.class_name for it in items]
    Tg = torch.as_tensor(np.stack([it.pose_gt for it in items]).astype(np.float32)).cuda()
    K = torch.as_tensor(np.stack([it.K for it in items]).astype(np.float32)).cuda()
    boxes = ops.mask_bbox(renderer.render_zbuf(names, Tg, K, (H, W)).float().contiguous()).cpu().numpy() + np.array([-8, -8, 8, 8], np.int32)
    boxes_dev = torch.as_tensor(boxes).cuda()
    g2 = items[0].geofea_2d.cuda()[None].float().contiguous()
    idx = ops.SourceIndex([0] * len(names), 1, "cuda")
    full, sub = DescriptorPoseInitializer(models, "cuda"), DescriptorPoseInitializer(models, "cuda", point_subset=1024)
    cf, cs = full.match(names, g2, idx, boxes_dev)[4], sub.match(names, g2, idx, boxes_dev)[4]
    res["matcher"] = dict(objects=len(names), size=[H, W], verts_per_object=int(models[names[0]].verts.shape[0]), point_subset=1024,
                          all_vertices=timed(lambda: full.match(names, g2, idx, boxes_dev), a.runs, a.warmup),
                          subset=timed(lambda: sub.match(names, g2, idx, boxes_dev), a.runs, a.warmup),
                          matches_all_vertices=cf.cpu().tolist(), matches_subset=cs.cpu().tolist())
    print(json.dumps(res["matcher"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
