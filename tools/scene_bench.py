#!/usr/bin/env python3
"""One camera frame with several different objects, refined two ways on the same items (device events, medians after warm-up):

  (a) one B = 1 `HipEpoch.refine` call per object -- what a one-class-per-batch refiner offers: the 2-D descriptor network, a copy of
      the image and of its descriptor map, and a PoseRefiner call at B = 1, once per object;
  (b) one `HipEpoch.refine_frame` call: the descriptor network once, one shared image, one PoseRefiner call at B = objects.

    python tools/scene_bench.py [--objects 8] [--runs 20] [--warmup 3] [--size 480,640] [--out profiles/scene_bench.json]

The two are timed alternately inside every run.  The parts are timed the same way on their own: the descriptor network (per object
/ once), the two zoom crops of the three outer iterations (B = 1 plain launches per object / one indexed launch per map), and the
PoseRefiner call with the descriptors given; "refinement" is that call without its crops.  The frame's image and descriptor map
live on the device throughout (a camera pipeline hands them over there), so no timing contains a host-to-device copy of them.
Objects: ellipsoids of 2562 vertices / 5120 faces with hash-generated 256 + 32 vertex features, 3 x 4 schedule, random weights.

    python tools/scene_bench.py --occlusion [--out profiles/scene_bench_occlusion.json]

measures the occlusion mask between the objects of the frame instead (PoseRefiner(occlusion="frame")): `refine_frame` with and
without the mask, alternating inside every run, on the same frame; and, at the 240 x 240 crops of the initial poses, the occlusion
entry point alone (rnnpose_raster_occlusion_f32, all ordered pairs) next to one own render of the batch (rnnpose_raster_mesh_f32 +
resolve with the resident tables).  Nothing is compared against a threshold.

    python tools/scene_bench.py --bop [--out profiles/scene_bench_bop.json]

times the BOP pose-error functions of the frame at its initial poses: `HipEpoch.bop_metrics` (two z-buffer renders of the batch at the
frame size, rnnpose_bop_vsd_f64, rnnpose_bop_sym_dist_f64 per class, the recalls on the host), `BOPEvaluator.errors` (the same without
the copy back), the two entry points alone on ready depth images, and -- wall clock, on the host -- their numpy restatement
tests/bop_ref.py on the same inputs.  Nothing is compared against a threshold.

    python tools/scene_bench.py --depth [--out profiles/scene_bench_depth.json]

measures the depth term of the LM step (PoseRefiner(depth_term=True)): `refine_frame` without (the parent's
behaviour) and with the term on the frame's observed depth, alternating inside every run; and the step alone at the 240 x 240 crops of the
initial poses -- ops.lm_step against ops.lm_step_rgbd on the same inputs, 50 launches per timed window.  Nothing is compared against a
threshold.

    python tools/scene_bench.py --init [--out profiles/scene_bench_init.json]

times the pose initialiser on the frame, boxes = ops.mask_bbox of every object's depth at its ground-truth pose
padded by 8 px: the matcher alone (ops.desc_match), RANSAC plus polish alone on its matches (ops.pnp_ransac, random words drawn
beforehand), `HipEpoch.initial_poses` (both, the random words, the copy back of the record), `refine_frame` on items without a pose, and
`refine_frame` with the poses given next to it.  The ADD of the initial poses against the ground truth is recorded.  Nothing is compared
against a threshold.

    python tools/scene_bench.py --score [--out profiles/scene_bench_score.json]

times the pose confidence on the frame and its observed depth, at the ground-truth poses: the kernel pair alone
(ops.pose_score on tensors rendered beforehand, with and without the depth), `PoseScorer` as a whole (window, render, kernel pair, record),
`HipEpoch.score_poses`, and `refine_frame` with `score=True` next to the plain one, alternating inside every run.  The scores at the
ground-truth poses, at the initial poses and of the refined poses are recorded.  Nothing is compared against a threshold.

    python tools/scene_bench.py --topk [--out profiles/scene_bench_topk.json]

times the top-K distinct RANSAC hypotheses on the frame, boxes and matches as for --init: ops.pnp_ransac against
ops.pnp_ransac_topk at 1, 4, 8 and 16 slots on the same matches and random words; `initial_poses` with init_candidates 1 and 4; and
`refine_frame` on items without a pose with init_candidates 1, with 4 selected by the score and with 4 selected after refinement -- all
alternating inside every run.  How many objects changed their start through the score is recorded.  Nothing is compared against a
threshold."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rnnpose_amd import eval_epoch as ee, ops  # noqa: E402
from rnnpose_amd.descriptor2d import SuperPoint2D  # noqa: E402
from rnnpose_amd.pose_refiner import default_config  # noqa: E402

NAMES = ("ape", "can", "cat", "driller", "duck", "eggbox", "glue", "holepuncher", "benchvise", "camera", "iron", "lamp", "phone")


def time_alternately(fns, runs, warmup):
    """{name: fn} -> {name: dict(median_ms, min_ms, max_ms)}; every run times each fn once, in turn"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ts.items()}


def occlusion_bench(a, models, cfg, net, hip, items, given, size, cover):
    """--occlusion: refine_frame without (the parent's behaviour) and with the mask; the pass and one own render alone"""
    from rnnpose_amd import zoom
    n, zs = len(items), tuple(cfg.zoom_crop_size)
    hip_on = ee.HipEpoch(models, cfg=cfg, desc2d=net, occlusion="frame")
    hip_on.refiner.load_state_dict(hip.refiner.state_dict())
    whole = time_alternately({"off": lambda: hip.refine_frame(given), "on": lambda: hip_on.refine_frame(given)}, a.runs, a.warmup)
    ren, names = hip_on.renderer, [it.class_name for it in items]
    T0 = torch.as_tensor(np.stack([it.pose_init for it in items]).astype(np.float32)).cuda()
    K = torch.as_tensor(np.stack([it.K for it in items]).astype(np.float32)).cuda()
    pc = ren.render_pointcloud(names, T=T0, K=K, render_image_size=size)
    _, K_crop, _ = zoom.gen_zoom_crop_grids(pc, K, T0, [n, 1, *zs], margin_ratio=0.4, want_grids=False)
    pairs = ops.OcclusionPairs([0] * n, n, "cuda")
    bt = ren._batch(names)
    keys = ren._raster(bt, T0, K_crop, zs, 0.1, perspective=True)
    geom = (ren.verts, ren.faces, bt["vert_off"], bt["face_off"], bt["face_cnt"], bt["max_faces"], T0, K_crop, zs, pairs)
    vis, occ = ops.raster_occlusion(*geom, own_keys=keys)
    own = keys.view(n, -1) != -1
    alone = time_alternately({"occlusion_pass": lambda: ops.raster_occlusion(*geom, own_keys=keys),
                              "own_render": lambda: ren(names, None, T=T0, K=K_crop, render_image_size=zs, render_tex=True)}, a.runs, a.warmup)
    med = lambda r, k: r[k]["median_ms"]
    added = med(whole, "on") - med(whole, "off")
    res = dict(device=torch.cuda.get_device_name(0), objects=n, size=list(size), crop=list(zs), schedule=[cfg.RENDER_ITER_COUNT, cfg.ITER_COUNT],
               verts_per_object=int(next(iter(models.values())).verts.shape[0]), frame_coverage=cover, runs=a.runs, warmup=a.warmup,
               pairs=len(pairs), refine_frame=whole, added_ms=added, added_share=added / med(whole, "off"), alone_at_initial_poses=alone,
               pass_over_own_render=med(alone, "occlusion_pass") / med(alone, "own_render"),
               own_pixels=int(own.sum()), hidden_pixels=int((occ >= 0).sum()), hidden_share_of_own=float((occ >= 0).sum()) / max(1, int(own.sum())),
               note="refine_frame off = the parent's behaviour, timed alternately with on in every run; occlusion_pass = the entry point "
                    "alone (clear + occluder pass + apply) on precomputed own keys; own_render = rnnpose_raster_mesh_f32 + resolve of the "
                    "same batch; nothing is compared against a threshold")
    print(f"refine_frame off {med(whole, 'off'):8.2f} ms   on {med(whole, 'on'):8.2f} ms   added {added:+.3f} ms ({res['added_share']:+.2%})")
    print(f"  at {zs[0]} x {zs[1]}, {len(pairs)} pairs: occlusion pass {med(alone, 'occlusion_pass'):.4f} ms   own render {med(alone, 'own_render'):.4f} ms   "
          f"hidden {res['hidden_pixels']} of {res['own_pixels']} own pixels")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def depth_bench(a, models, cfg, net, hip, items, given, size, cover):
    """--depth: refine_frame without and with the depth term; the LM step alone, plain and depth-aware"""
    from rnnpose_amd import zoom
    n, zs, reps = len(items), tuple(cfg.zoom_crop_size), 50
    depth_dev = items[0].depth.cuda()
    hip_on = ee.HipEpoch(models, cfg=cfg, desc2d=net, depth_term=True)
    hip_on.refiner.load_state_dict(hip.refiner.state_dict())
    with_depth = [ee.EvalItem(it.class_name, it.image, it.K, it.pose_init, it.pose_gt, it.geofea_2d, frame_id=it.frame_id, depth=depth_dev)
                  for it in given]
    whole = time_alternately({"off": lambda: hip.refine_frame(given), "on": lambda: hip_on.refine_frame(with_depth)}, a.runs, a.warmup)
    stats = hip_on.last_depth_stats.cpu()
    # the step alone: the crops of the initial poses, zero flow, weight 1 on the rendered object, one Gauss-Newton step from the identity
    ren, names = hip.renderer, [it.class_name for it in items]
    T0 = torch.as_tensor(np.stack([it.pose_init for it in items]).astype(np.float32)).cuda()
    K = torch.as_tensor(np.stack([it.K for it in items]).astype(np.float32)).cuda()
    pc = ren.render_pointcloud(names, T=T0, K=K, render_image_size=size)
    _, K_crop, theta = zoom.gen_zoom_crop_grids(pc, K, T0, [n, 1, *zs], margin_ratio=0.4, want_grids=False)
    _, syn_depth = ren(names, None, T=T0, K=K_crop, render_image_size=zs, render_tex=True)
    syn_depth = syn_depth.clamp(min=0).contiguous()
    flow = torch.zeros(n, 2, *zs, device="cuda")
    wgt = (syn_depth[:, 0] > 0).float().contiguous()
    G = torch.eye(4, device="cuda").repeat(n, 1, 1)
    obs, idx = depth_dev[None].contiguous(), ops.SourceIndex([0] * n, 1, "cuda")
    plain_out = tuple(torch.empty_like(x) for x in ops.lm_step(flow, wgt, syn_depth, K_crop, G))
    rgbd_out = tuple(torch.empty_like(x) for x in ops.lm_step_rgbd(flow, wgt, syn_depth, K_crop, G, obs, theta, K, idx))

    def plain():
        for _ in range(reps):
            ops.lm_step(flow, wgt, syn_depth, K_crop, G, out=plain_out)

    def rgbd():
        for _ in range(reps):
            ops.lm_step_rgbd(flow, wgt, syn_depth, K_crop, G, obs, theta, K, idx, out=rgbd_out)
    alone = time_alternately({"lm_step": plain, "lm_step_rgbd": rgbd}, a.runs, a.warmup)
    med = lambda r, k: r[k]["median_ms"]
    us = {k: med(alone, k) * 1e3 / reps for k in alone}
    added = med(whole, "on") - med(whole, "off")
    steps = cfg.RENDER_ITER_COUNT * cfg.ITER_COUNT * cfg.OPTIM_ITER_COUNT
    res = dict(device=torch.cuda.get_device_name(0), objects=n, size=list(size), crop=list(zs), schedule=[cfg.RENDER_ITER_COUNT, cfg.ITER_COUNT],
               frame_coverage=cover, runs=a.runs, warmup=a.warmup, depth_term=dict(ops.DEPTH_TERM_DEFAULTS), refine_frame=whole, added_ms=added,
               added_share=added / med(whole, "off"), lm_steps_per_refinement=steps, step_alone=alone, launches_per_window=reps, us_per_step=us,
               step_ratio=us["lm_step_rgbd"] / us["lm_step"], active_pixels_last_step=[float(v) for v in stats[:, 0]],
               depth_cost_last_step=[float(v) for v in stats[:, 1]],
               note="refine_frame off = the parent's behaviour, timed alternately with on in every run; the step alone: back-to-back eager "
                    "launches on one stream (launch overhead included in both), batch = the frame's objects; nothing is compared against a "
                    "threshold")
    print(f"refine_frame off {med(whole, 'off'):8.2f} ms   on {med(whole, 'on'):8.2f} ms   added {added:+.3f} ms ({res['added_share']:+.2%}) over {steps} LM steps")
    print(f"  step alone at B = {n}, {zs[0]} x {zs[1]}: lm_step {us['lm_step']:.1f} us   lm_step_rgbd {us['lm_step_rgbd']:.1f} us   ratio {res['step_ratio']:.2f}")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def views_bench(a, models, cfg, net, size):
    """--views: one frame, 4 objects x 2 cameras (the rig turned by +-10 degrees about the scene centre): refine_frame grouped by
    object_id against the same items ungrouped (the parent's behaviour); the LM step alone at B = 8, 480 x 640 on synthetic inputs
    (every pixel valid): the fused step, its three-launch form and the grouped step in the layouts [2] x 4 and [4] x 2, plain and
    depth-aware.  (grouped - three-launch form + finalize + solve) bounds the tail kernel; nothing is compared against a threshold."""
    import dataclasses
    H, W = size
    hip = ee.HipEpoch(models, cfg=cfg, desc2d=net)
    cams = []
    for deg in (10.0, -10.0):
        E = ee_rot_y(deg)
        c = np.array([0.0, 0.0, 0.83])
        E[:3, 3] = c - E[:3, :3] @ c
        cams.append(E)
    items = ee.synthetic_scenes(models, 1, 4, image_size=(H, W), seed=3, renderer=hip.renderer, cameras=cams)
    dev = {}
    put = lambda t: dev.setdefault(id(t), t.cuda())
    grouped = [dataclasses.replace(it, image=put(it.image), geofea_2d=put(it.geofea_2d), depth=None) for it in items]
    ungrouped = [dataclasses.replace(it, object_id=None, cam_from_rig=None) for it in grouped]
    hip_off = ee.HipEpoch(models, cfg=cfg, desc2d=net)
    hip_off.refiner.load_state_dict(hip.refiner.state_dict())
    whole = time_alternately({"ungrouped": lambda: hip_off.refine_frame(ungrouped), "grouped": lambda: hip.refine_frame(grouped)}, a.runs, a.warmup)
    # the step alone
    B, reps = 8, 50
    depth = torch.ones(B, 1, H, W, device="cuda")
    flow = torch.zeros(B, 2, H, W, device="cuda")
    wgt = torch.ones(B, H, W, device="cuda")
    K = torch.tensor([[572.4, 0, W / 2.0], [0, 573.6, H / 2.0], [0, 0, 1]], device="cuda").repeat(B, 1, 1)
    G = torch.eye(4, device="cuda").repeat(B, 1, 1)
    Ecam = torch.as_tensor(np.stack([cams[v % 2] for v in range(B)]).astype(np.float32))
    theta = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], device="cuda").repeat(B, 1, 1)
    rg = dict(obs_depth=torch.ones(B, H, W, device="cuda"), theta=theta, K_obs=K)
    fns = {}
    outs = {"lm_step": tuple(torch.empty_like(x) for x in ops.lm_step(flow, wgt, depth, K, G)),
            "lm_step_rgbd": tuple(torch.empty_like(x) for x in ops.lm_step_rgbd(flow, wgt, depth, K, G, rg["obs_depth"], theta, K))}

    def loop(fn):
        def run():
            for _ in range(reps):
                fn()
        return run
    fns["lm_step"] = loop(lambda: ops.lm_step(flow, wgt, depth, K, G, out=outs["lm_step"]))
    fns["lm_step_rgbd"] = loop(lambda: ops.lm_step_rgbd(flow, wgt, depth, K, G, rg["obs_depth"], theta, K, out=outs["lm_step_rgbd"]))
    for tag, sizes in (("2x4", [2] * 4), ("4x2", [4] * 2)):
        gr = ops.ViewGroups([0] + list(np.cumsum(sizes)), Ecam, B, "cuda")
        for term, kw in (("plain", {}), ("depth", dict(rgbd=rg))):
            o = tuple(torch.empty_like(x) for x in ops.lm_step_views(flow, wgt, depth, K, G, gr, **kw))
            fns[f"views_{tag}_{term}"] = loop(lambda gr=gr, kw=kw, o=o: ops.lm_step_views(flow, wgt, depth, K, G, gr, out=o, **kw))
    alone = time_alternately(fns, a.runs, a.warmup)
    ops.lm_fused_tail(False)
    try:
        unfused = time_alternately({"lm_step_three_launches": fns["lm_step"], "lm_step_rgbd_three_launches": fns["lm_step_rgbd"]}, a.runs, a.warmup)
    finally:
        ops.lm_fused_tail(True)
    alone.update(unfused)
    med = lambda r, k: r[k]["median_ms"]
    us = {k: med(alone, k) * 1e3 / reps for k in alone}
    res = dict(device=torch.cuda.get_device_name(0), objects=4, cameras=2, size=[H, W], crop=list(cfg.zoom_crop_size),
               schedule=[cfg.RENDER_ITER_COUNT, cfg.ITER_COUNT], runs=a.runs, warmup=a.warmup, refine_frame=whole,
               added_ms=med(whole, "grouped") - med(whole, "ungrouped"), step_alone_B8=alone, launches_per_window=reps, us_per_step=us,
               note="refine_frame ungrouped = the parent's behaviour on the same 8 items, timed alternately with grouped in every run; the "
                    "step alone: back-to-back eager launches on one stream (launch overhead included in all), B = 8 at the frame size")
    print(f"refine_frame ungrouped {med(whole, 'ungrouped'):8.2f} ms   grouped {med(whole, 'grouped'):8.2f} ms   added {res['added_ms']:+.3f} ms")
    for k, v in us.items():
        print(f"  {k:32s} {v:8.1f} us per step")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def ee_rot_y(deg):
    a = np.deg2rad(deg)
    E = np.eye(4)
    E[0, 0], E[0, 2], E[2, 0], E[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return E


def bop_bench(a, models, hip, items, size, cover):
    """--bop: the BOP errors of the frame's objects at their initial poses"""
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bop_ref as br
    H, W = size
    n = len(items)
    depth_dev = items[0].depth.cuda()
    dev_items = [ee.EvalItem(it.class_name, it.image, it.K, it.pose_init, it.pose_gt, None, frame_id=it.frame_id, depth=depth_dev) for it in items]
    names = [it.class_name for it in items]
    init = torch.as_tensor(np.stack([it.pose_init for it in items]).astype(np.float32)).cuda()
    gt = torch.as_tensor(np.stack([it.pose_gt for it in items]).astype(np.float32)).cuda()
    K = torch.as_tensor(np.stack([it.K for it in items]).astype(np.float32)).cuda()
    rec, err = hip.bop_metrics(dev_items, init, want_errors=True)
    ev = hip.bop
    idx = ops.SourceIndex([0] * n, 1, "cuda")
    obs = depth_dev[None].contiguous()
    d_est = ev.renderer.render_zbuf(names, init, K, (H, W))[:, 0].contiguous()
    d_gt = ev.renderer.render_zbuf(names, gt, K, (H, W))[:, 0].contiguous()
    diam = torch.tensor([ev.diameter[c] for c in names], dtype=torch.float32, device="cuda")
    pe, pg = init[:, :3].contiguous(), gt[:, :3].contiguous()

    def sym_all():
        for j, c in enumerate(names):
            ops.bop_sym_dist(ev.points[c], ev.sym[c], pe[j:j + 1], pg[j:j + 1], K[j:j + 1])
    whole = time_alternately({"bop_metrics": lambda: hip.bop_metrics(dev_items, init),
                              "errors_on_device": lambda: ev.errors(names, init, gt, K, obs, src_index=idx),
                              "two_depth_renders": lambda: (ev.renderer.render_zbuf(names, init, K, (H, W)), ev.renderer.render_zbuf(names, gt, K, (H, W))),
                              "vsd_kernels": lambda: ops.bop_vsd(d_est, d_gt, obs, idx, K, diam, ev.delta, ev.taus),
                              "sym_dist_kernels": sym_all}, a.runs, a.warmup)
    h = lambda t: t.detach().cpu().numpy()
    t0 = time.perf_counter()
    werr, wcounts, near = br.vsd(h(d_est), h(d_gt), h(obs), [0] * n, h(K), h(diam), ev.delta, ev.taus)
    t1 = time.perf_counter()
    wsd = np.concatenate([br.sym_dist(h(ev.points[c]), h(ev.sym[c]), h(pe[j:j + 1]), h(pg[j:j + 1]), h(K[j])) for j, c in enumerate(names)])
    t2 = time.perf_counter()
    same = bool(np.array_equal(h(err["counts"]), wcounts)) and bool(np.allclose(np.stack([h(err["mssd"]), h(err["mspd"])], 1), wsd, rtol=1e-6, atol=1e-9))
    med = lambda k: whole[k]["median_ms"]
    res = dict(device=torch.cuda.get_device_name(0), objects=n, size=[H, W], verts_per_object=int(next(iter(models.values())).verts.shape[0]),
               symmetries_per_object=[int(ev.sym[c].shape[0]) for c in names], taus=len(ev.taus), frame_coverage=cover, runs=a.runs, warmup=a.warmup,
               device_ms=whole, numpy_reference_ms=dict(vsd=(t1 - t0) * 1e3, sym_dist=(t2 - t1) * 1e3), equals_reference=same,
               reference_comparisons_near_a_threshold=int(near), mean_recalls=[float(v) for v in rec.mean(0)],
               note="bop_metrics = two z-buffer renders at the frame size + both entry points + recalls on the host (one copy back); the kernels "
                    "alone run on ready depth images; the numpy reference is tests/bop_ref.py, wall clock, one run; nothing is compared "
                    "against a threshold")
    print(f"bop_metrics {med('bop_metrics'):.3f} ms  errors on device {med('errors_on_device'):.3f} ms  renders {med('two_depth_renders'):.3f} ms  "
          f"vsd {med('vsd_kernels'):.4f} ms  sym_dist ({n} calls) {med('sym_dist_kernels'):.4f} ms")
    print(f"  numpy reference: vsd {(t1 - t0) * 1e3:.1f} ms  sym_dist {(t2 - t1) * 1e3:.1f} ms   equal to it: {same}")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def init_bench(a, models, cfg, net, hip, items, given, size, cover):
    """--init: the pose initialiser on the frame's rendered descriptor map"""
    import dataclasses
    H, W = size
    n = len(items)
    hip_i = ee.HipEpoch(models, cfg=cfg, desc2d=net, init="descriptors")
    hip_i.refiner.load_state_dict(hip.refiner.state_dict())
    ini = hip_i.init
    names = [it.class_name for it in items]
    Tg = torch.as_tensor(np.stack([it.pose_gt for it in items]).astype(np.float32)).cuda()
    K = torch.as_tensor(np.stack([it.K for it in items]).astype(np.float32)).cuda()
    boxes_dev = ops.mask_bbox(hip_i.renderer.render_zbuf(names, Tg, K, (H, W)).float().contiguous())
    boxes = boxes_dev.cpu().numpy() + np.array([-8, -8, 8, 8], np.int32)
    boxes_dev = torch.as_tensor(boxes).cuda()
    boxed = [dataclasses.replace(it, bbox=bb) for it, bb in zip(given, boxes)]
    bare = [dataclasses.replace(it, pose_init=None) for it in boxed]
    g2 = given[0].geofea_2d[None].float().contiguous()
    idx = ops.SourceIndex([0] * n, 1, "cuda")
    X, x, sim, pidx, count = ini.match(names, g2, idx, boxes_dev)
    words = ops.random_words(ini.random_words(n))
    T0 = hip_i.initial_poses(bare)
    rec = hip_i.last_init_info
    fed = [dataclasses.replace(it, pose_init=T0[j].cpu().numpy(), bbox=None) for j, it in enumerate(boxed)]
    times = time_alternately({"matcher": lambda: ini.match(names, g2, idx, boxes_dev),
                              "ransac_and_polish": lambda: ops.pnp_ransac(X, x, count, K, words, ini.tau, ini.n_polish, ini.min_count),
                              "initial_poses": lambda: hip_i.initial_poses(bare),
                              "refine_frame_without_poses": lambda: hip_i.refine_frame(bare),
                              "refine_frame_poses_given": lambda: hip_i.refine_frame(fed)}, a.runs, a.warmup)
    add = []
    for j, it in enumerate(items):
        v = models[it.class_name].verts.astype(np.float64)
        T = T0[j].cpu().numpy().astype(np.float64)
        g = np.asarray(it.pose_gt, np.float64)
        add.append(float(np.linalg.norm((v @ T[:3, :3].T + T[:3, 3]) - (v @ g[:3, :3].T + g[:3, 3]), axis=1).mean() / models[it.class_name].diameter))
    area = [int(max(0, min(b[2], W - 1) - max(b[0], 0) + 1) * max(0, min(b[3], H - 1) - max(b[1], 0) + 1)) for b in boxes]
    med = lambda k: times[k]["median_ms"]
    res = dict(device=torch.cuda.get_device_name(0), objects=n, size=[H, W], crop=list(cfg.zoom_crop_size), schedule=[cfg.RENDER_ITER_COUNT, cfg.ITER_COUNT],
               verts_per_object=int(next(iter(models.values())).verts.shape[0]), frame_coverage=cover, runs=a.runs, warmup=a.warmup,
               step=ini.step, min_sim=ini.min_sim, mutual=ini.mutual, hypotheses=ini.hypotheses, tau=ini.tau, n_polish=ini.n_polish,
               box_pixels=area, matches=[int(c) for c in rec["count"]], inliers=[int(c) for c in rec["n_inliers"]], info=[int(c) for c in rec["info"]],
               add_over_diameter=add, device_ms=times,
               note="matcher = ops.desc_match (clear, forward, backward, select: plain fp32 VALU form, the only form built); ransac_and_polish = "
                    "ops.pnp_ransac on the matcher's outputs with the random words drawn beforehand; initial_poses = both + the words + the copy "
                    "back of the record; the descriptor map is RENDERED from the models' own vertex descriptors (no trained weights); boxes = "
                    "mask_bbox of the ground-truth depth + 8 px; nothing is compared against a threshold")
    print(f"matcher {med('matcher'):.3f} ms   RANSAC + polish {med('ransac_and_polish'):.3f} ms   initial_poses {med('initial_poses'):.3f} ms")
    print(f"refine_frame without poses {med('refine_frame_without_poses'):.2f} ms   with poses given {med('refine_frame_poses_given'):.2f} ms")
    print(f"  matches {res['matches']}  inliers {res['inliers']}  ADD / diameter {[round(v, 4) for v in add]}")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def topk_bench(a, models, cfg, net, hip, items, given, size, cover):
    """--topk: the K best distinct RANSAC hypotheses, and the selection among them by the pose score"""
    import dataclasses
    H, W = size
    n = len(items)
    depth_dev = items[0].depth.cuda()

    def epoch(**kw):
        e = ee.HipEpoch(models, cfg=cfg, desc2d=net, init="descriptors", **kw)
        e.refiner.load_state_dict(hip.refiner.state_dict())
        return e
    hip_1, hip_4, hip_r = epoch(), epoch(init_candidates=4), epoch(init_candidates=4, init_select="refined")
    ini = hip_4.init
    names = [it.class_name for it in items]
    Tg = torch.as_tensor(np.stack([it.pose_gt for it in items]).astype(np.float32)).cuda()
    K = torch.as_tensor(np.stack([it.K for it in items]).astype(np.float32)).cuda()
    boxes = ops.mask_bbox(hip_1.renderer.render_zbuf(names, Tg, K, (H, W)).float().contiguous()).cpu().numpy() + np.array([-8, -8, 8, 8], np.int32)
    boxes_dev = torch.as_tensor(boxes).cuda()
    bare = [ee.EvalItem(it.class_name, it.image, it.K, None, it.pose_gt, it.geofea_2d, frame_id=it.frame_id, depth=depth_dev, bbox=bb)
            for it, bb in zip(given, boxes)]
    g2 = given[0].geofea_2d[None].float().contiguous()
    idx = ops.SourceIndex([0] * n, 1, "cuda")
    X, x, sim, pidx, count = ini.match(names, g2, idx, boxes_dev)
    words = ops.random_words(ini.random_words(n))
    topk = lambda k: ops.pnp_ransac_topk(X, x, count, K, words, ini.tau, ini.n_polish, ini.min_count, k, ini.sep_frac, ini.min_inliers)
    T1 = hip_1.initial_poses(bare)
    T4 = hip_4.initial_poses(bare)
    rec = hip_4.last_init_info
    hip_r.refine_frame(bare)
    rec_r = hip_r.last_init_info
    found = {k: [int(v) for v in topk(k)[9].cpu()] for k in (4, 8, 16)}
    fns = {"ransac_and_polish": lambda: ops.pnp_ransac(X, x, count, K, words, ini.tau, ini.n_polish, ini.min_count)}
    for k in (1, 4, 8, 16):
        fns[f"topk_{k}"] = (lambda k: lambda: topk(k))(k)
    fns.update({"initial_poses_1": lambda: hip_1.initial_poses(bare), "initial_poses_4": lambda: hip_4.initial_poses(bare),
                "refine_frame_1": lambda: hip_1.refine_frame(bare), "refine_frame_4_score": lambda: hip_4.refine_frame(bare),
                "refine_frame_4_refined": lambda: hip_r.refine_frame(bare)})
    times = time_alternately(fns, a.runs, a.warmup)

    def add(T):
        out = []
        for j, it in enumerate(items):
            v = models[it.class_name].verts.astype(np.float64)
            t, g = T[j].cpu().numpy().astype(np.float64), np.asarray(it.pose_gt, np.float64)
            out.append(float(np.linalg.norm((v @ t[:3, :3].T + t[:3, 3]) - (v @ g[:3, :3].T + g[:3, 3]), axis=1).mean() / models[it.class_name].diameter))
        return out
    med = lambda k: times[k]["median_ms"]
    res = dict(device=torch.cuda.get_device_name(0), objects=n, size=[H, W], crop=list(cfg.zoom_crop_size), schedule=[cfg.RENDER_ITER_COUNT, cfg.ITER_COUNT],
               verts_per_object=int(next(iter(models.values())).verts.shape[0]), frame_coverage=cover, runs=a.runs, warmup=a.warmup,
               hypotheses=ini.hypotheses, tau=ini.tau, n_polish=ini.n_polish, sep_frac=ini.sep_frac, min_inliers=ini.min_inliers,
               matches=[int(c) for c in rec["count"]], n_found=found, candidate_valid=rec["candidate_valid"].astype(int).tolist(),
               candidate_scores=[[float(v) for v in r] for r in rec["candidate_scores"]], selected_by_score=[int(v) for v in rec["selected"]],
               starts_changed_by_score=int((rec["selected"] != 0).sum()), selected_after_refinement=[int(v) for v in rec_r["selected"]],
               results_changed_by_refined_selection=int((rec_r["selected"] != 0).sum()),
               add_over_diameter_candidates_1=add(T1), add_over_diameter_candidates_4=add(T4), device_ms=times,
               note="ransac_and_polish = ops.pnp_ransac, topk_K = ops.pnp_ransac_topk with K slots, on the same matches and random words drawn "
                    "beforehand; initial_poses_1 / _4 = HipEpoch.initial_poses with init_candidates 1 / 4 (4: candidates + ONE PoseScorer call "
                    "over 4 n poses with the observed depth + the choice on the host); refine_frame_* on items without a pose.  The frame's "
                    "descriptor map is RENDERED from the models' own hash-noise vertex descriptors and the refiner's weights are random numbers: "
                    "the matches have one mode, so this shows the mechanism and its cost and says NOTHING about a trained network; nothing is "
                    "compared against a threshold")
    print("RANSAC + polish %.3f ms   top-K: " % med("ransac_and_polish") + "  ".join(f"K={k} {med(f'topk_{k}'):.3f} ms" for k in (1, 4, 8, 16)))
    print(f"initial_poses: 1 candidate {med('initial_poses_1'):.3f} ms   4 candidates {med('initial_poses_4'):.3f} ms")
    print(f"refine_frame: 1 candidate {med('refine_frame_1'):.2f} ms   4 by score {med('refine_frame_4_score'):.2f} ms   4 refined {med('refine_frame_4_refined'):.2f} ms")
    print(f"  n_found {found}  selected by score {res['selected_by_score']} ({res['starts_changed_by_score']} of {n} starts changed)  after refinement {res['selected_after_refinement']}")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def score_bench(a, models, cfg, net, hip, items, given, size, cover):
    """--score: the pose confidence on the frame, with its observed depth"""
    n = len(items)
    depth_dev = items[0].depth.cuda()
    with_depth = [ee.EvalItem(it.class_name, it.image, it.K, it.pose_init, it.pose_gt, it.geofea_2d, frame_id=it.frame_id, depth=depth_dev)
                  for it in given]
    hip_on = ee.HipEpoch(models, cfg=cfg, desc2d=net, score=True)
    hip_on.refiner.load_state_dict(hip.refiner.state_dict())
    scorer = hip_on.scorer
    names = [it.class_name for it in items]
    Tg = np.stack([it.pose_gt for it in items]).astype(np.float32)
    T0 = np.stack([it.pose_init for it in items]).astype(np.float32)
    K = np.stack([it.K for it in items]).astype(np.float32)
    g2, obs = given[0].geofea_2d[None].float().contiguous(), depth_dev[None].float().contiguous()
    idx = ops.SourceIndex([0] * n, 1, "cuda")
    rd, ra, win, _ = scorer.render(names, Tg, K, size)
    at_gt = hip_on.score_poses(with_depth, Tg)
    rec_gt = hip_on.last_score_info
    at_init = hip_on.score_poses(with_depth, T0)
    rec_init = hip_on.last_score_info
    times = time_alternately({"kernel_pair": lambda: ops.pose_score(rd, ra, win, g2, idx, obs, scorer.depth_tol),
                              "kernel_pair_without_depth": lambda: ops.pose_score(rd, ra, win, g2, idx, None, scorer.depth_tol),
                              "pose_scorer": lambda: scorer(names, Tg, K, g2, idx, obs),
                              "score_poses": lambda: hip_on.score_poses(with_depth, Tg),
                              "refine_frame_score_off": lambda: hip.refine_frame(with_depth),
                              "refine_frame_score_on": lambda: hip_on.refine_frame(with_depth)}, a.runs, a.warmup)
    med = lambda k: times[k]["median_ms"]
    added = med("refine_frame_score_on") - med("refine_frame_score_off")
    lst = lambda v: [float(x) for x in v]
    res = dict(device=torch.cuda.get_device_name(0), objects=n, size=list(size), crop=list(cfg.zoom_crop_size), schedule=[cfg.RENDER_ITER_COUNT, cfg.ITER_COUNT],
               verts_per_object=int(next(iter(models.values())).verts.shape[0]), frame_coverage=cover, runs=a.runs, warmup=a.warmup,
               depth_tol=scorer.depth_tol, window=list(rec_gt["window_size"]), rendered_pixels=[int(v) for v in rec_gt["n_rend"]],
               score_at_gt=lst(at_gt.cpu()), visible_fraction_at_gt=lst(rec_gt["visible_fraction"]), depth_factor_at_gt=lst(rec_gt["depth_factor"]),
               score_at_initial_poses=lst(at_init.cpu()), visible_fraction_at_initial_poses=lst(rec_init["visible_fraction"]),
               depth_factor_at_initial_poses=lst(rec_init["depth_factor"]), score_of_refined_poses=lst(hip_on.last_scores.cpu()),
               device_ms=times, refine_frame_added_ms=added, refine_frame_added_share=added / med("refine_frame_score_off"),
               note="kernel_pair = ops.pose_score (partial sums + final sum) on tensors rendered beforehand; pose_scorer = PoseScorer.__call__: the "
                    "window on the host, one MeshRenderer call (32 descriptor channels + z-buffer), the kernel pair, the copy back of the record; "
                    "score_poses = the same behind HipEpoch (frame maps stacked per call); refine_frame off / on alternate inside every run; the "
                    "frame's descriptor map is RENDERED from the models' own vertex descriptors and the refiner's weights are random numbers, so "
                    "the scores show the mechanism and no accuracy; nothing is compared against a threshold")
    print(f"kernel pair {med('kernel_pair'):.4f} ms (without depth {med('kernel_pair_without_depth'):.4f})   PoseScorer {med('pose_scorer'):.3f} ms   "
          f"score_poses {med('score_poses'):.3f} ms   window {res['window']}")
    print(f"refine_frame score off {med('refine_frame_score_off'):.2f} ms   on {med('refine_frame_score_on'):.2f} ms   added {added:+.3f} ms "
          f"({res['refine_frame_added_share']:+.2%})")
    print(f"  score at gt {[round(v, 3) for v in res['score_at_gt']]}  at the initial poses {[round(v, 3) for v in res['score_at_initial_poses']]}")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="480,640")
    ap.add_argument("--sub", type=int, default=4, help="icosphere subdivisions of the object meshes (4: 2562 vertices)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--occlusion", action="store_true", help="measure the occlusion mask between the objects instead (see above)")
    ap.add_argument("--bop", action="store_true", help="time the BOP pose-error functions of the frame instead (see above)")
    ap.add_argument("--depth", action="store_true", help="measure the depth term of the LM step instead (see above)")
    ap.add_argument("--views", action="store_true", help="measure multi-view refinement instead: 4 objects x 2 cameras, grouped against ungrouped")
    ap.add_argument("--init", action="store_true", help="time the pose initialiser (descriptor matcher + P3P RANSAC) on the frame instead (see above)")
    ap.add_argument("--score", action="store_true", help="time the pose confidence (render-and-compare score) on the frame instead (see above)")
    ap.add_argument("--topk", action="store_true", help="time the top-K distinct RANSAC hypotheses and the selection by the pose score instead (see above)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench measures on the GPU; none is visible")
    H, W = (int(v) for v in a.size.split(","))
    n = a.objects
    torch.manual_seed(0)
    models = ee.synthetic_models(NAMES[:min(n, len(NAMES))], sub=a.sub)
    cfg = default_config(RENDER_ITER_COUNT=3, ITER_COUNT=4, OPTIM_ITER_COUNT=1, render_image_size=(H, W), zoom_crop_size=(240, 240))
    net = SuperPoint2D(dict(input_dim=3, descriptor_dim=32, normalize_output=True, use_instance_norm=True), compute_scores=False).cuda().eval()
    if a.views:
        return views_bench(a, models, cfg, net, (H, W))
    hip = ee.HipEpoch(models, cfg=cfg, desc2d=net)
    items = ee.synthetic_scenes(models, 1, n, image_size=(H, W), seed=3, renderer=hip.renderer)
    image_dev, g2_dev = items[0].image.cuda(), items[0].geofea_2d.cuda()
    mk = lambda it, g2: ee.EvalItem(it.class_name, image_dev, it.K, it.pose_init, it.pose_gt, g2, frame_id=it.frame_id)
    given, bare = [mk(it, g2_dev) for it in items], [mk(it, None) for it in items]
    cover = float((items[0].image.sum(0) > 0).float().mean())
    if a.bop:
        return bop_bench(a, models, hip, items, (H, W), cover)
    if a.occlusion:
        return occlusion_bench(a, models, cfg, net, hip, items, given, (H, W), cover)
    if a.depth:
        return depth_bench(a, models, cfg, net, hip, items, given, (H, W), cover)
    if a.init:
        return init_bench(a, models, cfg, net, hip, items, given, (H, W), cover)
    if a.score:
        return score_bench(a, models, cfg, net, hip, items, given, (H, W), cover)
    if a.topk:
        return topk_bench(a, models, cfg, net, hip, items, given, (H, W), cover)

    per_object = lambda its: [hip.refine(it.class_name, [it]) for it in its]
    whole = time_alternately({"a_per_object": lambda: per_object(bare), "b_frame": lambda: hip.refine_frame(bare)}, a.runs, a.warmup)
    refiner = time_alternately({"a_per_object": lambda: per_object(given), "b_frame": lambda: hip.refine_frame(given)}, a.runs, a.warmup)

    image, g2 = image_dev[None].float().contiguous(), g2_dev[None].float().contiguous()
    desc = time_alternately({"a_per_object": lambda: [net.descriptors(image) for _ in range(n)], "b_frame": lambda: net.descriptors(image)},
                            a.runs, a.warmup)
    u = np.random.default_rng(0).uniform(size=(n, 4)).astype(np.float32)
    theta = torch.zeros(n, 2, 3)
    theta[:, 0, 0] = theta[:, 1, 1] = torch.from_numpy(0.25 + 0.15 * u[:, 0])
    theta[:, 0, 2], theta[:, 1, 2] = torch.from_numpy(u[:, 1] - 0.5), torch.from_numpy(u[:, 2] - 0.5)
    theta = theta.cuda()
    zs, outer = (240, 240), cfg.RENDER_ITER_COUNT
    idx = ops.SourceIndex([0] * n, 1, "cuda")

    def crops_a():          # per object: its own copy of both maps is what (a) crops; the copies themselves are part of (a)'s refine
        for _ in range(outer):
            for b in range(n):
                ops.zoom_crop(image, theta[b:b + 1], zs)
                ops.zoom_crop(g2, theta[b:b + 1], zs)

    def crops_b():
        for _ in range(outer):
            ops.zoom_crop(image, theta, zs, src_index=idx)
            ops.zoom_crop(g2, theta, zs, src_index=idx)
    crops = time_alternately({"a_per_object": crops_a, "b_frame": crops_b}, a.runs, a.warmup)

    med = lambda r, k: r[k]["median_ms"]
    parts = {}
    for k in ("a_per_object", "b_frame"):
        tot = med(whole, k)
        parts[k] = dict(total_ms=tot, superpoint2d_ms=med(desc, k), crops_ms=med(crops, k),
                        refinement_ms=med(refiner, k) - med(crops, k),
                        superpoint2d_share=med(desc, k) / tot, crops_share=med(crops, k) / tot,
                        refinement_share=(med(refiner, k) - med(crops, k)) / tot)
    res = dict(device=torch.cuda.get_device_name(0), objects=n, size=[H, W], crop=list(zs), schedule=[cfg.RENDER_ITER_COUNT, cfg.ITER_COUNT],
               verts_per_object=int(next(iter(models.values())).verts.shape[0]), frame_coverage=cover, runs=a.runs, warmup=a.warmup,
               whole=whole, refiner_call_descriptors_given=refiner, superpoint2d=desc, crops_3_outer_iterations=crops,
               ratio_a_over_b=med(whole, "a_per_object") / med(whole, "b_frame"), parts=parts,
               note="refinement = PoseRefiner call with descriptors given minus the crops timed alone; the parts are timed in "
                    "isolation, so they need not add up to the total exactly")
    print(f"(a) {n} x B=1 refine : {med(whole, 'a_per_object'):8.2f} ms   (b) one refine_frame : {med(whole, 'b_frame'):8.2f} ms   "
          f"ratio {res['ratio_a_over_b']:.2f}")
    for k, p in parts.items():
        print(f"  {k:13s} SuperPoint2D {p['superpoint2d_ms']:7.2f} ms ({p['superpoint2d_share']:.0%})  crops {p['crops_ms']:6.3f} ms "
              f"({p['crops_share']:.1%})  refinement {p['refinement_ms']:7.2f} ms ({p['refinement_share']:.0%})")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
