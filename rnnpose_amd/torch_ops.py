"""`torch.ops.rnnpose.*`: the SURVEY.md section 8(b) operator set registered with the PyTorch dispatcher on top of the C ABI.

    import rnnpose_amd.torch_ops            # registers the library (idempotent)
    pyr  = torch.ops.rnnpose.corr_pyramid(fmap1, fmap2, 4)        # Tensor[] of (B*N,1,h_l,w_l) levels (one buffer)
    corr = torch.ops.rnnpose.corr_lookup(pyr, coords, 4)           # (B, L*81, h, w)

Schemas are the ones SURVEY 8(b) lists.  Kernels are registered for the CUDA (= HIP on ROCm) dispatch key only: a CPU
tensor fails in the dispatcher ("could not run ... with arguments from the 'CPU' backend") -- there is no CPU product path.
Every op also has a fake (meta) implementation, so FakeTensorMode / torch.compile tracing see correct shapes and dtypes
without touching the GPU.  Inference only: no autograd formulas (tools/eval.py:526 runs under no_grad).

Reference call sites replaced: thirdparty/raft/corr.py:13-57 (CorrBlock), model/CFNet.py:95-106 (upsample_flow),
geometry/transformation.py:184-198,265-316 (SE3.transform, reprojction_optim), model/PoseRefiner.py:342-345 (weight),
geometry/cholesky.py:32-50 + geometry/se3.py:303-306 (solve + increment).
"""
from __future__ import annotations

import torch

from . import ops

_lib = None
_SCHEMAS = {
    "corr_pyramid": "(Tensor fmap1, Tensor fmap2, int levels=4) -> Tensor[]",
    "corr_lookup": "(Tensor[] pyramid, Tensor coords, int radius=4) -> Tensor",
    "convex_upsample": "(Tensor flow, Tensor mask, int scale=8) -> Tensor",
    "induced_flow": "(Tensor depth, Tensor K, Tensor G, float eps=1e-5) -> (Tensor flow, Tensor vmask)",
    "corr_weight": "(Tensor g1, Tensor g2, Tensor target, Tensor depth, Tensor sigma) -> Tensor",
    "lm_normal_eq": "(Tensor target, Tensor weight, Tensor depth, Tensor K, Tensor G) -> (Tensor H, Tensor b)",
    "lm_solve_update": "(Tensor H, Tensor b, Tensor G, float ep_lambda=100.0, float lm_lambda=1e-4, float max_update=1.0) -> (Tensor G_new, Tensor xi)",
    "zoom_crop": "(Tensor x, Tensor theta, int[] crop_size, Tensor? src_index=None) -> Tensor",
    "raster_occlusion": "(Tensor verts, Tensor faces, Tensor vert_off, Tensor face_off, Tensor face_cnt, int max_faces, Tensor T, Tensor K, int[] size, Tensor pair_target, Tensor pair_occluder, float margin=0.0, float near=0.1, float pixel_center=0.5) -> (Tensor visible, Tensor occluder)",
    "bop_sym_dist": "(Tensor model, Tensor sym, Tensor pose_est, Tensor pose_gt, Tensor K) -> Tensor",
    "bop_vsd": "(Tensor depth_est, Tensor depth_gt, Tensor depth_obs, Tensor src_index, Tensor K, Tensor diameter, float delta, float[] taus) -> (Tensor err, Tensor counts)",
    "lm_step": "(Tensor target, Tensor weight, Tensor depth, Tensor K, Tensor G, int num_iters=1, float ep_lambda=100.0, float lm_lambda=1e-4, float max_update=1.0) -> (Tensor G_new, Tensor xi)",
    "lm_step_rgbd": "(Tensor target, Tensor weight, Tensor depth, Tensor K, Tensor G, Tensor obs_depth, Tensor theta, Tensor K_obs, Tensor? src_index=None, float depth_weight=1.0, float depth_gate=0.05, float edge_tol=0.02, int num_iters=1, float ep_lambda=100.0, float lm_lambda=1e-4, float max_update=1.0) -> (Tensor G_new, Tensor xi, Tensor depth_stats)",
    "lm_step_views": "(Tensor target, Tensor weight, Tensor depth, Tensor K, Tensor G, Tensor group_start, Tensor cam_from_rig, int num_iters=1, float ep_lambda=100.0, float lm_lambda=1e-4, float max_update=1.0) -> (Tensor G_new, Tensor xi, Tensor Hg, Tensor bg)",
    "desc_match": "(Tensor desc3d, Tensor points, Tensor pt_off, Tensor desc2d, Tensor src_index, Tensor bbox, int step=2, float min_sim=0.5, bool mutual=True, float pixel_center=0.5, int M=0) -> (Tensor X, Tensor x, Tensor sim, Tensor point_idx, Tensor count)",
    "pnp_ransac": "(Tensor X, Tensor x, Tensor count, Tensor K, Tensor rnd, float tau=4.0, int n_polish=4, int min_count=4) -> (Tensor T, Tensor cost, Tensor inliers, Tensor best, Tensor inlier_mask, Tensor n_inliers, Tensor final_cost, Tensor info)",
    "pnp_ransac_topk": "(Tensor X, Tensor x, Tensor count, Tensor K, Tensor rnd, float tau=4.0, int n_polish=4, int min_count=4, int top_k=4, float sep_frac=0.1, int min_inliers=0) -> (Tensor T, Tensor cost, Tensor inliers, Tensor hyp, Tensor inlier_mask, Tensor n_inliers, Tensor final_cost, Tensor info, Tensor dup_of, Tensor n_found)",
    "pose_score": "(Tensor rend_depth, Tensor rend_desc, Tensor window, Tensor desc2d, Tensor src_index, Tensor? depth_obs=None, float depth_tol=0.015) -> (Tensor stats, Tensor score)",
    "point_diameter": "(Tensor points, Tensor? pt_off=None) -> (Tensor d2, Tensor diameter, Tensor pair, Tensor bounds)",
    "farthest_points": "(Tensor points, int n, Tensor? pt_off=None, Tensor? start=None) -> (Tensor idx, Tensor dist2)",
}


def _level_sizes(h, w, levels):
    return [(h >> l, w >> l) for l in range(levels)]


def _flat_pyramid(pyramid):
    """Tensor[] levels in the reference's shapes -> the flat buffer the lookup kernel reads (level 0 j-patch-major:
    include/rnnpose_hip.h).  The dispatcher-level operators carry the pyramid as the reference does, a list of dense levels, so
    this packs once per call; the refinement path (CorrBlock / the engine) keeps the buffer form and never comes through here."""
    return ops.pyramid_from_levels(list(pyramid))


# ---- CUDA (HIP) implementations ----------------------------------------------------------------------------------------
def _corr_pyramid(fmap1, fmap2, levels=4):
    _, views = ops.corr_pyramid(fmap1, fmap2, levels)
    return list(views)


def _corr_lookup(pyramid, coords, radius=4):
    return ops.corr_lookup(_flat_pyramid(pyramid), coords, len(pyramid), radius)


def _convex_upsample(flow, mask, scale=8):
    return ops.convex_upsample(flow, mask, scale)


def _induced_flow(depth, K, G, eps=1e-5):
    flow, vmask = ops.induced_flow(depth, K, G, eps, want_vmask=True)
    return flow, vmask


def _corr_weight(g1, g2, target, depth, sigma):
    return ops.corr_weight(g1, g2, target, depth, sigma)


def _lm_normal_eq(target, weight, depth, K, G):
    return ops.lm_normal_eq(target, weight, depth, K, G)


def _lm_solve_update(H, b, G, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    Gn, xi, _ = ops.lm_solve_update(H, b, G.reshape(-1, 4, 4), ep_lambda, lm_lambda, max_update)
    return Gn.reshape(G.shape), xi


def _lm_step(target, weight, depth, K, G, num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    Gn, _, _, xi, _ = ops.lm_step(target, weight, depth, K, G, num_iters, ep_lambda, lm_lambda, max_update)
    return Gn.reshape(G.shape), xi


def _lm_step_rgbd(target, weight, depth, K, G, obs_depth, theta, K_obs, src_index=None, depth_weight=1.0, depth_gate=0.05, edge_tol=0.02,
                  num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    """src_index: (B,) integer tensor, checked on the host (ValueError) before anything is launched."""
    Gn, _, _, xi, _, dstats = ops.lm_step_rgbd(target, weight, depth, K, G, obs_depth, theta, K_obs, src_index, depth_weight, depth_gate,
                                               edge_tol, num_iters, ep_lambda, lm_lambda, max_update)
    return Gn.reshape(G.shape), xi, dstats


def _lm_step_views(target, weight, depth, K, G, group_start, cam_from_rig, num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    """group_start: (n_groups + 1,) integer tensor, cam_from_rig (B,4,4): checked on the host (ValueError) before anything is launched.
    The plain sums; the depth-aware grouped step is ops.lm_step_views(..., rgbd=)."""
    if group_start.dim() != 1 or int(group_start[-1]) != depth.shape[0]:
        raise ValueError(f"lm_step_views: group_start must be 1-D and end at the number of views {depth.shape[0]}")
    groups = ops.ViewGroups(group_start, cam_from_rig, depth.shape[0], depth.device)
    Gn, _, _, Hg, bg, xi, _ = ops.lm_step_views(target, weight, depth, K, G, groups, None, num_iters, ep_lambda, lm_lambda, max_update)
    return Gn.reshape(G.shape), xi, Hg, bg


def _zoom_crop(x, theta, crop_size, src_index=None):
    return ops.zoom_crop(x, theta, crop_size, src_index=src_index)


def _raster_occlusion(verts, faces, vert_off, face_off, face_cnt, max_faces, T, K, size, pair_target, pair_occluder, margin=0.0, near=0.1,
                      pixel_center=0.5):
    """pair_target / pair_occluder: (P,) integer tensors, checked on the host (ValueError) before anything is launched."""
    pairs = ops.OcclusionPairs.from_pairs(zip(pair_target.detach().cpu().tolist(), pair_occluder.detach().cpu().tolist()), T.shape[0],
                                          T.device)
    return ops.raster_occlusion(verts, faces, vert_off, face_off, face_cnt, max_faces, T, K, size, pairs, margin=margin, near=near,
                                pixel_center=pixel_center, want_occluder=True)


def _bop_sym_dist(model, sym, pose_est, pose_gt, K):
    return ops.bop_sym_dist(model, sym, pose_est, pose_gt, K)


def _bop_vsd(depth_est, depth_gt, depth_obs, src_index, K, diameter, delta, taus):
    """src_index: (B,) integer tensor, checked on the host (ValueError) before anything is launched."""
    return ops.bop_vsd(depth_est, depth_gt, depth_obs, src_index, K, diameter, delta, taus)


def _desc_match(desc3d, points, pt_off, desc2d, src_index, bbox, step=2, min_sim=0.5, mutual=True, pixel_center=0.5, M=0):
    """pt_off (B+1,) and src_index (B,): integer tensors, checked on the host (ValueError) before anything is launched.  M = 0: the total
    number of points (a capacity no object exceeds, and one the fake kernel knows too)."""
    return ops.desc_match(desc3d, points, pt_off.detach().cpu().tolist(), desc2d, src_index, bbox.to(torch.int32).contiguous(), step, min_sim,
                          mutual, pixel_center, M if M > 0 else points.shape[0])


def _pnp_ransac(X, x, count, K, rnd, tau=4.0, n_polish=4, min_count=4):
    return ops.pnp_ransac(X, x, count.to(torch.int32).contiguous(), K, rnd, tau, n_polish, min_count)


def _pnp_ransac_topk(X, x, count, K, rnd, tau=4.0, n_polish=4, min_count=4, top_k=4, sep_frac=0.1, min_inliers=0):
    return ops.pnp_ransac_topk(X, x, count.to(torch.int32).contiguous(), K, rnd, tau, n_polish, min_count, top_k, sep_frac, min_inliers)


def _pose_score(rend_depth, rend_desc, window, desc2d, src_index, depth_obs=None, depth_tol=0.015):
    """src_index (B,): an integer tensor, checked on the host (ValueError) before anything is launched; window (B,2) any integer dtype."""
    return ops.pose_score(rend_depth, rend_desc, window.to(torch.int32).contiguous(), desc2d, src_index, depth_obs, depth_tol)


def _host_ints(t):
    return None if t is None else t.detach().cpu().tolist()


def _point_diameter(points, pt_off=None):
    """pt_off (B+1,): an integer tensor, checked on the host (ValueError) before anything is launched; None: one object."""
    return ops.point_diameter(points, _host_ints(pt_off))


def _farthest_points(points, n, pt_off=None, start=None):
    """pt_off (B+1,) and start (B,): integer tensors, checked on the host; start None: -1 for every object."""
    return ops.farthest_points(points, n, _host_ints(pt_off), -1 if start is None else _host_ints(start))


# ---- fake (meta) implementations: shapes / dtypes only -----------------------------------------------------------------
def _f_pose_score(rend_depth, rend_desc, window, desc2d, src_index, depth_obs=None, depth_tol=0.015):
    B = rend_desc.shape[0]
    return rend_desc.new_empty((B, len(ops.POSE_SCORE_COLUMNS)), dtype=torch.float64), rend_desc.new_empty((B,), dtype=torch.float64)


def _f_point_diameter(points, pt_off=None):
    B = 1 if pt_off is None else pt_off.shape[0] - 1
    e = lambda shape, dt: points.new_empty(shape, dtype=dt)
    return e((B,), torch.float64), e((B,), torch.float64), e((B, 2), torch.int32), e((B, 2, 3), torch.float32)


def _f_farthest_points(points, n, pt_off=None, start=None):
    B = 1 if pt_off is None else pt_off.shape[0] - 1
    return points.new_empty((B, n), dtype=torch.int32), points.new_empty((B, n), dtype=torch.float64)


def _f_desc_match(desc3d, points, pt_off, desc2d, src_index, bbox, step=2, min_sim=0.5, mutual=True, pixel_center=0.5, M=0):
    B, M = bbox.shape[0], (M if M > 0 else points.shape[0])
    e = lambda shape, dt: desc3d.new_empty(shape, dtype=dt)
    return e((B, M, 3), torch.float32), e((B, M, 2), torch.float32), e((B, M), torch.float32), e((B, M), torch.int32), e((B,), torch.int32)


def _f_pnp_ransac(X, x, count, K, rnd, tau=4.0, n_polish=4, min_count=4):
    B, M, Hyp = X.shape[0], X.shape[1], rnd.shape[1]
    e = lambda shape, dt: X.new_empty(shape, dtype=dt)
    return (e((B, 4, 4), torch.float32), e((B, Hyp), torch.float64), e((B, Hyp), torch.int32), e((B,), torch.int32), e((B, M), torch.uint8),
            e((B,), torch.int32), e((B,), torch.float64), e((B,), torch.int32))


def _f_pnp_ransac_topk(X, x, count, K, rnd, tau=4.0, n_polish=4, min_count=4, top_k=4, sep_frac=0.1, min_inliers=0):
    B, M, Hyp, Kt = X.shape[0], X.shape[1], rnd.shape[1], top_k
    e = lambda shape, dt: X.new_empty(shape, dtype=dt)
    return (e((B, Kt, 4, 4), torch.float32), e((B, Hyp), torch.float64), e((B, Hyp), torch.int32), e((B, Kt), torch.int32),
            e((B, Kt, M), torch.uint8), e((B, Kt), torch.int32), e((B, Kt), torch.float64), e((B, Kt), torch.int32), e((B, Kt), torch.int32),
            e((B,), torch.int32))


def _f_corr_pyramid(fmap1, fmap2, levels=4):
    B, _, h, w = fmap1.shape
    return [fmap1.new_empty((B * h * w, 1, hl, wl), dtype=torch.float32) for hl, wl in _level_sizes(h, w, levels)]


def _f_corr_lookup(pyramid, coords, radius=4):
    B, _, h, w = coords.shape
    return coords.new_empty((B, len(pyramid) * (2 * radius + 1) ** 2, h, w), dtype=torch.float32)


def _f_convex_upsample(flow, mask, scale=8):
    B, _, h, w = flow.shape
    return flow.new_empty((B, 2, scale * h, scale * w), dtype=torch.float32)


def _f_induced_flow(depth, K, G, eps=1e-5):
    B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    return depth.new_empty((B, 2, H, W), dtype=torch.float32), depth.new_empty((B, H, W), dtype=torch.float32)


def _f_corr_weight(g1, g2, target, depth, sigma):
    B, _, H, W = g1.shape
    return g1.new_empty((B, H, W), dtype=torch.float32)


def _f_lm_normal_eq(target, weight, depth, K, G):
    B = depth.shape[0]
    return depth.new_empty((B, 6, 6), dtype=torch.float64), depth.new_empty((B, 6), dtype=torch.float64)


def _f_lm_solve_update(H, b, G, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    return G.new_empty(G.shape, dtype=torch.float32), G.new_empty((H.shape[0], 6), dtype=torch.float32)


def _f_lm_step(target, weight, depth, K, G, num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    return G.new_empty(G.shape, dtype=torch.float32), G.new_empty((depth.shape[0], 6), dtype=torch.float32)


def _f_lm_step_rgbd(target, weight, depth, K, G, obs_depth, theta, K_obs, src_index=None, depth_weight=1.0, depth_gate=0.05, edge_tol=0.02,
                    num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    B = depth.shape[0]
    return G.new_empty(G.shape, dtype=torch.float32), G.new_empty((B, 6), dtype=torch.float32), G.new_empty((B, 2), dtype=torch.float64)


def _f_lm_step_views(target, weight, depth, K, G, group_start, cam_from_rig, num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    ng = group_start.shape[0] - 1
    return (G.new_empty(G.shape, dtype=torch.float32), G.new_empty((ng, 6), dtype=torch.float32), G.new_empty((ng, 6, 6), dtype=torch.float64),
            G.new_empty((ng, 6), dtype=torch.float64))


def _f_zoom_crop(x, theta, crop_size, src_index=None):
    return x.new_empty((theta.shape[0], x.shape[1], int(crop_size[0]), int(crop_size[1])), dtype=torch.float32)


def _f_raster_occlusion(verts, faces, vert_off, face_off, face_cnt, max_faces, T, K, size, pair_target, pair_occluder, margin=0.0, near=0.1,
                        pixel_center=0.5):
    shape = (T.shape[0], 1, int(size[0]), int(size[1]))
    return T.new_empty(shape, dtype=torch.float32), T.new_empty(shape, dtype=torch.int32)


def _f_bop_sym_dist(model, sym, pose_est, pose_gt, K):
    return model.new_empty((pose_est.shape[0], 2), dtype=torch.float64)


def _f_bop_vsd(depth_est, depth_gt, depth_obs, src_index, K, diameter, delta, taus):
    B, NT = depth_est.shape[0], len(taus)
    return depth_est.new_empty((B, NT), dtype=torch.float64), depth_est.new_empty((B, 2 + NT), dtype=torch.int64)


def register():
    """Define the `rnnpose` operator library and attach the HIP kernels (CUDA dispatch key) and fake implementations."""
    global _lib
    if _lib is not None:
        return _lib
    lib = torch.library.Library("rnnpose", "DEF")
    impls = {"corr_pyramid": (_corr_pyramid, _f_corr_pyramid), "corr_lookup": (_corr_lookup, _f_corr_lookup),
             "convex_upsample": (_convex_upsample, _f_convex_upsample), "induced_flow": (_induced_flow, _f_induced_flow),
             "corr_weight": (_corr_weight, _f_corr_weight), "lm_normal_eq": (_lm_normal_eq, _f_lm_normal_eq),
             "lm_solve_update": (_lm_solve_update, _f_lm_solve_update), "lm_step": (_lm_step, _f_lm_step),
             "lm_step_rgbd": (_lm_step_rgbd, _f_lm_step_rgbd), "lm_step_views": (_lm_step_views, _f_lm_step_views),
             "zoom_crop": (_zoom_crop, _f_zoom_crop), "raster_occlusion": (_raster_occlusion, _f_raster_occlusion),
             "bop_sym_dist": (_bop_sym_dist, _f_bop_sym_dist), "bop_vsd": (_bop_vsd, _f_bop_vsd),
             "desc_match": (_desc_match, _f_desc_match), "pnp_ransac": (_pnp_ransac, _f_pnp_ransac),
             "pose_score": (_pose_score, _f_pose_score), "pnp_ransac_topk": (_pnp_ransac_topk, _f_pnp_ransac_topk),
             "point_diameter": (_point_diameter, _f_point_diameter), "farthest_points": (_farthest_points, _f_farthest_points)}
    for name, schema in _SCHEMAS.items():
        lib.define(name + schema)
        real, fake = impls[name]
        lib.impl(name, real, "CUDA")
        torch.library.register_fake("rnnpose::" + name, fake, lib=lib)
    _lib = lib
    return lib


register()
