"""Pose confidence: the render-and-compare score of a pose against its frame.

    scorer = PoseScorer(renderer, models, device)                          # models: {class: eval_epoch.ClassModel}
    score, rec = scorer(names, T, K, geofea_2d, image_index, depth=None)   # (B) fp64 in [0, 1] and the record behind it

Every object's vertex descriptors (`ClassModel.geofea_3d`) and z-buffer are rendered under its pose into a window of the frame -- the
pixel box of its projected vertices -- with the principal point shifted by the window's integer corner, so that window pixels ARE
frame pixels; `ops.pose_score` then compares them with the frame's descriptor map and, where there is one, its observed depth.
Nothing here needs a ground-truth pose.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class PoseScorer:
    # `depth_tol` is a STARTING VALUE: BOP's 15 mm visibility delta written in metres.  No measurement of this project supports it, and no
    # threshold on the score is proposed ("not claimed").
    def __init__(self, renderer, models, device="cuda", depth_tol=0.015, max_window=None, near=0.1):
        """renderer: a rasterizer.MeshRenderer holding the meshes of `models`; depth_tol in the unit of the meshes and of the observed
        depth; max_window: None (each side of the shared window is capped at the frame's size) or an integer / (h, w) cap."""
        self.renderer, self.models = renderer, models
        self.device = torch.device(device)
        self.depth_tol, self.near = float(depth_tol), float(near)
        if isinstance(max_window, (int, np.integer)):
            max_window = (int(max_window), int(max_window))
        self.max_window = None if max_window is None else (int(max_window[0]), int(max_window[1]))
        if self.max_window is not None and min(self.max_window) < 1:
            raise ValueError("max_window must be positive")
        self._verts = {}        # class -> vertices, fp64 on the host (the window is found there)
        self._desc = {}         # class -> (P,32) descriptor table on the device

    def _table(self, name):
        t = self._desc.get(name)
        if t is None:
            m = self.models[name]
            t = m.geofea_3d.reshape(-1, m.geofea_3d.shape[-1]).to(self.device, torch.float32).contiguous()
            if t.shape != (np.asarray(m.verts).shape[0], ops.DESC_DIM):
                raise ValueError(f"class {name}: geofea_3d must hold {ops.DESC_DIM} channels for each of the {np.asarray(m.verts).shape[0]} vertices")
            self._desc[name] = t
            self._verts[name] = np.asarray(m.verts, np.float64)
        return t

    def windows(self, names, T, K, frame_size):
        """-> (h, w), window (B,2) int32 [x0, y0], clipped (B) bool, on the host.  The box of an object is the pixel box of its projected
        vertices (pixel i covers [i, i + 1) whatever the renderer's pixel centre) grown by 1 px, NOT intersected with the frame; (h, w) =
        the largest extents rounded up to a multiple of 8, each side capped; a box the cap cut is centred in its window and `clipped`; an
        object with a vertex behind `near` (or a projection that is not finite) gets the frame's corner -- the whole frame where (h, w)
        allows -- and `clipped`."""
        H, W = int(frame_size[0]), int(frame_size[1])
        cap = (H, W) if self.max_window is None else self.max_window
        B = len(names)
        lo, ext, clipped = np.zeros((B, 2), np.int64), np.zeros((B, 2), np.int64), np.zeros(B, bool)
        for b, n in enumerate(names):
            self._table(n)
            X = self._verts[n] @ T[b, :3, :3].T + T[b, :3, 3]
            with np.errstate(all="ignore"):
                u = K[b, 0, 0] * X[:, 0] / X[:, 2] + K[b, 0, 2]
                v = K[b, 1, 1] * X[:, 1] / X[:, 2] + K[b, 1, 2]
            if not (X[:, 2] > self.near).all() or not (np.isfinite(u).all() and np.isfinite(v).all()) or max(np.abs(u).max(), np.abs(v).max()) > 1e8:
                lo[b], ext[b], clipped[b] = (0, 0), (W, H), True
                continue
            x0, y0 = int(np.floor(u.min())) - 1, int(np.floor(v.min())) - 1
            x1, y1 = int(np.floor(u.max())) + 1, int(np.floor(v.max())) + 1
            lo[b], ext[b] = (x0, y0), (x1 - x0 + 1, y1 - y0 + 1)
        up8 = lambda n: -(-int(n) // 8) * 8
        h, w = min(up8(ext[:, 1].max()), cap[0]), min(up8(ext[:, 0].max()), cap[1])
        window = np.zeros((B, 2), np.int32)
        for b in range(B):
            for a, size in ((0, w), (1, h)):
                if ext[b, a] > size:                         # the cap cut the box: centre the window on it
                    clipped[b] = True
                    window[b, a] = lo[b, a] + (ext[b, a] - size) // 2
                else:
                    window[b, a] = lo[b, a]
        return (h, w), window, clipped

    def render(self, names, T, K, frame_size):
        """-> rend_depth (B,1,h,w), rend_desc (B,32,h,w), window (B,2) int32 on the device, clipped (B) bool on the host: what
        `ops.pose_score` is given.  T (B,4,4), K (B,3,3): tensors or arrays."""
        Th = (T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else np.asarray(T)).astype(np.float64).reshape(-1, 4, 4)
        Kh = (K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)).astype(np.float64)
        B = len(names)
        if B < 1 or Th.shape[0] != B:
            raise ValueError(f"{B} names for {Th.shape[0]} poses")
        Kh = np.broadcast_to(Kh, (B, 3, 3)).copy()
        (h, w), window, clipped = self.windows(names, Th, Kh, frame_size)
        Kw = Kh.copy()
        Kw[:, 0, 2] -= window[:, 0]
        Kw[:, 1, 2] -= window[:, 1]
        tables = [self._table(n) for n in names]
        desc, depth = self.renderer(names, tables, T=torch.as_tensor(Th.astype(np.float32)).to(self.device),
                                    K=torch.as_tensor(Kw.astype(np.float32)).to(self.device), render_image_size=(h, w), near=self.near)
        return depth, desc, torch.as_tensor(window).to(self.device), clipped

    def __call__(self, names, T, K, desc2d, src_index=None, depth=None):
        """names: B class names; T (B,4,4) poses; K (3,3) or (B,3,3); desc2d (S,32,H,W) on the device; src_index: B integers (the frame
        of every pose), an ops.SourceIndex or None (pose b reads frame b); depth (S,H,W) observed depth or None.
        -> score (B) fp64 on the device and a record of host arrays: the ten statistics by name (ops.POSE_SCORE_COLUMNS),
        visible_fraction = n_desc / n_rend (0 for 0), depth_factor, mean_cos, window (B,2), clipped (B) and window_size (h, w)."""
        desc2d = ops._chk(desc2d, "desc2d")
        if depth is not None:
            depth = ops._chk(depth, "depth")
        rend_depth, rend_desc, window, clipped = self.render(names, T, K, desc2d.shape[-2:])
        stats, score = ops.pose_score(rend_depth, rend_desc, window, desc2d, src_index, depth, self.depth_tol)
        st = stats.cpu().numpy()
        rec = {k: st[:, j].copy() for j, k in enumerate(ops.POSE_SCORE_COLUMNS)}
        ratio = lambda a, b, empty: np.divide(a, b, out=np.full_like(a, empty), where=b > 0)
        rec["visible_fraction"] = ratio(rec["n_desc"], rec["n_rend"], 0.0)
        rec["depth_factor"] = ratio(rec["n_cons"], rec["n_cons"] + rec["n_viol"], 1.0)
        rec["mean_cos"] = ratio(rec["sum_cos"], rec["n_desc"], 0.0)
        rec["window"], rec["clipped"], rec["window_size"] = window.cpu().numpy(), clipped, tuple(rend_desc.shape[-2:])
        return score, rec
