"""Initial poses from the picture: 2D-3D descriptor matches and P3P RANSAC.

    init = DescriptorPoseInitializer(models, device)                 # models: {class: eval_epoch.ClassModel}
    T0, rec = init(names, geofea_2d, image_index, K, bboxes)         # (B,4,4) and count / n_inliers / final_cost / info / fallback

The descriptor map of a frame (`SuperPoint2D.descriptors`, `EvalItem.geofea_2d`) is matched against the point descriptors of each
object's class (`ClassModel.geofea_3d`) inside the detector's box (`ops.desc_match`), and the matches go through a P3P RANSAC with an
MSAC score and a Gauss-Newton polish on the device (`ops.pnp_ransac`).  Nothing here detects objects: the boxes are an input.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class DescriptorPoseInitializer:
    # `tau` and `min_sim` are STARTING VALUES: no measurement of this project supports them ("not claimed").
    def __init__(self, models, device="cuda", step=2, min_sim=0.5, mutual=True, hypotheses=1024, tau=4.0, n_polish=4, seed=0,
                 pixel_center=0.5, min_count=4, top_k=1, sep_frac=0.1, min_inliers=0, point_subset=None):
        """point_subset: None, or N: the table of a class with more than N vertices holds only its N farthest-point vertices
        (ops.farthest_points from the vertex farthest from the origin, computed once per class) and their descriptors, so the matcher's
        cost no longer grows with the mesh; `point_idx` then indexes that subset and `subset_index[class]` (int64, on the device) maps it
        back to vertex indices (None for a class that kept all its vertices).  Not tuned.
        top_k, sep_frac, min_inliers: `candidates` returns the top_k best DISTINCT hypotheses (ops.pnp_ransac_topk, DESIGN.md section
        22; sep_frac is a starting value like tau); `__call__` does not read them.
        hypotheses: log 0.01 / log(1 - w^3) of them give 99 % confidence at inlier ratio w; 1024 covers w >= 0.17 (not tuned).
        seed: the random words of EVERY call come from a torch.Generator on the device re-seeded with it, so a call is a pure
        function of its inputs."""
        self.models = models
        self.device = torch.device(device)
        self.step, self.min_sim, self.mutual = int(step), float(min_sim), bool(mutual)
        self.hypotheses, self.tau, self.n_polish, self.min_count = int(hypotheses), float(tau), int(n_polish), int(min_count)
        self.seed, self.pixel_center = int(seed), float(pixel_center)
        if self.hypotheses < 1:
            raise ValueError("hypotheses must be >= 1")
        self.top_k, self.sep_frac, self.min_inliers = int(top_k), float(sep_frac), int(min_inliers)
        if not 1 <= self.top_k <= ops.PNP_TOPK_MAX or not 0.0 <= self.sep_frac < float("inf") or self.min_inliers < 0:
            raise ValueError(f"top_k in [1,{ops.PNP_TOPK_MAX}], sep_frac >= 0 and finite, min_inliers >= 0")
        self.point_subset = None if point_subset is None else int(point_subset)
        if self.point_subset is not None and self.point_subset < 4:
            raise ValueError("point_subset must be None or >= 4 (a P3P sample needs three matches and the score a fourth)")
        self.subset_index = {}  # class -> vertex index of every table row (None: the table holds all vertices)
        self._class = {}        # class -> (descriptors (P,32), points (P,3)) on the device
        self._tables = {}       # tuple of names -> (desc3d, points, offsets on the host, offsets on the device)
        self._gen = None

    def _tables_for(self, names):
        key = tuple(names)
        hit = self._tables.get(key)
        if hit is None:
            for n in set(names):
                if n not in self._class:
                    m = self.models[n]
                    d = m.geofea_3d.reshape(-1, m.geofea_3d.shape[-1]).to(self.device, torch.float32).contiguous()
                    p = torch.as_tensor(np.asarray(m.verts, np.float32)).to(self.device)
                    if d.shape != (p.shape[0], ops.DESC_DIM):
                        raise ValueError(f"class {n}: geofea_3d must hold {ops.DESC_DIM} channels for each of the {p.shape[0]} vertices")
                    self.subset_index[n] = None
                    if self.point_subset is not None and p.shape[0] > self.point_subset:
                        keep = ops.farthest_points(p, self.point_subset, None, -1)[0][0]
                        keep = keep[keep >= 0].long()
                        self.subset_index[n] = keep
                        d, p = d[keep].contiguous(), p[keep].contiguous()
                    self._class[n] = (d, p)
            off = [0]
            for n in names:
                off.append(off[-1] + self._class[n][1].shape[0])
            if len(self._tables) >= 8:
                self._tables.pop(next(iter(self._tables)))
            hit = self._tables[key] = (torch.cat([self._class[n][0] for n in names]).contiguous(),
                                       torch.cat([self._class[n][1] for n in names]).contiguous(), off,
                                       torch.tensor(off, dtype=torch.int32, device=self.device))
        return hit

    def random_words(self, B):
        """(B, hypotheses, 3) random 32-bit words (int64 values in [0, 2^32)) of a call with B objects."""
        if self._gen is None:
            self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self.seed)
        return torch.randint(0, 2 ** 32, (B, self.hypotheses, 3), generator=self._gen, device=self.device, dtype=torch.int64)

    def match(self, names, geofea_2d, image_index, bboxes):
        """The matcher alone -> X, x, sim, point_idx, count (ops.desc_match)."""
        desc3d, points, off, off_dev = self._tables_for(names)
        largest = max(b - a for a, b in zip(off, off[1:]))
        if not isinstance(image_index, ops.SourceIndex):
            image_index = ops.SourceIndex(range(len(names)) if image_index is None else image_index, geofea_2d.shape[0], self.device)
        return ops.desc_match(desc3d, points, off_dev, geofea_2d, image_index, bboxes, self.step, self.min_sim, self.mutual, self.pixel_center,
                              max_points=largest)

    def fallback(self, name, K, bbox, size):
        """The box-centre start of an object RANSAC gave no pose for: rotation = identity, t = K^-1 (box centre, 1) z with
        z = f diameter / max(box width, box height), f = (fx + fy) / 2.  The box is clamped to the image; an empty box counts as the
        whole image."""
        H, W = size
        x0, y0, x1, y1 = max(int(bbox[0]), 0), max(int(bbox[1]), 0), min(int(bbox[2]), W - 1), min(int(bbox[3]), H - 1)
        if x1 < x0 or y1 < y0:
            x0, y0, x1, y1 = 0, 0, W - 1, H - 1
        K = np.asarray(K, np.float64)
        z = 0.5 * (K[0, 0] + K[1, 1]) * float(self.models[name].diameter) / max(x1 - x0 + 1, y1 - y0 + 1)
        T = np.eye(4)
        T[:3, 3] = np.linalg.solve(K, np.array([0.5 * (x0 + x1) + self.pixel_center, 0.5 * (y0 + y1) + self.pixel_center, 1.0])) * z
        return T.astype(np.float32)

    def _inputs(self, B, geofea_2d, K, bboxes):
        if B < 1:
            raise ValueError("no objects")
        geofea_2d = ops._chk(geofea_2d, "geofea_2d")
        Kt = torch.as_tensor(np.asarray(K, np.float32)) if not isinstance(K, torch.Tensor) else K
        Kt = Kt.to(self.device, torch.float32)
        if Kt.shape == (3, 3):
            Kt = Kt.expand(B, 3, 3)
        Kt = Kt.contiguous()
        if not isinstance(bboxes, torch.Tensor):
            bboxes = torch.as_tensor(np.asarray(bboxes).astype(np.int32).reshape(B, 4))
        return geofea_2d, Kt, bboxes.to(self.device, torch.int32).contiguous()

    def _record(self, T, valid, names, Kt, bboxes, size, **tensors):
        """The host record of a call: the device `tensors` as numpy arrays, valid = valid(record) (B) or (B,top_k), and fallback (B):
        True where an object has nothing valid.  Those objects get their box-centre start (`fallback`) written into T (B,4,4), a view
        of the poses on the device."""
        rec = {k: t.cpu().numpy() for k, t in tensors.items()}
        rec["valid"] = valid(rec)
        rec["fallback"] = ~rec["valid"].reshape(len(names), -1).any(1)
        if rec["fallback"].any():
            Kh, bh = Kt.cpu().numpy(), bboxes.cpu().numpy()
            rows = np.nonzero(rec["fallback"])[0]
            fb = np.stack([self.fallback(names[j], Kh[j], bh[j], size) for j in rows])
            T[torch.as_tensor(rows, device=self.device)] = torch.as_tensor(fb).to(self.device)
        return rec

    def __call__(self, names, geofea_2d, image_index, K, bboxes):
        """names: B class names; geofea_2d (S,32,H,W) on the device; image_index: B integers (which map every object reads), an
        ops.SourceIndex or None (object b reads map b); K (3,3) or (B,3,3); bboxes (B,4) [xmin, ymin, xmax, ymax] inclusive pixels
        (a device int32 tensor as ops.mask_bbox gives, or host values).
        -> T0 (B,4,4) fp32 on the device and a record of host arrays: count (matches), n_inliers, final_cost, info (0 = RANSAC pose,
        -1 = none) and fallback (True where the box-centre start was taken instead).  Never raises for a pose it cannot find."""
        B = len(names)
        geofea_2d, Kt, bboxes = self._inputs(B, geofea_2d, K, bboxes)
        X, x, _, _, count = self.match(names, geofea_2d, image_index, bboxes)
        T, _, _, _, _, n_inl, fcost, info = ops.pnp_ransac(X, x, count, Kt, self.random_words(B), self.tau, self.n_polish, self.min_count)
        rec = self._record(T, lambda r: r["info"] == 0, names, Kt, bboxes, geofea_2d.shape[-2:], count=count, n_inliers=n_inl, final_cost=fcost, info=info)
        del rec["valid"]                                     # (one slot: fallback says it all)
        return T, rec

    def candidates(self, names, geofea_2d, image_index, K, bboxes):
        """The arguments of `__call__`.  -> T (B,top_k,4,4) fp32 on the device and a record of host arrays: count (B), hyp, n_inliers,
        final_cost, info, dup_of (B,top_k each), n_found (B), valid (B,top_k) = (info == 0) & (dup_of < 0) and fallback (B): True where
        NO slot is valid -- slot 0 then holds the box-centre start of `__call__`.  Every slot that is not valid holds a copy of slot 0's
        pose (of the first valid slot's, should slot 0's own polish have failed), so whatever renders it renders something sane.  Never raises for a pose it cannot find."""
        B = len(names)
        geofea_2d, Kt, bboxes = self._inputs(B, geofea_2d, K, bboxes)
        X, x, _, _, count = self.match(names, geofea_2d, image_index, bboxes)
        T, _, _, hyp, _, n_inl, fcost, info, dup_of, n_found = ops.pnp_ransac_topk(
            X, x, count, Kt, self.random_words(B), self.tau, self.n_polish, self.min_count, self.top_k, self.sep_frac, self.min_inliers)
        rec = self._record(T[:, 0], lambda r: (r["info"] == 0) & (r["dup_of"] < 0), names, Kt, bboxes, geofea_2d.shape[-2:], count=count, hyp=hyp,
                           n_inliers=n_inl, final_cost=fcost, info=info, dup_of=dup_of, n_found=n_found)
        # (the copy comes from the FIRST valid slot: slot 0, unless its own polish failed where a later slot's did not)
        first = torch.as_tensor(rec["valid"].argmax(1)).to(self.device)
        src = T[torch.arange(B, device=self.device), first][:, None]
        T = torch.where(torch.as_tensor(rec["valid"]).to(self.device)[:, :, None, None], T, src).contiguous()
        return T, rec
