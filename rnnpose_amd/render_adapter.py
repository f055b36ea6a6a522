"""Render hand-off of every outer refinement iteration (model/PoseRefiner.py:246-304) and checkpoint loading
(tools/eval.py:386-413) -- the two pieces of glue that make `PoseRefiner(cfg, renderer=diff_renderer)` and a reference
`.tckpt` usable with this package unchanged.

RendererAdapter turns ANY object with the call shape of the reference's `DiffRendererWrapper`
(geometry/diff_render_optim.py:404-494)

    renderer.render_pointcloud(model_names, T=, K=, render_image_size=)                       -> (B,1,H,W) vertex depth splat
    renderer(model_names, vert_attribute, T=, K=, render_image_size=, near=, far=, render_tex=True)
                                                                                              -> (B,3+C,h,w) colour|features, (B,1,h,w) depth (-1 = empty)
    renderer.render_depth(model_names, T=, K=, render_image_size=, near=, far=)               -> (B,1,h,w)

into the `render_views` protocol of rnnpose_amd.PoseRefiner.  The zoom window is computed on the device
(csrc/zoom_crop.hip: mask bounding box -> affine -> cropped intrinsics -> fused affine_grid+grid_sample); the reference
does the same arithmetic on the host behind two device->host synchronisations per outer iteration
(model/PoseRefiner.py:154,213).  `rnnpose_amd.rasterizer.MeshRenderer` is a HIP implementation of that call shape; the
reference's PyTorch3D renderer plugs in the same way.
"""
from __future__ import annotations

import re

import torch

from . import zoom


class RendererAdapter:
    def __init__(self, renderer, render_image_size=(480, 640), zoom_crop_size=(240, 240), legacy=True, margin_ratio=0.4,
                 near=0.1, far=6, occlusion=None, occlusion_margin=0.0):
        """render_image_size / zoom_crop_size: `BASIC.render_image_size` / `BASIC.zoom_crop_size` of the reference config
        (config/default.py:48-49, config/linemod/template_fw0.5.yml:14-15).
        occlusion: None (default: every object is refined against its own render alone) or "frame": after the render of every outer
        iteration, `renderer.occlusion` finds the pixels of each object's synthetic view that ANOTHER object of the same frame (same
        image_index entry), under its current pose estimate, is in front of, and `syn_depth` is zeroed there -- on the legacy
        nearest-vertex path and on the z-buffer path alike.  Validity in the refinement loop is `syn_depth > 0`, so those pixels drop
        out of the descriptor weight, the induced flow and the LM normal equations.  The rendered maps (syn_img, cfea, geofea1) are
        NOT touched: the encoder still sees the whole object; only validity changes.  The views gain `occlusion_visible`
        (B,1,h,w) bool and `occluder` (B,1,h,w) int32 (batch index of the nearest occluder, -1 elsewhere).
        occlusion_margin: in the meshes' length unit; a pixel is hidden iff an occluder's depth D there has D + margin < own depth.
        0 (default) is the pure depth test; no value has been tuned against a dataset."""
        for name in ("render_pointcloud", "render_depth"):
            if not callable(getattr(renderer, name, None)):
                raise TypeError(f"renderer must provide {name}() (geometry/diff_render_optim.py:404-494)")
        if not callable(renderer):
            raise TypeError("renderer must be callable: renderer(model_names, vert_attribute, T=, K=, render_image_size=, ...)")
        self.renderer = renderer
        self.render_image_size = tuple(int(v) for v in render_image_size)
        self.zoom_crop_size = tuple(int(v) for v in zoom_crop_size)
        self.legacy = legacy
        self.margin_ratio = float(margin_ratio)
        self.near, self.far = near, far
        if occlusion not in (None, "frame"):
            raise ValueError(f'occlusion must be None or "frame", got {occlusion!r}')
        self.occlusion = occlusion
        self.occlusion_margin = float(occlusion_margin)

    def prepare_inputs(self, B, obj_cls=None, image=None, fea_3d=None, geofea_3d=None, geofea_2d=None, image_index=None):
        """Host-side checks of one PoseRefiner.forward() call, before anything is launched (ValueError on a batch the
        render hand-off cannot serve) -> the ops.SourceIndex of a batch that shares source images, or None.
        image (S,3,H,W) / geofea_2d (S,32,H,W): S == B without image_index (crop b reads image b), else image_index (B,)
        names the source of every object, 0 <= image_index[b] < S.  fea_3d / geofea_3d: one tensor for the whole batch, a
        list of B per-image (P_b, C) tables, or None when the renderer holds a resident table for every class of obj_cls."""
        from . import ops
        r = self.renderer
        if self.occlusion is not None and not callable(getattr(r, "occlusion", None)):
            raise ValueError('occlusion="frame" needs a renderer with an occlusion() method (rnnpose_amd.rasterizer.MeshRenderer)')
        names = getattr(r, "names", None)
        if names is not None and obj_cls is not None:
            unknown = sorted({str(n) for n in obj_cls if n not in names})
            if unknown:
                raise ValueError(f"unknown object class {unknown}: the renderer holds {sorted(names)}")
        if obj_cls is not None and len(obj_cls) != B:
            raise ValueError(f"obj_cls names {len(obj_cls)} objects, the poses {B}")
        for name, t in (("fea_3d", fea_3d), ("geofea_3d", geofea_3d)):
            if isinstance(t, (list, tuple)):
                if len(t) != B:
                    raise ValueError(f"{name} lists {len(t)} tables for {B} objects")
                if len({int(a.shape[-1]) for a in t}) != 1:
                    raise ValueError(f"{name}: tables of different C {sorted({int(a.shape[-1]) for a in t})}")
        if fea_3d is None:
            if geofea_3d is not None:
                raise ValueError("geofea_3d without fea_3d: pass both, or neither to render from the resident tables")
            has = getattr(r, "has_vertex_attributes", None)
            if has is None or obj_cls is None or not has(obj_cls):
                raise ValueError("fea_3d=None needs a renderer with a resident attribute table for every class of obj_cls "
                                 "(MeshRenderer.set_vertex_attributes)")
        S = None
        for name, t in (("image", image), ("geofea_2d", geofea_2d)):
            if t is None:
                continue
            if S is not None and t.shape[0] != S:
                raise ValueError(f"image holds {S} sources, geofea_2d {t.shape[0]}")
            S = int(t.shape[0])
        if image_index is None:
            if S is not None and S != B:
                raise ValueError(f"{S} source images for {B} objects need image_index (which source each object crops from)")
            return None
        if S is None:
            raise ValueError("image_index without an image")
        if isinstance(image_index, ops.SourceIndex):
            idx = image_index
            if idx.S != S:
                raise ValueError(f"image_index was built for {idx.S} sources, image holds {S}")
        else:
            idx = ops.SourceIndex(image_index, S, image.device)
        if len(idx) != B:
            raise ValueError(f"image_index names {len(idx)} objects, the poses {B}")
        return idx

    @staticmethod
    def _per_image(t, b):
        """Table b of a per-batch attribute argument: a list entry, row b of (B,P,C), or the one shared (1,P,C) / (P,C) table."""
        if isinstance(t, (list, tuple)):
            return t[b].reshape(-1, t[b].shape[-1])
        return t.reshape(-1, t.shape[-1]) if t.dim() == 2 or t.shape[0] == 1 else t[b]

    @torch.no_grad()
    def render_views(self, Ti, intrinsics, obj_cls=None, image=None, fea_3d=None, geofea_3d=None, geofea_2d=None,
                     image_index=None, occlusion_pairs=None):
        """Ti (B,4,4) current absolute pose, intrinsics (B,3,3) of the full image -> views dict of one outer iteration.
        image_index (ops.SourceIndex or B integers; see prepare_inputs): object b crops image / geofea_2d [image_index[b]].
        occlusion_pairs (occlusion="frame"): the ops.OcclusionPairs of this batch (PoseRefiner builds them once per forward); None:
        built here from image_index.  The occluders' poses are the rows of Ti, the current estimates of the whole batch."""
        r, zs = self.renderer, self.zoom_crop_size
        pc_depth = r.render_pointcloud(obj_cls, T=Ti, K=intrinsics, render_image_size=self.render_image_size)       # :253-254
        B = pc_depth.shape[0]
        # foreground mask = pc_depth > 0 (:259); window, grids and cropped intrinsics on the device (:145-218)
        _, K_crop, theta = zoom.gen_zoom_crop_grids(pc_depth, intrinsics, Ti, [B, 1, *zs], margin_ratio=self.margin_ratio,
                                                    want_grids=False)
        lists = isinstance(fea_3d, (list, tuple)) or isinstance(geofea_3d, (list, tuple))
        if fea_3d is None:                       # resident tables of the renderer: [context | descriptor] channels per class
            fea_cat, c3, cg = None, None, (geofea_2d.shape[1] if geofea_2d is not None else 0)
        elif lists:                              # one (P_b, C) table per image: a mixed-class batch
            c3 = self._per_image(fea_3d, 0).shape[-1]
            cg = self._per_image(geofea_3d, 0).shape[-1] if geofea_3d is not None else 0
            fea_cat = [self._per_image(fea_3d, b) if geofea_3d is None else
                       torch.cat([self._per_image(fea_3d, b), self._per_image(geofea_3d, b)], dim=-1) for b in range(B)]
        else:
            c3, cg = fea_3d.shape[-1], (geofea_3d.shape[-1] if geofea_3d is not None else 0)
            fea_cat = torch.cat([fea_3d, geofea_3d], dim=-1) if geofea_3d is not None else fea_3d                    # :269-272
        color, depth = r(obj_cls, fea_cat, T=Ti, K=K_crop, render_image_size=zs, near=self.near, far=self.far,
                         render_tex=True)                                                                            # :135-137
        depth = depth.detach().masked_fill(depth == -1, 0.0)                                                         # :139 (no host sync)
        if c3 is None:
            c3 = color.shape[1] - 3 - cg
        if cg:
            syn_img, cfea, geofea1 = torch.split(color, [3, c3, cg], dim=1)                                          # :277
        else:
            syn_img, cfea = torch.split(color, [3, c3], dim=1)
            geofea1 = None
        cfea = (cfea * 0.1).contiguous()                                                                             # :283
        # image_index: the objects of one frame crop ONE copy of its image / descriptor map (csrc/zoom_crop.hip, indexed kernel)
        image_crop = zoom.zoom_crop(image, theta, zs, src_index=image_index)                                         # :287
        geofea2_crop = None
        if geofea1 is not None and geofea_2d is not None:
            geofea1 = geofea1.contiguous()
            geofea2_crop = zoom.zoom_crop(geofea_2d, theta, zs, src_index=image_index)                               # :291
        syn_depth = depth
        if self.legacy:                                                                                              # :295-304
            syn_depth = r.render_depth(obj_cls, T=Ti, K=K_crop, render_image_size=zs, near=self.near, far=self.far)
        extra = {}
        if self.occlusion == "frame":
            extra = self._occlude(Ti, K_crop, obj_cls, image_index, occlusion_pairs, syn_depth)
            syn_depth = extra.pop("syn_depth")
        return dict(syn_img=syn_img.contiguous(), image_crop=image_crop, cfea=cfea, geofea1=geofea1,
                    geofea2_crop=geofea2_crop, syn_depth=syn_depth.contiguous(), intrinsics_crop=K_crop,
                    fmap1=None, fmap2=None, theta=theta, pc_depth=pc_depth, **extra)

    def _occlude(self, Ti, K_crop, obj_cls, image_index, pairs, syn_depth):
        """occlusion="frame": zero the pixels of syn_depth another object of the frame hides -> syn_depth, occlusion_visible, occluder.
        A batch without pairs (no image_index: one image per object) launches nothing: every covered pixel is visible."""
        from . import ops
        B = Ti.shape[0]
        if pairs is None:
            pairs = ops.OcclusionPairs(image_index, B, Ti.device)
        if len(pairs) == 0:
            return dict(syn_depth=syn_depth, occlusion_visible=syn_depth > 0,
                        occluder=torch.full(syn_depth.shape, -1, dtype=torch.int32, device=syn_depth.device))
        syn_depth = syn_depth.float().contiguous()
        vis, occ = self.renderer.occlusion(obj_cls, T=Ti, K=K_crop, render_image_size=self.zoom_crop_size, pairs=pairs,
                                           margin=self.occlusion_margin, near=self.near, depth=syn_depth, want_occluder=True)
        return dict(syn_depth=syn_depth, occlusion_visible=vis, occluder=occ)


def filter_param_dict(state_dict, include=None, exclude=None):
    """tools/eval.py:110-127: keep keys matching `include` (re.match) and not matching `exclude`."""
    inc = re.compile(include) if include is not None else None
    exc = re.compile(exclude) if exclude is not None else None
    return {k: p for k, p in state_dict.items()
            if (inc is None or inc.match(k) is not None) and (exc is None or exc.match(k) is None)}


def load_motion_net_checkpoint(refiner, checkpoint, prefix="motion_net.", include=None, exclude=None, strict=False):
    """Load the `motion_net.*` sub-tree of a reference checkpoint (`.tckpt` = torch.save(RNNPose.state_dict()),
    torchplus/train/checkpoint.py:92) into a rnnpose_amd.PoseRefiner, with the selection rule of tools/eval.py:386-413:
    include/exclude regular expressions on the FULL key, then only keys that exist in the model with the same shape
    are taken; the others are reported.  -> (loaded_keys, skipped_keys).  `checkpoint`: path or state dict."""
    sd = torch.load(checkpoint, map_location="cpu") if isinstance(checkpoint, (str, bytes)) or hasattr(checkpoint, "__fspath__") else checkpoint
    sd = filter_param_dict(dict(sd), include, exclude)
    model = refiner.state_dict()
    loaded, skipped = {}, []
    for k, v in sd.items():
        if not k.startswith(prefix):
            continue
        kk = k[len(prefix):]
        if kk in model and tuple(v.shape) == tuple(model[kk].shape):
            loaded[kk] = v
        else:
            skipped.append(k)
    missing = [k for k in model if k not in loaded]
    if strict and (missing or skipped):
        raise RuntimeError(f"checkpoint does not cover the model: missing {missing[:5]}..., skipped {skipped[:5]}...")
    model.update(loaded)
    refiner.load_state_dict(model)
    return sorted(loaded), skipped
