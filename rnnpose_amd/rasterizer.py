"""MeshRenderer: a HIP implementation of the call shape PoseRefiner expects from its `renderer`
(`DiffRendererWrapper`, geometry/diff_render_optim.py:404-494), so that the whole render hand-off of an outer refinement
iteration stays on the GPU without PyTorch3D:

    renderer = MeshRenderer({"cat": dict(verts=..., faces=..., colors=...)})
    refiner = PoseRefiner(cfg, renderer=renderer)                 # wrapped by rnnpose_amd.render_adapter.RendererAdapter

    renderer.render_pointcloud(model_names, T=, K=, render_image_size=)          vertex depth splat      (:474-480)
    renderer(model_names, vert_attribute, T=, K=, render_image_size=, near=, far=, render_tex=)           (:482-494, :283-325)
        -> ([shaded colour (3) |] interpolated vertex attributes (C), depth (-1 = empty))
    renderer.render_depth(model_names, T=, K=, render_image_size=, near=, far=)  nearest-vertex depth    (:327-367)

Textured meshes (DiffRender.render_mesh, :104-120 and :201-242: `load_objs_as_meshes` + TexturesUV + SoftPhongShader):

    renderer = MeshRenderer.from_obj({"cat": "models/cat/textured.obj"}, shading="phong")    # DiffRendererWrapper + cls2idx
    renderer = MeshRenderer({"cat": dict(verts=, faces=, verts_uvs=, faces_uvs=, texture=)}, shading="phong")

With render_tex=True the first three channels are then the texture sampled at the interpolated UV (grid_sample semantics of
TexturesUV.sample_textures) and Phong-shaded per pixel with interpolated vertex normals (csrc/raster.hip,
rnnpose_raster_resolve_tex_f32); a batch without a textured mesh under shading="flat" keeps the vertex-colour entry point.

Kernels: csrc/raster.hip (z-buffer by 64-bit atomicMin keys, launched through ops.raster_keys, + ONE per-pixel resolve kernel behind both
resolve entry points -- they differ in the colour of a hit pixel only; _resolve_launch here) and csrc/zoom_crop.hip (vertex splat).
PARITY UNPINNED against PyTorch3D (absent here): semantics documented in include/rnnpose_hip.h, checked against
oracle/raster_oracle.py and by properties in tests/test_raster.py; textures and Phong against tests/texture_ref.py (a CPU
restatement of PyTorch3D's chain on torch's grid_sample).  Mesh files: .obj through rnnpose_amd.mesh_io (no .ply).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops

SHADINGS = ("flat", "phong")


def vertex_normals(verts, faces):
    """PyTorch3D's Meshes.verts_normals_packed on the CPU in fp32: the area-weighted sum of the face normals
    (v2 - v1) x (v0 - v1) at each vertex, normalised with eps 1e-6."""
    v = torch.as_tensor(np.asarray(verts, dtype=np.float32))
    f = torch.as_tensor(np.asarray(faces, dtype=np.int64))
    vf = v[f]
    fn = torch.cross(vf[:, 2] - vf[:, 1], vf[:, 0] - vf[:, 1], dim=1)
    n = torch.zeros_like(v)
    for k in range(3):
        n.index_add_(0, f[:, k], fn)
    return torch.nn.functional.normalize(n, eps=1e-6, dim=1)


class MeshRenderer:
    def __init__(self, meshes: dict, device="cuda", pixel_center: float = 0.5, shade: bool = True,
                 depth_perspective_correct: bool = True, shading: str = "flat"):
        """meshes: {class name: dict(verts (P,3) float, faces (F,3) int, colors (P,3) float in [0,1] or None,
        optional verts_uvs (U,2) float, faces_uvs (F,3) int (uv rows of each face) and texture (Ht,Wt,3) float in [0,1], row 0 =
        the image's top row as read from the file)}.  A class without colours renders white, also next to classes that have them.
        shading: "flat" (the two-sided flat-normal terms) or "phong" (PyTorch3D's phong_shading: interpolated vertex normals,
        one-sided); shade=False renders the albedo unshaded.  Textured meshes and shading="phong" render their colour through
        the textured resolve, where a mesh without a texture has its own vertex colours as albedo, or white without them.
        depth_perspective_correct: barycentrics of render_depth's nearest-vertex choice.  PyTorch3D resolves
        RasterizationSettings.perspective_correct=None to True for the PerspectiveCameras the reference builds
        (geometry/diff_render_optim.py:327-367), so True is the default; False = screen-space barycentrics.
        Faces with a vertex behind `near` are dropped whole (csrc/raster.hip); PyTorch3D clips them at znear / 2 -- objects are
        ~0.5-1 m from the camera in every LINEMOD / LM-O frame, so no face is near the plane."""
        self.depth_perspective_correct = bool(depth_perspective_correct)
        self.device = torch.device(device)
        self.pixel_center = float(pixel_center)
        self.shade = bool(shade)
        if shading not in SHADINGS:
            raise ValueError(f"shading must be one of {SHADINGS}, got {shading!r}")
        self.shading = shading
        self.names = list(meshes)
        vo, fo, verts, faces, cols = {}, {}, [], [], []
        nv = nf = 0
        # one colour table for the plain entry as soon as ANY class has colours, white rows for the classes without (as the textured
        # entry's albedo table, _texture_data): with classes of both kinds the coloured ones came out white
        self.has_colors = any(meshes[n].get("colors") is not None for n in self.names)
        for n in self.names:
            m = meshes[n]
            v = torch.as_tensor(np.asarray(m["verts"], dtype=np.float32))
            f = torch.as_tensor(np.asarray(m["faces"], dtype=np.int32))
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
                raise ValueError(f"mesh {n!r}: verts must be (P,3), faces (F,3)")
            if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
                raise ValueError(f"mesh {n!r}: face indices out of range")
            vo[n], fo[n] = (nv, v.shape[0]), (nf, f.shape[0])
            verts.append(v)
            faces.append(f)
            if self.has_colors:
                c = m.get("colors")
                cols.append(torch.ones(v.shape[0], 3) if c is None else torch.as_tensor(np.asarray(c, dtype=np.float32)).reshape(-1, 3))
                if cols[-1].shape[0] != v.shape[0]:
                    raise ValueError(f"mesh {n!r}: colors must be (P,3) with the P of verts")
            nv += v.shape[0]
            nf += f.shape[0]
        self._vo, self._fo = vo, fo
        self.verts = torch.cat(verts).contiguous().to(self.device)
        self.faces = torch.cat(faces).contiguous().to(self.device)
        self.colors = torch.cat(cols).contiguous().to(self.device) if self.has_colors else None
        self._batches = {}
        self._attr = None                 # set_vertex_attributes(): resident per-class attribute tables
        self._tex = self._texture_data(meshes)

    def _texture_data(self, meshes):
        """Device arrays of the textured resolve, or None when no mesh is textured and shading is "flat"."""
        tex_in = {}
        for n in self.names:
            m = meshes[n]
            uv, fuv, tx = m.get("verts_uvs"), m.get("faces_uvs"), m.get("texture")
            if tx is None:
                continue
            if uv is None or fuv is None:
                raise ValueError(f"mesh {n!r}: a texture needs verts_uvs and faces_uvs")
            uv = np.asarray(uv, dtype=np.float32)
            fuv = np.asarray(fuv, dtype=np.int32)
            tx = np.asarray(tx, dtype=np.float32)
            if uv.ndim != 2 or uv.shape[1] != 2 or fuv.shape != (self._fo[n][1], 3):
                raise ValueError(f"mesh {n!r}: verts_uvs must be (U,2), faces_uvs (F,3) with the F of faces")
            if fuv.size and (int(fuv.min()) < 0 or int(fuv.max()) >= uv.shape[0]):
                raise ValueError(f"mesh {n!r}: faces_uvs indices out of range")
            if tx.ndim != 3 or tx.shape[2] != 3 or tx.shape[0] < 1 or tx.shape[1] < 1:
                raise ValueError(f"mesh {n!r}: texture must be (Ht,Wt,3)")
            tex_in[n] = (uv, fuv, tx)
        self.textured = {n: n in tex_in for n in self.names}
        if not tex_in and self.shading == "flat":
            return None
        d = dict(uv_off={}, tex_off={}, tex_hw={})
        uvs, fuvs, texels, alb = [], [], [], []
        nu = nt = 0
        for n in self.names:
            nv, nf = self._vo[n][1], self._fo[n][1]
            c = meshes[n].get("colors")
            alb.append(np.ones((nv, 3), np.float32) if c is None else np.asarray(c, dtype=np.float32).reshape(-1, 3))
            if alb[-1].shape[0] != nv:
                raise ValueError(f"mesh {n!r}: colors must be (P,3) with the P of verts")
            if n in tex_in:
                uv, fuv, tx = tex_in[n]
                rgba = np.zeros(tx.shape[:2] + (4,), np.float32)
                rgba[..., :3] = tx[::-1]                      # stored flipped: the kernel samples TexturesUV's flip(map, H) directly
                d["uv_off"][n], d["tex_off"][n], d["tex_hw"][n] = nu, nt, tx.shape[:2]
                uvs.append(uv)
                fuvs.append(fuv)
                texels.append(rgba.reshape(-1, 4))
                nu += uv.shape[0]
                nt += rgba.shape[0] * rgba.shape[1]
            else:
                d["uv_off"][n], d["tex_off"][n], d["tex_hw"][n] = 0, 0, (0, 0)
                fuvs.append(np.zeros((nf, 3), np.int32))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate(a))).to(self.device)
        d["albedo"] = dev(alb)
        d["uvs"] = dev(uvs) if tex_in else None
        d["face_uvs"] = dev(fuvs) if tex_in else None
        d["texels"] = dev(texels) if tex_in else None
        d["vnormals"] = None
        if self.shading == "phong":
            d["vnormals"] = torch.cat([vertex_normals(meshes[n]["verts"], meshes[n]["faces"]) for n in self.names]) \
                .contiguous().to(self.device)
        return d

    @classmethod
    def from_obj(cls, paths: dict, device="cuda", shading: str = "phong", **kw):
        """{class name: path of a .obj} -> MeshRenderer (rnnpose_amd.mesh_io.load_obj: UVs and the first material's texture
        map; meshes without one are white).  The drop-in for the reference's DiffRendererWrapper(obj_paths) + cls2idx."""
        from .mesh_io import load_obj
        meshes = {}
        for n, p in paths.items():
            m = load_obj(p)
            meshes[n] = dict(verts=m["verts"], faces=m["faces"], colors=None, verts_uvs=m["verts_uvs"],
                             faces_uvs=m["faces_uvs"], texture=m["texture"])
        return cls(meshes, device=device, shading=shading, **kw)

    def set_vertex_attributes(self, tables: dict):
        """Lay the per-vertex attribute tables {class name: (P, C) or (1, P, C) tensor} out ONCE in one device buffer;
        `renderer(model_names, None, ...)` then renders every image with the table of its class, without the per-call
        concatenation a list of tables costs.  All tables share C and have at least as many rows as their mesh has
        vertices; classes left out keep no table (asking for one raises ValueError).  Replaces earlier tables."""
        rows, off, n, Cc = [], {}, 0, None
        for name, t in tables.items():
            if name not in self._vo:
                raise ValueError(f"set_vertex_attributes: {name!r} is not a mesh of this renderer")
            t = t.reshape(-1, t.shape[-1]) if t.dim() == 3 and t.shape[0] == 1 else t
            if t.dim() != 2:
                raise ValueError(f"set_vertex_attributes: table of {name!r} must be (P, C), got {tuple(t.shape)}")
            if Cc is not None and t.shape[1] != Cc:
                raise ValueError(f"set_vertex_attributes: tables of different C ({Cc} and {t.shape[1]} for {name!r})")
            if t.shape[0] < self._vo[name][1]:
                raise ValueError(f"set_vertex_attributes: {name!r} has {t.shape[0]} rows, its mesh {self._vo[name][1]} vertices")
            Cc = int(t.shape[1])
            off[name] = n
            n += int(t.shape[0]) * Cc
            rows.append(t)
        if not rows:
            raise ValueError("set_vertex_attributes: no table given")
        self._attr = dict(buf=torch.cat([r.to(self.device).float() for r in rows]).contiguous(), off=off, C=Cc)
        for bt in self._batches.values():
            bt.pop("attr_off", None)

    def _resident_attr(self, bt, model_names):
        """(attr, attr_off, C) of a batch rendered from the resident tables; attr_off is cached with the batch."""
        at = self._attr
        if at is None:
            raise ValueError("vert_attribute=None needs resident tables: call set_vertex_attributes() first")
        if "attr_off" not in bt:
            missing = sorted({n for n in model_names if n not in at["off"]})
            if missing:
                raise ValueError(f"no resident attribute table for {missing}")
            bt["attr_off"] = torch.tensor([at["off"][n] for n in model_names], dtype=torch.int64, device=self.device)
        return at["buf"], bt["attr_off"], at["C"]

    def has_vertex_attributes(self, model_names):
        return self._attr is not None and all(n in self._attr["off"] for n in model_names)

    def _batch(self, model_names):
        key = tuple(model_names)
        hit = self._batches.get(key)
        if hit is None:
            i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=self.device)
            hit = dict(vert_off=i32([self._vo[n][0] for n in key]), face_off=i32([self._fo[n][0] for n in key]),
                       face_cnt=i32([self._fo[n][1] for n in key]), max_faces=max(self._fo[n][1] for n in key),
                       nverts=[self._vo[n][1] for n in key],
                       pc_off=i32(np.concatenate([[0], np.cumsum([self._vo[n][1] for n in key])])),
                       same=all(n == key[0] for n in key))
            if self._tex is not None:
                tx = self._tex
                hit.update(uv_off=i32([tx["uv_off"][n] for n in key]), tex_hw=i32([tx["tex_hw"][n] for n in key]),
                           tex_off=torch.tensor([tx["tex_off"][n] for n in key], dtype=torch.int64, device=self.device),
                           any_tex=any(self.textured[n] for n in key))
            if len(self._batches) > 64:
                self._batches.clear()
            self._batches[key] = hit
        return hit

    @staticmethod
    def _tk(T, K):
        T = T.float()
        if T.shape[-2] == 3:
            pad = torch.tensor([0, 0, 0, 1], dtype=T.dtype, device=T.device).expand(T.shape[0], 1, 4)
            T = torch.cat([T, pad], dim=1)
        return T.contiguous(), K.float().contiguous()

    # ---- vertex depth splat ------------------------------------------------------------------------------------------
    def render_pointcloud(self, model_names, T, K, render_image_size, near=0.1, far=6):
        bt = self._batch(model_names)
        T, K = self._tk(T, K)
        verts = torch.cat([self.verts[self._vo[n][0]:self._vo[n][0] + self._vo[n][1]] for n in model_names])
        return ops.pointcloud_depth(verts.contiguous(), bt["pc_off"], T, K, render_image_size)

    # ---- mesh rasteriser ---------------------------------------------------------------------------------------------
    def _raster(self, bt, T, K, size, near, perspective):
        return ops.raster_keys(self.verts, self.faces, bt["vert_off"], bt["face_off"], bt["face_cnt"], bt["max_faces"], T, K, size, near,
                               self.pixel_center, perspective)

    def _resolve_launch(self, entry, bt, T, K, size, near, perspective, ws, attr, attr_off, Cc, nch, want_zbuf, want_vdepth, own):
        """One resolve launch: the outputs allocated, then `entry` with the leading arguments both entries share, its `own` ones
        (colour sources, shade, empty depth) and out / zbuf / vdepth / stream."""
        B, (H, W) = T.shape[0], (int(size[0]), int(size[1]))
        new = lambda c, want: torch.empty(B, c, H, W, device=self.device, dtype=torch.float32) if want else None
        out, zb, vd = new(nch, nch), new(1, want_zbuf), new(1, want_vdepth)
        ops._launch(entry, ops._ptr(self.verts), ops._ptr(self.faces), ops._ptr(bt["vert_off"]), ops._ptr(bt["face_off"]), ops._ptr(T),
                    ops._ptr(K), B, H, W, float(near), self.pixel_center, int(perspective), ops._ptr(ws), ops._ptr(attr),
                    ops._ptr(attr_off), Cc, *own, ops._ptr(out), ops._ptr(zb), ops._ptr(vd), ops._stream())
        return out, zb, vd

    def _resolve(self, bt, T, K, size, near, perspective, ws, attr=None, attr_off=None, Cc=0, with_color=False,
                 want_zbuf=False, want_vdepth=False, empty_depth=-1.0):
        own = (ops._ptr(self.colors) if with_color else C.c_void_p(0), int(with_color), int(self.shade), float(empty_depth))
        return self._resolve_launch("rnnpose_raster_resolve_f32", bt, T, K, size, near, perspective, ws, attr, attr_off, Cc,
                                    (3 if with_color else 0) + Cc, want_zbuf, want_vdepth, own)

    def _resolve_tex(self, bt, T, K, size, near, ws, attr, attr_off, Cc):
        """The textured resolve of __call__(render_tex=True): (B, 3 + Cc, H, W) maps and (B,1,H,W) depth (-1 = empty)."""
        tx = self._tex
        shade = 0 if not self.shade else (2 if self.shading == "phong" else 1)
        own = (ops._ptr(tx["albedo"]), ops._ptr(tx["uvs"]), ops._ptr(tx["face_uvs"]), ops._ptr(bt["uv_off"]), ops._ptr(tx["texels"]),
               ops._ptr(bt["tex_off"]), ops._ptr(bt["tex_hw"]), ops._ptr(tx["vnormals"]), shade, -1.0)
        return self._resolve_launch("rnnpose_raster_resolve_tex_f32", bt, T, K, size, near, 1, ws, attr, attr_off, Cc, 3 + Cc, True, False,
                                    own)[:2]

    def render_depth(self, model_names, T, K, render_image_size, near=0.1, far=6):
        """(B,1,h,w): camera z of the nearest vertex of the visible face, 0 where empty (diff_render_optim.py:327-367)."""
        bt = self._batch(model_names)
        T, K = self._tk(T, K)
        pc = self.depth_perspective_correct
        ws = self._raster(bt, T, K, render_image_size, near, perspective=pc)
        return self._resolve(bt, T, K, render_image_size, near, pc, ws, want_vdepth=True)[2]

    def render_zbuf(self, model_names, T, K, render_image_size, near=0.1, empty_depth=-1.0):
        """(B,1,h,w): the z-buffer depth alone -- the interpolated camera z of the nearest face, the depth channel of __call__ without
        its attribute maps; `empty_depth` (non-positive) where no face covers the pixel.  The depth images of the BOP visible
        surface discrepancy (evaluator.BOPEvaluator)."""
        bt = self._batch(model_names)
        T, K = self._tk(T, K)
        ws = self._raster(bt, T, K, render_image_size, near, perspective=True)
        return self._resolve(bt, T, K, render_image_size, near, True, ws, want_zbuf=True, empty_depth=empty_depth)[1]

    def _explicit_attr(self, bt, vert_attribute, B):
        if isinstance(vert_attribute, (list, tuple)):
            if len(vert_attribute) < B:
                raise ValueError(f"vert_attribute lists {len(vert_attribute)} tables for {B} images")
            rows = [a.float().reshape(-1, a.shape[-1]) for a in vert_attribute]
            Cc = rows[0].shape[1]
            if any(r.shape[1] != Cc for r in rows):
                raise ValueError(f"vert_attribute tables of different C: {sorted({int(r.shape[1]) for r in rows})}")
            attr = torch.cat(rows).contiguous()
            offs = np.concatenate([[0], np.cumsum([r.shape[0] * Cc for r in rows])])[:B]
        else:
            va = vert_attribute.float().contiguous()
            if va.dim() == 2:
                va = va[None]
            Bv, P, Cc = va.shape
            attr = va
            offs = np.array([(b if Bv > 1 else 0) * P * Cc for b in range(B)])
        for b, nverts in enumerate(bt["nverts"]):
            have = (rows[b].shape[0] if isinstance(vert_attribute, (list, tuple)) else attr.shape[1])
            if have < nverts:
                raise ValueError(f"vert_attribute has {have} rows for image {b}, its model has {nverts} vertices")
        return attr, torch.tensor(offs, dtype=torch.int64, device=self.device), Cc

    def __call__(self, model_names, vert_attribute=None, T=None, K=None, render_image_size=None, near=0.1, far=6, render_tex=False):
        """vert_attribute: (B or 1, P, C) per-vertex rows, a list of (P_b, C), or None = the resident table of every image's
        class (set_vertex_attributes) -> (maps (B,[3+]C,h,w), depth (B,1,h,w), -1 = empty)."""
        if T is None or K is None or render_image_size is None:
            raise TypeError("MeshRenderer() needs T, K and render_image_size")
        bt = self._batch(model_names)
        T, K = self._tk(T, K)
        B = T.shape[0]
        if vert_attribute is None:
            attr, attr_off, Cc = self._resident_attr(bt, model_names)
        else:
            attr, attr_off, Cc = self._explicit_attr(bt, vert_attribute, B)
        ws = self._raster(bt, T, K, render_image_size, near, perspective=True)
        if render_tex and self._tex is not None and (bt["any_tex"] or self.shading == "phong"):
            return self._resolve_tex(bt, T, K, render_image_size, near, ws, attr, attr_off, Cc)
        out, zb, _ = self._resolve(bt, T, K, render_image_size, near, True, ws, attr=attr, attr_off=attr_off, Cc=Cc,
                                   with_color=bool(render_tex), want_zbuf=True, empty_depth=-1.0)
        return out, zb

    # ---- occlusion between the objects of one frame ------------------------------------------------------------------
    def occlusion(self, model_names, T, K, render_image_size, pairs, margin=0.0, near=0.1, depth=None, want_occluder=False):
        """Which pixels of every object's own view are hidden by another object of the same frame (csrc/raster.hip,
        rnnpose_raster_occlusion_f32).  T (B,4,4) the poses of ALL objects, K (B,3,3) the (crop) intrinsics of every object's own
        view, pairs an ops.OcclusionPairs of this batch: for pair (b, j) object j is rasterised under T[j] into the window K[b].
        A pixel of b is occluded iff an occluder's depth D there satisfies D + margin < z_own, both from the z-buffer arithmetic of
        __call__ (strict: a coincident surface hides nothing at margin 0).  margin is in the meshes' length unit; 0 is the pure depth
        test, a positive value keeps pixels whose occluder is less than that far in front.
        depth (B,1,h,w) fp32: occluded pixels are zeroed in place, all others stay bit for bit.
        -> visible (B,1,h,w) bool (covered by the object and not occluded) [, occluder (B,1,h,w) int32 batch index, -1 elsewhere].
        Stateless: the own z-buffer is rasterised here (the same launch as __call__'s first pass)."""
        if not isinstance(pairs, ops.OcclusionPairs):
            raise TypeError("pairs must be an ops.OcclusionPairs")
        bt = self._batch(model_names)
        T, K = self._tk(T, K)
        if pairs.B != T.shape[0] or len(model_names) != T.shape[0]:
            raise ValueError(f"{len(model_names)} models, {T.shape[0]} poses, occlusion pairs of {pairs.B} objects")
        if float(margin) != float(margin):
            raise ValueError("occlusion: margin is NaN")
        keys = self._raster(bt, T, K, render_image_size, near, perspective=True)
        vis, occ = ops.raster_occlusion(self.verts, self.faces, bt["vert_off"], bt["face_off"], bt["face_cnt"], bt["max_faces"], T, K,
                                        render_image_size, pairs, margin=margin, near=near, pixel_center=self.pixel_center,
                                        own_keys=keys, depth=depth, want_occluder=want_occluder)
        vis = vis > 0
        return (vis, occ) if want_occluder else vis
