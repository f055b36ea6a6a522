"""TEST INFRASTRUCTURE ONLY -- CPU restatement (float64) of the textured, Phong-shaded render of the reference's DiffRender.render_mesh
(geometry/diff_render_optim.py:201-242: TexturesUV + SoftPhongShader, faces_per_pixel = 1) that MeshRenderer's textured resolve
(csrc/raster.hip, rnnpose_raster_resolve_tex_f32) follows:
  * faces and perspective-correct barycentrics from oracle/raster_oracle.py;
  * TexturesUV.sample_textures: UVs interpolated with those barycentrics, then the real torch.nn.functional.grid_sample on
    flip(map, H) at uv * 2 - 1 (bilinear, align_corners=True, padding_mode="border");
  * phong_shading at PyTorch3D's defaults, shininess 0, a point light at (1,1,-1): (0.5 + 0.3 relu(n.l)) * albedo + 0.2 with
    n = F.normalize(interpolated vertex normals, eps=1e-6) and l = F.normalize(light - p, eps=1e-6); the specular term is the
    constant 0.2 because pow(0, 0) = 1;
  * vertex normals as Meshes.verts_normals_packed: index_add_ of (v2 - v1) x (v0 - v1) per vertex, F.normalize(eps=1e-6).
PARITY UNPINNED against PyTorch3D itself (absent here): this states its documented arithmetic, not its code."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import raster_oracle as ro

LIGHT = (1.0, 1.0, -1.0)


def vertex_normals(verts, faces):
    v = torch.as_tensor(np.asarray(verts, np.float64))
    f = torch.as_tensor(np.asarray(faces, np.int64))
    vf = v[f]
    fn = torch.cross(vf[:, 2] - vf[:, 1], vf[:, 0] - vf[:, 1], dim=1)
    n = torch.zeros_like(v)
    for k in range(3):
        n.index_add_(0, f[:, k], fn)
    return F.normalize(n, eps=1e-6, dim=1).numpy()


def sample_texture(texture, uv):
    """texture (Ht,Wt,3) as loaded (row 0 = top), uv (2,H,W) -> (3,H,W): TexturesUV.sample_textures"""
    m = torch.flip(torch.as_tensor(np.asarray(texture, np.float64)).permute(2, 0, 1)[None], [2])
    g = torch.as_tensor(np.asarray(uv, np.float64)).permute(1, 2, 0)[None] * 2.0 - 1.0
    return F.grid_sample(m, g, mode="bilinear", align_corners=True, padding_mode="border")[0].numpy()


def render(verts, faces, T, K, H, W, colors=None, verts_uvs=None, faces_uvs=None, texture=None, shading="phong"):
    """-> colour (3,H,W) float64 (0 where empty), face index (H,W) (-1 empty), barycentrics (H,W,3)"""
    f, _, w, _ = ro.rasterize(verts, faces, T, K, H, W, perspective=True)
    hit = f >= 0
    if texture is not None:
        alb = sample_texture(texture, ro.interpolate(f, w, faces_uvs, verts_uvs))
    elif colors is not None:
        alb = ro.interpolate(f, w, faces, colors)
    else:
        alb = np.ones((3, H, W))
    if shading is None:
        col = alb
    else:
        p = torch.as_tensor(ro.interpolate(f, w, faces, verts))
        l = F.normalize(torch.tensor(LIGHT, dtype=torch.float64)[:, None, None] - p, eps=1e-6, dim=0)
        if shading == "phong":
            n = F.normalize(torch.as_tensor(ro.interpolate(f, w, faces, vertex_normals(verts, faces))), eps=1e-6, dim=0)
            cos = torch.relu((n * l).sum(0))
        else:                                         # the flat two-sided terms of rnnpose_raster_resolve_f32
            v = np.asarray(verts, np.float64)[np.asarray(faces)[np.clip(f, 0, None)]]          # (H,W,3,3)
            n = torch.as_tensor(np.cross(v[..., 1, :] - v[..., 0, :], v[..., 2, :] - v[..., 0, :])).permute(2, 0, 1)
            cos = ((F.normalize(n, eps=1e-30, dim=0) * l).sum(0)).abs()
        col = (0.5 + 0.3 * cos.numpy()) * alb + 0.2
    return col * hit, f, w
