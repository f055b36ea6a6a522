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
PARITY UNPINNED against PyTorch3D itself (absent here): this states its documented arithmetic, not its code; its own arithmetic is
pinned by tests/test_texture_ref.py (hand-written bilinear taps, analytic normals).

`color_at` is the colour at explicit (face, barycentrics) pairs -- `render` is that at the oracle's winners -- so that the candidate
faces of an uncertain pixel (tests/raster_ref.py) can be checked like its depth.  `color_bound` is the per-pixel acceptance bound of
tests/test_gpu_texture_edges.py, derived in its docstring from the fp32 input error of the weights and the kernel's roundings."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import raster_oracle as ro

LIGHT = (1.0, 1.0, -1.0)
EPS = 2.0 ** -24                       # unit round-off of fp32 (tests/raster_ref.py)
MARGIN4 = 4.0                          # the project's margin on a counted number of roundings (raster_ref.MARGIN = 4 x 8)
K_IX = 8                               # roundings behind ix / iy, in units of EPS * (size - 1): see color_bound
K_ALB, K_NRM, K_LGT, K_DOT, K_FIN = 8, 21, 11, 5, 4       # roundings of the rest, see color_bound


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


def _unit(x, eps):
    """x (N,3) -> x / max(|x|, eps) (F.normalize), |x|"""
    n = np.sqrt((x * x).sum(1))
    return x / np.maximum(n, eps)[:, None], n


def color_at(mesh, face, w, shading="phong", detail=False):
    """The fp64 colour of mesh = dict(verts, faces[, colors, verts_uvs, faces_uvs, texture]) at N surface points given as face index
    (N,) and barycentrics (N,3) (any real weights: points beyond an edge continue the face's plane and its UV map).
    Albedo: the texture at the interpolated UV, else the interpolated vertex colours, else white.  shading None | "flat" (two-sided,
    the face's own normal) | "phong" (one-sided, interpolated vertex normals).
    -> colour (N,3) [, dict(alb (N,3), ndl (N,) the SIGNED n.l before relu / abs, nlen, llen (N,) the lengths normalised away,
    sin (N,) |a x b| / (|a||b|) of the face's edge vectors (flat), uv (N,2))]"""
    v = np.asarray(mesh["verts"], np.float64)
    fc = np.asarray(mesh["faces"], np.int64)
    face = np.asarray(face, np.int64).reshape(-1)
    w = np.asarray(w, np.float64).reshape(-1, 3)
    fv = fc[face]                                                               # (N,3)
    lerp = lambda tab, idx: (np.asarray(tab, np.float64)[idx] * w[:, :, None]).sum(1)
    d = {}
    if mesh.get("texture") is not None:
        d["uv"] = lerp(mesh["verts_uvs"], np.asarray(mesh["faces_uvs"], np.int64)[face])
        alb = sample_texture(mesh["texture"], d["uv"].T[:, None, :])[:, 0].T if face.size else np.zeros((0, 3))
    elif mesh.get("colors") is not None:
        alb = lerp(np.asarray(mesh["colors"], np.float64).reshape(-1, 3), fv)
    else:
        alb = np.ones((face.size, 3))
    d["alb"] = alb
    if shading is None:
        return (alb, d) if detail else alb
    if shading not in ("flat", "phong"):
        raise ValueError(shading)
    l, d["llen"] = _unit(np.asarray(LIGHT) - lerp(v, fv), 1e-6)
    if shading == "phong":
        vn = mesh.get("_vn64")
        if vn is None:
            vn = vertex_normals(v, fc)
        n, d["nlen"] = _unit(lerp(vn, fv), 1e-6)
        d["ndl"] = (n * l).sum(1)
        cos = np.maximum(d["ndl"], 0.0)
    else:                                                                       # the flat two-sided terms of plain_color
        a, b = v[fv[:, 1]] - v[fv[:, 0]], v[fv[:, 2]] - v[fv[:, 0]]
        c = np.cross(a, b)
        n, d["nlen"] = _unit(c, 1e-30)
        with np.errstate(all="ignore"):
            d["sin"] = d["nlen"] / (np.sqrt((a * a).sum(1)) * np.sqrt((b * b).sum(1)))
        d["ndl"] = (n * l).sum(1)
        cos = np.abs(d["ndl"])
    col = (0.5 + 0.3 * cos)[:, None] * alb + 0.2
    return (col, d) if detail else col


def render(verts, faces, T, K, H, W, colors=None, verts_uvs=None, faces_uvs=None, texture=None, shading="phong", pixel_center=0.5):
    """-> colour (3,H,W) float64 (0 where empty), face index (H,W) (-1 empty), barycentrics (H,W,3)"""
    f, _, w, _ = ro.rasterize(verts, faces, T, K, H, W, perspective=True, pixel_center=pixel_center)
    hit = f >= 0
    mesh = dict(verts=verts, faces=faces, colors=colors, verts_uvs=verts_uvs, faces_uvs=faces_uvs, texture=texture)
    col = color_at(mesh, np.clip(f, 0, None).ravel(), w.reshape(-1, 3), shading)
    return col.T.reshape(3, H, W) * hit, f, w


def tap_range(texture, uv, dix, diy):
    """(N,3): per channel the largest difference among the texels of the flipped map that a bilinear sample at uv (N,2) can read when its
    unnormalised, clipped coordinates are off by at most dix, diy (N,) texels: the texels from floor(ix - dix) to floor(ix + dix) + 1,
    clipped to the map (up to 3 x 3 when the offsets are < 1, the whole map otherwise)."""
    m = np.asarray(texture, np.float64)[::-1]
    Ht, Wt = m.shape[:2]
    ix = np.clip(uv[:, 0] * (Wt - 1), 0, Wt - 1)
    iy = np.clip(uv[:, 1] * (Ht - 1), 0, Ht - 1)
    x0, y0 = np.floor(np.clip(ix - dix, 0, Wt - 1)).astype(np.int64), np.floor(np.clip(iy - diy, 0, Ht - 1)).astype(np.int64)
    x1 = np.minimum(np.floor(np.clip(ix + dix, 0, Wt - 1)).astype(np.int64) + 1, Wt - 1)
    y1 = np.minimum(np.floor(np.clip(iy + diy, 0, Ht - 1)).astype(np.int64) + 1, Ht - 1)
    lo, hi = np.full((uv.shape[0], 3), np.inf), np.full((uv.shape[0], 3), -np.inf)
    for dy in range(3):
        for dx in range(3):
            t = m[np.minimum(y0 + dy, y1), np.minimum(x0 + dx, x1)]
            lo, hi = np.minimum(lo, t), np.maximum(hi, t)
    wide = (x1 - x0 > 2) | (y1 - y0 > 2)                   # (dix, diy >= 1, a UV of ~1e6 on the face: anything on the map)
    return np.where(wide[:, None], np.ptp(m.reshape(-1, 3), 0), hi - lo)


def arithmetic_bound(mesh, face, w, shading, col=None, d=None):
    """(N,3): the ARITHMETIC term of color_bound (its docstring has the count): what the kernel's own fp32 roundings can move the colour
    by when its weights are exactly w."""
    if col is None:
        col, d = color_at(mesh, face, w, shading, detail=True)
    face = np.asarray(face, np.int64).reshape(-1)
    N = face.size
    out = np.zeros((N, 3))
    shade = 1.0 if shading is None else 0.8                                      # d colour / d albedo = lit <= 0.8
    amax = np.abs(d["alb"])
    if mesh.get("texture") is not None:
        tex = np.asarray(mesh["texture"], np.float64)
        Ht, Wt = tex.shape[:2]
        cuv = np.abs(np.asarray(mesh["verts_uvs"], np.float64)[np.asarray(mesh["faces_uvs"], np.int64)[face]]).max((1, 2))
        s = MARGIN4 * K_IX * EPS * np.maximum(1.0, cuv)
        dix, diy = s * (Wt - 1), s * (Ht - 1)
        out += shade * ((dix + diy)[:, None] * tap_range(tex, d["uv"], dix, diy))
        amax = np.broadcast_to(np.abs(tex).max((0, 1)), (N, 3))                 # (a weighted sum of taps: rounded relative to the taps)
    elif mesh.get("colors") is not None:
        amax = np.abs(np.asarray(mesh["colors"], np.float64).reshape(-1, 3)[np.asarray(mesh["faces"], np.int64)[face]]).max(1)
    k = K_ALB * np.maximum(amax, np.abs(d["alb"])) * shade
    if shading is not None:
        with np.errstate(all="ignore"):
            amp = lambda x: np.where(x > 0, 1.0 / np.where(x > 0, x, 1.0), 0.0)  # (a length of exactly 0 normalises exact zeros: no error)
            an = np.maximum(1.0, amp(d["nlen"])) * (d["nlen"] > 0) if shading == "phong" else np.maximum(1.0, amp(d["sin"]))
            vmax = max(1.0, float(np.abs(np.asarray(mesh["verts"], np.float64)).max()))
            al = np.maximum(1.0, amp(d["llen"]) * vmax) * (d["llen"] > 0)
        k = k + (0.3 * (K_NRM * an + K_LGT * al + K_DOT))[:, None] * np.abs(d["alb"])
    k = k + K_FIN * np.maximum(1.0, np.abs(col))
    return out + MARGIN4 * EPS * k


def color_bound(mesh, face, w, dw, shading):
    """The per-pixel, per-channel ACCEPTANCE BOUND of the kernel's fp32 colour against color_at(mesh, face, w, shading), for weights the
    kernel knows to within dw (N,) -> (bound (N,3), colour (N,3), detail).  Nothing here is fitted to what the kernel produces.

    INPUT TERM.  The kernel interpolates with weights computed in fp32 from fp32 screen coordinates.  raster_ref derives that a projected
    vertex is within delta_f px of its true place (32 * 2^-24 * the largest coordinate: 8 roundings, 4x margin), which moves a
    screen-space weight by at most delta_f / a_f, a_f the smallest projected altitude of the face; the perspective division
    b_i = (w_i / z_i) / sum_j (w_j / z_j) scales that by at most z_max / z_min of the face and adds its own six roundings on numbers <= 1
    (16 * 2^-24 with the margin): the caller passes dw = delta_f / a_f * z_max / z_min + 16 * 2^-24 (weight_slack below).  The weights sum
    to 1 on both sides, so the error is a combination of the three exchange directions e_i - e_j; the colour is evaluated IN FP64, with
    the actual map, normals and light, at the six points w +- dw (e_i - e_j), and the term is the largest deviation from the colour at
    w, per channel.  A noise map therefore needs no tolerance of its own: where neighbouring texels differ by 1 and the face is a
    sliver at the limb the term is large because the input really is ill-conditioned there, and in a face's interior it is ~1e-6.

    ARITHMETIC TERM (arithmetic_bound), contract(off), the operations as written in tex_color / sample_bilinear_border:
      ix = ((u * 2 - 1 + 1) / 2) * (size - 1), u = (w0 u0 + w1 u1) + w2 u2: 5 roundings in u, 1 in u * 2 - 1, 1 in + 1, 1 in the product;
        * 2 and / 2 are exact: K_IX = 8 roundings relative to max(1, |uv| of the face's corners) * (size - 1), so ix and iy are off by at
        most 4 * 8 * 2^-24 * (size - 1) texels each, and a bilinear sample moves by at most that times the largest difference among
        the texels it can then read (tap_range; 0 on a constant map or a 1 x 1 map), times lit <= 0.8 when shaded;
      the rest, in units of 2^-24, times 4:
        K_ALB = 8: the four tap weights (2 subtractions, 1 product each -> 3), their products with the taps (1) and three additions,
          relative to the largest texel; vertex colours: 5, relative to the largest corner colour; white: exact;
        K_NRM = 21 (phong): a vertex normal of rasterizer.vertex_normals (fp32: edge differences 1, cross product 2 relative to
          |a||b|, a sum over the vertex's faces ~6, normalisation 5 => ~14, taken as 16) and its interpolation (5), relative to the
          length of the interpolated normal when that is < 1 (normals that nearly cancel); a length of exactly 0 divides exact zeros by
          the 1e-6 clamp and costs nothing.  Flat: the same count stands for p1 - p0, the cross product and rsqrt, relative to
          sin(angle between the face's edge vectors) (a sliver's normal is ill-conditioned);
        K_LGT = 11: the surface point (5, relative to the largest vertex coordinate), light - p (1), its normalisation (5), relative to
          |light - p| when that is < 1; exactly 0 costs nothing;
        K_DOT = 5: n . l; the three enter the colour through 0.3 * albedo;
        K_FIN = 4: 0.5 + 0.3 cos and albedo * lit + 0.2, relative to max(1, |colour|).
      For white albedo under phong on a well-shaped mesh this is 4 * 2^-24 * (0.3 * 37 + 4) = 3.6e-6.
    plain_color computes the same terms with contraction and rsqrtf (fewer roundings; v_rsq_f32 is within 1 ulp): the same count bounds
    it."""
    face = np.asarray(face, np.int64).reshape(-1)
    w = np.asarray(w, np.float64).reshape(-1, 3)
    dw = np.broadcast_to(np.asarray(dw, np.float64), face.shape)
    col, d = color_at(mesh, face, w, shading, detail=True)
    inp = np.zeros_like(col)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for s in (1.0, -1.0):
            wp = w.copy()
            wp[:, i] += s * dw
            wp[:, j] -= s * dw
            inp = np.maximum(inp, np.abs(color_at(mesh, face, wp, shading) - col))
    return inp + arithmetic_bound(mesh, face, w, shading, col, d), col, d


def weight_slack(ref, faces, face):
    """dw of color_bound for the faces `face` (N,) of one raster_ref.raycast result"""
    z = ref["cam_z"][np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    with np.errstate(all="ignore"):
        return ref["delta"][face] / ref["alt"][face] * (z.max(1) / z.min(1)) + 16.0 * EPS
