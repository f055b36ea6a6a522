"""tests/texture_ref.py (the fp64 colour reference the GPU tests of the textured, Phong-shaded render compare against) pinned WITHOUT
the kernel: its sampler against hand-written bilinear taps, its vertex normals against analytic ones, color_at against the chain as
it was first written on the oracle's images, the acceptance bound's two terms on maps where they are known, and the renderer's fp32
vertex normals against the fp64 ones."""
import numpy as np
import torch
import torch.nn.functional as F

import texture_ref as tr
from oracle import raster_oracle as ro
from rnnpose_amd import rasterizer
from rnnpose_amd import synthetic as syn
from test_raster import icosphere, scene


def hand_bilinear(tex, u, v):
    """TexturesUV on one point, written out: the map is flipped (file row 0 is v = 1), x = u (Wt - 1), y = v (Ht - 1) on the flipped
    map, clamped to it, and the four texels around (x, y) are mixed by their areas"""
    m = np.asarray(tex, np.float64)[::-1]
    Ht, Wt = m.shape[:2]
    x, y = min(max(u * (Wt - 1), 0.0), Wt - 1.0), min(max(v * (Ht - 1), 0.0), Ht - 1.0)
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    x1, y1 = min(x0 + 1, Wt - 1), min(y0 + 1, Ht - 1)
    a, b = x - x0, y - y0
    return (1 - a) * (1 - b) * m[y0, x0] + a * (1 - b) * m[y0, x1] + (1 - a) * b * m[y1, x0] + a * b * m[y1, x1]


def contrast_map(Ht, Wt):
    rr, cc = np.mgrid[0:Ht, 0:Wt]
    ch = ((rr + cc) % 2).astype(np.float64)
    return np.stack([0.1 + 0.8 * ch, 0.05 * cc / Wt + 0.5 * ch, 0.9 - 0.04 * rr - 0.3 * ch], -1)


def test_sample_texture_is_the_hand_written_bilinear():
    for Ht, Wt in ((3, 5), (9, 17), (1, 4), (4, 1), (1, 1), (2, 2)):
        tex = contrast_map(Ht, Wt)
        us = [i / max(Wt - 1, 1) for i in range(Wt)] + [(i + 0.5) / max(Wt - 1, 1) for i in range(max(Wt - 1, 1))] + [0.0, 1.0, -3.0, -0.4, 1.3, 2.5, 1e6, -1e6, 0.3]
        vs = [j / max(Ht - 1, 1) for j in range(Ht)] + [(j + 0.25) / max(Ht - 1, 1) for j in range(max(Ht - 1, 1))] + [0.0, 1.0, -3.0, -0.4, 1.3, 2.5, 1e6, -1e6, 0.7]
        uu, vv = np.meshgrid(us, vs)
        got = tr.sample_texture(tex, np.stack([uu, vv]))
        want = np.array([[hand_bilinear(tex, u, v) for u in us] for v in vs]).transpose(2, 0, 1)
        assert np.abs(got - want).max() <= 1e-9, (Ht, Wt, np.abs(got - want).max())   # (u = 1e6: ~1e-10 of cancellation in uv * 2 - 1)
    tex = contrast_map(3, 5)                                                    # the flip, stated on file rows: v = 1 is the file's top row
    corners = tr.sample_texture(tex, np.array([[[0.0, 1.0], [0.0, 1.0]], [[1.0, 1.0], [0.0, 0.0]]]))
    assert np.array_equal(corners[:, 0, 0], tex[0, 0]) and np.array_equal(corners[:, 0, 1], tex[0, 4])
    assert np.array_equal(corners[:, 1, 0], tex[2, 0]) and np.array_equal(corners[:, 1, 1], tex[2, 4])
    centre = tr.sample_texture(tex, np.array([[[0.25]], [[0.5]]]))[:, 0, 0]     # texel centre (column 1, middle row)
    assert np.abs(centre - tex[1, 1]).max() <= 1e-15


def _degenerate_mesh():
    """sub-1 sphere + an unreferenced vertex + a zero-area face (a repeated index) + one face present twice"""
    v, f = icosphere(sub=1, scale=(1.0, 1.0, 1.0))
    v2 = np.concatenate([v, [[0.3, 0.2, 0.1]]]).astype(np.float32)
    f2 = np.concatenate([f, [[3, 3, 7]], f[5:6]]).astype(np.int32)
    return v, f, v2, f2


def test_vertex_normals_are_analytic_on_a_sphere_and_defined_on_degenerate_input():
    v, f = icosphere(sub=3, scale=(1.0, 1.0, 1.0))
    n = tr.vertex_normals(v, f)
    r = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12
    edge = np.linalg.norm(v[f[:, 0]].astype(np.float64) - v[f[:, 1]], axis=1).max()
    assert np.abs(n - r).max() < edge ** 2 < 0.03          # (the area-weighted mean over a vertex's faces: outward, radial to O(edge^2))
    v, f = icosphere(sub=0, scale=(1.0, 1.0, 1.0))         # the icosahedron's symmetry makes the mean exactly radial
    assert np.abs(tr.vertex_normals(v, f) - v / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)).max() < 1e-6
    v, f, v2, f2 = _degenerate_mesh()
    n1, n2 = tr.vertex_normals(v, f), tr.vertex_normals(v2, f2)
    assert np.all(n2[-1] == 0.0)                                                # unreferenced: the sum is empty, 0 / max(0, eps) = 0
    touched = np.unique(f[5])
    rest = np.setdiff1d(np.arange(v.shape[0]), touched)
    assert np.array_equal(n1[rest], n2[:-1][rest])                              # the zero-area face adds exact zeros
    fn = np.cross(v[f[5, 2]].astype(np.float64) - v[f[5, 1]], v[f[5, 0]].astype(np.float64) - v[f[5, 1]])
    for k in touched:                                                           # the doubled face counts twice
        s = sum(np.cross(v[t[2]].astype(np.float64) - v[t[1]], v[t[0]].astype(np.float64) - v[t[1]]) for t in f if k in t) + fn
        assert np.abs(n2[k] - s / np.linalg.norm(s)).max() < 1e-12
        assert np.abs(n2[k] - n1[k]).max() > 1e-3


def test_fp32_vertex_normals_of_the_renderer_match_the_fp64_ones():
    for v, f in (icosphere(sub=3), icosphere(sub=2, scale=(0.07, 0.08, 0.06)), _degenerate_mesh()[2:]):
        n32 = rasterizer.vertex_normals(v, f)
        assert n32.dtype == torch.float32
        n64 = tr.vertex_normals(v, f)
        assert np.abs(n32.numpy() - n64).max() <= 16 * tr.EPS                    # (K_NRM's share for a vertex normal, without the margin)
    assert np.all(n32.numpy()[-1] == 0) and np.all(n64[-1] == 0)                 # the unreferenced vertex, in both


def _first_render(verts, faces, T, K, H, W, colors=None, verts_uvs=None, faces_uvs=None, texture=None, shading="phong"):
    """texture_ref.render as it was before color_at: torch's normalize on whole images of the oracle's interpolate"""
    f, _, w, _ = ro.rasterize(verts, faces, T, K, H, W, perspective=True)
    hit = f >= 0
    if texture is not None:
        alb = tr.sample_texture(texture, ro.interpolate(f, w, faces_uvs, verts_uvs))
    elif colors is not None:
        alb = ro.interpolate(f, w, faces, colors)
    else:
        alb = np.ones((3, H, W))
    if shading is None:
        return alb * hit
    p = torch.as_tensor(ro.interpolate(f, w, faces, verts))
    l = F.normalize(torch.tensor(tr.LIGHT, dtype=torch.float64)[:, None, None] - p, eps=1e-6, dim=0)
    if shading == "phong":
        n = F.normalize(torch.as_tensor(ro.interpolate(f, w, faces, tr.vertex_normals(verts, faces))), eps=1e-6, dim=0)
        cos = torch.relu((n * l).sum(0))
    else:
        v = np.asarray(verts, np.float64)[np.asarray(faces)[np.clip(f, 0, None)]]
        n = torch.as_tensor(np.cross(v[..., 1, :] - v[..., 0, :], v[..., 2, :] - v[..., 0, :])).permute(2, 0, 1)
        cos = ((F.normalize(n, eps=1e-30, dim=0) * l).sum(0)).abs()
    return ((0.5 + 0.3 * cos.numpy()) * alb + 0.2) * hit


def _textured_sphere(Ht=9, Wt=17, sub=2):
    v, f = icosphere(sub=sub)
    uv = (0.05 + 0.9 * (v[:, :2] - v[:, :2].min(0)) / np.ptp(v[:, :2], 0)).astype(np.float32)
    return dict(verts=v, faces=f, colors=None, verts_uvs=uv, faces_uvs=f, texture=contrast_map(Ht, Wt).astype(np.float32))


def test_color_at_equals_the_whole_image_render():
    H, W = 48, 64
    m = _textured_sphere()
    _, _, K, G = scene(1, seed=3)
    K = K.copy()
    K[:, :2] *= W / 160.0
    cols = syn.uniform("ref.col", (m["verts"].shape[0], 3), 1)
    for shading in (None, "flat", "phong"):
        for kw in (dict(verts_uvs=m["verts_uvs"], faces_uvs=m["faces_uvs"], texture=m["texture"]), dict(colors=cols), dict()):
            want = _first_render(m["verts"], m["faces"], G[0], K[0], H, W, shading=shading, **kw)
            got, f, w = tr.render(m["verts"], m["faces"], G[0], K[0], H, W, shading=shading, **kw)
            assert (f >= 0).mean() > 0.1 and np.abs(got - want).max() < 1e-13
            if shading is not None:
                assert np.ptp(got[:, f >= 0]) > 0.05


def test_bound_is_the_arithmetic_term_on_a_constant_map_and_grows_with_contrast():
    m = _textured_sphere()
    rng = np.random.default_rng(0)
    N = 200
    face = rng.integers(0, m["faces"].shape[0], N)
    w = rng.dirichlet((1, 1, 1), N)
    dw = np.full(N, 1e-4)
    flat_map = dict(m, texture=np.full((9, 17, 3), 0.6, np.float32))
    b, col, _ = tr.color_bound(flat_map, face, w, dw, None)
    assert np.allclose(col, np.float32(0.6)) and np.allclose(b, tr.arithmetic_bound(flat_map, face, w, None), rtol=0, atol=1e-15)
    assert np.allclose(b, tr.MARGIN4 * tr.EPS * (tr.K_ALB * np.float64(np.float32(0.6)) + tr.K_FIN), rtol=1e-9, atol=1e-15)   # no tap differs: no sampler term
    prev, prev_in = b.max(), 0.0
    for c in (0.01, 0.1, 1.0):                                                  # the same checker at growing contrast
        mc = dict(m, texture=(0.5 + c * (contrast_map(9, 17) - 0.5)).astype(np.float32))
        b, _, _ = tr.color_bound(mc, face, w, dw, None)
        inp = (b - tr.arithmetic_bound(mc, face, w, None)).max()                # the input term: the map's slope times dw
        assert b.max() > prev and inp > 5 * prev_in and inp > 1e-4 * c
        prev, prev_in = b.max(), inp
    # the input term is linear in dw where the map is: |d colour| = dw * |slope| on an affine map
    uu, vv = np.meshgrid(np.arange(17) / 16.0, 1.0 - np.arange(9) / 8.0)
    ramp = dict(m, texture=np.stack([uu, vv, 0.5 * uu + 0.25 * vv], -1))
    b1, _, _ = tr.color_bound(ramp, face, w, dw, None)
    b2, _, _ = tr.color_bound(ramp, face, w, 2 * dw, None)
    a = tr.arithmetic_bound(ramp, face, w, None)
    assert np.allclose(b2 - a, 2 * (b1 - a), rtol=1e-6, atol=1e-15)
    duv = m["verts_uvs"].astype(np.float64)[m["faces"][face]]
    worst = np.maximum(np.maximum(np.abs(duv[:, 0] - duv[:, 1]), np.abs(duv[:, 0] - duv[:, 2])), np.abs(duv[:, 1] - duv[:, 2]))
    assert np.allclose((b1 - a)[:, :2], 1e-4 * worst, rtol=1e-6, atol=1e-15)
    # shading: exact zeros cost nothing, a short interpolated normal is amplified
    zero = dict(verts=np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), colors=None,
                faces=np.array([[0, 1, 2], [0, 2, 1], [0, 2, 3], [0, 3, 2]], np.int32))
    assert np.all(tr.vertex_normals(zero["verts"], zero["faces"]) == 0)
    col, d = tr.color_at(zero, [0, 2], [[0.2, 0.3, 0.5], [0.6, 0.2, 0.2]], "phong", detail=True)
    assert np.all(col == 0.5 + 0.2) and np.all(d["nlen"] == 0)
    b = tr.arithmetic_bound(zero, [0, 2], [[0.2, 0.3, 0.5], [0.6, 0.2, 0.2]], "phong")
    good = tr.arithmetic_bound(dict(zero, faces=zero["faces"][[0, 2]]), [0, 1], [[0.2, 0.3, 0.5], [0.6, 0.2, 0.2]], "phong")
    assert np.all(b < good) and np.all(good < 8e-6)
