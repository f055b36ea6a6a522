"""GPU tests of the textured, Phong-shaded render (csrc/raster.hip rnnpose_raster_resolve_tex_f32, MeshRenderer(shading=...),
MeshRenderer.from_obj): the reference's DiffRender.render_mesh (TexturesUV + SoftPhongShader, faces_per_pixel = 1).
PARITY UNPINNED against PyTorch3D; checked analytically (affine textures are reproduced exactly by bilinear sampling, texel
centres and the border clamp reproduce texels) and against tests/texture_ref.py (the PyTorch3D chain restated on the CPU in
fp64 with torch's own grid_sample)."""
import numpy as np
import pytest
import torch

import texture_ref as tr
from oracle import raster_oracle as ro
from oracle import rnnpose_oracle as orc
from rnnpose_amd import synthetic as syn
from test_raster import icosphere, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from rnnpose_amd import build, ops as _ops
    build.build()
    return _ops


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def planar_uvs(verts, lo=0.05, hi=0.95):
    """(U,2) = an affine map of the object x, y onto [lo, hi]^2 (faces_uvs = faces)"""
    a, b = verts[:, :2].min(0), verts[:, :2].max(0)
    return (lo + (hi - lo) * (verts[:, :2] - a) / (b - a)).astype(np.float32)


def same_face(f_o, w_o, z_o, depth):
    """pixels where the oracle's face is unambiguous (all barycentrics > 1e-4) and the GPU's depth is that face's: both chose
    the same face"""
    return (f_o >= 0) & (depth > 0) & (w_o.min(-1) > 1e-4) & (np.abs(depth - z_o) < 1e-5)


def test_linear_texture_unshaded_is_exact_at_the_surface_point(ops):
    """Texture affine in (u, v), UVs affine in the object coordinates: bilinear sampling reproduces the affine function, so the
    colour must be the analytic value at the surface point each pixel's ray hits (cf. test_depth_ordering_and_linear_attributes)."""
    from rnnpose_amd.rasterizer import MeshRenderer
    quad = lambda z, s: np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], np.float32)
    verts = np.concatenate([quad(0.0, 0.05), quad(0.1, 0.1)])
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    H, W = 96, 128
    K = np.array([[[500.0, 0, 64.0], [0, 500.0, 48.0], [0, 0, 1]]], np.float32)
    G = syn.se3_exp_np(np.array([[0, 0, 0, 0.3, -0.2, 0.1]]))
    G[:, :3, 3] = [0.005, -0.004, 0.6]
    G = G.astype(np.float32)
    Auv = np.array([[3.0, 0.4, 1.0], [-0.5, 2.5, -1.0]], np.float32)             # uv = Auv @ X_obj + cuv, inside (0.1, 0.9)
    cuv = np.array([0.5, 0.45], np.float32)
    uvs = verts @ Auv.T + cuv
    assert uvs.min() > 0.02 and uvs.max() < 0.98
    Ht, Wt = 48, 64                                                                 # (non-square: a transposed map fails)
    Atex = np.array([[0.5, 0.2], [-0.3, 0.4], [0.1, -0.6]], np.float64)            # colour = Atex @ (u, v) + ctex
    ctex = np.array([0.2, 0.4, 0.65])
    u = np.arange(Wt) / (Wt - 1)
    v = 1.0 - np.arange(Ht) / (Ht - 1)                                              # row 0 of the file = v = 1 (TexturesUV flips)
    uu, vv = np.meshgrid(u, v)
    tex = (np.stack([uu, vv], -1) @ Atex.T + ctex).astype(np.float32)
    assert tex.min() > 0 and tex.max() < 1
    attr = verts @ np.array([[2.0, -1.0, 0.5]], np.float32).T
    ren = MeshRenderer({"q": dict(verts=verts, faces=faces, verts_uvs=uvs, faces_uvs=faces, texture=tex)}, shade=False)
    out, depth = ren(["q"], T(attr)[None].cuda(), T=T(G).cuda(), K=T(K).cuda(), render_image_size=(H, W), render_tex=True)
    assert out.shape == (1, 4, H, W)
    z = depth[0, 0].cpu().numpy()
    hit = z > 0
    ys, xs = np.mgrid[0:H, 0:W]
    ray = np.stack([(xs + 0.5 - K[0, 0, 2]) / K[0, 0, 0], (ys + 0.5 - K[0, 1, 2]) / K[0, 1, 1], np.ones_like(xs, float)], -1)
    Xo = (ray * z[..., None] - G[0, :3, 3]) @ G[0, :3, :3]
    want = (Xo @ Auv.T.astype(np.float64) + cuv) @ Atex.T + ctex
    got = out[0, :3].cpu().numpy().transpose(1, 2, 0)
    assert hit.mean() > 0.2 and np.abs(got - want)[hit].max() < 2e-4
    assert np.all(got[~hit] == 0.0) and np.all(z[~hit] == -1.0)
    assert np.abs(out[0, 3].cpu().numpy() - (Xo @ np.array([2.0, -1.0, 0.5])))[hit].max() < 2e-4   # attribute channels as before


def _constant_uv_mesh(Ht, Wt):
    """icosphere whose every face has ONE uv at all three corners: a texel centre (i/(Wt-1), j/(Ht-1)), or for every fifth face a
    point outside [0,1]^2 (the border clamp) -> (verts, faces, verts_uvs, faces_uvs, expected texel index (F,2) in the FILE's rows)"""
    verts, faces = icosphere(sub=2)
    F = faces.shape[0]
    rng = np.random.default_rng(5)
    i, j = rng.integers(0, Wt, F), rng.integers(0, Ht, F)
    uv = np.stack([i / (Wt - 1), j / (Ht - 1)], 1)
    out = np.arange(F) % 5 == 0
    far = rng.choice([-3.0, -0.4, 1.3, 2.5], (F, 2))
    uv[out] = far[out]
    col = np.where(uv[:, 0] < 0, 0, np.where(uv[:, 0] > 1, Wt - 1, i))
    row_f = np.where(uv[:, 1] < 0, 0, np.where(uv[:, 1] > 1, Ht - 1, j))           # row of the FLIPPED map
    fuv = np.repeat(np.arange(F, dtype=np.int32)[:, None], 3, 1)
    return verts, faces, uv.astype(np.float32), fuv, np.stack([Ht - 1 - row_f, col], 1), out


def test_texel_centres_reproduce_texels_and_outside_uvs_take_the_border(ops):
    from rnnpose_amd.rasterizer import MeshRenderer
    Ht, Wt = 9, 17                                                                  # (size - 1 a power of two: i / (size - 1) exact)
    rr, cc = np.mgrid[0:Ht, 0:Wt]
    checker = ((rr + cc) % 2).astype(np.float32)
    tex = np.stack([0.1 + 0.8 * checker, 0.05 * cc / Wt + 0.5 * checker, 0.9 - 0.04 * rr - 0.3 * checker], -1).astype(np.float32)
    verts, faces, uv, fuv, texel, outside = _constant_uv_mesh(Ht, Wt)
    B, H, W = 2, 128, 160
    _, _, K, G = scene(B, seed=3)
    ren = MeshRenderer({"s": dict(verts=verts, faces=faces, verts_uvs=uv, faces_uvs=fuv, texture=tex)}, shade=False)
    out, depth = ren(["s"] * B, torch.zeros(1, verts.shape[0], 0, device="cuda"), T=T(G).cuda(), K=T(K).cuda(),
                     render_image_size=(H, W), render_tex=True)
    n_border = 0
    for b in range(B):
        f, z, w, _ = ro.rasterize(verts, faces, G[b], K[b], H, W)
        m = same_face(f, w, z, depth[b, 0].cpu().numpy())
        assert m.mean() > 0.1
        got = out[b].cpu().numpy().transpose(1, 2, 0)[m]
        fi = f[m]
        want = tex[texel[fi, 0], texel[fi, 1]]
        bo = outside[fi]
        assert np.array_equal(got[bo], want[bo])                                    # border clamp: the texel itself, bit for bit
        assert np.abs(got[~bo] - want[~bo]).max() <= 1e-5               # centres: up to the fp32 rounding of sum w_i uv (~2e-6)
        n_border += int(bo.sum())
    assert n_border > 100


def _two_classes():
    vt, ft = icosphere(sub=3)
    vc, fc = icosphere(sub=3, scale=(0.07, 0.08, 0.06))
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8).astype(np.float32) / np.float32(255.0)
    return dict(tex=dict(verts=vt, faces=ft, colors=None, verts_uvs=planar_uvs(vt), faces_uvs=ft, texture=noise),
                col=dict(verts=vc, faces=fc, colors=syn.uniform("colc", (vc.shape[0], 3), 4)))


def _against_ref(ren, meshes, names, shading, seed):
    B, H, W = len(names), 128, 160
    _, _, K, G = scene(B, seed=seed)
    out, depth = ren(names, torch.zeros(1, max(m["verts"].shape[0] for m in meshes.values()), 4, device="cuda"), T=T(G).cuda(),
                     K=T(K).cuda(), render_image_size=(H, W), render_tex=True)
    errs = []
    for b, n in enumerate(names):
        m = meshes[n]
        want, f, w = tr.render(m["verts"], m["faces"], G[b], K[b], H, W, colors=m.get("colors"), verts_uvs=m.get("verts_uvs"),
                               faces_uvs=m.get("faces_uvs"), texture=m.get("texture"), shading=shading)
        _, z, _, _ = ro.rasterize(m["verts"], m["faces"], G[b], K[b], H, W)
        d = depth[b, 0].cpu().numpy()
        sel = same_face(f, w, z, d)
        assert sel.mean() > 0.1
        assert np.all(out[b, :3].cpu().numpy()[:, d < 0] == 0.0)
        errs.append(np.abs(out[b, :3].cpu().numpy() - want)[:, sel].ravel())
    return errs


def test_textured_phong_matches_texture_ref(ops):
    """B = 3, two classes in one batch (one textured with a 256^2 noise map, one vertex-coloured), different poses."""
    from rnnpose_amd.rasterizer import MeshRenderer
    meshes = _two_classes()
    ren = MeshRenderer(meshes, shading="phong")
    errs = _against_ref(ren, meshes, ["tex", "col", "tex"], "phong", seed=7)
    e = np.concatenate(errs)
    assert e.max() <= 2e-3 and np.quantile(e, 0.99) <= 1e-5, (e.max(), np.quantile(e, 0.99))


def test_phong_on_untextured_mesh_matches_texture_ref(ops):
    """White albedo (an OBJ without a map): everywhere <= 1e-5.  Random vertex colours: the colour changes by O(1) across a face,
    so the fp32 screen-space barycentrics of grazing faces at the limb show (up to ~3e-5 here, as for the attribute channels of
    test_raster_matches_oracle); the 99th percentile stays <= 1e-6."""
    from rnnpose_amd.rasterizer import MeshRenderer
    meshes = _two_classes()
    del meshes["tex"]
    e = np.concatenate(_against_ref(MeshRenderer(meshes, shading="phong"), meshes, ["col", "col"], "phong", seed=8))
    assert e.max() <= 1e-4 and np.quantile(e, 0.99) <= 1e-6
    meshes["col"]["colors"] = None
    e = np.concatenate(_against_ref(MeshRenderer(meshes, shading="phong"), meshes, ["col", "col"], "phong", seed=8))
    assert e.max() <= 1e-5


def test_textured_flat_shading_matches_texture_ref(ops):
    """shading="flat" on a textured mesh: the texture through the flat two-sided terms of the vertex-colour path."""
    from rnnpose_amd.rasterizer import MeshRenderer
    meshes = _two_classes()
    ren = MeshRenderer(meshes)
    e = np.concatenate(_against_ref(ren, meshes, ["tex", "col"], "flat", seed=9))
    assert e.max() <= 2e-3 and np.quantile(e, 0.99) <= 1e-5


def test_vertex_colour_entry_point_unchanged_next_to_a_textured_mesh(ops):
    """rnnpose_raster_resolve_f32's outputs are bit-identical when a textured mesh is merely loaded next to untextured ones."""
    from rnnpose_amd.rasterizer import MeshRenderer
    meshes = _two_classes()
    meshes["tex"]["colors"] = syn.uniform("colt", (meshes["tex"]["verts"].shape[0], 3), 5)
    plain = {k: dict(verts=m["verts"], faces=m["faces"], colors=m["colors"]) for k, m in meshes.items()}
    col2 = dict(plain["col"])
    a = MeshRenderer(dict(col=plain["col"], col2=col2))
    b = MeshRenderer(dict(tex=meshes["tex"], col=meshes["col"], col2=col2))
    assert b._tex is not None and a._tex is None
    _, _, K, G = scene(2, seed=4)
    attr = T(syn.normal("a", (1, meshes["col"]["verts"].shape[0], 8), 1)).cuda()
    kw = dict(T=T(G).cuda(), K=T(K).cuda(), render_image_size=(128, 160))
    for tex in (True, False):
        oa, da = a(["col", "col2"], attr, render_tex=tex, **kw)
        ob, db = b(["col", "col2"], attr, render_tex=tex, **kw)
        assert torch.equal(oa, ob) and torch.equal(da, db)
    assert torch.equal(a.render_depth(["col", "col2"], **kw), b.render_depth(["col", "col2"], **kw))


def _write_textured_obj(d):
    from PIL import Image
    verts, faces = icosphere(sub=3)
    uv = planar_uvs(verts)
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:64, 0:64]
    img = np.stack([4 * xx, 4 * yy, 255 - 2 * (xx + yy)], -1).astype(np.uint8) // 2 + rng.integers(0, 64, (64, 64, 3), dtype=np.uint8)
    Image.fromarray(img).save(d / "texture_map.png")
    (d / "textured.mtl").write_text("newmtl material_0\nKd 1 1 1\nmap_Kd texture_map.png\n")
    lines = ["mtllib textured.mtl"] + [f"v {a:.8f} {b:.8f} {c:.8f}" for a, b, c in verts] + [f"vt {a:.8f} {b:.8f}" for a, b in uv]
    lines += ["usemtl material_0"] + [f"f {a + 1}/{a + 1} {b + 1}/{b + 1} {c + 1}/{c + 1}" for a, b, c in faces]
    (d / "textured.obj").write_text("\n".join(lines) + "\n")
    return str(d / "textured.obj"), verts.shape[0]


def test_from_obj_drives_pose_refiner_graph_equals_eager(ops, tmp_path):
    """MeshRenderer.from_obj(...) as PoseRefiner's renderer (model/RNNPose.py:76-79, 151-152): the textured, Phong-shaded
    syn_img is finite and varies across the object; hipGraph replay == eager launches."""
    from rnnpose_amd.pose_refiner import PoseRefiner, default_config
    from rnnpose_amd.rasterizer import MeshRenderer
    from rnnpose_amd.transformation import SE3Sequence
    path, P = _write_textured_obj(tmp_path)
    ren = MeshRenderer.from_obj({"cat": path})
    assert ren.shading == "phong" and ren.textured["cat"]
    B, H, W = 2, 240, 320
    K = np.tile(np.array([[572.4114, 0, 160.0], [0, 573.57043, 120.0], [0, 0, 1]], np.float32), (B, 1, 1))
    G = syn.se3_exp_np(syn.normal("g", (B, 6), 4, std=0.3))
    G[:, :3, 3] = [0.01, -0.01, 0.8]
    G = G.astype(np.float32)
    names = ["cat"] * B
    cfg = default_config(RENDER_ITER_COUNT=2, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=(H, W), zoom_crop_size=(128, 160))
    t = lambda n, s, sd: T(syn.normal(n, s, sd, std=0.2)).cuda()
    inputs = dict(intrinsics=T(K).cuda(), image=T(syn.uniform("img", (B, 3, H, W), 5)).cuda(), fea_3d=t("f3", (1, P, 256), 6),
                  Tj_gt=None, obj_cls=names, geofea_2d=t("g2", (B, 32, H, W), 7), geofea_3d=t("g3", (1, P, 32), 8))
    outs = {}
    for mode in (False, True):
        ref = PoseRefiner(cfg, renderer=ren, use_graph=mode).cuda().eval()
        ref.cf_net.update_block.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
        ref.image_fea_enc.fnet.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
        for _ in range(2):                                                      # the second call replays every graph
            out = ref(Ts=SE3Sequence(matrix=T(G).cuda()[:, None]), **inputs)
        outs[mode] = out
        syn_img, depth = out["syn_img"][0], out["syn_depth"][0]
        fg = (depth > 0).expand_as(syn_img)
        assert torch.isfinite(syn_img).all() and torch.isfinite(out["Ti_pred"].G).all()
        assert float((depth > 0).float().mean()) > 0.1
        vals = syn_img[fg]
        assert float(vals.std()) > 0.02 and float(vals.min()) >= 0.2 - 1e-6 and float(vals.max()) <= 1.0 + 1e-6   # 0.2 + 0.8 * albedo
        assert float(syn_img[~fg].abs().max()) == 0.0
    e, g = outs[False], outs[True]
    assert torch.equal(e["Ti_pred"].G, g["Ti_pred"].G) and torch.equal(e["flow_last"], g["flow_last"])
    for a, b in zip(e["syn_img"], g["syn_img"]):
        assert torch.equal(a, b)


def test_hip_epoch_picks_phong_for_textured_models(ops):
    from rnnpose_amd.eval_epoch import HipEpoch, synthetic_models
    models = synthetic_models(("ape", "cat"), sub=2)
    assert HipEpoch(models).renderer.shading == "flat"
    m = models["cat"]
    m.verts_uvs, m.faces_uvs = planar_uvs(m.verts), m.faces
    m.texture = np.full((4, 4, 3), 0.5, np.float32)
    ep = HipEpoch(models)
    assert ep.renderer.shading == "phong" and ep.renderer.textured == {"ape": False, "cat": True}
