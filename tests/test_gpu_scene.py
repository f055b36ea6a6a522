"""Several objects of ONE camera frame in one call (mixed-class batches): the zoom crop with a source index
(csrc/zoom_crop.hip, rnnpose_zoom_crop_indexed_f32), MeshRenderer's resident per-class attribute tables, and PoseRefiner /
RendererAdapter with `image_index` and per-image feature tables.  The first three tests also run on the host-executed kernels
(tests/test_scene_on_host.py)."""
import numpy as np
import pytest
import torch

from oracle import rnnpose_oracle as orc
from rnnpose_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from rnnpose_amd import build, ops as _ops
    build.build()
    return _ops


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _thetas(B, seed):
    """Axis-aligned crop windows of different sizes; every second one reaches outside the image (zero padding)."""
    th = np.zeros((B, 2, 3), np.float32)
    u = syn.uniform("theta", (B, 4), seed)
    for b in range(B):
        th[b, 0, 0], th[b, 1, 1] = 0.25 + 0.5 * u[b, 0], 0.25 + 0.5 * u[b, 1]
        th[b, 0, 2], th[b, 1, 2] = (u[b, 2] - 0.5) * (2.2 if b % 2 else 0.6), (u[b, 3] - 0.5) * (2.2 if b % 2 else 0.6)
    return T(th).cuda()


# ---- 1: the indexed crop with src_index = 0..B-1 is the existing crop ------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 32])
@pytest.mark.parametrize("H,W,hc,wc", [(480, 640, 240, 240), (37, 53, 24, 40)])
def test_indexed_crop_with_identity_index_equals_plain_crop_bitwise(ops, C, H, W, hc, wc):
    B = 3
    x = T(syn.normal("x", (B, C, H, W), 11)).cuda()
    theta = _thetas(B, 5)
    want, want_grid = ops.zoom_crop(x, theta, (hc, wc), want_grid=True)
    got, got_grid = ops.zoom_crop(x, theta, (hc, wc), want_grid=True, src_index=torch.arange(B))
    assert torch.equal(got, want) and torch.equal(got_grid, want_grid)
    assert float((want == 0).float().mean()) > 0.02, "some window must reach outside the image"
    again = ops.zoom_crop(x, theta, (hc, wc), src_index=list(range(B)))
    assert torch.equal(again, got)                                   # two runs are bit-identical


# ---- 2: shared sources ------------------------------------------------------------------------------------------------------
IDX = [1, 0, 1, 1, 0]


@pytest.mark.parametrize("C,H,W,hc,wc", [(32, 120, 160, 64, 64), (32, 48, 64, 24, 32), (3, 37, 53, 24, 40)])
def test_indexed_crop_equals_crop_of_the_gathered_copy(ops, C, H, W, hc, wc):
    """S = 2 sources, B = 5 crops: bit for bit the plain crop of x[src_index], for every accepted form of the index."""
    from rnnpose_amd import zoom
    x = T(syn.normal("x", (2, C, H, W), 12)).cuda()
    theta = _thetas(len(IDX), 6)
    gathered = x[torch.tensor(IDX, device=x.device)].contiguous()
    want = ops.zoom_crop(gathered, theta, (hc, wc))
    for src_index in (IDX, torch.tensor(IDX, dtype=torch.int64), torch.tensor(IDX, dtype=torch.int32).cuda(),
                      ops.SourceIndex(IDX, 2, x.device)):
        assert torch.equal(ops.zoom_crop(x, theta, (hc, wc), src_index=src_index), want)
    assert torch.equal(zoom.zoom_crop(x, theta, (hc, wc), src_index=IDX), want)


def test_indexed_crop_matches_torch_grid_sample_on_the_cpu(ops):
    """Against F.grid_sample(x[src_index], F.affine_grid(theta)) run by torch on the CPU, at the bound tests/test_zoom.py holds
    the plain kernel to against torch: atol 2e-5.  That bound was set on the golden fixture tests/golden/zoom_small.npz (two
    48 x 64 images of unit-variance noise, the two windows of its masks), so this comparison uses the fixture's images as the two
    sources and its windows, five crops with src_index = [1, 0, 1, 1, 0], every crop pairing a source with BOTH windows over the
    batch.  The bound is not a property of the kernel at other inputs: the kernel and torch round the sampling coordinate
    differently in fp32 (~1e-6 of the normalised range, test_zoom.py:125), a pixel offset that multiplies the image gradient.
    Measured on the plain kernel (to which the indexed one is bit-identical) with random windows on unit-variance noise:
    max 7.4e-5 at 120 x 160 and 2.3e-5 (one element of 122 880) at 48 x 64; tests/test_zoom.py allows 2e-3 at 480 x 640."""
    import os
    import torch.nn.functional as F
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "zoom_small.npz")))
    hc, wc = [int(v) for v in g["crop_size"]]
    x = T(g["x"][:2]).cuda()
    theta = T(g["theta_oracle"][[1, 0, 0, 1, 0]]).cuda()
    got = ops.zoom_crop(x, theta, (hc, wc), src_index=IDX)
    xs = T(g["x"][:2])[torch.tensor(IDX)]
    ref = F.grid_sample(xs, F.affine_grid(theta.cpu(), [len(IDX), xs.shape[1], hc, wc], align_corners=False), mode="bilinear",
                        padding_mode="zeros", align_corners=False)
    err = float((got.cpu() - ref).abs().max())
    print(f"indexed crop vs torch CPU grid_sample: max abs err {err:.3e} (bound 2e-5)")
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=2e-5, rtol=0)
    np.testing.assert_allclose(got[[0, 1]].cpu().numpy(), g["crop_torch"][[1, 0]], atol=2e-5, rtol=0)     # the fixture's own pairs


def test_indexed_crop_through_the_torch_ops_namespace(ops):
    import rnnpose_amd.torch_ops  # noqa: F401
    x = T(syn.normal("x", (2, 3, 37, 53), 12)).cuda()
    theta = _thetas(len(IDX), 6)
    gathered = x[torch.tensor(IDX, device=x.device)].contiguous()
    want = ops.zoom_crop(gathered, theta, (24, 40))
    assert torch.equal(torch.ops.rnnpose.zoom_crop(x, theta, [24, 40], torch.tensor(IDX).cuda()), want)
    assert torch.equal(torch.ops.rnnpose.zoom_crop(gathered, theta, [24, 40]), want)


def test_indexed_crop_refuses_an_index_out_of_range_before_launching(ops, monkeypatch):
    x = T(syn.normal("x", (2, 3, 16, 24), 13)).cuda()
    theta = _thetas(3, 7)
    launched = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: (launched.append(name), real(name, *a, **k))[1])
    for bad in ([0, 2, 1], [0, -1, 1], torch.tensor([0, 1, 5]).cuda()):
        with pytest.raises(ValueError):
            ops.zoom_crop(x, theta, (8, 8), src_index=bad)
    with pytest.raises(ValueError):
        ops.zoom_crop(x, theta, (8, 8), src_index=[0, 1])            # two entries for three crops
    with pytest.raises(ValueError):
        ops.zoom_crop(x, theta, (8, 8), src_index=ops.SourceIndex([0, 1, 2], 3, x.device))      # built for three sources
    assert launched == []
    ops.zoom_crop(x, theta, (8, 8), src_index=[0, 1, 1])
    assert launched == ["rnnpose_zoom_crop_indexed_f32"]


# ---- 3: resident attribute tables ---------------------------------------------------------------------------------------------
def _meshes(subs=(1, 2, 3), textured=("b",), seed=0):
    """Ellipsoids of different vertex counts; the classes named in `textured` carry spherical UVs and a noise texture."""
    from rnnpose_amd.eval_epoch import _ellipsoid
    meshes = {}
    for k, (name, sub) in enumerate(zip("abc", subs)):
        verts, faces = _ellipsoid(sub, (0.06 + 0.01 * k, 0.05, 0.04 + 0.005 * k))
        m = dict(verts=verts, faces=faces, colors=syn.uniform(f"col:{name}", (verts.shape[0], 3), seed))
        if name in textured:
            n = verts / np.linalg.norm(verts, axis=1, keepdims=True)
            m.update(verts_uvs=np.stack([np.arctan2(n[:, 1], n[:, 0]) / (2 * np.pi) + 0.5, np.arccos(n[:, 2]) / np.pi], 1)
                     .astype(np.float32), faces_uvs=faces, texture=syn.uniform(f"tex:{name}", (16, 16, 3), seed))
        meshes[name] = m
    return meshes


def _poses(B, seed, z=0.8):
    G = syn.se3_exp_np(syn.normal("g", (B, 6), seed, std=0.4))
    G[:, :3, 3] = syn.uniform("t", (B, 3), seed, -0.02, 0.02) + np.array([0, 0, z])
    return G.astype(np.float32)


@pytest.mark.parametrize("shading,textured", [("flat", ()), ("phong", ("b",))])
def test_resident_attribute_tables_equal_the_explicit_list_bitwise(ops, shading, textured):
    from rnnpose_amd.rasterizer import MeshRenderer
    meshes = _meshes(textured=textured)
    ren = MeshRenderer(meshes, shading=shading)
    C, H, W = 9, 48, 64
    tables = {n: T(syn.normal(f"attr:{n}", (m["verts"].shape[0], C), 3)).cuda() for n, m in meshes.items()}
    assert len({t.shape[0] for t in tables.values()}) == 3
    names = ["c", "a", "b", "a"]
    B = len(names)
    K = T(np.tile(np.array([[300.0, 0, W / 2], [0, 300.0, H / 2], [0, 0, 1]], np.float32), (B, 1, 1))).cuda()
    G = T(_poses(B, 4)).cuda()
    kw = dict(T=G, K=K, render_image_size=(H, W))
    want = {tex: ren(names, [tables[n] for n in names], render_tex=tex, **kw) for tex in (False, True)}
    with pytest.raises(ValueError):
        ren(names, None, **kw)                                       # no resident table yet
    ren.set_vertex_attributes(tables)
    for tex in (False, True):
        got = ren(names, None, render_tex=tex, **kw)
        assert got[0].shape == (B, (3 if tex else 0) + C, H, W) and float((got[1] > 0).float().mean()) > 0.05
        assert torch.equal(got[0], want[tex][0]) and torch.equal(got[1], want[tex][1])
        again = ren(names, [tables[n] for n in names], render_tex=tex, **kw)         # the explicit form still works as before
        assert torch.equal(again[0], want[tex][0])
    ren.set_vertex_attributes({n: tables[n] for n in "ab"})
    with pytest.raises(ValueError):
        ren(names, None, **kw)                                       # class c has no table now
    assert torch.equal(ren(["a", "b"], None, T=G[:2], K=K[:2], render_image_size=(H, W))[0],
                       ren(["a", "b"], [tables["a"], tables["b"]], T=G[:2], K=K[:2], render_image_size=(H, W))[0])
    with pytest.raises(ValueError):
        ren.set_vertex_attributes({"a": tables["a"], "b": tables["b"][:, :5]})       # tables of different C
    with pytest.raises(ValueError):
        ren.set_vertex_attributes({"a": tables["a"][:3]})                            # fewer rows than vertices
    with pytest.raises(ValueError):
        ren.set_vertex_attributes({"nope": tables["a"]})


# ---- 4, 5, 7: PoseRefiner on a mixed-class batch that shares one image ------------------------------------------------------
H0, W0, ZS = 240, 320, (128, 160)


def _frame_scene(seed=3):
    from rnnpose_amd.rasterizer import MeshRenderer
    meshes = _meshes(subs=(2, 3, 1), textured=())
    ren = MeshRenderer({n: meshes[n] for n in "ab"})
    dev = "cuda"
    fea = {n: T(syn.normal(f"f3:{n}", (1, meshes[n]["verts"].shape[0], 256), seed, std=0.5)).to(dev) for n in "ab"}
    geo = {n: T(syn.normal(f"g3:{n}", (1, meshes[n]["verts"].shape[0], 32), seed, std=0.2)).to(dev) for n in "ab"}
    B = 4
    K = np.tile(np.array([[572.4114, 0, W0 / 2], [0, 573.57043, H0 / 2], [0, 0, 1]], np.float32), (B, 1, 1))
    G = _poses(B, seed)
    G[:, 0, 3] += np.array([-0.08, 0.07, 0.02, -0.03], np.float32)                   # four places in the frame
    return dict(renderer=ren, fea=fea, geo=geo, K=T(K).to(dev), G0=T(G).to(dev)[:, None],
                image=T(syn.uniform("image", (1, 3, H0, W0), seed)).to(dev),
                geofea_2d=T(syn.normal("geo2d", (1, 32, H0, W0), seed, std=0.2)).to(dev))


def _refiner(sc, use_graph, outer=2, inner=2):
    from rnnpose_amd.pose_refiner import PoseRefiner, default_config
    cfg = default_config(RENDER_ITER_COUNT=outer, ITER_COUNT=inner, OPTIM_ITER_COUNT=1, render_image_size=(H0, W0), zoom_crop_size=ZS)
    ref = PoseRefiner(cfg, renderer=sc["renderer"], use_graph=use_graph).cuda().eval()
    ref.cf_net.update_block.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
    ref.image_fea_enc.fnet.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
    return ref


def _ts(sc):
    from rnnpose_amd.transformation import SE3Sequence
    return SE3Sequence(matrix=sc["G0"].clone())


def _single_class(ref, sc, n):
    """the four slots as ONE class, image expanded to four copies, through the existing un-indexed path"""
    return ref(sc["image"].expand(4, -1, -1, -1).contiguous(), _ts(sc), sc["K"], fea_3d=sc["fea"][n], obj_cls=[n] * 4,
               geofea_3d=sc["geo"][n], geofea_2d=sc["geofea_2d"].expand(4, -1, -1, -1).contiguous())


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("tables", ["list", "resident"])
def test_mixed_class_shared_image_batch_equals_its_single_class_batches(ops, use_graph, tables):
    """Batch [a, b, a, b] on ONE frame image against the same four slots as two single-class calls of the same batch size:
    slots 0 and 2 must equal the all-a run, slots 1 and 3 the all-b run, bit for bit.  Also: syn_img keeps its length and
    syn_img_tail holds the reference's four extra maps."""
    sc = _frame_scene()
    ref = _refiner(sc, use_graph)
    names = ["a", "b", "a", "b"]
    if tables == "resident":
        sc["renderer"].set_vertex_attributes({n: torch.cat([sc["fea"][n], sc["geo"][n]], -1)[0] for n in "ab"})
        kw = dict(fea_3d=None, geofea_3d=None)
    else:
        kw = dict(fea_3d=[sc["fea"][n][0] for n in names], geofea_3d=[sc["geo"][n][0] for n in names])
    for _ in range(2):                                               # the second call replays whatever was captured
        mixed = ref(sc["image"], _ts(sc), sc["K"], obj_cls=names, geofea_2d=sc["geofea_2d"], image_index=[0, 0, 0, 0], **kw)
    assert float((mixed["syn_depth"][0] > 0).float().mean()) > 0.03 and torch.isfinite(mixed["Ti_pred"].G).all()
    assert len(mixed["syn_img"]) == 2 * 2 and len(mixed["syn_img_tail"]) == 4
    assert all(t.shape == (4, 3, *ZS) for t in mixed["syn_img_tail"])
    for n, slots in (("a", [0, 2]), ("b", [1, 3])):
        single = _single_class(ref, sc, n)
        for key in ("Ti_pred", "flow_last", "weight"):
            got, want = (o[key].G if key == "Ti_pred" else o[key] for o in (mixed, single))
            diff = float((got[slots] - want[slots]).abs().max())
            print(f"graph={use_graph} tables={tables} class {n} {key}: max abs diff {diff:.3e}")
            assert torch.equal(got[slots], want[slots]), (n, key, diff)
        assert len(single["syn_img"]) == 2 * 2 and len(single["syn_img_tail"]) == 4


def test_batches_the_render_hand_off_cannot_serve_raise_before_any_launch(ops, monkeypatch):
    sc = _frame_scene()
    ref = _refiner(sc, use_graph=False)
    names = ["a", "b", "a", "b"]
    fea, geo = [sc["fea"][n][0] for n in names], [sc["geo"][n][0] for n in names]
    launched = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: (launched.append(name), real(name, *a, **k))[1])
    call = lambda **kw: ref(kw.pop("image", sc["image"]), _ts(sc), sc["K"], obj_cls=kw.pop("obj_cls", names),
                            geofea_2d=kw.pop("geofea_2d", sc["geofea_2d"]), **kw)
    with pytest.raises(ValueError):
        call(fea_3d=fea, geofea_3d=geo)                                              # S = 1 < B = 4 without an index
    with pytest.raises(ValueError):
        call(fea_3d=fea[:3], geofea_3d=geo, image_index=[0] * 4)                     # mismatched list lengths
    with pytest.raises(ValueError):
        call(fea_3d=fea, geofea_3d=geo, image_index=[0] * 3)
    with pytest.raises(ValueError):
        call(fea_3d=fea, geofea_3d=geo, image_index=[0, 0, 1, 0])                    # index outside [0, S)
    with pytest.raises(ValueError):
        call(fea_3d=fea, geofea_3d=geo, image_index=[0] * 4, obj_cls=["a", "b", "a", "zebra"])     # unknown class
    with pytest.raises(ValueError):
        call(fea_3d=fea[:3] + [fea[3][:, :100]], geofea_3d=geo, image_index=[0] * 4)               # tables of different C
    with pytest.raises(ValueError):
        call(fea_3d=None, geofea_3d=None, image_index=[0] * 4)                       # no resident tables registered
    with pytest.raises(ValueError):
        call(fea_3d=fea, geofea_3d=geo, image_index=[0] * 4, geofea_2d=sc["geofea_2d"].expand(2, -1, -1, -1))
    assert launched == []


# ---- 6: the frame epoch -----------------------------------------------------------------------------------------------------------
def test_frame_epoch_through_refine_frame(ops):
    """synthetic_scenes, 3 classes, 4 frames x 3 objects: run_epoch(group="frame") through HipEpoch.refine_frame gives the per-class
    counts and (to 1e-12) the initial-pose table of group="class" on the same items; every refined metric of a class with n > 0 is
    finite (the criterion of tests/test_eval_epoch.py; the weights are random, so no improvement is asserted); the 2-D descriptor
    network runs once per frame, not once per item."""
    from rnnpose_amd import eval_epoch as ee
    from rnnpose_amd.descriptor2d import SuperPoint2D
    from rnnpose_amd.pose_refiner import default_config
    torch.manual_seed(0)
    models = ee.synthetic_models(("ape", "cat", "glue"), sub=3)
    cfg = default_config(RENDER_ITER_COUNT=2, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=(240, 320), zoom_crop_size=(128, 128))
    hip = ee.HipEpoch(models, cfg=cfg, desc2d=SuperPoint2D(dict(input_dim=3, descriptor_dim=32, normalize_output=True, use_instance_norm=True), compute_scores=False).cuda().eval())
    hip.refiner.cf_net.update_block.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
    hip.refiner.image_fea_enc.fnet.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
    items = ee.synthetic_scenes(models, 4, 3, image_size=(240, 320), seed=3, renderer=hip.renderer)
    frame0 = items[:3]
    assert all(it.image is frame0[0].image for it in frame0) and float((frame0[0].image > 0).float().mean()) > 0.02
    for it in items:
        it.geofea_2d = None                                          # the epoch computes the descriptors itself
    seen = []
    real = hip.desc2d.descriptors
    hip.desc2d.descriptors = lambda image: (seen.append(int(image.shape[0])), real(image))[1]
    by_frame = ee.run_epoch(items, models, lambda _, batch: hip.refine_frame(batch), hip.metrics, batch_size=4, symmetric=("glue",),
                            group="frame")
    assert sum(seen) == 4 and len(seen) == 4, seen                   # one image per frame: 4, not 12
    assert hip.renderer.has_vertex_attributes(list(models))          # rendered from tables registered once
    seen.clear()
    by_class = ee.run_epoch(items, models, hip.refine, hip.metrics, batch_size=4, symmetric=("glue",))
    assert sum(seen) == 12                                           # what the per-class epoch costs on the same items
    for cls in models:
        assert by_frame["refined"][cls]["n"] == by_class["refined"][cls]["n"] == by_frame["init"][cls]["n"] == 4
        for name, v in by_class["init"][cls].items():
            assert abs(by_frame["init"][cls][name] - v) <= 1e-12, (cls, name)
        assert all(np.isfinite(v) for v in by_frame["refined"][cls].values()), by_frame["refined"][cls]
