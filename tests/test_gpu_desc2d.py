"""SuperPoint2D on the HIP kernels (rnnpose_amd/descriptor2d.py): against the reference's own outputs (tests/golden/desc2d.npz,
tests/golden/gen_golden_desc2d.py), against an fp64 restatement at the LINEMOD image size, and the three glue kernels on their own
(maxpool2x2_nhwc, upsample2x_nhwc, pixel_head_nhwc).  Run with -m gpu; tests/test_desc2d_on_host.py runs a subset on the
host-executed kernels."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rnnpose_amd import synthetic as syn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_golden_desc2d as gen  # noqa: E402  (seeds, shapes and config of the fixture; the reference is imported only by its main())


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rnnpose_amd import build, ops as _ops
    build.build()
    return _ops


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def maxabs(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


def make_net(compute_scores=True, chunk=None, config=None):
    from rnnpose_amd.descriptor2d import SuperPoint2D
    net = SuperPoint2D(dict(config or gen.CONFIG), compute_scores=compute_scores, chunk=chunk)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gen.weights(shapes).items()}, strict=True)
    return net.cuda().eval()


def restate_fp64(net, image, scores=True):
    """model/descriptor2D.py:113-173 in float64 on the CPU from the module's own parameters."""
    p = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    conv = lambda x, k: F.conv2d(x, p[k + ".weight"], p[k + ".bias"], padding=p[k + ".weight"].shape[-1] // 2)
    up = lambda x: F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    x = torch.as_tensor(image).detach().cpu().double()
    skips = []
    for i, (a, b) in enumerate((("conv1a", "conv1b"), ("conv2a", "conv2b"), ("conv3a", "conv3b"), ("conv4a", "conv4b"))):
        x = F.relu(conv(F.relu(conv(x, a)), b))
        if i < 3:
            skips.append(x)
            x = F.max_pool2d(x, 2, 2)
    x = F.relu(F.instance_norm(conv(up(x), "decode1.1"), eps=1e-5))
    x = F.relu(F.instance_norm(conv(up(torch.cat([x, skips[2]], 1)), "decode2.1"), eps=1e-5))
    x = F.relu(F.instance_norm(conv(up(torch.cat([x, skips[1]], 1)), "decode3.1"), eps=1e-5))
    d = F.normalize(conv(F.relu(conv(x, "convDa")), "convDb"), p=2, dim=1)
    s = torch.sigmoid(conv(F.relu(F.instance_norm(conv(x, "convPa.0"), eps=1e-5)), "convPb")) if scores else None
    return d, s


# ------------------------------------------------------------------------------------------------ 1. fixture parity
@pytest.mark.parametrize("case", ["a", "b"])
def test_desc2d_matches_the_reference_fixture(ops, golden, case):
    """Descriptors and scores against the reference's fp32 outputs: max |d| <= 1e-4.  Should that fail, the gate is the one of
    test_gpu_parity's encoder at gain 1: no further from the fp64 restatement than max(1e-4, the fixture's own distance from it)."""
    g = golden("desc2d")
    net = make_net()
    img = gen.image(case)
    out = net(D(img))
    torch.cuda.synchronize()
    desc = gen.descriptor_sample(case, out["descriptors"])              # (the fixture's pixel lattice)
    dd = maxabs(desc, g[f"{case}_descriptors"])
    ds = maxabs(out["scores"], g[f"{case}_scores"])
    print(f"case {case}: max|desc - ref| {dd:.3e}  max|scores - ref| {ds:.3e}")
    if dd <= 1e-4 and ds <= 1e-4:
        return
    d64, s64 = restate_fp64(net, img)
    for what, got, ref, want in (("descriptors", desc, g[f"{case}_descriptors"], gen.descriptor_sample(case, d64)),
                                 ("scores", out["scores"], g[f"{case}_scores"], s64)):
        e_gpu, e_ref = maxabs(got, want), maxabs(ref, want)
        print(f"case {case} {what}: |gpu - fp64| {e_gpu:.3e}  |ref fp32 - fp64| {e_ref:.3e}")
        assert e_gpu <= max(1e-4, e_ref), (what, e_gpu, e_ref)


# ------------------------------------------------------------------------------------------------ 2. LINEMOD size
def test_desc2d_linemod_size_vs_fp64(ops):
    """B = 2 at 480 x 640 (the LINEMOD image) against the fp64 restatement: descriptors within 1e-4; no range-guard events."""
    ops.saturation_count(reset=True)
    net = make_net()
    img = syn.uniform("desc2d_linemod", (2, 3, 480, 640), 7) * 255.0        # raw image values, as RNNPose.forward passes them
    out = net(D(img))
    torch.cuda.synchronize()
    d64, s64 = restate_fp64(net, img)
    dd, ds = maxabs(out["descriptors"], d64), maxabs(out["scores"], s64)
    print(f"480x640: max|desc - fp64| {dd:.3e}  max|scores - fp64| {ds:.3e}")
    assert dd <= 1e-4
    assert ds <= 1e-4
    assert int(out["f16x3_range_events"].item()) == 0


# ------------------------------------------------------------------------------------------------ 3. the kernels alone
@pytest.mark.parametrize("B,H,W,cs,co,C,dcs,dco", [(2, 8, 12, 64, 0, 64, 64, 0), (1, 11, 9, 136, 4, 128, 132, 4), (3, 6, 14, 12, 8, 4, 8, 0)])
def test_maxpool2x2_is_max_pool2d(ops, B, H, W, cs, co, C, dcs, dco):
    x = D(syn.normal("mp", (B, H, W, cs), 1))
    dst = torch.full((B, H // 2, W // 2, dcs), 7.0, device="cuda")
    ops.maxpool2x2_nhwc(x, dst, src_c_offset=co, c_count=C, dst_c_offset=dco)
    want = F.max_pool2d(x[..., co:co + C].permute(0, 3, 1, 2).cpu(), 2, 2).permute(0, 2, 3, 1)
    got = dst.cpu()
    assert torch.equal(got[..., dco:dco + C], want)
    assert bool((got[..., :dco] == 7.0).all()) and bool((got[..., dco + C:] == 7.0).all())


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("B,h,w,cs,co,C,dcs,dco", [(2, 5, 7, 128, 0, 128, 192, 0), (1, 3, 1, 72, 8, 64, 192, 128), (2, 1, 4, 8, 4, 4, 12, 4)])
def test_upsample2x_is_interpolate(ops, norm, B, h, w, cs, co, C, dcs, dco):
    x = D(syn.normal("up", (B, h, w, cs), 2, std=2.0))
    mr = None
    src = x[..., co:co + C].permute(0, 3, 1, 2).cpu()
    if norm:                                # the taps as the kernel forms them (fp32), the interpolation in fp64
        mean = syn.normal("upm", (B, C), 3)
        rstd = syn.uniform("upr", (B, C), 3, 0.2, 2.0)
        mr = D(np.stack([mean, rstd], -1))
        src = F.relu((src - torch.from_numpy(mean)[..., None, None]) * torch.from_numpy(rstd)[..., None, None])
    src = src.double()
    dst = torch.full((B, 2 * h, 2 * w, dcs), 7.0, device="cuda")
    ops.upsample2x_nhwc(x, dst, src_c_offset=co, c_count=C, dst_c_offset=dco, mean_rstd=mr, relu=norm)
    want = F.interpolate(src, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    got = dst.cpu()
    assert maxabs(got[..., dco:dco + C], want) <= 1e-6
    assert bool((got[..., :dco] == 7.0).all()) and bool((got[..., dco + C:] == 7.0).all())


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,H,W,cs,co,cin,cout,norm", [(2, 9, 13, 256, 0, 256, 32, False), (1, 7, 10, 264, 8, 256, 1, True),
                                                         (2, 5, 6, 100, 4, 96, 20, True)])
def test_pixel_head_vs_fp64(ops, mode, B, H, W, cs, co, cin, cout, norm):
    x = syn.normal("ph", (B, H, W, cs), 4)
    x[0, 1, 2] = 0.0                                       # an all-zero pixel: with a zero bias, L2 mode hits the 1e-12 clamp
    wt = syn.normal("phw", (cout, cin), 4, std=float(np.sqrt(2.0 / cin)))
    bias = syn.uniform("phb", (cout,), 4, -0.05, 0.05) * (mode != 1)
    src = torch.from_numpy(x[..., co:co + cin]).double()
    mr = None
    if norm:
        mean, rstd = syn.normal("phm", (B, cin), 5), syn.uniform("phr", (B, cin), 5, 0.5, 2.0)
        mr = D(np.stack([mean, rstd], -1))
        src = F.relu((src - torch.from_numpy(mean).double()[:, None, None]) * torch.from_numpy(rstd).double()[:, None, None])
    y = src @ torch.from_numpy(wt).double().t() + torch.from_numpy(bias).double()
    if mode == 1:
        y = F.normalize(y, p=2, dim=-1, eps=1e-12)
    elif mode == 2:
        y = torch.sigmoid(y)
    want = y.permute(0, 3, 1, 2)
    got = ops.pixel_head_nhwc(D(x), D(wt), D(bias), mode, src_c_offset=co, c_in=cin, mean_rstd=mr, relu=norm)
    assert maxabs(got, want) <= 1e-5
    if mode == 1 and not norm:
        assert bool((got[0, :, 1, 2] == 0).all())


# ------------------------------------------------------------------------------------------------ 4. descriptors only, chunking
def test_desc2d_descriptors_only_and_chunking_are_bit_identical(ops):
    img = D(syn.uniform("desc2d_chunk", (5, 3, 48, 64), 8) * 255.0)
    full = make_net(compute_scores=True, chunk=5)(img)
    only = make_net(compute_scores=False, chunk=5)(img)
    assert only["scores"] is None
    assert torch.equal(only["descriptors"], full["descriptors"])
    c2 = make_net(compute_scores=True, chunk=2)(img)
    assert torch.equal(c2["descriptors"], full["descriptors"]) and torch.equal(c2["scores"], full["scores"])
    assert torch.equal(make_net(chunk=2).descriptors(img), full["descriptors"])


# ------------------------------------------------------------------------------------------------ 5. API
def test_desc2d_api(ops, golden):
    from rnnpose_amd.descriptor2d import SuperPoint2D
    net = make_net()
    assert sorted(net.state_dict().keys()) == list(golden("desc2d")["keys"])
    # non-strict load: shape-mismatched keys are skipped, the rest loads
    before = net.convDb.weight.detach().clone()
    bad = {"convDb.weight": torch.zeros(64, 256, 1, 1), "conv1a.bias": torch.full((64,), 0.5), "unknown.weight": torch.zeros(3)}
    net.load_state_dict(bad, strict=False)
    assert torch.equal(net.convDb.weight.detach(), before)
    assert bool((net.conv1a.bias.detach() == 0.5).all())
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 60, 64, device="cuda"))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 64, 63, device="cuda"))
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 64, 64))
    for bad_cfg in (dict(input_dim=1), dict(use_instance_norm=False), dict(saliency_score_normalization_fuc="softmax")):
        with pytest.raises(NotImplementedError):
            SuperPoint2D(dict(gen.CONFIG, **bad_cfg))
    # normalize_output=False: the linear head
    lin = make_net(config=dict(gen.CONFIG, normalize_output=False))
    img = gen.image("b")
    d64, _ = restate_fp64(lin, img, scores=False)
    raw = lin.descriptors(D(img))
    assert maxabs(F.normalize(raw.double().cpu(), p=2, dim=1), d64) <= 1e-4
    assert float((raw.norm(dim=1) - 1).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------------ 6. eval hook
def test_hip_epoch_computes_missing_descriptors(ops):
    from rnnpose_amd import eval_epoch as ee
    from rnnpose_amd.pose_refiner import default_config
    models = ee.synthetic_models(("ape",), sub=2)
    net = make_net(compute_scores=False)
    cfg = default_config(RENDER_ITER_COUNT=1, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=(240, 320), zoom_crop_size=(128, 128))
    ep = ee.HipEpoch(models, cfg=cfg, desc2d=net)
    plain = ee.HipEpoch(models, cfg=cfg, refiner=ep.refiner)
    items = ee.synthetic_dataset(models, 2, image_size=(240, 320), seed=3, renderer=ep.renderer)
    image = torch.stack([it.image for it in items]).cuda()
    want = net.descriptors(image)
    # items that keep geofea_2d: the same poses as without desc2d
    assert torch.equal(ep.refine("ape", items), plain.refine("ape", items))
    # items without: descriptors of the stacked batch image, exactly
    given = [ee.EvalItem(it.class_name, it.image, it.K, it.pose_init, it.pose_gt, want[j].cpu()) for j, it in enumerate(items)]
    none = [ee.EvalItem(it.class_name, it.image, it.K, it.pose_init, it.pose_gt, None) for it in items]
    assert torch.equal(ep.refine("ape", none), plain.refine("ape", given))
    mixed = [none[0], given[1]]
    assert torch.equal(ep.refine("ape", mixed), plain.refine("ape", given))
    with pytest.raises(ValueError):
        plain.refine("ape", none)
