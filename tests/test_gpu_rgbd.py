"""The depth-aware LM step (csrc/lm.hip: lm_eq_kernel<DEPTH = true>; rnnpose_lm_normal_eq_rgbd_f64, rnnpose_lm_step_rgbd_io_f32) against the numpy
restatement tests/rgbd_ref.py in fp32 and fp64, its bit-identity with the plain step when the term is off, the two launch forms, exact
recovery of a displaced pose, bad arguments, and the refiner end to end (run with -m gpu on an MI355X; everything but the end-to-end and
dispatcher tests also runs on the host-executed kernels, tests/test_rgbd_on_host.py).

Scenes of the normal-equation cases are built so that every discrete decision of the term -- tap corner, nearest tap, present taps,
edge test, gate, valid mask -- comes out the same in fp32 and fp64 (asserted, `_assert_decisions_are_precision_independent`):
  * the crop map theta and the targets are dyadic, so a target's exact position in the frame lies on a grid that stays 1/128 px (x) and
    1/512 px (y) away from every integer and half-integer, three orders above the fp32 error of the position;
  * observed depths are multiples of 2^-10, so differences of taps are exact and never equal edge_tol = 0.02;
  * the gate compares a continuous quantity; the seeds were checked on the CPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rgbd_ref as rr
from rnnpose_amd import synthetic as syn
from test_gpu_lm_geometry import _clone, _grid, _guarded, _same
from test_gpu_parity import D, N, T, close, ops  # noqa: F401  (ops: the module-scoped build fixture)

pytestmark = pytest.mark.gpu

HO, WO = 48, 64
PARAMS = dict(depth_weight=1.0, depth_gate=0.05, edge_tol=0.02)
# (id, H, W): 8 x 8 has fewer pixels than the workgroup has threads; 64 x 96 two workgroups; 67 x 131 = 8777 px: three workgroups, ragged last trip
CROPS = [("8x8", 8, 8), ("64x96", 64, 96), ("67x131", 67, 131)]
PATTERNS = ["desc", "ones"]


def _theta(B, H, W):
    """crop -> frame maps with ix = (tx + .5)/2 + (ty + .5)/16 + ox, iy = 3 (ty + .5)/8 + 3 (tx + .5)/64 + oy (module docstring)"""
    th = np.zeros((B, 2, 3), np.float64)
    for b in range(B):
        ax, s, ay, sp = 0.5, 1.0 / 16, 3.0 / 8, 3.0 / 64
        ox, oy = 2 + 3 * b + 1.0 / 128 - (6 if W > 100 else 0), 3 + 2 * b + 1.0 / 512          # (the widest crop starts left of the frame)
        th[b] = [[ax * W / WO, s * H / WO, (2.0 / WO) * (ox + 0.5 + ax * W / 2 + s * H / 2) - 1],
                 [sp * W / HO, ay * H / HO, (2.0 / HO) * (oy + 0.5 + ay * H / 2 + sp * W / 2) - 1]]
    return th.astype(np.float32)


def _scene(name, B, H, W, shared, seed):
    """Crop depth: a slanted surface (~20 % background zeros and the top quarter), chosen to agree with the observed frame under the
    crop map; pose exp(xi), xi ~ N(0, 0.01) with tz = 0.01; targets x + flow with flow a multiple of 1/4 px in [-3, 3].  Observed frames:
    the same surface in multiples of 2^-10 with holes (0, negative, NaN, inf), a step edge of 2^-5 and an occluder slab at 0.6."""
    theta = _theta(B, H, W)
    S = 1 if shared else B
    src = [0] * B if shared else None
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cu, cv, z0 = 1.0 / 512, 1.0 / 256, 1.0
    fv, fu = np.meshgrid(np.arange(HO, dtype=np.float64), np.arange(WO, dtype=np.float64), indexing="ij")
    obs = np.zeros((S, HO, WO), np.float32)
    for s in range(S):
        o = np.round((z0 + cu * fu + cv * fv) * 1024) / 1024
        o[:, 40:] += 2.0 ** -5                                           # a step edge above edge_tol
        o[10:21, 10:26] = 0.6                                           # an occluder slab, far outside the gate
        hole = syn.uniform("rg.hole", (HO, WO), seed + s)
        o[hole < 0.03] = 0.0
        o[30, 5], o[31, 7], o[5, 33], o[6, 50] = np.nan, np.inf, -1.0, -np.inf
        obs[s] = o
    depth = np.zeros((B, 1, H, W), np.float32)
    for b in range(B):
        ix, iy = rr.obs_position(xs, ys, H, W, theta[b], HO, WO, np.float64)
        depth[b, 0] = z0 + cu * ix + cv * iy
    sel = syn.uniform("rg.sel", (B, 1, H, W), seed)
    depth[sel > 0.8] = 0.0
    depth[:, :, : H // 4] = 0.0
    K = syn.intrinsics(B, H, W)
    K[:, 0, 0] *= 1.0 + 0.03 * np.arange(B, dtype=np.float32)
    K[:, 0, 2] = 0.43 * W + 1.7
    K[:, 1, 2] = 0.58 * H - 0.6
    K_obs = np.tile(np.array([[60.0, 0, 31.3], [0, 58.0, 23.9], [0, 0, 1]], np.float32), (B, 1, 1))
    K_obs[:, 0, 0] += np.arange(B)
    xi = syn.normal("rg.xi", (B, 6), seed, std=0.01)
    xi[:, 2] = 0.01
    G = syn.se3_exp_np(xi).astype(np.float32).reshape(B, 4, 4)
    flow = (np.round(syn.uniform("rg.flow", (B, 2, H, W), seed, -3.0, 3.0) * 4) / 4).astype(np.float32)
    flow = T(flow)
    absolute = (flow + _grid(H, W)[None]).permute(0, 2, 3, 1).contiguous()
    return dict(depth=T(depth), K=T(K), G=T(G), flow=flow.contiguous(), absolute=absolute, obs=T(obs), src=src, theta=T(theta), K_obs=T(K_obs),
                seed=seed, B=B, H=H, W=W, S=S)


def _weight(pat, s):
    B, H, W = s["B"], s["H"], s["W"]
    if pat == "ones":
        return torch.ones(B, H, W)
    w = T(syn.uniform("rg.w", (B, H, W), s["seed"])) * (s["depth"][:, 0] > 0).float()        # 0 on the background: the top quarter is zero-weight waves
    w[:, H // 2: H // 2 + max(1, H // 8)] = 0.0                                             # and whole zero-weight rows inside the foreground
    return w


def _ref(s, wgt, f, **over):
    p = dict(PARAMS, **over)
    return rr.normal_eq(N(s["absolute"]), N(wgt), N(s["depth"]), N(s["K"]), N(s["G"]), N(s["obs"]), s["src"], N(s["theta"]), N(s["K_obs"]),
                        f=f, want_terms=True, **p)


def _assert_decisions_are_precision_independent(s, t32, t64, what):
    """PRECONDITION (asserted, not skipped): a decision that flips between fp32 and fp64 would make the bound against fp64 meaningless."""
    names = ("valid", "tiny", "mode", "x0", "y0", "east", "south", "active")
    for b, (d32, d64) in enumerate(zip(rr.decisions(t32), rr.decisions(t64))):
        for nm, a32, a64 in zip(names, d32, d64):
            assert np.array_equal(a32, a64), f"{what} image {b}: `{nm}` differs between fp32 and fp64 at {int((a32 != a64).sum())} pixels"


def _coverage(s, terms, what):
    """every path of the sampling rule and of the gate is taken by the scene (the small crop only has to have active pixels)"""
    mode = np.stack([t["mode"] for t in terms])
    act = np.stack([t["active"] for t in terms])
    val = np.stack([t["valid"] for t in terms])
    assert act.any(), what
    if s["H"] * s["W"] >= 4096:
        assert (mode == 0).any() and (mode == 1).any() and (mode == 2).any(), f"{what}: sampling modes {np.unique(mode)}"
        assert ((mode > 0) & val & ~act).any(), f"{what}: nothing is gated out"


def _rgbd_args(s, layout, wgt):
    tgt = s["absolute"] if layout == "absolute" else s["flow"]
    return (_guarded(tgt), _guarded(wgt), _guarded(s["depth"]), D(s["K"]), D(s["G"]), _guarded(s["obs"]), D(s["theta"]), D(s["K_obs"]), s["src"])


def _seed(name, B, shared):
    return (sum(name.encode()) * 7 + 13 * B + (5 if shared else 0)) % 1000


# ------------------------------------------------------------------------------------------------ 1. normal equations against the restatement
@pytest.mark.parametrize("shared", [False, True], ids=["own_frames", "one_shared_frame"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,H,W", CROPS, ids=[c[0] for c in CROPS])
def test_rgbd_normal_eq_vs_restatement(ops, name, H, W, B, shared):
    s = _scene(name, B, H, W, shared, _seed(name, B, shared))
    for pat in PATTERNS:
        wgt = _weight(pat, s)
        oH, ob, od, t32 = _ref(s, wgt, np.float32)
        eH, eb, ed, t64 = _ref(s, wgt, np.float64)
        what0 = f"{name} B={B} shared={shared} {pat}"
        _assert_decisions_are_precision_independent(s, t32, t64, what0)
        _coverage(s, t32, what0)
        pH, pb, _ = rr.normal_eq(N(s["absolute"]), N(wgt), N(s["depth"]), N(s["K"]), N(s["G"]), N(s["obs"]), s["src"], N(s["theta"]), N(s["K_obs"]),
                                 **dict(PARAMS, depth_weight=0.0))
        if pat == "ones":
            assert float(np.abs(oH - pH).max()) > 1e-3 * float(np.abs(oH).max()), f"{what0}: the depth term does not show in H"
        sH, sb = max(1.0, float(np.abs(oH).max())), max(1.0, float(np.abs(ob).max()))
        got = {}
        for layout in ("absolute", "planar"):
            args = _rgbd_args(s, layout, wgt)
            Hm, bv, ds = ops.lm_normal_eq_rgbd(*args, **PARAMS)
            Hm2, bv2, ds2 = ops.lm_normal_eq_rgbd(*args, **PARAMS)
            what = f"{what0} {layout}"
            kH, kb, kd = N(Hm), N(bv), N(ds)
            for b in range(B):
                eoH, ekH = float(np.abs(oH[b] - eH[b]).max()), float(np.abs(kH[b] - eH[b]).max())
                eob, ekb = float(np.abs(ob[b] - eb[b]).max()), float(np.abs(kb[b] - eb[b]).max())
                print(f"RATIO {what} image {b}: H kernel {ekH:.3e} ref32 {eoH:.3e} | b kernel {ekb:.3e} ref32 {eob:.3e} | scale {sH:.3e} {sb:.3e} | "
                      f"active {kd[b, 0]:.0f} cost {kd[b, 1]:.6e}")
            close(Hm, oH, 1e-7 * sH, what=f"H restatement ({what})")
            close(bv, ob, 1e-7 * sb, what=f"b restatement ({what})")
            assert torch.equal(Hm, Hm.transpose(1, 2)), what
            for b in range(B):
                assert float(np.abs(kH[b] - eH[b]).max()) <= 2.0 * float(np.abs(oH[b] - eH[b]).max()) + 1e-7 * sH, f"H exact ({what}, image {b})"
                assert float(np.abs(kb[b] - eb[b]).max()) <= 2.0 * float(np.abs(ob[b] - eb[b]).max()) + 1e-7 * sb, f"b exact ({what}, image {b})"
            assert torch.equal(Hm, Hm2) and torch.equal(bv, bv2) and torch.equal(ds, ds2), f"two launches differ ({what})"
            assert np.array_equal(kd[:, 0], od[:, 0]) and np.array_equal(od[:, 0], ed[:, 0]), f"count of active pixels ({what}): {kd[:, 0]} vs {od[:, 0]}"
            close(ds[:, 1], od[:, 1], 1e-7 * max(1.0, float(od[:, 1].max())), what=f"cost statistic ({what})")
            got[layout] = (Hm, bv, ds)
        assert all(torch.equal(a, b) for a, b in zip(got["absolute"], got["planar"])), f"layouts differ ({what0})"


# ------------------------------------------------------------------------------------------------ 2. the term off == the plain step, bit for bit
def _step_out(ops, args, iters, **kw):
    return _clone(ops.lm_step_rgbd(*args, num_iters=iters, **kw))


@pytest.mark.parametrize("name,H,W", CROPS, ids=[c[0] for c in CROPS])
def test_rgbd_term_off_is_the_plain_step_bit_for_bit(ops, name, H, W):
    B = 3
    s = _scene(name, B, H, W, False, _seed(name, B, False))
    wgt = _weight("desc", s)
    nan_obs = s["obs"].clone()
    nan_obs[:, ::2] = float("nan")
    nan_obs[:, 1::2, ::3] = float("inf")
    nan_obs[:, 1::2, 1::3] = -float("inf")
    nan_obs[:, 1::2, 2::3] = -2.0
    for layout in ("absolute", "planar"):
        args = _rgbd_args(s, layout, wgt)
        plain_eq = ops.lm_normal_eq(*args[:5], eps=1e-5)
        empty = torch.zeros_like(args[5])
        for what, a, kw in (("depth_weight = 0", args, dict(PARAMS, depth_weight=0.0)),
                            ("all-zero observed depth", args[:5] + (empty,) + args[6:], PARAMS),
                            ("non-finite observed depth", args[:5] + (_guarded(nan_obs),) + args[6:], dict(PARAMS, depth_weight=3.0))):
            Hm, bv, ds = ops.lm_normal_eq_rgbd(*a, **kw)
            assert _same((Hm, bv), plain_eq), f"{name} {layout}: normal equations with {what}"
            assert torch.isfinite(Hm).all() and torch.isfinite(bv).all() and torch.isfinite(ds).all()
            if what != "depth_weight = 0":
                assert float(ds.abs().max()) == 0.0, f"{name} {layout} {what}: statistics {ds}"
            else:
                assert float(ds[:, 0].min()) > 0 and float(ds[:, 1].abs().max()) == 0.0
            for iters in (1, 3):
                plain = _clone(ops.lm_step(*args[:5], num_iters=iters))
                got = _step_out(ops, a, iters, **kw)
                assert _same(got[:5], plain), f"{name} {layout} iters={iters}: step with {what}"
                assert all(bool(torch.isfinite(x).all()) for x in got[:4] + got[5:])


# ------------------------------------------------------------------------------------------------ 3. launch forms
CANARY = 1234.5


def _out_views6(B):
    """the six outputs of lm_step_rgbd as views into ONE canary-filled fp64 buffer, four doubles apart"""
    sizes = [8 * B, 36 * B, 6 * B, 3 * B, (B + 1) // 2, 2 * B]
    buf = torch.full((sum(sizes) + 4 * (len(sizes) + 1),), CANARY, dtype=torch.float64, device="cuda")
    outside = torch.ones(buf.numel(), dtype=torch.bool)
    off, seg = 4, []
    for n in sizes:
        seg.append(buf[off:off + n])
        outside[off:off + n] = False
        off += n + 4
    views = (seg[0].view(torch.float32).view(B, 4, 4), seg[1].view(B, 6, 6), seg[2].view(B, 6), seg[3].view(torch.float32).view(B, 6),
             seg[4].view(torch.int32)[:B], seg[5].view(B, 2))
    return buf, views, outside


@pytest.mark.parametrize("shared", [False, True], ids=["own_frames", "one_shared_frame"])
@pytest.mark.parametrize("name,H,W", CROPS, ids=[c[0] for c in CROPS])
def test_rgbd_step_forms_and_slots_are_bit_identical(ops, name, H, W, shared):
    B = 3
    s = _scene(name, B, H, W, shared, _seed(name, B, shared))
    wgt = _weight("desc", s)
    for layout in ("absolute", "planar"):
        args = _rgbd_args(s, layout, wgt)
        ops.lm_fused_tail(True)
        for iters in (1, 3):
            fused = _step_out(ops, args, iters, **PARAMS)
            ops.lm_fused_tail(False)
            try:
                unfused = _step_out(ops, args, iters, **PARAMS)
            finally:
                ops.lm_fused_tail(True)
            assert _same(fused, unfused), f"{name} {layout} iters={iters}: fused tail != three launches"
            assert _same(fused, _step_out(ops, args, iters, **PARAMS)), f"{name} {layout} iters={iters}: third call differs (ticket reset)"
            assert int(fused[4].abs().sum()) == 0 and float(fused[5][:, 0].max()) > 0        # (the 8 x 8 crops of some images see no gated depth)
            if iters == 1:                                              # one step == normal equations + the solve of the plain path
                Hm, bv, ds = ops.lm_normal_eq_rgbd(*args, **PARAMS)
                Gn, xi, info = ops.lm_solve_update(Hm, bv, args[4])
                assert _same((fused[1], fused[2], fused[5]), (Hm, bv, ds)) and _same((fused[0], fused[3], fused[4]), (Gn, xi, info))
            # out= views with canaries around them; sub-ranges of the batch in their own workspace slots (the refiner's batch halves)
            buf, views, outside = _out_views6(B)
            got = ops.lm_step_rgbd(*args, num_iters=iters, out=views, **PARAMS)
            assert _same(got, fused) and bool((buf.cpu()[outside] == CANARY).all()), f"{name} {layout} iters={iters}: out= views"
            buf, views, outside = _out_views6(B)
            src = ops.SourceIndex(s["src"], s["S"], "cuda") if shared else None
            for b0, b1 in ((0, 2), (2, 3)):
                sub = tuple(a[b0:b1] for a in args[:5])
                obs = args[5] if shared else args[5][b0:b1]
                ops.lm_step_rgbd(*sub, obs, args[6][b0:b1], args[7][b0:b1], src, num_iters=iters, out=tuple(v[b0:b1] for v in views), slot=b0,
                                 index_rows=(b0, b1) if shared else None, **PARAMS)
            assert _same(views, fused) and bool((buf.cpu()[outside] == CANARY).all()), f"{name} {layout} iters={iters}: slot sub-ranges"


# ------------------------------------------------------------------------------------------------ 4. exact recovery
def _sphere_plane_depth(K, H, W, centre, radius, plane_z):
    """analytic z-buffer of a sphere in front of a fronto-parallel plane, at pixel centres = integer pixel indices (fp64)"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)           # ray with z = 1
    a = (d * d).sum(-1)
    bq = d @ centre
    disc = bq * bq - a * (centre @ centre - radius * radius)
    z = np.where(disc > 0, (bq - np.sqrt(np.maximum(disc, 0))) / a, plane_z)
    return z, disc > 0


def test_rgbd_exact_recovery_of_a_displaced_pose(ops):
    """A sphere in front of a plane, rendered where the estimate stands (G = identity); targets and observed depth are those of the
    scene displaced by G*, whose tz is ten times its lateral part.  The crop is the frame (theta = identity), weights are 1 on the plane
    and on the sphere's cap (away from the silhouette, where no interpolation of a depth image is exact).  Iterating the step reaches
    G* to the 1e-5 of test_gpu_parity.test_lm_exact_target_recovery_and_facade; the cost statistic falls monotonically."""
    H, W = 96, 128
    K = np.array([[140.0, 0, 63.5], [0, 140.0, 47.5], [0, 0, 1]], np.float64)
    centre, radius, plane_z = np.array([0.02, -0.01, 1.0]), 0.2, 1.3
    dep, on_sphere = _sphere_plane_depth(K, H, W, centre, radius, plane_z)
    xi = np.array([[0.004, -0.003, 0.04, 0.01, -0.015, 0.02]])
    Gs = syn.se3_exp_np(xi)[0]
    # the scene's points in the first camera, displaced: exact correspondences and exact depth of the displaced points
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    Z0 = dep + 1e-5
    P0 = np.stack([Z0 * (xs - K[0, 2]) / K[0, 0], Z0 * (ys - K[1, 2]) / K[1, 1], Z0], -1)
    P1 = P0 @ Gs[:3, :3].T + Gs[:3, 3]
    target = np.stack([K[0, 0] * P1[..., 0] / P1[..., 2] + K[0, 2], K[1, 1] * P1[..., 1] / P1[..., 2] + K[1, 2]], -1)
    # the observed frame: the displaced scene's analytic z-buffer (the plane tilts with G*: exact per pixel through its own ray)
    cs = Gs[:3, :3] @ centre + Gs[:3, 3]
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)
    a, bq = (d * d).sum(-1), d @ cs
    disc = bq * bq - a * (cs @ cs - radius * radius)
    n, p0 = Gs[:3, :3] @ np.array([0, 0, 1.0]), Gs[:3, :3] @ np.array([0, 0, plane_z]) + Gs[:3, 3]
    obs = np.where(disc > 0, (bq - np.sqrt(np.maximum(disc, 0))) / a, (n @ p0) / (d @ n))
    rho = np.linalg.norm(P0[..., :2] - centre[:2], axis=-1)
    wgt = np.where(on_sphere, rho < 0.6 * radius, rho > 1.5 * radius).astype(np.float32)
    args = (D(target[None].astype(np.float32)), D(wgt[None]), D(dep[None, None].astype(np.float32)), D(K[None].astype(np.float32)))
    depth_args = (D(obs[None].astype(np.float32)), D(np.array([[[1, 0, 0], [0, 1, 0]]], np.float32)), D(K[None].astype(np.float32)), None)
    G = torch.eye(4, device="cuda")[None].clone()
    errs, costs, moved = [], [], []
    for k in range(8):
        G, Hm, bv, xi_k, info, ds = ops.lm_step_rgbd(*args, G, *depth_args, num_iters=1, **PARAMS)
        errs.append(float(np.abs(N(G)[0] - Gs).max()))
        costs.append(float(ds[0, 1]))                                   # (the statistic belongs to the pose BEFORE the step)
        moved.append(float(xi_k.abs().max()))
        print(f"RECOVERY step {k}: max |G - G*| {errs[-1]:.3e}  |xi| {moved[-1]:.3e}  active {float(ds[0, 0]):.0f}  cost {costs[-1]:.6e}")
        assert int(info.abs().sum()) == 0
    assert errs[-1] < 1e-5 and errs[0] > errs[1], errs
    # monotone for as long as the steps move the pose by more than the 1e-5 the pose is compared at; below that the cost sits on the
    # interpolation error of the depth image, which no pose removes
    falls = [costs[k + 1] < costs[k] for k in range(7) if moved[k] > 1e-5]
    assert len(falls) >= 2 and all(falls), (costs, moved)
    assert float(ds[0, 0]) > 0.5 * float(wgt.sum())


# ------------------------------------------------------------------------------------------------ 5. bad arguments
def test_rgbd_bad_arguments(ops):
    from rnnpose_amd import _lib
    import rnnpose_amd.torch_ops  # noqa: F401
    lib = _lib.load()
    B, H, W = 2, 8, 8
    s = _scene("8x8", B, H, W, False, 1)
    wgt = _weight("ones", s)
    t, w, d, K, G, obs, th, Ko = (D(x) for x in (s["absolute"], wgt, s["depth"], s["K"], s["G"], s["obs"], s["theta"], s["K_obs"]))
    idx = torch.zeros(B, dtype=torch.int32).cuda()
    n = int(lib.rnnpose_lm_workspace_bytes(B, H, W))
    ws = torch.zeros(n // 8, dtype=torch.float64).cuda()
    Hm, bv = torch.full((B, 6, 6), 7.0, dtype=torch.float64).cuda(), torch.full((B, 6), 7.0, dtype=torch.float64).cuda()
    Gn, xi, info = torch.full((B, 4, 4), 7.0).cuda(), torch.full((B, 6), 7.0).cuda(), torch.full((B,), 7, dtype=torch.int32).cuda()
    ds = torch.full((B, 2), 7.0, dtype=torch.float64).cuda()
    ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)
    nan, inf = float("nan"), float("inf")

    def eq(o=obs, si=None, tt=th, ko=Ko, S=B, dw=1.0, dg=0.05, et=0.02):
        return lib.rnnpose_lm_normal_eq_rgbd_f64(ptr(t), 0, ptr(w), ptr(d), 1e-5, ptr(K), ptr(G), B, H, W, ptr(o), ptr(si), ptr(tt), ptr(ko), S, HO, WO,
                                                 dw, dg, et, ptr(ws), n, ptr(Hm), ptr(bv), ptr(ds), ops._stream())

    def step(o=obs, si=None, tt=th, ko=Ko, S=B, dw=1.0, dg=0.05, et=0.02):
        return lib.rnnpose_lm_step_rgbd_io_f32(ptr(t), 0, ptr(w), ptr(d), 1e-5, ptr(K), ptr(G), ptr(Gn), B, H, W, 1, 100.0, 1e-4, 1.0, ptr(o), ptr(si),
                                               ptr(tt), ptr(ko), S, HO, WO, dw, dg, et, ptr(ws), n, ptr(Hm), ptr(bv), ptr(xi), ptr(info), ptr(ds),
                                               ops._stream())
    cases = [(dict(o=None), b"null"), (dict(tt=None), b"null"), (dict(ko=None), b"null"), (dict(S=0), b"S >= 1"), (dict(S=-1), b"S >= 1"),
             (dict(S=1), b"src_index"), (dict(S=B + 1), b"src_index")]
    for key, msg in (("dw", b"depth_weight"), ("dg", b"depth_gate"), ("et", b"edge_tol")):
        cases += [({key: v}, msg) for v in (-1.0, -1e-30, nan, inf, -inf)]
    for fn in (eq, step):
        for kw, msg in cases:
            assert fn(**kw) == 1 and msg in lib.rnnpose_last_error(), (fn.__name__, kw, lib.rnnpose_last_error())
    torch.cuda.synchronize()
    assert all(bool((x == 7).all()) for x in (Hm, bv, Gn, xi, info, ds)) and not bool(ws.any())      # refused before any launch
    assert eq(S=1, si=idx) == 0 and eq(dw=0.0, dg=0.0, et=0.0) == 0 and step(S=1, si=idx) == 0          # (the accepted edges of the same list)
    torch.cuda.synchronize()
    # the Python layer refuses the same on the host, before any launch
    a = (t, w, d, K, G)
    for fn in (ops.lm_normal_eq_rgbd, ops.lm_step_rgbd):
        with pytest.raises(ValueError, match="frame per object"):
            fn(*a, obs[:1], th, Ko)
        with pytest.raises(ValueError, match="src_index"):
            fn(*a, obs, th, Ko, [0, 2])
        with pytest.raises(ValueError, match="src_index"):
            fn(*a, obs, th, Ko, [0])
        with pytest.raises(ValueError, match="theta"):
            fn(*a, obs, th[:1], Ko)
        with pytest.raises(ValueError, match="K_obs"):
            fn(*a, obs, th, Ko[:1])
        with pytest.raises(ValueError, match="obs_depth"):
            fn(*a, obs[0, 0], th, Ko)
        for key in ("depth_weight", "depth_gate", "edge_tol"):
            for v in (-1.0, nan, inf):
                with pytest.raises(ValueError, match=key):
                    fn(*a, obs, th, Ko, **{key: v})
    with pytest.raises(ValueError, match="num_iters"):
        ops.lm_step_rgbd(*a, obs, th, Ko, num_iters=0)
    for bad in (dict(depth_weight=-1.0), dict(depth_gate=nan), dict(gate=0.1)):
        with pytest.raises(ValueError):
            ops.depth_term_params(bad)
    assert ops.depth_term_params(None) is None and ops.depth_term_params(True) == PARAMS and ops.depth_term_params({"depth_gate": 0.1})["depth_gate"] == 0.1
    # the dispatcher has no CPU kernel: tensors that are not on the GPU never reach the library
    cpu = [x.detach().cpu() for x in (t, w, d, K, G, obs, th, Ko)]
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.rnnpose.lm_step_rgbd(*cpu)


def test_rgbd_dispatcher_op_and_fake_kernel(ops):
    import rnnpose_amd.torch_ops  # noqa: F401
    B, H, W = 3, 64, 96
    s = _scene("64x96", B, H, W, True, _seed("64x96", B, True))
    wgt = _weight("desc", s)
    t, w, d, K, G, obs, th, Ko = (D(x) for x in (s["flow"], wgt, s["depth"], s["K"], s["G"], s["obs"], s["theta"], s["K_obs"]))
    src = torch.tensor(s["src"], device="cuda")
    want = ops.lm_step_rgbd(t, w, d, K, G, obs, th, Ko, s["src"], num_iters=2, **PARAMS)
    Gn, xi, ds = torch.ops.rnnpose.lm_step_rgbd(t, w, d, K, G, obs, th, Ko, src, 1.0, 0.05, 0.02, 2)
    assert _same((Gn, xi, ds), (want[0], want[3], want[5]))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        fk = [mode.from_tensor(x) for x in (t, w, d, K, G, obs, th, Ko)]
        fG, fxi, fds = torch.ops.rnnpose.lm_step_rgbd(*fk)
    assert (fG.shape, fxi.shape, fds.shape) == (Gn.shape, xi.shape, ds.shape) and (fG.dtype, fxi.dtype, fds.dtype) == (Gn.dtype, xi.dtype, ds.dtype)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_rgbd_end_to_end_refine_frame(ops):
    """synthetic_scenes, 2 frames x 3 objects at 240 x 320, observed depth = the frames' z-buffer at the ground-truth poses (the
    project's rasteriser); initial poses = ground truth moved 3 cm along the optical axis (alternating sign).  HipEpoch.refine_frame:
    graph replay == eager bit for bit with the term on; the term off (no depth_term, or depth_weight = 0) == a refiner constructed
    without it; with the term on the mean |tz| error over the six objects is smaller than with it off (random network weights: the
    comparison is against the term-off run of the same call, not against a fixed value).
    Measured on one MI355X: mean |tz| error 0.0336 with the term off, 0.0089 with it on (initial 0.0300)."""
    from oracle import rnnpose_oracle as orc
    from rnnpose_amd import eval_epoch as ee
    from rnnpose_amd.pose_refiner import default_config
    torch.manual_seed(0)
    models = ee.synthetic_models(("ape", "cat", "glue"), sub=3)
    cfg = lambda **kw: default_config(RENDER_ITER_COUNT=2, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=(240, 320), zoom_crop_size=(128, 128), **kw)

    def epoch(use_graph=True, **kw):
        hip = ee.HipEpoch(models, cfg=cfg(), **kw)
        hip.refiner.use_graph = use_graph
        hip.refiner.cf_net.update_block.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
        hip.refiner.image_fea_enc.fnet.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
        return hip

    plain = epoch()
    items = ee.synthetic_scenes(models, 2, 3, image_size=(240, 320), seed=3, renderer=plain.renderer)
    for j, it in enumerate(items):
        assert it.depth is not None and float((it.depth > 0).float().mean()) > 0.01
        it.pose_init = it.pose_gt.copy()
        it.pose_init[2, 3] += 0.03 if j % 2 == 0 else -0.03
    gt_z = np.array([it.pose_gt[2, 3] for it in items])
    tz_err = lambda P: np.abs(N(P)[:, 2, 3].astype(np.float64) - gt_z)

    off = plain.refine_frame(items).clone()
    assert plain.last_depth_stats is None
    on_epoch = epoch(depth_term=True)
    on = on_epoch.refine_frame(items).clone()
    stats = on_epoch.last_depth_stats.clone()
    on_replay = on_epoch.refine_frame(items).clone()                    # a second call replays the captured graphs
    on_eager = epoch(use_graph=False, depth_term=True).refine_frame(items)
    assert torch.equal(on, on_eager) and torch.equal(on_replay, on_eager), "graph replay != eager launches with the depth term"
    ref = on_epoch.refiner
    assert ref.use_graph and (ref._graph is not None or ref._graph_static is not None), "the depth-aware loop was not captured"
    assert stats.shape == (6, 2) and stats.dtype == torch.float64 and float(stats[:, 0].min()) > 0 and bool(torch.isfinite(stats).all())
    # the term off
    assert torch.equal(epoch(depth_term=None).refine_frame(items), off)
    zero = epoch(depth_term=dict(depth_weight=0.0))
    assert torch.equal(zero.refine_frame(items), off), "depth_weight = 0 != the refiner without the term"
    assert float(zero.last_depth_stats[:, 0].min()) > 0 and float(zero.last_depth_stats[:, 1].abs().max()) == 0.0
    # items without depth: a clear error when the term is on, nothing changes when it is off
    bare = [ee.EvalItem(it.class_name, it.image, it.K, it.pose_init, it.pose_gt, it.geofea_2d, frame_id=it.frame_id) for it in items]
    with pytest.raises(ValueError, match="depth"):
        on_epoch.refine_frame(bare)
    assert torch.equal(plain.refine_frame(bare), off)
    e_off, e_on = tz_err(off), tz_err(on)
    print(f"END_TO_END mean |tz| error: initial 0.03, term off {e_off.mean():.6f}, term on {e_on.mean():.6f}; per object off {np.round(e_off, 5)} on {np.round(e_on, 5)}")
    assert bool(torch.isfinite(on).all()) and e_on.mean() < e_off.mean(), (e_on, e_off)
