"""The LM pose step and the per-pixel geometry kernels across launch geometry and regimes (run with -m gpu on an MI355X; the small
shapes also run on the host-executed kernels, tests/test_kernels_on_host.py).

tests/test_gpu_parity.py meets the oracle at ONE shape (B = 2, 64 x 96: two workgroups per image, absolute targets, a 0.03 pose).  Here
every shape is chosen for a code path of csrc/lm.hip / pointwise.hip (see SHAPES), every case runs in both target layouts and at two
pose scales, and every input is seeded by rnnpose_amd.synthetic and checked against oracle/rnnpose_oracle.py -- in fp32 (the project's
tolerances) and against the same oracle evaluated in fp64 (`orc.precision`), the value both fp32 evaluations approximate.

Tests whose name contains `full_size` are the large shapes: the host tier leaves them out by that keyword.
"""
import numpy as np
import pytest
import torch

from oracle import rnnpose_oracle as orc
from rnnpose_amd import synthetic as syn
from test_gpu_parity import D, N, T, close, ops  # noqa: F401  (ops: the module-scoped build fixture)

pytestmark = pytest.mark.gpu

# (id, B, H, W): the path of csrc/lm.hip a shape is here for.  LM_PIX_PER_BLOCK = 4096, LM_THREADS = 256, LM_BATCH = 8, LM_MAX_BLOCKS = 256.
# No 2 x 2 shape: ops._target_mode cannot tell (B,2,2,2) absolute from (B,2,2,2) planar -- the two layouts are one shape there.
SMALL = [
    ("fewer_px_than_threads_9x2", 2, 9, 2),            # P = 18 < 256 threads: most lanes only ever take the clamped tail load
    ("single_px_1x1", 2, 1, 1),                        # P = 1: every load of every lane is the clamped one
    ("one_wg_ragged_37x41", 2, 37, 41),                # one workgroup, P = 1517: not a multiple of 64 / 256 / LM_BATCH * stride
    ("one_wg_exactly_4096_64x64", 2, 64, 64),          # the last pixel count with one workgroup
    ("two_wg_4097_17x241", 2, 17, 241),                # one pixel more: two workgroups, the second nearly idle
    ("ten_wg_ragged_163x227", 1, 163, 227),            # 10 partial records: lm_finalize_block_one's groups 0 and 1 take a second record
    ("batch1_72x100", 1, 72, 100),                     # batch sizes at a mid-sized shape (2 workgroups per image)
    ("batch2_72x100", 2, 72, 100),
    ("batch5_72x100", 5, 72, 100),
    ("batch16_72x100", 16, 72, 100),
]
LARGE = [
    ("wg19_240x320", 2, 240, 320),                     # 19 workgroups: finalize groups 0..2 take three records, 3..7 two
    ("wg20_ragged_241x323", 1, 241, 323),              # 77843 px: 20 workgroups, ragged everywhere
    ("wg75_480x640", 1, 480, 640),                     # 75 workgroups
    ("wg_cap256_960x1280", 1, 960, 1280),              # 300 wanted, 256 launched: the outer loop takes a second, partial trip
    ("wg_cap256_past_1024x1025", 1, 1024, 1025),       # 1025 px past 256 * 4096: every workgroup takes the partial trip
]
SIGMAS = [0.03, 0.3]
PATTERNS = ["desc", "ones", "sparse", "zero"]
_ids = lambda cases: [c[0] for c in cases]


def _seed(name, sigma):
    return (sum(name.encode()) * 7 + (11 if sigma > 0.1 else 0)) % 1000


def _grid(H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], 0)                                     # (2,H,W)


def _scene(name, B, H, W, sigma):
    """Depth: ~20 % background zeros (plus the top quarter), foreground 0.9..2 with 5 % in 0.3..0.9 and 3 % in a band on both sides of
    MIN_DEPTH_VALID (0.080..0.095 and 0.105..0.120: 5e-3 from the threshold, fp32 spacing there is 7e-9); non-centred intrinsics that
    differ per image; poses exp(xi), xi ~ N(0, sigma).  Targets: the induced flow (clipped) + 2 px of noise, planar, and the SAME fp32
    sum flow + grid as absolute coordinates."""
    seed = _seed(name, sigma)
    depth = syn.uniform("lg.depth", (B, 1, H, W), seed, 0.9, 2.0)
    sel = syn.uniform("lg.sel", (B, 1, H, W), seed)
    aux = syn.uniform("lg.aux", (B, 1, H, W), seed)
    depth = np.where(sel < 0.05, 0.3 + 0.6 * aux, depth)
    depth = np.where((sel >= 0.05) & (sel < 0.065), 0.080 + 0.015 * aux, depth)
    depth = np.where((sel >= 0.065) & (sel < 0.08), 0.105 + 0.015 * aux, depth)
    depth = np.where(sel > 0.8, 0.0, depth).astype(np.float32)
    depth[:, :, : H // 4] = 0.0
    if H * W < 64:                                                      # (tiny maps: make sure the first image has a weighted pixel)
        depth[0, 0, -1, -1] = 1.3
    K = syn.intrinsics(B, H, W)
    K[:, 0, 0] *= 1.0 + 0.03 * np.arange(B, dtype=np.float32)
    K[:, 0, 2] = 0.43 * W + 1.7
    K[:, 1, 2] = 0.58 * H - 0.6
    xi = syn.normal("lg.xi", (B, 6), seed, std=sigma)
    if sigma > 0.1:            # the large pose moves the camera 0.25..0.45 forward: the 0.3..0.9 depths land near, the band behind the plane
        xi[:, 2] = -0.25 - np.minimum(np.abs(xi[:, 2]), 0.2)
    G = syn.se3_exp_np(xi).astype(np.float32).reshape(B, 1, 4, 4)
    depth, K, G = T(depth), T(K), T(G)
    flow = orc.induced_flow(depth, K, G)[0].clamp(-40.0, 40.0) + T(syn.uniform("lg.noise", (B, 2, H, W), seed, -2.0, 2.0))
    absolute = (flow + _grid(H, W)[None]).permute(0, 2, 3, 1).contiguous()           # the kernel's own fp32 addition in planar mode
    return dict(depth=depth, K=K, G=G, flow=flow.contiguous(), absolute=absolute, seed=seed)


def _weight(pat, s):
    B, _, H, W = s["depth"].shape
    return {
        "desc": T(syn.uniform("lg.wdesc", (B, H, W), s["seed"])) * (s["depth"][:, 0] > 0).float(),     # like the descriptor weight: 0 on background
        "ones": torch.ones(B, H, W),
        "sparse": (T(syn.uniform("lg.wsp", (B, H, W), s["seed"])) > 0.97).float() * 2.5,
        "zero": torch.zeros(B, H, W),
    }[pat]


def _guarded(x):
    """x on the device as the contiguous slice [1:B+1] of a tensor whose images 0 and B+1 are NaN: a read outside the B images that
    reaches an accumulator poisons the result."""
    g = torch.full((x.shape[0] + 2,) + tuple(x.shape[1:]), float("nan"), dtype=x.dtype)
    g[1:-1] = x
    return D(g)[1:-1]


def _points(s, dtype=None):
    """(X1, Y1, Z1, Z0) of the oracle, in its working precision (fp64 inside orc.precision)."""
    Z = orc._t(s["depth"])[:, 0] + orc.EPS_DEPTH
    X0, Y0, Z0 = orc.backproject(Z, s["K"])
    return orc.transform_points(s["G"], X0, Y0, Z0) + (Z0,)


def _assert_masks_are_precision_independent(s, what):
    """PRECONDITION (asserted, not skipped): the oracle's `valid` mask and its projection clamp come out the same in fp32 and fp64 --
    a pixel that flips would make an error bound against the fp64 value meaningless.  Z0 = depth + 1e-5 is kept 5e-3 from 0.1 by
    construction; Z1 depends on the pose and is checked here (seeds were chosen on the CPU)."""
    X1, Y1, Z1, Z0 = _points(s)
    with orc.precision(torch.float64):
        X1d, Y1d, Z1d, Z0d = _points(s)
    fg = s["depth"][:, 0] > 0
    assert float((Z0[fg] - orc.MIN_DEPTH_VALID).abs().min()) > 1e-3 if fg.any() else True, what
    v32 = (Z0 > orc.MIN_DEPTH_VALID) & (Z1 > orc.MIN_DEPTH_VALID)
    v64 = (Z0d > orc.MIN_DEPTH_VALID) & (Z1d > orc.MIN_DEPTH_VALID)
    assert torch.equal(v32, v64), f"{what}: the valid mask differs between fp32 and fp64 at {int((v32 != v64).sum())} pixels"
    assert torch.equal(Z1 < orc.MIN_DEPTH_PROJ, Z1d < orc.MIN_DEPTH_PROJ), f"{what}: the projection clamp differs between fp32 and fp64"
    small32, small64 = Z1.clamp(min=orc.MIN_DEPTH_PROJ) <= orc.MIN_DEPTH_PROJ + 0.01, Z1d.clamp(min=orc.MIN_DEPTH_PROJ) <= orc.MIN_DEPTH_PROJ + 0.01
    assert torch.equal(small32 & v32, small64 & v64), what
    return v32, Z1


def _oracle_normal_eq(s, wgt, dtype=None):
    """one image at a time: J is 96 bytes per pixel"""
    Hs, bs = [], []
    for b in range(wgt.shape[0]):
        sl = slice(b, b + 1)
        args = (s["absolute"][sl], wgt[sl], s["depth"][sl], s["K"][sl], s["G"][sl])
        if dtype is None:
            Hm, bv = orc.lm_normal_eq(*args)
        else:
            with orc.precision(dtype):
                Hm, bv = orc.lm_normal_eq(*args)
        Hs.append(Hm)
        bs.append(bv)
    return torch.cat(Hs), torch.cat(bs)


def _check_normal_eq(ops, name, B, H, W, sigma):
    s = _scene(name, B, H, W, sigma)
    valid, _ = _assert_masks_are_precision_independent(s, name)
    if sigma > 0.1 and H * W >= 1000:                                   # the large pose puts points near / behind the camera: `valid` works
        fgv = (s["depth"][:, 0] + orc.EPS_DEPTH) > orc.MIN_DEPTH_VALID
        assert int((fgv & ~valid).sum()) > 0, "no pixel is invalid by its transformed depth"
    depth, K, G = _guarded(s["depth"]), D(s["K"]), D(s["G"])
    targets = {"absolute": _guarded(s["absolute"]), "planar": _guarded(s["flow"])}
    for pat in PATTERNS:
        wgt = _weight(pat, s)
        oH, ob = _oracle_normal_eq(s, wgt)
        eH, eb = _oracle_normal_eq(s, wgt, torch.float64)
        sH, sb = max(1.0, float(oH.abs().max())), max(1.0, float(ob.abs().max()))
        wd = _guarded(wgt)
        got = {}
        for layout, tgt in targets.items():
            Hm, bv = ops.lm_normal_eq(tgt, wd, depth, K, G, eps=1e-5)
            Hm2, bv2 = ops.lm_normal_eq(tgt, wd, depth, K, G, eps=1e-5)
            what = f"{name} sigma={sigma} {pat} {layout}"
            # against the exact value, per matrix, max norm: kernel and oracle are two fp32 evaluations of one expression that differ
            # in summation order only -> the kernel may be at most twice as far from the exact value (+ the 1e-7 of the check below)
            kH, kb = Hm.cpu(), bv.cpu()
            for b in range(B):
                eoH, ekH = float((oH[b] - eH[b]).abs().max()), float((kH[b] - eH[b]).abs().max())
                eob, ekb = float((ob[b] - eb[b]).abs().max()), float((kb[b] - eb[b]).abs().max())
                print(f"RATIO {what} image {b}: H kernel {ekH:.3e} oracle32 {eoH:.3e} ratio {ekH / max(eoH, 1e-300):.3f} | "
                      f"b kernel {ekb:.3e} oracle32 {eob:.3e} ratio {ekb / max(eob, 1e-300):.3f} | scale {sH:.3e} {sb:.3e}")
            close(Hm, oH, 1e-7 * sH, what=f"H oracle ({what})")
            close(bv, ob, 1e-7 * sb, what=f"b oracle ({what})")
            assert torch.equal(Hm, Hm.transpose(1, 2)), what
            for b in range(B):
                assert float((kH[b] - eH[b]).abs().max()) <= 2.0 * float((oH[b] - eH[b]).abs().max()) + 1e-7 * sH, f"H exact ({what}, image {b})"
                assert float((kb[b] - eb[b]).abs().max()) <= 2.0 * float((ob[b] - eb[b]).abs().max()) + 1e-7 * sb, f"b exact ({what}, image {b})"
            assert torch.equal(Hm, Hm2) and torch.equal(bv, bv2), f"two launches differ ({what})"          # fixed-order reduction
            got[layout] = (Hm, bv)
        # `absolute` IS fp32(flow + grid), the sum the kernel forms in planar mode: the layouts see the same numbers in the same order
        assert torch.equal(got["absolute"][0], got["planar"][0]) and torch.equal(got["absolute"][1], got["planar"][1]), f"layouts differ ({name} {pat})"
        if pat == "zero":
            assert float(got["planar"][0].abs().max()) == 0.0 and float(got["planar"][1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 1. normal equations
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("name,B,H,W", SMALL, ids=_ids(SMALL))
def test_lm_normal_eq_launch_geometry(ops, name, B, H, W, sigma):
    _check_normal_eq(ops, name, B, H, W, sigma)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("name,B,H,W", LARGE, ids=_ids(LARGE))
def test_lm_normal_eq_full_size_launch_geometry(ops, name, B, H, W, sigma):
    _check_normal_eq(ops, name, B, H, W, sigma)


# ------------------------------------------------------------------------------------------------ 2. fused step, tickets, workspace
CANARY = 1234.5


def _out_views(B):
    """The five outputs of lm_step as views into ONE fp64 buffer filled with a canary, four doubles apart -> (buffer, views, mask of the
    doubles that belong to no output)."""
    sizes = [8 * B, 36 * B, 6 * B, 3 * B, (B + 1) // 2]                  # doubles: G (B,4,4) f32, Hm, bv f64, xi (B,6) f32, info (B) i32
    buf = torch.full((sum(sizes) + 4 * (len(sizes) + 1),), CANARY, dtype=torch.float64, device="cuda")
    outside = torch.ones(buf.numel(), dtype=torch.bool)
    off, seg = 4, []
    for n in sizes:
        seg.append(buf[off:off + n])
        outside[off:off + n] = False
        off += n + 4
    views = (seg[0].view(torch.float32).view(B, 4, 4), seg[1].view(B, 6, 6), seg[2].view(B, 6), seg[3].view(torch.float32).view(B, 6),
             seg[4].view(torch.int32)[:B])
    return buf, views, outside


def _same(a, b):
    return all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32), y.view(torch.int64) if y.dtype == torch.float64 else y.view(torch.int32))
               for x, y in zip(a, b))


def _clone(out):
    return tuple(x.clone() for x in out)


def _check_step(ops, name, B, H, W, layout, other):
    s = _scene(name, B, H, W, 0.03)
    tgt_cpu = s["absolute"] if layout == "absolute" else s["flow"]
    wgt = _weight("desc", s)
    args = (_guarded(tgt_cpu), _guarded(wgt), _guarded(s["depth"]), D(s["K"]), D(s["G"]))
    ops.lm_fused_tail(True)
    for iters in (1, 3):
        fused = _clone(ops.lm_step(*args, num_iters=iters))
        ops.lm_fused_tail(False)
        try:
            unfused = _clone(ops.lm_step(*args, num_iters=iters))
        finally:
            ops.lm_fused_tail(True)
        assert _same(fused, unfused), f"{name} {layout} iters={iters}: fused tail != three launches"
        assert _same(fused, ops.lm_step(*args, num_iters=iters)), f"{name} {layout} iters={iters}: third call differs (ticket reset)"
        wG, trace = orc.lm_step(s["absolute"], wgt, s["depth"], s["K"], s["G"], num_iters=iters)
        close(fused[0], wG[:, 0], 1e-5, what=f"G ({name} {layout} iters={iters})")
        close(fused[3], trace[-1][2], 1e-6, what=f"xi ({name} {layout} iters={iters})")
        assert int(fused[4].abs().sum()) == 0
        # out= views with canaries around them, both workspace slots
        for slot in (0, 1):
            buf, views, outside = _out_views(B)
            got = ops.lm_step(*args, num_iters=iters, out=views, slot=slot)
            assert _same(got, fused), f"{name} {layout} iters={iters} slot={slot}: out= views differ"
            assert bool((buf.cpu()[outside] == CANARY).all()), f"{name} {layout} iters={iters} slot={slot}: bytes outside the outputs were written"
    # a second live shape of equal B in between: A, B, A must each equal its solo result (shape-keyed workspace, per-image tickets)
    oname, oH, oW = other
    so = _scene(oname, B, oH, oW, 0.03)
    oargs = (_guarded(so["absolute"] if layout == "absolute" else so["flow"]), _guarded(_weight("desc", so)), _guarded(so["depth"]), D(so["K"]), D(so["G"]))
    solo_a = _clone(ops.lm_step(*args, num_iters=3))
    solo_b = _clone(ops.lm_step(*oargs, num_iters=3))
    a1 = _clone(ops.lm_step(*args, num_iters=3))
    b1 = _clone(ops.lm_step(*oargs, num_iters=3))
    a2 = _clone(ops.lm_step(*args, num_iters=3))
    assert _same(a1, solo_a) and _same(b1, solo_b) and _same(a2, solo_a), f"{name} / {oname}: interleaved shapes disturb each other"
    ops.lm_fused_tail(False)
    try:
        assert _same(_clone(ops.lm_step(*oargs, num_iters=3)), solo_b)
    finally:
        ops.lm_fused_tail(True)


# (shape under test, the other live shape of the interleaving: equal B, equal or different workspace size)
STEP_SMALL = [("fewer_px_than_threads_9x2", 2, 9, 2, ("single_px_1x1", 1, 1)),
              ("one_wg_ragged_37x41", 2, 37, 41, ("one_wg_exactly_4096_64x64", 64, 64)),       # equal workspace BYTES, different shape
              ("two_wg_4097_17x241", 2, 17, 241, ("one_wg_ragged_37x41", 37, 41)),
              ("ten_wg_ragged_163x227", 1, 163, 227, ("batch1_72x100", 72, 100)),
              ("batch5_72x100", 5, 72, 100, ("batch5_other_33x70", 33, 70))]
STEP_LARGE = [("wg75_480x640", 1, 480, 640, ("wg20_ragged_241x323", 241, 323)),
              ("wg_cap256_960x1280", 1, 960, 1280, ("wg_cap256_past_1024x1025", 1024, 1025))]   # both 256 workgroups: equal workspace bytes


@pytest.mark.parametrize("layout", ["absolute", "planar"])
@pytest.mark.parametrize("name,B,H,W,other", STEP_SMALL, ids=_ids(STEP_SMALL))
def test_lm_step_tickets_and_workspace(ops, name, B, H, W, other, layout):
    _check_step(ops, name, B, H, W, layout, other)


@pytest.mark.parametrize("layout", ["absolute", "planar"])
@pytest.mark.parametrize("name,B,H,W,other", STEP_LARGE, ids=_ids(STEP_LARGE))
def test_lm_step_full_size_tickets_and_workspace(ops, name, B, H, W, other, layout):
    _check_step(ops, name, B, H, W, layout, other)


# ------------------------------------------------------------------------------------------------ 3. solve and SE(3)
BATCHES = [1, 64, 65, 130]              # lm_solve_update_kernel / the se3 kernels have 64 threads per block: image 65 is in a second block


def _spd(B, tag, gain=50.0):
    A = syn.normal("lg.A." + tag, (B, 12, 6), 5).astype(np.float64)
    return gain * np.einsum("bki,bkj->bij", A, A)


def _poses(B, tag, sigma=0.5):
    return syn.se3_exp_np(syn.normal("lg.pose." + tag, (B, 6), 9, std=sigma)).astype(np.float32)


def _solve(ops, Hm, bv, G):
    return ops.lm_solve_update(D(Hm, torch.float64), D(bv, torch.float64), D(G))


def _check_solve_vs_oracle(ops, Hm, bv, G, what):
    Gn, xi, info = _solve(ops, Hm, bv, G)
    want = orc.lm_solve(Hm, bv)
    close(xi, want, 1e-6, what=f"xi ({what})")
    close(Gn, orc.se3_increment(T(G), want), 1e-5, what=f"G ({what})")
    return Gn, xi, info, want


@pytest.mark.parametrize("B", BATCHES)
def test_lm_solve_update_systems(ops, B):
    G = _poses(B, "solve")
    Hw = _spd(B, "well")
    bw = syn.normal("lg.b", (B, 6), 5, std=300.0).astype(np.float64)
    _, xi, info, _ = _check_solve_vs_oracle(ops, Hw, bw, G, "well-conditioned")
    assert int(info.abs().sum()) == 0 and float(xi.abs().max()) > 1e-3
    # one weighted pixel: H = w J^T J has rank 2, the ep_lambda = 100 of the damping carries the other four pivots
    J = syn.normal("lg.J", (B, 2, 6), 6, std=30.0).astype(np.float64)
    r = syn.normal("lg.r", (B, 2), 6, std=2.0).astype(np.float64)
    _, _, info, _ = _check_solve_vs_oracle(ops, 0.7 * np.einsum("bki,bkj->bij", J, J), 0.7 * np.einsum("bki,bk->bi", J, r), G, "rank 2")
    assert int(info.abs().sum()) == 0
    for scale in (1e12, 1e-12):
        _, _, info, _ = _check_solve_vs_oracle(ops, Hw * scale, bw * scale, G, f"scaled by {scale:g}")
        assert int(info.abs().sum()) == 0
    # right-hand sides whose solution is +-3 in component b % 6: the +-1 clamp fires in each component, with both signs
    x = 0.2 * syn.normal("lg.x", (B, 6), 7).astype(np.float64)
    for b in range(B):
        x[b, b % 6] = 3.0 if (b // 6) % 2 == 0 else -3.0
    for sign in (1.0, -1.0):
        Hd = Hw + 100.0 * np.eye(6) + 1e-4 * Hw * np.eye(6)
        _, xi, _, want = _check_solve_vs_oracle(ops, Hw, sign * np.einsum("bij,bj->bi", Hd, x), G, "clamp")
        for b in range(B):
            assert float(xi[b, b % 6]) == sign * (1.0 if (b // 6) % 2 == 0 else -1.0), (b, xi[b])
    # the Cholesky test fails at minor j = 1..6 (image b: j = b % 6 + 1): info == j, zero update, pose unchanged bit for bit
    for shift in range(6):
        Hf = Hw.copy()
        js = np.array([(b + shift) % 6 + 1 for b in range(B)])
        for b in range(B):
            Hf[b, js[b] - 1, js[b] - 1] = -1.0e4 - 37.0 * b
        Gn, xi, info, want = _check_solve_vs_oracle(ops, Hf, bw, G, "not positive definite")
        assert np.array_equal(N(info), js.astype(np.int32)), (N(info), js)
        assert float(xi.abs().max()) == 0.0 and float(np.abs(want).max()) == 0.0
        assert torch.equal(Gn, D(G)), "pose changed by a failed solve"
    # NaN in H / in b (image b: position b % 36 / b % 6): NaN -> zero update, the pose stays
    for which in ("H", "b"):
        Hn, bn = Hw.copy(), bw.copy()
        for b in range(B):
            if which == "H":
                i, j = divmod(b % 36, 6)
                Hn[b, i, j] = Hn[b, j, i] = np.nan
            else:
                bn[b, b % 6] = np.nan
        Gn, xi, info, want = _check_solve_vs_oracle(ops, Hn, bn, G, f"NaN in {which}")
        assert np.array_equal(N(xi) == 0, want == 0)
        if which == "b":
            assert float(xi.abs().max()) == 0.0 and torch.equal(Gn, D(G))


def _exp_exact(xi):
    """SE(3) exponential in fp64 with the closed form away from 0 and the power series (to theta^10) below 0.05: exact to ~1e-16."""
    xi = np.asarray(xi, np.float64).reshape(-1, 6)
    out = np.tile(np.eye(4), (len(xi), 1, 1))
    for n, (v, w) in enumerate(zip(xi[:, :3], xi[:, 3:])):
        t2 = float(w @ w)
        th = np.sqrt(t2)
        if th < 0.05:
            A = 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72 * (1 - t2 / 110))))
            Bc = 0.5 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56 * (1 - t2 / 90 * (1 - t2 / 132)))))
            Cc = (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72 * (1 - t2 / 110 * (1 - t2 / 156))))) / 6
        else:
            A, Bc, Cc = np.sin(th) / th, (1 - np.cos(th)) / t2, (th - np.sin(th)) / (t2 * th)
        Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        out[n, :3, :3] = np.eye(3) + A * Wx + Bc * Wx @ Wx
        out[n, :3, 3] = (np.eye(3) + Bc * Wx + Cc * Wx @ Wx) @ v
    return out


# rotation angle, then |orc.se3_exp (fp32) - exact| in max norm over the axes below, for unit-scale translations | translations of 50
# (measured on the CPU).  The reference's closed form loses its accuracy just above MIN_THETA = 1e-4: fp32 cos(1.01e-4) IS 1, so
# (1 - cos theta) / theta^2 comes out 0 instead of 1/2 and the translation is off by theta |v| / 2; at 1e-3 the quotient still has
# only three bits.  An absolute bound there would test the formula, not the kernel: the kernel's error is bounded by the oracle's own.
ANGLES = [
    0.0,            # 0       | 0
    1e-8,           # 1.3e-08 | 6.4e-07
    0.99e-4,        # 5.0e-08 | 2.1e-06      just below MIN_THETA: the series
    1.01e-4,        # 8.3e-05 | 4.1e-03      just above: the closed form at its worst
    1e-3,           # 3.2e-05 | 1.6e-03
    1.0,            # 6.0e-08 | 3.0e-06
    np.pi - 1e-3,   # 1.0e-07 | 1.0e-05
    np.pi,          # 1.7e-07 | 8.7e-06
    2 * np.pi,      # 2.1e-07 | 3.4e-06
    10.0,           # 1.1e-07 | 4.1e-06
]
AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0.6, -0.8, 0.0], [-0.36, 0.48, 0.8]], np.float64)
AXES /= np.linalg.norm(AXES, axis=1, keepdims=True)


def _twists():
    rows = []
    for k, th in enumerate(ANGLES):
        for a, ax in enumerate(AXES):
            for scale in (1.0, 50.0):                                   # 50: large translations
                v = syn.normal(f"lg.v{k}.{a}", (3,), 3).astype(np.float64) * scale
                rows.append(np.concatenate([v, th * ax]))
    return np.asarray(rows).astype(np.float32)


def _chunks(x, B):
    """all rows of x in launches of exactly B (the last one filled up from the start)"""
    n = -(-len(x) // B) * B
    idx = np.arange(n) % len(x)
    return [idx[i:i + B] for i in range(0, n, B)]


@pytest.mark.parametrize("B", BATCHES)
def test_se3_exp_twists(ops, B):
    xi = _twists()
    want, exact = N(orc.se3_exp(xi)), _exp_exact(xi)
    for idx in _chunks(xi, B):
        got = N(ops.se3_exp(D(xi[idx])))
        assert got.shape == (B, 4, 4)
        # the same formulas in the same precision: 1e-6, relative to the entry for the translations of 50 (fp32 has 6e-8 per operation)
        close(got, want[idx], 1e-6, 1e-6, what="se3_exp oracle")
        ek = np.abs(got - exact[idx]).reshape(B, -1).max(1)
        eo = np.abs(want[idx] - exact[idx]).reshape(B, -1).max(1)
        bound = 2.0 * eo + 1e-6 * np.maximum(1.0, np.abs(exact[idx]).reshape(B, -1).max(1))
        assert (ek <= bound).all(), (idx[np.argmax(ek - bound)], ek.max(), eo.max())


@pytest.mark.parametrize("B", BATCHES)
def test_se3_compose_inverse_outer_update_vs_fp64(ops, B):
    xa = syn.normal("lg.ca", (B, 6), 21).astype(np.float64)
    xb = syn.normal("lg.cb", (B, 6), 22).astype(np.float64)
    xa[:, 3:] *= np.linspace(0.0, 3.2, B)[:, None] if B > 1 else 2.5                # rotation angles from 0 to beyond pi
    xb[:, 3:] *= 1.7
    A, Bm = _exp_exact(xa).astype(np.float32), _exp_exact(xb).astype(np.float32)
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    close(ops.se3_compose(D(A), D(Bm)), A64 @ B64, 1e-6, 1e-6, what="compose")
    inv = np.tile(np.eye(4), (B, 1, 1))
    inv[:, :3, :3] = A64[:, :3, :3].transpose(0, 2, 1)
    inv[:, :3, 3] = -np.einsum("bji,bj->bi", A64[:, :3, :3], A64[:, :3, 3])
    close(ops.se3_inverse(D(A)), inv, 1e-6, 1e-6, what="inverse")
    for literal in (True, False):
        Ti_new, Tij_new = ops.se3_outer_update(D(A), D(Bm), literal)
        close(Ti_new, A64 @ B64, 1e-6, 1e-6, what="outer update Ti")
        assert torch.equal(Ti_new, ops.se3_compose(D(A), D(Bm)))
        if literal:
            assert torch.equal(Tij_new, ops.se3_compose(Ti_new, ops.se3_inverse(Ti_new)))
        close(Tij_new, np.tile(np.eye(4), (B, 1, 1)), 1e-5, what="outer update Tij")


# ------------------------------------------------------------------------------------------------ 4. geometry kernels
# fp32 oracle's own maximum relative error |oracle32 - oracle64| / max(1, |oracle64|) on the pixels near / behind the camera plane,
# measured per case: 7e-8 .. 2e-5 at the small shapes, up to 8.0e-4 at the large ones (a Z1 within 1e-6 of the 0.01 clamp; the MI355X
# kernels gave the oracle's figure to every printed digit in all cases); a kernel may be 4 x as far from the fp64 value as the oracle is.
NEAR_PLANE_FACTOR = 4.0


def _lowres_all_taps(mask, h, w):
    """mask (B,H,W) bool -> (B,h,w): all four taps of the align_corners down-sampling satisfy it"""
    H, W = mask.shape[-2:]
    sy, sx = ((H - 1) / (h - 1) if h > 1 else 0.0), ((W - 1) / (w - 1) if w > 1 else 0.0)
    ys, xs = torch.arange(h, dtype=torch.float32) * np.float32(sy), torch.arange(w, dtype=torch.float32) * np.float32(sx)
    y0, x0 = torch.floor(ys).long().clamp(0, H - 1), torch.floor(xs).long().clamp(0, W - 1)
    y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
    r0, r1 = mask[:, y0], mask[:, y1]
    return r0[:, :, x0] & r0[:, :, x1] & r1[:, :, x0] & r1[:, :, x1]


def _coords_check(got, want32, want64, good, what):
    """got / want (B,2,...) with good (B,...): the project's tolerance where the clamped depth is >= MIN_DEPTH_VALID; elsewhere finite and
    at most NEAR_PLANE_FACTOR x the fp32 oracle's own relative error from the fp64 oracle."""
    got, want32, want64 = N(got).astype(np.float64), N(want32).astype(np.float64), N(want64)
    g = np.broadcast_to(N(good)[:, None], got.shape)
    close(np.where(g, got, 0.0), np.where(g, want32, 0.0), 1e-4, 1e-6, what=f"{what}: regular pixels")
    if (~g).any():
        assert np.isfinite(got[~g]).all(), f"{what}: non-finite coordinate near the camera plane"
        den = np.maximum(1.0, np.abs(want64[~g]))
        ro, rk = float((np.abs(want32[~g] - want64[~g]) / den).max()), float((np.abs(got[~g] - want64[~g]) / den).max())
        print(f"NEAR_PLANE {what}: {int((~g).sum())} values, relative error oracle32 {ro:.3e} kernel {rk:.3e}")
        assert rk <= NEAR_PLANE_FACTOR * ro, f"{what}: relative error {rk:.3e} near the camera plane, the fp32 oracle's own is {ro:.3e}"


def _check_geometry(ops, name, B, H, W, sigma):
    s = _scene(name, B, H, W, sigma)
    _, Z1 = _assert_masks_are_precision_independent(s, name)
    fg = s["depth"][:, 0] > 0
    good = ~fg | (Z1.clamp(min=orc.MIN_DEPTH_PROJ) >= orc.MIN_DEPTH_VALID)
    if int(fg.sum()) >= 10:
        share = float((good & fg).sum()) / float(fg.sum())
        assert share >= 0.9, f"{name} sigma={sigma}: only {share:.3f} of the foreground has clamped depth >= MIN_DEPTH_VALID"
    what = f"{name} sigma={sigma}"
    depth, K, G = _guarded(s["depth"]), D(s["K"]), D(s["G"])
    wf, wv = orc.induced_flow(s["depth"], s["K"], s["G"])
    with orc.precision(torch.float64):
        ef, _ = orc.induced_flow(s["depth"], s["K"], s["G"])
    flow, vmask = ops.induced_flow(depth, K, G, eps=1e-5)
    assert np.array_equal(N(vmask), N(wv)), f"{what}: vmask"
    _coords_check(flow, wf, ef, good, f"{what} induced flow")
    # absolute coordinates (SE3.transform): the depth comes in with its epsilon, background included
    deps = s["depth"] + 1e-5
    reproject = lambda: torch.stack(orc.project(*orc.transform_points(s["G"], *orc.backproject(orc._t(deps)[:, 0], s["K"])), s["K"])[:2], 1)
    uv32 = reproject()
    with orc.precision(torch.float64):
        uv64 = reproject()
    uv, _ = ops.induced_flow(_guarded(deps), K, G, eps=0.0, absolute=True)
    _coords_check(uv, uv32, uv64, good & fg, f"{what} absolute")      # (background: a point 1e-5 in front of the first camera -- the near-plane class)
    h, w = H // 8, W // 8
    if h >= 1 and w >= 1:
        c32 = orc.flow_init_to_coords1(wf)
        with orc.precision(torch.float64):
            c64 = orc.flow_init_to_coords1(ef)
        good_lr = _lowres_all_taps(good, h, w)
        c1 = ops.induced_coords_lowres(depth, K, G, h, w, 1e-5)
        _coords_check(c1, c32, c64, good_lr, f"{what} lowres")
        # the interpolation alone, on the oracle's flow: one input, so `exact` is the fp64 interpolation of the fp32 flow
        with orc.precision(torch.float64):
            f64 = orc.flow_init_to_coords1(wf)
        _coords_check(ops.flow_to_coords(_guarded(wf), h, w), c32, f64, good_lr, f"{what} flow_to_coords")


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("name,B,H,W", SMALL + [("lowres_not_8x_35x53", 2, 35, 53)], ids=_ids(SMALL) + ["lowres_not_8x_35x53"])
def test_geometry_kernels_vs_oracle(ops, name, B, H, W, sigma):
    _check_geometry(ops, name, B, H, W, sigma)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("name,B,H,W", LARGE + [("lowres_not_8x_483x645", 1, 483, 645)], ids=_ids(LARGE) + ["lowres_not_8x_483x645"])
def test_geometry_kernels_full_size_vs_oracle(ops, name, B, H, W, sigma):
    _check_geometry(ops, name, B, H, W, sigma)


def _check_corr_weight(ops, name, B, H, W, Dd):
    from rnnpose_amd import _lib
    s = _scene(name, B, H, W, 0.03)
    g = []
    for nm in ("lg.g1", "lg.g2"):
        x = syn.normal(nm, (B, Dd, H, W), s["seed"]).astype(np.float64)
        g.append(T((x / (np.sqrt((x * x).sum(1, keepdims=True)) + 1e-12)).astype(np.float32)))
    flow = T(syn.uniform("lg.cwflow", (B, 2, H, W), s["seed"], -4.0, 4.0))
    nx, ny = max(1, W // 8), max(1, H // 8)
    flow[:, 0, :, :nx] -= W + 5.0                                       # targets outside the left / right / top / bottom border,
    flow[:, 0, :, W - nx:] += W + 5.0                                   # the corners outside two of them
    flow[:, 1, :ny] -= H + 5.0
    flow[:, 1, H - ny:] += H + 5.0
    flow[:, :, H // 2, W // 2] = 1e5                                    # and far outside
    absolute = (flow + _grid(H, W)[None]).permute(0, 2, 3, 1).contiguous()
    sigma = torch.tensor([0.7])
    want = orc.corr_weight(g[0], g[1], absolute, s["depth"], sigma)
    g1, g2, depth = D(g[0]), D(g[1]), _guarded(s["depth"])
    try:
        for layout, tgt in (("absolute", _guarded(absolute)), ("planar", _guarded(flow))):
            got = {}
            for pairs in (1, 0):
                _lib.call("rnnpose_corr_weight_pairs", pairs)
                got[pairs] = ops.corr_weight(g1, g2, tgt, depth, D(sigma)).clone()
                close(got[pairs], want, 1e-5, what=f"weight oracle ({name} D={Dd} {layout} pairs={pairs})")
                assert np.array_equal(N(got[pairs]) == 0, N(want) == 0)
            assert torch.equal(got[1], got[0]), f"{name} D={Dd} {layout}: tap pairs != four taps"
    finally:
        _lib.call("rnnpose_corr_weight_pairs", 0)                       # (the library's default, RP_CW_PAIRS)


CW_SMALL = [c for c in SMALL if c[2] > 1 and c[3] > 1 and c[1] <= 5]       # (the entry requires H > 1 and W > 1: 1 / (W - 1))


@pytest.mark.parametrize("Dd", [1, 7, 32])                               # D > 0 is all the entry asks; the loads come in batches of 4 channels
@pytest.mark.parametrize("name,B,H,W", CW_SMALL, ids=_ids(CW_SMALL))
def test_corr_weight_shapes_and_descriptor_depths(ops, name, B, H, W, Dd):
    _check_corr_weight(ops, name, B, H, W, Dd)


@pytest.mark.parametrize("name,B,H,W,Dd", [("wg20_ragged_241x323", 1, 241, 323, 32), ("wg75_480x640", 1, 480, 640, 7),
                                           ("wg_cap256_past_1024x1025", 1, 1024, 1025, 1)], ids=["241x323-D32", "480x640-D7", "1024x1025-D1"])
def test_corr_weight_full_size_shapes(ops, name, B, H, W, Dd):
    _check_corr_weight(ops, name, B, H, W, Dd)
