"""The per-pixel and layout kernels between the convolutions of the refinement loop -- csrc/pointwise.hip and the non-KPConv half of
csrc/nhwc_ops.hip -- against fp64 at their edges and beyond their grid caps (run with -m gpu on an MI355X; every shape whose test name
does not contain `full_size` also runs on the host-executed kernels, tests/test_kernels_on_host.py).

tests/test_gpu_parity.py meets most of these kernels at one shape and some only through another HIP path of the same code.  Here every
shape is in a table with the code path it is there for; inputs are seeded by rnnpose_amd.synthetic; the reference is a plain fp64
expression on the CPU (torch, or oracle/rnnpose_oracle.py under `orc.precision`).

Gates.  Layout kernels, untouched bytes and the one-hot softmax are exact (torch.equal).  For an approximate kernel the same expression is
also evaluated in fp32 on the CPU: err_gpu = max|HIP - ref64|, err_ref = max|ref32 - ref64|, and the test passes iff
err_gpu <= max(2 * err_ref, floor): both are fp32 evaluations of one formula that differ in operation order and contraction only, while
a wrong tap, row or channel errs at the scale of the data.  The floors are the project's tolerances for each kernel (FLOOR).  Both
errors are printed per case.  Destinations are pre-filled with a sentinel: bytes outside the written window must come back untouched.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rnnpose_oracle as orc
from rnnpose_amd import synthetic as syn
from test_gpu_parity import D, N, T, close, ops  # noqa: F401  (ops: the module-scoped build fixture)

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
FLOOR = dict(context_prep=1e-6, gru=1e-6, coords=1e-5, coords_rel=1e-6, convex=1e-4, instnorm=2e-6, flow_conv=2e-5, head_delta=2e-5,
             head_coords=5e-5, pixel_head=1e-5)
_ids = lambda cases: [c[0] for c in cases]


def gate(kernel, case, got, ref64, ref32, floor, rel=0.0, extra=None):
    """err_gpu <= max(2 * err_ref, floor + rel * |ref| [+ extra]) at every element; prints both errors."""
    g, r = got.detach().cpu().to(F64), ref64.to(F64)
    assert g.shape == r.shape, f"{kernel} {case}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    eg = (g - r).abs()
    err_ref = float((ref32.to(F64) - r).abs().max()) if r.numel() else 0.0
    bound = floor + rel * r.abs()
    if extra is not None:
        bound = bound + extra
    bound = bound.clamp(min=2.0 * err_ref) if torch.is_tensor(bound) else torch.full_like(r, max(2.0 * err_ref, bound))
    err_gpu = float(eg.max()) if r.numel() else 0.0
    print(f"glue_edges {kernel} [{case}] err_gpu {err_gpu:.3e} err_ref {err_ref:.3e}")
    bad = ~(eg <= bound)                      # (NaN fails)
    if bad.any():
        i = tuple(int(k) for k in torch.nonzero(bad)[0])
        raise AssertionError(f"{kernel} [{case}]: {int(bad.sum())}/{bad.numel()} elements beyond max(2 * err_ref, floor); first at {i}: got "
                             f"{float(g[i])!r} want {float(r[i])!r}, bound {float(bound[i]):.3e}, err_gpu {err_gpu:.3e}, err_ref {err_ref:.3e}")


def both(fn):
    """fn(dtype) -> tensor or tuple, evaluated in fp64 and in fp32"""
    return fn(F64), fn(F32)


def grid_lowres(B, h, w):
    return orc.coords_grid_lowres(B, h, w)            # (B,2,h,w) fp32: x, y


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ================================================================================================== 1. context_prep
# (id, B, C, hdim, H, W, h, w).  One thread per output element, 32-bit index arithmetic, grid capped at 65536 x 256 threads.
CONTEXT_PREP = [
    ("odd_35x53_to_4x6", 1, 6, 2, 35, 53, 4, 6),            # H, W not 8x the output: fractional taps in both directions
    ("identity_8x8_hdim1", 2, 5, 1, 8, 8, 8, 8),            # h = H, w = W: every tap fraction is 0; hdim = 1
    ("to_1x1", 1, 4, 3, 17, 9, 1, 1),                       # h = w = 1: scale 0, the tap is pixel (0, 0); inp has one channel
    ("row_3x100_to_1x12", 1, 4, 2, 3, 100, 1, 12),          # h = 1 alone: only the x direction interpolates
    ("full_channels_35x53_to_4x6", 2, 256, 128, 35, 53, 4, 6),   # the shipped channel split at an odd size, 48 workgroups
]


def _resized(x, h, w, dtype):
    with orc.precision(dtype):
        return orc.resize_bilinear_ac(orc._t(x), h, w)


@pytest.mark.parametrize("name,B,C,hdim,H,W,h,w", CONTEXT_PREP, ids=_ids(CONTEXT_PREP))
def test_context_prep_vs_fp64(ops, name, B, C, hdim, H, W, h, w):
    ctx = T(syn.normal("ge.ctx." + name, (B, C, H, W), 3, std=1.5))
    net, inp = ops.context_prep(D(ctx), h, w, hdim)
    assert tuple(net.shape) == (B, hdim, h, w) and tuple(inp.shape) == (B, C - hdim, h, w)
    r64, r32 = both(lambda dt: _resized(ctx, h, w, dt))
    gate("context_prep.net", name, net, torch.tanh(r64[:, :hdim]), torch.tanh(r32[:, :hdim]), FLOOR["context_prep"])
    gate("context_prep.inp", name, inp, torch.relu(r64[:, hdim:]), torch.relu(r32[:, hdim:]), FLOOR["context_prep"])


def test_context_prep_full_size_grid_stride(ops):
    """(1,257,128,256,256 -> 256,256): 16,842,752 elements > 65536 x 256 threads, so the grid-stride loop takes a second, partial trip.
    Output size = input size: every tap fraction is 0 and the resize is the identity, so the reference is tanh / relu of the input."""
    B, C, hdim, S = 1, 257, 128, 256
    ctx = T(syn.uniform("ge.ctx.full", (B, C, S, S), 3, -3.0, 3.0))
    assert ctx.numel() > 65536 * 256
    net, inp = ops.context_prep(D(ctx), S, S, hdim)
    assert torch.equal(inp.cpu(), torch.relu(ctx[:, hdim:]))
    gate("context_prep.net", "full_size", net, torch.tanh(ctx[:, :hdim].to(F64)), torch.tanh(ctx[:, :hdim]), FLOOR["context_prep"])


# ================================================================================================== 2. flow_to_coords
# (id, B, H, W, h, w).  ds = W // w divides the flow before the align_corners resize.
FLOW_TO_COORDS = [
    ("odd_35x53_to_4x6", 2, 35, 53, 4, 6),                  # ds = 8 with a remainder in both directions
    ("identity_8x8", 1, 8, 8, 8, 8),                        # ds = 1, tap fractions 0
    ("to_1x1", 1, 17, 9, 1, 1),                             # one output pixel: the tap is pixel (0, 0), ds = 9
    ("remainder_64x100_to_8x12", 1, 64, 100, 8, 12),        # W // w = 8 with a remainder, H = 8 h exactly
    ("ds4_9x9_to_3x2", 1, 9, 9, 3, 2),                      # ds = 4: h and w give different ratios, the kernel takes W // w
]


@pytest.mark.parametrize("name,B,H,W,h,w", FLOW_TO_COORDS, ids=_ids(FLOW_TO_COORDS))
def test_flow_to_coords_vs_fp64(ops, name, B, H, W, h, w):
    flow = T(syn.normal("ge.f2c." + name, (B, 2, H, W), 5, std=4.0))
    dev = D(flow)
    got = ops.flow_to_coords(dev, h, w)
    assert torch.equal(dev.cpu(), flow), "flow_to_coords changed its input"
    ds = W // w
    r64, r32 = both(lambda dt: grid_lowres(B, h, w).to(dt) + _resized(flow.to(dt) / ds, h, w, dt))
    gate("flow_to_coords", name, got, r64, r32, FLOOR["coords"], rel=FLOOR["coords_rel"])


@pytest.mark.parametrize("name,B,H,W,h,w", FLOW_TO_COORDS, ids=_ids(FLOW_TO_COORDS))
def test_induced_coords_lowres_is_induced_flow_then_flow_to_coords(ops, name, B, H, W, h, w):
    """the four-tap form == the full-resolution flow followed by flow_to_coords, bit for bit, at the same shapes"""
    depth = syn.uniform("ge.ic.depth." + name, (B, 1, H, W), 6, 0.9, 2.0)
    depth = np.where(syn.uniform("ge.ic.bg." + name, (B, 1, H, W), 6) > 0.8, 0.0, depth).astype(np.float32)      # 20 % background
    K = syn.intrinsics(B, H, W)
    G = syn.se3_exp_np(syn.normal("ge.ic.xi." + name, (B, 6), 6, std=0.03)).astype(np.float32).reshape(B, 4, 4)
    c1 = ops.induced_coords_lowres(D(depth), D(K), D(G), h, w)
    flow, _ = ops.induced_flow(D(depth), D(K), D(G))
    c2 = ops.flow_to_coords(flow, h, w)
    assert torch.isfinite(c1).all() and torch.equal(c1, c2)


# ================================================================================================== 3. convex up-sampling
# (id, B, h, w).  NCHW kernel: 64-wide X tiles, two passes of 256 threads over 512 sub-pixels; NHWC kernel: 4 pixels per workgroup;
# fused mask kernel: 64-pixel tiles.
CONVEX = [
    ("single_px_1x1", 1, 1, 1),                             # every neighbour but the centre is across the border
    ("column_3x1", 2, 3, 1),                                # w = 1: left and right neighbours always outside
    ("row_1x63", 2, 1, 63),                                 # one short of the NCHW kernel's 64-wide tile
    ("row_1x64", 1, 1, 64),                                 # exactly one tile
    ("row_1x65", 2, 1, 65),                                 # a second tile with one pixel; 65 = 16 x 4 + 1 for the NHWC kernel
    ("two_tiles_2x129", 1, 2, 129),                         # three X tiles, 258 pixels = 4 x 64 + 2 for the fused kernel
]
MU_CS, MU_CO = 264, 8                                       # the fused kernel's 256 input channels at offset 8 of a 264-channel row


def _convex(flow, logits, dtype):
    with orc.precision(dtype):
        return orc.convex_upsample(flow.to(dtype), logits.to(dtype))


def _conv1x1_in_order(xs, wt, bs, dtype):
    """0.25 (sum_c x_c w_c + b), the 256 products added one channel after the other in `dtype`.  The fp32 evaluation goes through
    here and not through a library matrix product: the order in which sgemm adds depends on the CPU it runs on, and with it err_ref
    -- max over a handful of near-tie softmax pixels -- moved by a factor 2 between two machines (two_tiles_2x129 at std 30: 3.46e-4
    and 1.86e-4 for the same inputs, against 3.89e-4 of the kernel on an MI355X and 4.44e-4 of this fixed order)."""
    acc = torch.zeros(tuple(xs.shape[:-1]) + (wt.shape[0],), dtype=dtype)
    for c in range(xs.shape[-1]):
        acc = acc + xs[..., c:c + 1].to(dtype) * wt[:, c].to(dtype)
    return nchw(0.25 * (acc + bs.to(dtype)))


@pytest.mark.parametrize("std", [2, 30], ids=["std2", "std30"])
@pytest.mark.parametrize("name,B,h,w", CONVEX, ids=_ids(CONVEX))
def test_convex_upsample_three_forms_vs_fp64(ops, name, B, h, w, std):
    """convex_upsample (NCHW mask), convex_upsample_nhwc and mask_upsample against ONE fp64 reference: the logits are an fp64 1x1
    convolution 0.25 (W x + b) (update.py:183-187); the two kernels that read a mask tensor get those logits rounded to fp32."""
    key = f"{name}.{std}"
    x = T(syn.normal("ge.mu.x." + key, (B, h, w, MU_CS), 11)).clamp(min=0)
    wt = T(syn.normal("ge.mu.w." + key, (576, 256), 11, std=float(np.sqrt(2.0 / 256)) * 4.0 * std))      # logits of std `std`
    bs = T(syn.uniform("ge.mu.b." + key, (576,), 11, -0.5, 0.5))
    flow = T(syn.normal("ge.mu.f." + key, (B, 2, h, w), 11, std=2.0))
    xs = x[..., MU_CO:MU_CO + 256]
    l64 = _conv1x1_in_order(xs, wt, bs, F64)
    assert 0.5 * std < float(l64.std()) < 2.0 * std
    mask = l64.to(F32).contiguous()
    ref64 = _convex(flow, l64, F64)
    ref32_mask = _convex(flow, mask, F32)
    nan = lambda: torch.full((B, 2, 8 * h, 8 * w), float("nan"), device="cuda")
    gate("convex_upsample", key, ops.convex_upsample(D(flow), D(mask)), ref64, ref32_mask, FLOOR["convex"])
    gate("convex_upsample_nhwc", key, ops.convex_upsample_nhwc(D(nhwc(flow)), D(nhwc(mask)), out=nan()), ref64, ref32_mask, FLOOR["convex"])
    pm = ops.PackedMaskHead(D(wt.reshape(576, 256, 1, 1)), D(bs), post_scale=0.25)
    gate("mask_upsample", key, ops.mask_upsample(pm, D(x), MU_CO, D(nhwc(flow)), out=nan()), ref64,
         _convex(flow, _conv1x1_in_order(xs, wt, bs, F32), F32), FLOOR["convex"])


@pytest.mark.parametrize("name,B,h,w", CONVEX, ids=_ids(CONVEX))
def test_convex_upsample_one_hot_is_exact(ops, name, B, h, w):
    """One tap at +80, the rest at -80 per sub-pixel (exp(-160) is 0 in fp32), the hot tap cycling through all nine: the output is
    8 x the neighbour's flow, or 0 across the border, exactly -- in both kernels that read a mask tensor."""
    flow = T(syn.normal("ge.oh.f." + name, (B, 2, h, w), 12, std=2.0))
    b_, i_, j_, y_, x_ = torch.meshgrid(torch.arange(B), torch.arange(8), torch.arange(8), torch.arange(h), torch.arange(w), indexing="ij")
    hot = (b_ + 8 * i_ + j_ + 5 * y_ + x_) % 9                                                  # (B,8,8,h,w)
    mask = torch.full((B, 9, 8, 8, h, w), -80.0)
    mask.scatter_(1, hot[:, None], 80.0)
    fp = F.pad(8.0 * flow, (1, 1, 1, 1))                                                        # exact: a power of two
    nb = torch.stack([fp[:, :, k // 3:k // 3 + h, k % 3:k % 3 + w] for k in range(9)], 2)       # (B,2,9,h,w)
    want = torch.gather(nb[:, :, :, None, None].expand(B, 2, 9, 8, 8, h, w), 2, hot[:, None, None].expand(B, 2, 1, 8, 8, h, w))[:, :, 0]
    want = want.permute(0, 1, 4, 2, 5, 3).reshape(B, 2, 8 * h, 8 * w)
    assert len(set(hot.flatten().tolist())) == 9
    mask = mask.reshape(B, 576, h, w)
    a = ops.convex_upsample(D(flow), D(mask))
    b = ops.convex_upsample_nhwc(D(nhwc(flow)), D(nhwc(mask)), out=torch.full((B, 2, 8 * h, 8 * w), float("nan"), device="cuda"))
    assert torch.equal(a.cpu(), want), "convex_upsample (NCHW mask)"
    assert torch.equal(b.cpu(), want), "convex_upsample_nhwc"


# ================================================================================================== 4. gru_gate / gru_update
# (id, B, C, Ctot, h, w).  One thread per (image, channel < C, pixel); the state tensors carry Ctot >= C channels.
GRU = [
    ("single_1x1_c4", 1, 4, 4, 1, 1),                       # n = 4 elements in one workgroup, Ctot = C: nothing beyond the window
    ("odd_5x7_c12_of_20", 3, 12, 20, 5, 7),                 # n = 1260: not a multiple of 256, C and Ctot unlike 128 / 384
    ("shipped_9x13_c128_of_384", 2, 128, 384, 9, 13),       # the shipped channel counts, n = 29952 = 117 workgroups
]


def _preact(tag, shape, seed):
    """std 30 with +-100 planted: sigmoid and tanh saturate, exp overflows in fp32"""
    v = syn.normal(tag, shape, seed, std=30.0)
    flat = v.reshape(-1)
    step = max(1, flat.size // 4)
    flat[0::step][:4] = np.array([100.0, 100.0, 100.0, 100.0], np.float32)[:len(flat[0::step][:4])]
    flat[1::step][:4] = np.array([-100.0, -100.0, -100.0, -100.0], np.float32)[:len(flat[1::step][:4])]
    return T(v)


@pytest.mark.parametrize("name,B,C,Ctot,h,w", GRU, ids=_ids(GRU))
def test_gru_pointwise_vs_fp64(ops, name, B, C, Ctot, h, w):
    zr = torch.cat([_preact("ge.gru.z." + name, (B, C, h, w), 1), _preact("ge.gru.r." + name, (B, C, h, w), 3)], 1)
    q = _preact("ge.gru.q." + name, (B, C, h, w), 2)
    hcat = T(syn.normal("ge.gru.h." + name, (B, Ctot, h, w), 1))
    z = torch.full((B, C, h, w), float("nan"), device="cuda")
    rhx = torch.full((B, Ctot, h, w), 7.0, device="cuda")
    hdev = D(hcat)
    ops.gru_gate(D(zr), hdev, z, rhx, C)
    z64, z32 = both(lambda dt: torch.sigmoid(zr[:, :C].to(dt)))
    r64, r32 = both(lambda dt: torch.sigmoid(zr[:, C:].to(dt)) * hcat[:, :C].to(dt))
    zc = z.cpu()
    assert torch.isfinite(zc).all() and torch.isfinite(rhx).all()
    gate("gru_gate.z", name, z, z64, z32, FLOOR["gru"])
    gate("gru_gate.rh", name, rhx[:, :C], r64, r32, FLOOR["gru"])
    assert torch.equal(zc[z32 == 0], torch.zeros_like(zc[z32 == 0])) and torch.equal(zc[z32 == 1], torch.ones_like(zc[z32 == 1]))
    assert int((z32 == 0).sum()) > 0 and int((z32 == 1).sum()) > 0
    assert torch.equal(rhx[:, C:].cpu(), torch.full((B, Ctot - C, h, w), 7.0)), "gru_gate wrote channels >= C of rhx"
    # the update reads z as the gate kernel left it and writes a SEPARATE state tensor with another channel count
    hout = torch.full((B, Ctot + 3, h, w), -3.0, device="cuda")
    ops.gru_update(z, D(q), hdev, hout, C)
    u64, u32 = both(lambda dt: (1 - zc.to(dt)) * hcat[:, :C].to(dt) + zc.to(dt) * torch.tanh(q.to(dt)))
    assert torch.isfinite(hout).all()
    gate("gru_update", name, hout[:, :C], u64, u32, FLOOR["gru"])
    assert torch.equal(hout[:, C:].cpu(), torch.full((B, Ctot + 3 - C, h, w), -3.0)), "gru_update wrote channels >= C of hout"
    assert torch.equal(hdev.cpu(), hcat)


# ================================================================================================== 5. layout
# (id, B, C, H, W, Cs, co): 32 x 32 tiles through LDS, channel window [co, co + C) of a Cs-channel NHWC tensor.
LAYOUT = [
    ("single_element", 1, 1, 1, 1, 1, 0),
    ("ragged_33ch_35px_window", 2, 33, 5, 7, 40, 7),        # one channel and three pixels past a tile, odd window offset
    ("31ch_33px", 1, 31, 1, 33, 31, 0),                     # one short / one past, no spare channels
    ("two_tiles_64ch_window", 3, 64, 3, 11, 70, 6),         # exactly two channel tiles, 33 pixels
]


@pytest.mark.parametrize("name,B,C,H,W,Cs,co", LAYOUT, ids=_ids(LAYOUT))
def test_layout_kernels_are_exact(ops, name, B, C, H, W, Cs, co):
    src = T(syn.normal("ge.lay." + name, (B, C, H, W), 1))
    wide = torch.full((B, H, W, Cs), -5.0, device="cuda")
    ops.nchw_to_nhwc(D(src), wide, co)
    wc = wide.cpu()
    assert torch.equal(wc[..., co:co + C], nhwc(src))
    assert torch.equal(wc[..., :co], torch.full((B, H, W, co), -5.0)) and torch.equal(wc[..., co + C:], torch.full((B, H, W, Cs - co - C), -5.0))
    back = ops.nhwc_to_nchw(wide, co, C, out=torch.full((B, C, H, W), float("nan"), device="cuda"))
    assert torch.equal(back.cpu(), src)
    assert torch.equal(wide.cpu(), wc), "nhwc_to_nchw changed its input"
    if co == 0 and Cs == C:
        assert torch.equal(ops.nchw_to_nhwc(D(src)).cpu(), nhwc(src))


# ================================================================================================== 6. flow_prep / flow_conv7x7_relu / flow_features
# Widths around the 20-pixel row tile of conv7x7_cin2_kernel (1, one short, exact, one past, two tiles + 1) x heights 1 (every row
# tap but the centre outside), 5 (< 7: the halo reaches past both borders at once), 9; c_out = 128 (all threads), 96, 38 (threads
# without a channel; 38: a split group that is written in part).
FLOW_W, FLOW_H, FLOW_COUT = [1, 19, 20, 21, 41], [1, 5, 9], [128, 96, 38]
SPLIT_REL, SPLIT_ABS = 2.0 ** -21, 2.0 ** -25 / 8.0       # ops.py, A_SCALE: 21-22 bits while lo is a normal fp16, else 2^-25 / a_scale absolute


def _split_window(shape, co, c):
    """fp16 elements of a split tensor (..., Cs) that hold channels [co, co + c): (..., Cs // 8, 2, 8)"""
    m = torch.zeros(tuple(shape[:-1]) + (shape[-1] // 8, 2, 8), dtype=torch.bool)
    for ch in range(co, co + c):
        m[..., ch // 8, :, ch % 8] = True
    return m


@pytest.mark.parametrize("cout", FLOW_COUT)
@pytest.mark.parametrize("w", FLOW_W)
def test_flow_features_family_vs_fp64(ops, w, cout):
    B, mco, mcs = 2, 126, 128
    wt = T(syn.normal(f"ge.ff.w.{cout}", (cout, 2, 7, 7), 5, std=0.2))
    bias = T(syn.normal(f"ge.ff.b.{cout}", (cout,), 5, std=0.1))
    w_t = D(wt.reshape(cout, 98).t().contiguous())
    for hi, h in enumerate(FLOW_H):
        for sg in (True, False):
            co = 8 * ((hi + int(sg)) % 2)
            case = f"{h}x{w}-c{cout}-sg{int(sg)}-co{co}"
            grid = grid_lowres(B, h, w)
            coords = T(syn.normal("ge.ff.x." + case, (B, 2, h, w), 5, std=3.0)) + (grid if sg else 0.0)
            flow = coords - grid if sg else coords                      # the kernel's own fp32 subtraction: one IEEE operation
            r64, r32 = both(lambda dt: F.relu(F.conv2d(flow.to(dt), wt.to(dt), bias.to(dt), padding=3)))
            floor = FLOOR["flow_conv"] * float(r64.abs().max())
            cdev = D(coords)
            # two launches: flow_prep + flow_conv7x7_relu
            flow4 = torch.full((B, h, w, 4), float("nan"), device="cuda")
            mot_a = torch.full((B, h, w, mcs), 9.0, device="cuda")
            out_a = torch.full((B, h, w, co + cout + 4), -7.0, device="cuda")
            ops.flow_prep(cdev, flow4, mot_a, mco, subtract_grid=sg)
            ops.flow_conv7x7_relu(flow4, w_t, D(bias), out_a, out_c_offset=co)
            assert torch.equal(flow4.cpu(), torch.cat([nhwc(flow), torch.zeros(B, h, w, 2)], -1)), case
            # one launch
            mot_b = torch.full((B, h, w, mcs), 9.0, device="cuda")
            out_b = torch.full((B, h, w, co + cout + 4), -7.0, device="cuda")
            ops.flow_features(cdev, w_t, D(bias), out_b, mot_b, mco, out_c_offset=co, subtract_grid=sg)
            assert torch.equal(out_a, out_b) and torch.equal(mot_a, mot_b), case + ": flow_prep + flow_conv7x7_relu != flow_features"
            ob, mb = out_b.cpu(), mot_b.cpu()
            assert torch.equal(mb[..., mco:], nhwc(flow)) and torch.equal(mb[..., :mco], torch.full((B, h, w, mco), 9.0)), case
            assert torch.equal(ob[..., :co], torch.full((B, h, w, co), -7.0)) and torch.equal(ob[..., co + cout:], torch.full((B, h, w, 4), -7.0)), case
            gate("flow_conv7x7", case, nchw(ob[..., co:co + cout]), r64, r32, floor)
            # split destinations
            ocs = (co + cout + 7) // 8 * 8 + 8
            out_s = torch.full((B, h, w, ocs), -7.0, device="cuda")
            mot_s = torch.full((B, h, w, mcs), 9.0, device="cuda")
            ops.flow_features(cdev, w_t, D(bias), out_s, mot_s, mco, out_c_offset=co, subtract_grid=sg, out_split=True, motion_split=True)
            for t, fill, c0, cn in ((out_s, -7.0, co, cout), (mot_s, 9.0, mco, 2)):
                raw = t.cpu().contiguous().view(torch.float16).view(_split_window(t.shape, c0, cn).shape)
                keep = ~_split_window(t.shape, c0, cn)
                sent = torch.full(tuple(t.shape), fill).view(torch.float16).view(keep.shape)
                assert torch.equal(raw[keep].view(torch.int16), sent[keep].view(torch.int16)), case + ": split store outside its channel window"
            got = ops.unsplit_hl(out_s).cpu()[..., co:co + cout]
            gate("flow_conv7x7.split", case, nchw(got), r64, r32, floor, extra=torch.clamp(SPLIT_REL * r64.abs(), min=SPLIT_ABS))
            gm = ops.unsplit_hl(mot_s).cpu()[..., mco:]
            assert bool(((gm.to(F64) - nhwc(flow).to(F64)).abs() <= torch.clamp(SPLIT_REL * nhwc(flow).to(F64).abs(), min=SPLIT_ABS)).all()), case


# ================================================================================================== 7. flow_head_out
# (id, B, h, w, cin).  Fast path (cin <= 256): a wave per run of 4 pixels, at most 512 workgroups = 2048 runs per sweep; general path:
# a wave per pixel, at most 4096 workgroups = 16384 pixels per sweep.
FLOW_HEAD = [
    ("fast_2112_runs_64x132_c64", 1, 64, 132, 64),          # 2112 runs > 2048: 64 waves take a second run
    ("fast_2178_runs_ragged_33x130_c128", 2, 33, 130, 128), # 33 runs per row, the last with 2 pixels; two images
]


def _flow_head_case(ops, name, B, h, w, cin, coff=4):
    cs = coff + cin + 4
    x = T(syn.normal("ge.fh.x." + name, (B, h, w, cs), 13, std=1.0))
    wt = T(syn.normal("ge.fh.w." + name, (2, cin, 3, 3), 13, std=0.05))
    bias = T(syn.normal("ge.fh.b." + name, (2,), 13, std=0.1))
    grid = grid_lowres(B, h, w)
    coords1 = grid + T(syn.normal("ge.fh.c." + name, (B, 2, h, w), 13, std=2.0))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    delta, c1o, flr = nan(B, h, w, 2), nan(B, 2, h, w), nan(B, h, w, 2)
    cdev = D(coords1)
    ops.flow_head_out(D(x), coff, cin, D(wt), D(bias), cdev, delta, c1o, flr)
    xin = nchw(x[..., coff:coff + cin])
    d64, d32 = both(lambda dt: F.conv2d(xin.to(dt), wt.to(dt), bias.to(dt), padding=1))
    gate("flow_head_out.delta", name, nchw(delta), d64, d32, FLOOR["head_delta"])
    gate("flow_head_out.coords", name, c1o, coords1.to(F64) + d64, coords1 + d32, FLOOR["head_coords"])
    gate("flow_head_out.flow_lr", name, nchw(flr), coords1.to(F64) + d64 - grid.to(F64), (coords1 + d32) - grid, FLOOR["head_coords"])
    assert torch.equal(cdev.cpu(), coords1)


@pytest.mark.parametrize("name,B,h,w,cin", FLOW_HEAD, ids=_ids(FLOW_HEAD))
def test_flow_head_out_beyond_the_fast_path_cap(ops, name, B, h, w, cin):
    assert B * h * ((w + 3) // 4) > 2048
    _flow_head_case(ops, name, B, h, w, cin)


def test_flow_head_out_full_size_general_path_beyond_its_cap(ops):
    """cin = 260 > 256 takes the general kernel; 128 x 129 = 16512 pixels > 4 x 4096: 128 waves take a second pixel"""
    _flow_head_case(ops, "general_16512_px_128x129_c260", 1, 128, 129, 260)


# ================================================================================================== 8. instnorm_nhwc
# (id, B, HW, C).  Partial sums per chunk of IN_ROWS = 512 rows, 256 / (C / 4) rows per sweep; every accepted channel count.
INSTNORM = [
    ("one_row_c32", 1, 1, 32),                              # variance 0: rstd = 1 / sqrt(eps); C = 32: 32 rows per sweep, one present
    ("two_chunks_513_c96", 2, 513, 96),                     # C = 96 (24 lanes per row, 10 row groups + 16 idle threads); second chunk holds one row
    ("one_short_511_c192", 1, 511, 192),                    # C = 192 (48 lanes, 5 row groups + 16 idle threads)
    ("three_chunks_1025_c32", 2, 1025, 32),                 # chunk index 2 holds one row
    ("four_chunks_1537_c64", 1, 1537, 64),                  # chunk index 3 holds one row
    ("seven_rows_c256", 1, 7, 256),                         # 4 rows per sweep: a second, partial sweep
    ("exact_chunk_512_c64", 1, 512, 64),                    # exactly one full chunk
]
EPS_IN = 1e-5


def _inorm(x, dtype):
    """x (B,HW,C) -> (B,HW,C), biased variance, eps inside the square root (F.instance_norm)"""
    x = x.to(dtype)
    m = x.mean(1, keepdim=True)
    v = ((x - m) ** 2).mean(1, keepdim=True)
    return (x - m) / torch.sqrt(v + EPS_IN)


@pytest.mark.parametrize("name,B,HW,C", INSTNORM, ids=_ids(INSTNORM))
def test_instnorm_nhwc_vs_fp64(ops, name, B, HW, C):
    """Channel 0 is constant: its output is exactly 0.  Channel 1 has mean 1000 and std 3e-3: the fp32 (B,C,2) mean / rstd hand-over
    costs 0.5 ulp32(mean) rstd there, the derived bound.  The other channels: max(2 err_ref, 2e-6)."""
    x = T(syn.normal("ge.in.x." + name, (B, HW, C), 4, std=3.0)) + 1.5
    x[..., 0] = 2.5
    x[..., 1] = 1000.0 + T(syn.normal("ge.in.big." + name, (B, HW), 4, std=3e-3))
    res = T(syn.normal("ge.in.r." + name, (B, HW, C), 5))
    n64, n32 = both(lambda dt: _inorm(x, dt))
    x64 = x.to(F64)
    mean1 = x64[..., 1].mean(1)
    rstd1 = 1.0 / torch.sqrt(((x64[..., 1] - mean1[:, None]) ** 2).mean(1) + EPS_IN)
    big = (0.5 * torch.from_numpy(np.spacing(mean1.numpy().astype(np.float32)).astype(np.float64)) * rstd1 + FLOOR["instnorm"])[:, None]      # (B,1)
    xd, rd = D(x.view(B, HW, 1, C)), D(res.view(B, HW, 1, C))
    for tag, relu, r in (("plain", False, None), ("relu", True, None), ("residual", True, res)):
        out = torch.full((B, HW, 1, C), float("nan"), device="cuda")
        ops.instnorm_nhwc(xd, relu=relu, residual=rd if r is not None else None, out=out)
        got = out.cpu().view(B, HW, C)
        f = lambda y: (torch.relu(r.to(y.dtype) + torch.relu(y)) if r is not None else (torch.relu(y) if relu else y))
        want0 = torch.relu(res[..., 0]) if r is not None else torch.zeros(B, HW)
        assert torch.equal(got[..., 0], want0), f"{name} {tag}: the constant channel"
        w64 = f(n64)
        e1 = (got[..., 1].to(F64) - w64[..., 1]).abs()
        print(f"glue_edges instnorm_nhwc.large_mean [{name}.{tag}] err_gpu {float(e1.max()):.3e} bound {float(big.max()):.3e}")
        assert bool((e1 <= big).all()), f"{name} {tag}: large-mean channel {float(e1.max()):.3e} > {float(big.max()):.3e}"
        gate("instnorm_nhwc", f"{name}.{tag}", got[..., 2:], w64[..., 2:], f(n32)[..., 2:], FLOOR["instnorm"])
    assert torch.equal(xd.cpu().view(B, HW, C), x)


# ================================================================================================== 9. instnorm_tiles_nhwc
# (id, B, HW, C) x tiles per image.  instnorm_finalize_tiles_kernel: 8 channels x 32 tile groups per workgroup, group g sums tiles
# g, g + 32, ...: 1 tile (31 idle groups), 31, 32 (every group one), 33 (group 0 takes two), 65 (group 0 takes three).
TILES_SHAPES = [
    ("one_row_c4", 1, 1, 4),                                # C < 8: half of the finalize workgroup's channel lanes idle; empty tiles
    ("77_rows_c12", 2, 77, 12),                             # C = 12: a second, half-filled channel block
    ("300_rows_c100", 1, 300, 100),                         # C = 100: not a multiple of 8, 13 channel blocks
    ("130_rows_c64", 3, 130, 64),
]
TPI = [1, 31, 32, 33, 65]


def _group_sizes(tag, HW, tpi):
    """HW rows in tpi contiguous groups of any sizes (every group non-empty where HW >= tpi, else most are empty)"""
    sizes = np.ones(tpi, np.int64) if HW >= tpi else np.zeros(tpi, np.int64)
    rest = HW - int(sizes.sum())
    if rest:
        sizes += np.bincount(np.minimum((syn.uniform(tag, (rest,), 9) * tpi).astype(np.int64), tpi - 1), minlength=tpi)
    assert int(sizes.sum()) == HW
    return sizes


@pytest.mark.parametrize("tpi", TPI)
@pytest.mark.parametrize("name,B,HW,C", TILES_SHAPES, ids=_ids(TILES_SHAPES))
def test_instnorm_tiles_nhwc_vs_fp64(ops, name, B, HW, C, tpi):
    case = f"{name}.tpi{tpi}"
    x = T(syn.normal("ge.it.x." + name, (B, HW, C), 4, std=3.0)) + 1.5
    res = T(syn.normal("ge.it.r." + name, (B, HW, C), 5, std=2.0)) - 0.7
    x64, res64 = x.to(F64), res.to(F64)
    ts = torch.zeros(B, tpi, C, 2, dtype=F64)
    for b in range(B):
        r0 = 0
        for k, n in enumerate(_group_sizes(f"ge.it.cut.{case}.{b}", HW, tpi)):
            ts[b, k, :, 0], ts[b, k, :, 1] = x64[b, r0:r0 + n].sum(0), (x64[b, r0:r0 + n] ** 2).sum(0)
            r0 += int(n)
    tsd = D(ts.view(B * tpi, C, 2), F64)
    xd, rd = D(x.view(B, HW, 1, C)), D(res.view(B, HW, 1, C))
    mean = x64.mean(1)
    rstd = 1.0 / torch.sqrt(((x64 - mean[:, None]) ** 2).mean(1) + EPS_IN)
    mr = ops.instnorm_tiles_nhwc(xd, tsd, stats_only=True).cpu().to(F64)
    assert tuple(mr.shape) == (B, C, 2)
    em, er = float(((mr[..., 0] - mean).abs() / mean.abs()).max()), float(((mr[..., 1] - rstd).abs() / rstd).max())
    print(f"glue_edges instnorm_tiles.stats [{case}] mean rel {em:.3e} rstd rel {er:.3e}")
    assert em <= 1e-6 and er <= 1e-6
    # the residual's own statistics, handed over in fp32 as the producing layer's finalize does: the reference reads the same numbers
    rm = res64.mean(1)
    rmr = torch.stack([rm, 1.0 / torch.sqrt(((res64 - rm[:, None]) ** 2).mean(1) + EPS_IN)], -1).to(F32)
    n64, n32 = both(lambda dt: _inorm(x, dt))
    rn = lambda dt: (res.to(dt) - rmr[None, :, :, 0].permute(1, 0, 2).to(dt)) * rmr[None, :, :, 1].permute(1, 0, 2).to(dt)
    forms = [
        ("plain", dict(relu=False), lambda y, dt: y),
        ("residual_raw", dict(relu=True, residual=rd), lambda y, dt: torch.relu(res.to(dt) + torch.relu(y))),
        ("residual_norm", dict(relu=True, residual=rd, residual_norm=D(rmr), residual_relu=False), lambda y, dt: torch.relu(rn(dt) + torch.relu(y))),
        ("residual_norm_relu", dict(relu=True, residual=rd, residual_norm=D(rmr), residual_relu=True),
         lambda y, dt: torch.relu(torch.relu(rn(dt)) + torch.relu(y))),
    ]
    for tag, kw, f in forms:
        out = torch.full((B, HW, 1, C), float("nan"), device="cuda")
        ops.instnorm_tiles_nhwc(xd, tsd, out=out, **kw)
        gate("instnorm_tiles_nhwc", f"{case}.{tag}", out.cpu().view(B, HW, C), f(n64, F64), f(n32, F32), FLOOR["instnorm"])
    assert torch.equal(rd.cpu().view(B, HW, C), res) and torch.equal(xd.cpu().view(B, HW, C), x)


# ================================================================================================== 10. pixel_head_nhwc
# 64-pixel tiles, at most 3 x CUs workgroups: a workgroup walks tile, tile + gridDim.x, ...
PIXEL_HEAD_MODES = [0, 1, 2]


def _pixel_head_case(ops, name, B, H, W, cin, cout, mode, norm):
    cs, co = cin + 8, 4
    x = syn.normal("ge.ph.x." + name, (B, H, W, cs), 4)
    x[0, H // 2, W // 3] = 0.0                               # an all-zero pixel (L2 mode with a zero bias: the 1e-12 clamp)
    wt = T(syn.normal("ge.ph.w." + name, (cout, cin), 4, std=float(np.sqrt(2.0 / cin))))
    bias = T(syn.uniform("ge.ph.b." + name, (cout,), 4, -0.05, 0.05)) * (mode != 1)
    mr = None
    if norm:
        mr = T(np.stack([syn.normal("ge.ph.m." + name, (B, cin), 5), syn.uniform("ge.ph.s." + name, (B, cin), 5, 0.5, 2.0)], -1))

    def ref(dt):
        src = T(x[..., co:co + cin]).to(dt)
        if norm:
            src = F.relu((src - mr[:, None, None, :, 0].to(dt)) * mr[:, None, None, :, 1].to(dt))
        y = src @ wt.to(dt).t() + bias.to(dt)
        if mode == 1:
            y = F.normalize(y, p=2, dim=-1, eps=1e-12)
        elif mode == 2:
            y = torch.sigmoid(y)
        return nchw(y)
    out = torch.full((B, cout, H, W), float("nan"), device="cuda")
    got = ops.pixel_head_nhwc(D(x), D(wt), D(bias), mode, src_c_offset=co, c_in=cin, mean_rstd=None if mr is None else D(mr), relu=norm, out=out)
    r64, r32 = both(ref)
    gate("pixel_head_nhwc", f"{name}.mode{mode}.norm{int(norm)}", got, r64, r32, FLOOR["pixel_head"])
    if mode == 1 and not norm:
        assert bool((got[0, :, H // 2, W // 3] == 0).all())


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "mean_rstd"])
@pytest.mark.parametrize("mode", PIXEL_HEAD_MODES)
def test_pixel_head_tile_walk_13_tiles(ops, mode, norm):
    """832 pixels = 13 tiles: a walk wherever fewer than 13 workgroups are launched (the host-executed device has 4 CUs: 12)"""
    _pixel_head_case(ops, "13_tiles_26x32", 1, 26, 32, 8, 3, mode, norm)


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "mean_rstd"])
@pytest.mark.parametrize("mode", PIXEL_HEAD_MODES)
def test_pixel_head_full_size_tile_walk_772_tiles(ops, mode, norm):
    """49408 pixels = 772 tiles > 3 x 256 workgroups: four workgroups of an MI355X take a second tile"""
    _pixel_head_case(ops, "772_tiles_193x256", 1, 193, 256, 8, 3, mode, norm)
