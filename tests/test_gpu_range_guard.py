"""The fp16x3 RANGE GUARD at every split site (csrc/f16x3.cuh; include/rnnpose_hip.h "fp16x3 range guard").

Every matrix-core kernel multiplies fp32 activations as fp16 hi + lo parts; beyond |x * a_scale| > 65504 (8188 at the package's a_scale = 8)
the split clamps, and a NaN becomes a finite value.  Each split site counts what it clamps, PoseRefiner returns the counter -- and on the
split-tensor schedule a consumer with src_hl checks nothing, so the producers' epilogue checks are the only guard there is.  This module
plants ONE element at a time into a clean tensor at every site (input staging of the 128-row and strip convolutions incl. stride 2 and the
fused input norm, stem, resident 1x1, lookup + convc1, mask head, volume pre-pass, split_hl, flow features; the split-form outputs and GRU
epilogues of every convolution family, the resident tile's epilogue) and asserts, per site:
  1. clean tensor: count 0;
  2. out of range (-9000), NaN, +Inf: count >= 1 and every output finite -- EXACTLY the number of offending quads where a value is staged
     once (resident 1x1, mask head, split_hl, flow features, pre-pass, every split-form output; lookup + convc1: (|corr| > 8188).sum());
  3. exactly at the limit (8188.0): count 0; at nextafter(8188, inf): counted;
  4. the same garbage (9e4, NaN) in channels outside the launch's windows, or in rows behind its last pixel: count 0;
  5. guard off: count 0 and outputs bit-identical; the device-side peek equals the host read;
  6. src_bounded launches count nothing, input or output (documented in the header: pinned so that a change is deliberate).
Accuracy at the top of the range (|x| ~ 7.9e3): silent guard, fp32-class against fp64 by tests/test_gpu_conv.py's own check().
Shapes are tiny (at most 3 x 11 x 19 pixels; the 16 x 17 pyramid of the lookup and the 20 x 32 stride-2 layer apart): the module also runs on
the host-execution tier (tests/test_kernels_on_host.py), where profiles/range_guard_mutation.txt records that deleting any one site's count
fails a test here."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rnnpose_amd import synthetic as syn
from test_gpu_conv import D, check, nchw, nhwc, ops  # noqa: F401  (ops: the module-scoped build fixture)

pytestmark = pytest.mark.gpu

LIM = 65504.0 / 8.0                                              # 8188: the largest magnitude that fits at a_scale = 8
NEXT = float(np.nextafter(np.float32(LIM), np.float32(np.inf)))
NAN, INF = float("nan"), float("inf")
BAD = (-9000.0, NAN, INF)


@contextmanager
def guarded(ops):
    """Guard on and counter zero inside; the process-wide switches back at their defaults afterwards, whatever happened."""
    from rnnpose_amd import _lib
    ops.saturation_check(True)
    ops.saturation_count(reset=True)
    try:
        yield
    finally:
        ops.saturation_check(True)
        ops.conv_strip(1)
        _lib.call("rnnpose_stem_workgroups", 0)
        ops.saturation_count(reset=True)


def count(ops, run):
    """-> (events of one run() on a zeroed counter, what run() returned)."""
    ops.saturation_count(reset=True)
    outs = run()
    return ops.saturation_count(), outs


def bits(t):
    return t.contiguous().view(torch.int32)


def finite(outs):
    return all(bool(torch.isfinite(o).all()) for o in outs)


def gen(name, shape, seed, std=1.0):
    return D(syn.normal("rg." + name, shape, seed, std=std))


class Site:
    """One split site: `run()` launches it on the tensors it closes over and returns the fp32 views of what it wrote (split-form
    outputs decoded); `plants` = [(tensor, index, exact count or None for "at least one")]; `outside` = [(tensor, index)] positions the
    launch must not look at.  `bad` are planted one after the other; `lim` must stay silent, `nxt` (if any) must be counted."""

    def __init__(self, run, plants, outside=(), bad=BAD, lim=LIM, nxt=NEXT):
        self.run, self.plants, self.outside, self.bad, self.lim, self.nxt = run, list(plants), list(outside), tuple(bad), lim, nxt


def exercise(ops, s, what=""):
    """Assertions 1-5 of the module docstring on one site."""
    with guarded(ops):
        n, outs = count(ops, s.run)
        assert n == 0 and finite(outs), f"{what}: clean tensor counted {n}"
        first = True
        for t, idx, want in s.plants:
            keep = float(t[idx])
            for v in s.bad + ((s.nxt,) if s.nxt is not None else ()):
                t[idx] = v
                n, outs = count(ops, s.run)
                assert finite(outs), f"{what}: {v} at {idx} gave a non-finite output"
                if want is None:
                    assert n >= 1, f"{what}: {v} at {idx} was not counted"
                else:
                    assert n == want, f"{what}: {v} at {idx} counted {n}, not {want}"
            if first and (want is None or want > 0):              # 5. (the last planted value is still in place)
                first = False
                s.run()
                peek = int(ops.saturation_events().item())
                assert peek == ops.saturation_count(reset=False) == n, f"{what}: device-side peek {peek}, host read {n}"
                ops.saturation_check(False)
                try:
                    n_off, off = count(ops, s.run)
                finally:
                    ops.saturation_check(True)
                assert n_off == 0 and ops.saturation_count() == 0, f"{what}: counted with the guard off"
                assert all(torch.equal(bits(a), bits(b)) for a, b in zip(outs, off)), f"{what}: the guard changes the output"
            t[idx] = s.lim
            n, _ = count(ops, s.run)
            assert n == 0, f"{what}: the limit {s.lim} at {idx} counted {n}"
            t[idx] = keep
        for t, idx in s.outside:                                 # 4.
            keep = float(t[idx])
            for v in (9.0e4, NAN):
                t[idx] = v
                n, _ = count(ops, s.run)
                assert n == 0, f"{what}: {v} outside the window at {idx} counted {n}"
            t[idx] = keep
        n, _ = count(ops, s.run)
        assert n == 0, f"{what}: not clean after the plants were taken back"


# ---- sites that stage every value once: exact counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [4, 36, 324])
def test_resident_1x1_input(ops, cin):
    """conv1x1_resident: 35 pixels (a ragged second tile of 3 rows + 29 padding rows that re-read pixel 34), source at channel offset 4 of a
    wider tensor that also has a row of pixels behind the launch's last one."""
    big = torch.ones(1, 6, 7, cin + 8, device="cuda")
    x = big[:, :5]
    pc = ops.PackedConv1x1(gen("r1w", (256, cin, 1, 1), 3, std=0.05), gen("r1b", (256,), 3, std=0.1))
    out = torch.empty(1, 5, 7, 256, device="cuda")

    def run():
        ops.conv1x1_resident(pc, (x, 4), (out, 0), relu=False)
        return [out]
    plants = [(x, (0, 0, 0, 4), 1), (x, (0, 4, 6, 4), 1), (x, (0, 4, 6, 4 + cin - 1), 1), (x, (0, 2, 3, 4 + cin - 4), 1)]
    outside = [(x, (0, 0, 0, 3)), (x, (0, 4, 6, 4 + cin)), (big, (0, 5, 0, 4)), (big, (0, 5, 6, 4 + cin - 1))]
    exercise(ops, Site(run, plants, outside), f"resident 1x1, c_in {cin}")


def test_mask_head_input(ops):
    """mask_upsample: 39 pixels (a ragged second tile: 7 rows + 25 padding rows that re-read pixel 38), x at channel offset 8 of 264."""
    big = torch.ones(1, 4, 13, 264, device="cuda")
    x = big[:, :3]
    pm = ops.PackedMaskHead(gen("mw", (576, 256, 1, 1), 5, std=0.01), gen("mb", (576,), 5, std=0.1))
    flow = gen("mf", (1, 3, 13, 2), 5, std=2.0)

    def run():
        return [ops.mask_upsample(pm, x, 8, flow)]
    plants = [(x, (0, 0, 0, 8), 1), (x, (0, 2, 12, 263), 1), (x, (0, 1, 6, 8 + 100), 1), (x, (0, 2, 12, 8), 1)]
    outside = [(x, (0, 0, 0, 7)), (x, (0, 2, 12, 0)), (big, (0, 3, 0, 8)), (big, (0, 3, 12, 263))]
    exercise(ops, Site(run, plants, outside), "mask head")


def test_split_hl_input(ops):
    """split_hl with source and destination offsets: one event per 8-channel group."""
    src = gen("sh", (2, 3, 5, 40), 7)
    dst = torch.zeros(2, 3, 5, 48, device="cuda")

    def run():
        ops.split_hl(src, dst, src_c_offset=8, c_count=24, dst_c_offset=16)
        return [ops.unsplit_hl(dst)]
    plants = [(src, (0, 0, 0, 8), 1), (src, (1, 2, 4, 31), 1), (src, (0, 1, 2, 19), 1)]
    outside = [(src, (0, 0, 0, 7)), (src, (1, 2, 4, 32)), (src, (0, 0, 0, 0)), (src, (1, 2, 4, 39))]
    exercise(ops, Site(run, plants, outside), "split_hl")


@pytest.mark.parametrize("layout", [0, 1])
def test_volume_prepass_input(ops, layout):
    """The operand split of the fp16x3 volume build, NCHW (an event per element) and pixel-major (per 8-channel group) sources."""
    shape = (1, 64, 5, 7) if layout == 0 else (1, 5, 7, 64)
    f1, f2 = gen("pf1", shape, 9), gen("pf2", shape, 9)

    def run():
        _, lv = ops.corr_pyramid(f1, f2, 2, precision="f16x3") if layout == 0 else ops.corr_pyramid_nhwc(f1, f2, 2)
        return list(lv)
    last = tuple(n - 1 for n in shape)
    plants = [(f1, (0, 0, 0, 0), 1), (f1, last, 1), (f2, (0, 0, 0, 0), 1), (f2, last, 1)]
    exercise(ops, Site(run, plants), f"volume pre-pass, layout {layout}")


def _flow_features(ops, out_split, motion_split, tap=24):
    B, h, w = 2, 5, 23                                           # two 20-pixel row segments per line, the second ragged
    coords = gen("fc", (B, 2, h, w), 11, std=3.0)
    w_t = torch.zeros(98, 128, device="cuda")
    w_t[tap, 5] = 2.0                                            # out[..., 5] = relu(2 * flow.x) (tap 24: the centre tap of input channel 0)
    bias = torch.zeros(128, device="cuda")
    out, motion = torch.zeros(B, h, w, 128, device="cuda"), torch.zeros(B, h, w, 128, device="cuda")

    def run():
        ops.flow_features(coords, w_t, bias, out, motion, 126, subtract_grid=False, out_split=out_split, motion_split=motion_split)
        res = []
        if out_split:
            res.append(ops.unsplit_hl(out))
        if motion_split:
            res.append(ops.unsplit_hl(motion)[..., 126:])
        return res
    return coords, run


def test_flow_features_motion_split(ops):
    """flow_features(motion_split=True): the flow itself is split into the motion tensor -- one event per pixel whose pair leaves the range."""
    coords, run = _flow_features(ops, False, True)
    plants = [(coords, (0, 0, 0, 0), 1), (coords, (1, 1, 4, 22), 1), (coords, (0, 1, 2, 20), 1)]
    exercise(ops, Site(run, plants), "flow features, motion")


def test_flow_features_out_split(ops):
    """flow_features(out_split=True): in-range flow, one weight of 2: relu(2 * 4094) = 8188 fits, the next float does not; one event per
    (channel, 20-pixel row segment).  The fp32 destinations of the same launch count nothing."""
    coords, run = _flow_features(ops, True, False)
    half = LIM / 2
    plants = [(coords, (0, 0, 0, 0), 1), (coords, (1, 0, 4, 22), 1), (coords, (0, 0, 2, 19), 1)]
    exercise(ops, Site(run, plants, bad=(5000.0, 8000.0), lim=half, nxt=float(np.nextafter(np.float32(half), np.float32(np.inf)))), "flow features, out")
    # a ragged row segment (w = 23: positions 20 .. 22 of 20 .. 39) computes all 20 positions; the three behind the line's end still see real
    # flow through the 7-tap window, but no pixel receives them: with the weight on the LEFTMOST tap (out[x] = 2 flow[x - 3]) the last three
    # columns feed only such positions
    coords, run = _flow_features(ops, True, False, tap=21)
    with guarded(ops):
        for xx, want in ((22, 0), (21, 0), (20, 0), (19, 1), (16, 1), (0, 1)):
            keep = float(coords[1, 0, 3, xx])
            coords[1, 0, 3, xx] = 5000.0
            n, outs = count(ops, run)
            assert n == want and finite(outs), f"flow features, out, leftmost tap: 5000 in column {xx} counted {n}, not {want}"
            coords[1, 0, 3, xx] = keep
    coords32, run32 = _flow_features(ops, False, False)
    with guarded(ops):
        coords32[0, 0, 0, 0] = 8000.0
        coords32[1, 1, 4, 22] = 9000.0
        assert count(ops, run32)[0] == 0


# ---- convolutions, fp32 sources: the staging loops (a quad is counted once per staging: at least one) ----------------------------------
def _conv_in(ops, B, H, W, segs, cout, kh, kw, stride=1):
    """Clean sources (small normals in channels [8, 8 + c) of wider tensors that hold one more image than the launch sees), small weights."""
    bigs = [gen(f"ci{i}", (B + 1, H, W, c + 16), 13) for i, c in enumerate(segs)]
    pc = ops.PackedConv(gen("cw", (cout, sum(segs), kh, kw), 13, std=0.01), gen("cb", (cout,), 13, std=0.1), segs)
    out = torch.empty(B, -(-H // stride), -(-W // stride), cout, device="cuda")
    return bigs, [(b[:B], 8) for b in bigs], pc, out


# (tile, strip mode): the 128-row kernels in both tile shapes; 160- / 32- / 96-row strips, register path; two column tiles per wave
KH_KW = [(3, 3), (1, 5), (5, 1)]
CONV_IN = [(t, 1, kh, kw) for t in (1, 2) for kh, kw in KH_KW + [(1, 1)]] + [(t, 1, kh, kw) for t in (5, 6, 7) for kh, kw in KH_KW] + \
          [(5, 3, 3, 3), (5, 3, 1, 5), (5, 7, 3, 3)]


@pytest.mark.parametrize("tile,mode,kh,kw", CONV_IN)
def test_conv_input(ops, tile, mode, kh, kw):
    """Two fp32 sources at channel offset 8.  One output column tile (48 channels; 96 for two tiles per wave), so a count taken in any
    column tile but the first would be lost.  mode 7: the persistent form of the 160-row 3x3 launch where the device is small enough for 12
    three-wave workgroups to be 1.5 rounds (the host tier's 4 CUs: the last image's patches are every workgroup's SECOND tile; an ordinary
    launch on a whole chip)."""
    B, H, W = (3, 11, 19) if mode == 7 else (2, 5, 7)
    bigs, srcs, pc, out = _conv_in(ops, B, H, W, [64, 32], 96 if mode in (3, 7) else 48, kh, kw)
    x0, x1 = srcs[0][0], srcs[1][0]

    def run():
        ops.conv_strip(mode)
        ops.conv2d_nhwc(pc, srcs, (out, 0), tile=tile)
        return [out]
    plants = [(x0, (0, 0, 0, 8), None), (x1, (B - 1, H - 1, W - 1, 8 + 31), None), (x0, (0, H - 1, W - 1, 8 + 5), None),
              (x0, (1, 0, 0, 8 + 5), None), (x0, (0, H // 2, W // 2, 8 + 40), None)]
    outside = [(x0, (0, 0, 0, 7)), (x0, (B - 1, H - 1, W - 1, 8 + 64)), (x1, (0, 0, 0, 0)), (bigs[0], (B, 0, 0, 8)), (bigs[1], (B, H - 1, W - 1, 8 + 31))]
    exercise(ops, Site(run, plants, outside), f"conv {kh}x{kw}, tile {tile}, strip mode {mode}")


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("tile", [0, 1, 5])
def test_conv_input_stride2(ops, tile, k):
    """The encoder's stride-2 layers, 20 x 32 x 64 -> 96.  A 1x1 stride-2 launch never reads an odd position: it counts NOTHING there."""
    bigs, srcs, pc, out = _conv_in(ops, 1, 20, 32, [64], 96, k, k, stride=2)
    x = srcs[0][0]

    def run():
        ops.conv2d_nhwc(pc, srcs, (out, 0), stride=2, tile=tile)
        return [out]
    odd = None if k == 3 else 0
    plants = [(x, (0, 0, 0, 8 + 3), None), (x, (0, 19, 31, 8 + 63), odd), (x, (0, 19, 30, 8 + 3), odd), (x, (0, 18, 31, 8 + 3), odd)]
    outside = [(x, (0, 0, 0, 7)), (x, (0, 18, 30, 8 + 64)), (bigs[0], (1, 0, 0, 8))]
    exercise(ops, Site(run, plants, outside), f"conv {k}x{k} stride 2, tile {tile}")


@pytest.mark.parametrize("tile", [1, 5, 6, 7])
def test_conv_input_fused_norm(ops, tile):
    """in_norm: relu((x - mean) * rstd) is what is split, so that is what is tested: a raw in-range element that leaves the range once
    normalised counts, a raw out-of-range one that comes back does not; 9188 - 1000 = 8188 fits, the next float does not.  (The ReLU is
    part of the load: what it turns into 0 -- -Inf, and a NaN, which fmaxf drops -- is in range when it is split.  No NaN is planted here.)"""
    B, H, W, Cs, o = 2, 5, 7, 64, 8                              # channels [8, 72) of an 80-channel tensor that holds one more image than the launch sees
    big = gen("nx", (B + 1, H, W, Cs + 16), 15)
    x = big[:B]
    pc = ops.PackedConv(gen("nw", (48, Cs, 3, 3), 15, std=0.01), gen("nb", (48,), 15, std=0.1), [Cs])
    mr = torch.zeros(B, Cs + 16, 2, device="cuda")               # (indexed by the channel of the TENSOR)
    mr[..., 1] = 1.0
    mr[:, o + 3, 1] = 100.0
    mr[:, o + 40, 1] = 0.5
    mr[:, o + 63, 0] = 1000.0
    x[..., o + 20] = -100.0 + 0.01 * x[..., o + 20]              # channel 20: mean -100, rstd 100 -- every pixel normalises to ~ 1, but a padding
    mr[:, o + 20, 0], mr[:, o + 20, 1] = -100.0, 100.0           # row's zero WOULD normalise to 1e4: halo rows become zeros AFTER the norm and never count
    out = torch.empty(B, H, W, 48, device="cuda")

    def run():
        ops.conv2d_nhwc(pc, [(x, o)], (out, 0), in_norm=mr, tile=tile)
        return [out]
    # channel 63 (mean 1000, rstd 1) through every assertion of exercise(): with the guard on, a launch with in_norm on the 128-row kernels takes
    # instantiations of its own (csrc/conv_igemm.hip), so "guard off: bit-identical" compares two kernels here
    plants = [(x, (0, 0, 0, o + 63), None), (x, (B - 1, H - 1, W - 1, o + 63), None), (x, (0, H // 2, W // 2, o + 63), None)]
    outside = [(x, (0, 0, 0, o - 1)), (x, (B - 1, H - 1, W - 1, o + Cs)), (x, (0, 2, 3, 0)), (big, (B, 0, 0, o + 63)), (big, (B, H - 1, W - 1, o + 3))]
    exercise(ops, Site(run, plants, outside, bad=(1.0e4, INF), lim=9188.0, nxt=float(np.nextafter(np.float32(9188.0), np.float32(np.inf)))),
             f"fused norm, tile {tile}")
    with guarded(ops):
        assert count(ops, run)[0] == 0
        for idx, v, counted in (((0, 0, 0, o + 3), 100.0, True), ((1, 4, 6, o + 3), 100.0, True), ((1, 4, 6, o + 40), 9000.0, False), ((0, 2, 3, o + 40), 16000.0, False),
                                ((1, 0, 0, o + 3), INF, True), ((0, 2, 3, o + 40), -INF, False)):
            keep = float(x[idx])
            x[idx] = v
            n, outs = count(ops, run)
            assert finite(outs) and (n >= 1 if counted else n == 0), f"fused norm, tile {tile}: {v} at {idx} counted {n}"
            if counted:                                              # guard off: nothing counted, the same bits (two kernels on the 128-row path)
                ops.saturation_check(False)
                try:
                    off = torch.empty_like(out)
                    n_off, _ = count(ops, lambda: ops.conv2d_nhwc(pc, [(x, o)], (off, 0), in_norm=mr, tile=tile))
                finally:
                    ops.saturation_check(True)
                assert n_off == 0 and torch.equal(bits(out), bits(off)), f"fused norm, tile {tile}: guard off differs at {idx}"
            x[idx] = keep


@pytest.mark.parametrize("tile", [1, 5])
def test_conv_src_bounded_counts_nothing(ops, tile):
    """include/rnnpose_hip.h: with src_bounded "the range guard skips this launch" and "split-form outputs of such a launch are not
    range-checked either".  Pinned: whoever changes it does so on purpose."""
    bigs, srcs, pc, out = _conv_in(ops, 2, 5, 7, [64, 32], 48, 3, 3)
    outs = torch.zeros(2, 5, 7, 48, device="cuda")
    with guarded(ops):
        srcs[0][0][1, 2, 3, 8 + 9] = -9000.0
        assert count(ops, lambda: ops.conv2d_nhwc(pc, srcs, (out, 0), tile=tile))[0] >= 1
        assert count(ops, lambda: ops.conv2d_nhwc(pc, srcs, (out, 0), tile=tile, src_bounded=True))[0] == 0
        srcs[0][0][1, 2, 3, 8 + 9] = 1.0
        run, plant, _, _ = _one_weight_conv(ops, tile, 1, False, "dst_hl")
        plant[1, 1, 3, 8 + 3] = 2000.0
        assert count(ops, run)[0] == 1
        assert count(ops, lambda: run(src_bounded=True))[0] == 0


# ---- stem ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (1, 9, 5), (2, 37, 41)])
@pytest.mark.parametrize("normalize", [False, True])
def test_stem_input(ops, normalize, N, H, W):
    """stem_conv with 8 workgroups walking all tiles; a texel in the overlap of two 16 x 32 input patches is staged (and counted) twice.
    With `normalize` the limit is on 2 x / 255 - 1: 8189 * 127.5 fits exactly, the next float does not."""
    from rnnpose_amd import _lib
    ps = ops.PackedStem(gen("sw", (64, 3, 7, 7), 17, std=0.05), gen("sb", (64,), 17, std=0.1))
    img = gen("si", (N, 3, H, W), 17) * 50.0 + 128.0 if normalize else gen("si", (N, 3, H, W), 17)

    def run():
        _lib.call("rnnpose_stem_workgroups", 8)
        return [ops.stem_conv(ps, img, normalize=normalize)[0]]
    plants = [(img, (N - 1, 2, H - 1, W - 1), None), (img, (0, 0, 0, 0), None)] + ([(img, (0, 1, 5, 30), None), (img, (1, 2, 16, 9), None)] if H > 16 else [])
    if normalize:
        top = 8189.0 * 127.5
        site = Site(run, plants, bad=(1.1e6, -1.1e6, NAN, INF), lim=top, nxt=float(np.nextafter(np.float32(top), np.float32(np.inf))))
    else:
        site = Site(run, plants)
    exercise(ops, site, f"stem, normalize {normalize}, {N} x {H} x {W}")
    if normalize:
        with guarded(ops):
            img[0, 0, 0, 0] = 9000.0                             # beyond 8188 as a raw value, far inside once normalised
            assert count(ops, run)[0] == 0


# ---- lookup + convc1 -------------------------------------------------------------------------------------------------------------------
def _grid(nb, h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], 0)[None].repeat(nb, 1, 1, 1).cuda()


def _big_pyramid(ops, factor, at=(2, 3)):
    """2 x 16 x 17 pyramid (four levels of at least 2 x 2 need 16 lines) whose image 1 holds level-0 values of magnitude ~ factor * 8 at the target pixel `at`."""
    f1, f2 = gen("lf1", (2, 64, 16, 17), 19), gen("lf2", (2, 64, 16, 17), 19)
    f2[1, :, at[0], at[1]] = factor * f1[1, :, at[0], at[1]]
    return ops.corr_pyramid(f1, f2, 4)[0]


@pytest.mark.parametrize("shift", [0.0, 0.5, 1.0, 100.0], ids=["on", "between", "next", "far"])
def test_lookup_convc1_input(ops, shift):
    """corr_lookup_convc1 forms its window taps itself and splits each once: the count is exactly the number of taps beyond the range, as
    corr_lookup_nhwc_part delivers them for the same centres (the same operations per element).  272 pixels: a ragged ninth tile."""
    buf = _big_pyramid(ops, 8000.0, at=(15, 16))         # the LAST pixel: the 16 padding rows of the ragged tile form its taps again
    pc = ops.PackedConv1x1(gen("lw", (256, 324, 1, 1), 19, std=0.01), gen("lb", (256,), 19, std=0.1))
    out = torch.empty(1, 16, 17, 256, device="cuda")
    corr = torch.empty(1, 16, 17, 324, device="cuda")
    with guarded(ops):
        for b0, expect_some in ((1, shift < 50), (0, False)):
            coords = _grid(1, 16, 17) + shift
            ops.corr_lookup_nhwc_part(buf, coords, corr, 2, b0, b0 + 1)
            want = int((~(corr.abs() <= LIM)).sum())
            assert (want > 0) == expect_some, (shift, b0, want)
            n, _ = count(ops, lambda: ops.corr_lookup_convc1(pc, buf, coords, (out, 0), 2, b0, b0 + 1))
            assert n == want and finite([out]), f"lookup + convc1, centres + {shift}, image {b0}: counted {n}, {want} taps are beyond the range"
            if want:
                ops.corr_lookup_convc1(pc, buf, coords, (out, 0), 2, b0, b0 + 1)
                assert int(ops.saturation_events().item()) == ops.saturation_count(reset=False) == want    # the device-side peek
                ops.saturation_check(False)
                try:
                    off = torch.empty_like(out)
                    n_off, _ = count(ops, lambda: ops.corr_lookup_convc1(pc, buf, coords, (off, 0), 2, b0, b0 + 1))
                finally:
                    ops.saturation_check(True)
                assert n_off == 0 and torch.equal(bits(out), bits(off))


# ---- split-form outputs: inputs in range, the result is not ----------------------------------------------------------------------------
HALF_UP = float(np.nextafter(np.float32(1023.5), np.float32(np.inf)))


def _one_weight_conv(ops, tile, mode, src_hl, form, kh=3, kw=3):
    """3x3 convolution 64 -> 96 with ONE weight of 8 (output channel 5 <- input channel 3, centre tap), bias 0, sources of ones: 2000 at a
    pixel gives exactly 16000 there, 1023.5 exactly 8188.  form: "dst_hl" (the destination is split) or "dst_split" (the extra copy)."""
    B, cout = 2, 96
    H, W = (11, 19) if (tile >= 5 and mode == 1) else (5, 7)      # strips: a whole first patch (the fast epilogue) and ragged ones (the general one)
    w = torch.zeros(cout, 64, kh, kw, device="cuda")
    w[5, 3, kh // 2, kw // 2] = 8.0
    pc = ops.PackedConv(w, torch.zeros(cout, device="cuda"), [32, 32])
    xa, xb = torch.ones(B, H, W, 48, device="cuda"), torch.ones(B, H, W, 48, device="cuda")
    dst, extra = torch.zeros(B, H, W, cout + 16, device="cuda"), torch.zeros(B, H, W, cout + 16, device="cuda")

    def run(**kw_):
        ops.conv_strip(mode)
        srcs = [(ops.split_hl(xa), 8), (ops.split_hl(xb), 8)] if src_hl else [(xa, 8), (xb, 8)]
        if form == "dst_hl":
            ops.conv2d_nhwc(pc, srcs, (dst, 8), src_hl=src_hl, dst_hl=True, tile=tile, **kw_)
            return [ops.unsplit_hl(dst)[..., 8:8 + cout]]
        ops.conv2d_nhwc(pc, srcs, (dst, 8), src_hl=src_hl, dst_split=(extra, 8), tile=tile, **kw_)
        return [dst[..., 8:8 + cout], ops.unsplit_hl(extra)[..., 8:8 + cout]]
    return run, xa, H, W


@pytest.mark.parametrize("form", ["dst_hl", "dst_split"])
@pytest.mark.parametrize("src_hl", [False, True], ids=["fp32-sources", "split-sources"])
@pytest.mark.parametrize("tile,mode", [(1, 1), (2, 1), (5, 1), (6, 1), (7, 1), (5, 3)])
def test_conv_split_output(ops, tile, mode, src_hl, form):
    """The epilogues that write split tensors (store_quad_hl; the strips' fast epilogue, and the general one with two tiles per wave): with
    split sources this check is the only one the value ever meets.  Exactly one quad leaves the range."""
    run, x, H, W = _one_weight_conv(ops, tile, mode, src_hl, form)
    plants = [(x, (0, 0, 0, 8 + 3), 1), (x, (1, H - 1, W - 1, 8 + 3), 1), (x, (1, 1, 3, 8 + 3), 1)]
    exercise(ops, Site(run, plants, bad=(2000.0, -2000.0), lim=1023.5, nxt=HALF_UP), f"conv split output {form}, tile {tile}, mode {mode}, src_hl {src_hl}")


def _gru(ops, tile, mode, C=96):
    B, H, W = (2, 11, 19) if (tile >= 5 and mode == 1) else (2, 5, 7)      # strips: whole runs of 160 / 96 / 32 pixels (the fast epilogue) and a ragged last one
    hN, xN = gen("gh", (B, H, W, C), 21, std=0.5), gen("gx", (B, H, W, 32), 21)
    haux = gen("ga", (B, H, W, C), 21, std=0.5)
    bias = torch.zeros(2 * C, device="cuda")
    bias[C:] = 20.0                                              # r = sigmoid(20) = 1 in fp32: r * h = h
    pzr = ops.PackedConv(torch.zeros(2 * C, C + 32, 1, 5, device="cuda"), bias, [C, 32])
    pq = ops.PackedConv(torch.zeros(C, C + 32, 1, 5, device="cuda"), torch.zeros(C, device="cuda"), [C, 32])
    am = torch.zeros(B, H, W, 3 * C, device="cuda")
    return B, H, W, C, hN, xN, haux, pzr, pq, am


GRU_TILES = [(1, 1), (5, 1), (6, 1), (7, 1), (5, 3)]


@pytest.mark.parametrize("tile,mode", GRU_TILES)
def test_gru_zr_epilogue_split_output(ops, tile, mode):
    """EPI_GRU_ZR: r * h goes to dst2; in split form (dst2_hl) an h beyond the range (or not finite) is counted once, the fp32 form of the
    same launch counts nothing."""
    B, H, W, C, hN, xN, haux, pzr, pq, am = _gru(ops, tile, mode)
    z, rh = torch.empty(B, H, W, C, device="cuda"), torch.zeros(B, H, W, C, device="cuda")

    def run(hl=True):
        ops.conv_strip(mode)
        ops.conv2d_nhwc(pzr, [(hN, 0), (xN, 0)], (z, 0), ops.EPI_GRU_ZR, aux0=(haux, 0), dst2=(rh, 0), dst2_hl=hl, gru_c=C, add_map=(am, 0), tile=tile)
        return [z, ops.unsplit_hl(rh)] if hl else [z]
    plants = [(haux, (0, 0, 0, 0), 1), (haux, (1, H - 1, W - 1, C - 1), 1), (haux, (0, 2, 3, 17), 1)]
    exercise(ops, Site(run, plants, bad=(2.0e4, NAN, INF)), f"GRU z|r epilogue, tile {tile}, mode {mode}")
    with guarded(ops):
        haux[0, 2, 3, 17] = 2.0e4
        assert count(ops, lambda: run(False))[0] == 0


@pytest.mark.parametrize("tile,mode", GRU_TILES)
def test_gru_q_epilogue_split_output(ops, tile, mode):
    """EPI_GRU_Q with z = 0: h' = h.  The split copy (dst_split) of an h' beyond the range is counted once; the fp32-only form counts nothing."""
    B, H, W, C, hN, xN, haux, pzr, pq, am = _gru(ops, tile, mode)
    z = torch.zeros(B, H, W, C, device="cuda")
    hnew, hs = torch.empty(B, H, W, C, device="cuda"), torch.zeros(B, H, W, C, device="cuda")

    def run(split=True):
        ops.conv_strip(mode)
        ops.conv2d_nhwc(pq, [(hN, 0), (xN, 0)], (hnew, 0), ops.EPI_GRU_Q, aux0=(haux, 0), aux1=(z, 0), dst_split=(hs, 0) if split else None,
                        add_map=(am, 2 * C), tile=tile)
        return [ops.unsplit_hl(hs)] if split else []
    plants = [(haux, (0, 0, 0, 0), 1), (haux, (1, H - 1, W - 1, C - 1), 1), (haux, (0, 2, 3, 17), 1)]
    exercise(ops, Site(run, plants, bad=(2.0e4, NAN, INF)), f"GRU state epilogue, tile {tile}, mode {mode}")
    with guarded(ops):
        haux[0, 2, 3, 17] = 2.0e4
        assert count(ops, lambda: run(False))[0] == 0


@pytest.mark.parametrize("cin", [4, 36])
def test_resident_1x1_split_output(ops, cin):
    """conv1x1_resident(dst_split=True): resident_tile.cuh's epilogue, one weight of 8, 35 pixels."""
    w = torch.zeros(256, cin, 1, 1, device="cuda")
    w[250, 1] = 8.0
    pc = ops.PackedConv1x1(w, torch.zeros(256, device="cuda"))
    x, dst = torch.ones(1, 5, 7, cin + 8, device="cuda"), torch.zeros(1, 5, 7, 264, device="cuda")

    def run():
        ops.conv1x1_resident(pc, (x, 4), (dst, 8), relu=True, dst_split=True)
        return [ops.unsplit_hl(dst)[..., 8:]]
    plants = [(x, (0, 0, 0, 5), 1), (x, (0, 4, 6, 5), 1), (x, (0, 2, 3, 5), 1)]
    exercise(ops, Site(run, plants, bad=(2000.0,), lim=1023.5, nxt=HALF_UP), f"resident 1x1 split output, c_in {cin}")


def test_lookup_convc1_split_output(ops):
    """corr_lookup_convc1(dst_split=True): every tap in range, one weight of 8 on the window centre of level 0: the count is exactly the
    number of quads of the fp32 form of the same launch that hold a value beyond the range."""
    buf = _big_pyramid(ops, 150.0)
    w = torch.zeros(256, 324, 1, 1, device="cuda")
    w[9, 40] = 8.0
    pc = ops.PackedConv1x1(w, torch.zeros(256, device="cuda"))
    coords = _grid(1, 16, 17)
    y32, ys = torch.empty(1, 16, 17, 256, device="cuda"), torch.zeros(1, 16, 17, 256, device="cuda")
    with guarded(ops):
        for b0 in (1, 0):
            n32, _ = count(ops, lambda: ops.corr_lookup_convc1(pc, buf, coords, (y32, 0), 2, b0, b0 + 1))
            assert n32 == 0, "a tap left the range: the test's own inputs are wrong"
            want = int((~(y32.view(1, 16, 17, 64, 4).abs() <= LIM)).any(-1).sum())
            assert (want >= 1) == (b0 == 1)
            n, _ = count(ops, lambda: ops.corr_lookup_convc1(pc, buf, coords, (ys, 0), 2, b0, b0 + 1, dst_split=True))
            assert n == want and finite([ops.unsplit_hl(ys)]), f"lookup + convc1 split output, image {b0}: counted {n}, {want} quads are beyond the range"


# ---- accuracy at the top of the range: a silent guard is not enough ---------------------------------------------------------------------
MAG = 7.9e3


def _top(name, shape, seed):
    """|x| < 7.9e3 (the hash generator's normal is bounded by 3.47 sigma), the largest element 1.03 x that: just inside the range."""
    x = syn.normal("rg." + name, shape, seed, std=1.0 / 3.6) * MAG
    x.reshape(-1)[x.size // 3] = MAG * 1.03
    return D(x)


def _silent(ops, run):
    with guarded(ops):
        n, out = count(ops, run)
    assert n == 0, f"{n} range events for inputs inside the range"
    return out


def test_stem_accuracy_at_the_top_of_the_range(ops):
    img = _top("ai", (2, 3, 37, 41), 23)
    w, b = gen("aw", (64, 3, 7, 7), 23, std=float(np.sqrt(2.0 / 147))), gen("ab", (64,), 23) * (0.1 * MAG)
    y = _silent(ops, lambda: ops.stem_conv(ops.PackedStem(w, b), img, normalize=False)[0])
    check(nchw(y), F.conv2d(img.double(), w.double(), b.double(), stride=2, padding=3), F.conv2d(img, w, b, stride=2, padding=3), "stem, |x| ~ 7.9e3")


def test_resident_1x1_accuracy_at_the_top_of_the_range(ops):
    x = _top("ax", (1, 324, 5, 7), 25)
    w, b = gen("rw", (256, 324, 1, 1), 25, std=0.4 * float(np.sqrt(2.0 / 324))), gen("rb", (256,), 25) * (0.05 * MAG)
    y, ys = torch.empty(1, 5, 7, 256, device="cuda"), torch.empty(1, 5, 7, 256, device="cuda")
    pc = ops.PackedConv1x1(w, b)

    def run():
        ops.conv1x1_resident(pc, (nhwc(x), 0), (y, 0), relu=True)
        ops.conv1x1_resident(pc, (nhwc(x), 0), (ys, 0), relu=True, dst_split=True)
    _silent(ops, run)
    check(nchw(y), F.relu(F.conv2d(x.double(), w.double(), b.double())), F.relu(F.conv2d(x, w, b)), "resident 1x1, |x| ~ 7.9e3")
    rel = float(((ops.unsplit_hl(ys) - y).abs() / y.abs().clamp(min=1e-2)).max())
    print(f"resident 1x1 split output vs fp32 output: {rel:.3e} relative, max|y| {float(y.abs().max()):.1f}")
    assert rel < 2.0 ** -20


def test_mask_head_accuracy_at_the_top_of_the_range(ops):
    B, h, w = 1, 3, 13
    x = _top("mx", (B, 256, h, w), 27)
    wt, bs = gen("mw2", (576, 256, 1, 1), 27, std=float(np.sqrt(2.0 / 256)) / (0.3 * MAG)), gen("mb2", (576,), 27, std=0.3)
    flow = gen("mf2", (B, 2, h, w), 27, std=2.0)
    got = _silent(ops, lambda: ops.mask_upsample(ops.PackedMaskHead(wt, bs, post_scale=0.25), nhwc(x), 0, nhwc(flow)))

    def ref(t):                                                   # update.py:183-187 + CFNet.py:95-106 in the precision of t
        m = 0.25 * F.conv2d(x.to(t), wt.to(t), bs.to(t))
        sm = torch.softmax(m.view(B, 1, 9, 8, 8, h, w), dim=2)
        upf = F.unfold(8 * flow.to(t), [3, 3], padding=1).view(B, 2, 9, 1, 1, h, w)
        return torch.sum(sm * upf, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2, 8 * h, 8 * w)
    check(got, ref(torch.float64), ref(torch.float32), "mask head, |x| ~ 7.9e3")


@pytest.mark.parametrize("tile", [1, 5], ids=["rows128", "rows160"])
def test_conv_split_output_accuracy_at_the_top_of_the_range(ops, tile):
    B, H, W, cin, cout = 2, 11, 19, 96, 128
    x = _top("cx", (B, cin, H, W), 29)
    w, b = gen("cw2", (cout, cin, 3, 3), 29, std=0.4 * float(np.sqrt(2.0 / (cin * 9)))), gen("cb2", (cout,), 29) * (0.05 * MAG)
    pc = ops.PackedConv(w, b, [cin])
    y, extra, ys = (torch.empty(B, H, W, cout, device="cuda") for _ in range(3))

    def run():
        ops.conv2d_nhwc(pc, [(nhwc(x), 0)], (y, 0), ops.EPI_LINEAR, dst_split=(extra, 0), tile=tile)
        ops.conv2d_nhwc(pc, [(nhwc(x), 0)], (ys, 0), ops.EPI_LINEAR, dst_hl=True, tile=tile)
    _silent(ops, run)
    check(nchw(y), F.conv2d(x.double(), w.double(), b.double(), padding=1), F.conv2d(x, w, b, padding=1), f"3x3 tile {tile}, |x| ~ 7.9e3")
    for name, sp in (("dst_split", extra), ("dst_hl", ys)):
        rel = float(((ops.unsplit_hl(sp) - y).abs() / y.abs().clamp(min=1e-2)).max())
        print(f"tile {tile} {name} vs fp32 output: {rel:.3e} relative, max|y| {float(y.abs().max()):.1f}")
        assert rel < 2.0 ** -20
