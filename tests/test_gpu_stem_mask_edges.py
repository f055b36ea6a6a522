"""The two MFMA kernels outside the convolution dispatch -- csrc/stem.hip (stem_conv7x7_s2_kernel: persistent tile walk, 7x7 stride-2
convolution with fused input normalisation and tile statistics; the weight pack kernel) and csrc/mask_upsample.hip (mask_upsample_kernel:
mask.2 as a 1x1 convolution + online-softmax convex up-sampling, the default 16 x 16-tile form) -- against fp64 at their edges (run with
-m gpu on an MI355X; the whole module also runs on the host-executed kernels, tests/test_kernels_on_host.py).

tests/test_gpu_parity.py and tests/test_gpu_conv.py meet the stem at shapes where no XCD chunk of the tile list straddles an image and
no step of the walk crosses one, and the mask head at one channel window (cs = 512, co = 256) and N(0,2) logits.  Here every shape is in
a table next to the code path it is there for; inputs are seeded by rnnpose_amd.synthetic; references are plain fp64 torch expressions
on the CPU.  Both kernels are launched through the C ABI on buffers of this module: every output is pre-filled with NaN and followed by a
guard zone of NaN that must come back untouched -- a tile written to the wrong image leaves another one unwritten, and a buffer from the
caching allocator may still hold the right values of an earlier call.

The stem's walk depends on the launch: per = gridDim.x / 8 workgroups share the contiguous chunk of ceil(ntiles / 8) tiles of an XCD, and
a workgroup steps by `per` tiles = (dn, dy, dx) images / tile rows / tile columns with two carries.  rnnpose_stem_workgroups caps the grid:
cap 8 gives per = 1 everywhere; caps 16 and 24 give per = 2 and 3 on an MI355X (256 CUs: 2 * 256 / 8 = 64 uncapped).  The host-executed
device has 4 CUs, so per stays 1 at every cap there: the cases of caps 16 and 24 still run on the host, redundantly (they repeat cap 8).
`walk_model` restates the walk in Python; test_stem_table_reaches_the_walk_paths asserts from it, without a device, that the table
holds every path it claims, for the MI355X's geometry.

Gates.  Stem values: err <= max(3 * err32, 2e-6) with err32 from the same convolution in fp32 on the CPU (the gate of
test_encoder_stem_kernel); bit-identity between all caps.  Tile statistics, weight pack, mask head: bounds derived in the docstrings of
their tests, per element.  err_gpu, err_ref (the same formula in fp32 on the CPU) and err / bound are printed per case.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rnnpose_amd import synthetic as syn
from test_gpu_parity import D, T, ops  # noqa: F401  (ops: the module-scoped build fixture)

pytestmark = pytest.mark.gpu

F64, F32, F16 = torch.float64, torch.float32, torch.float16
NAN = float("nan")
U32, U64 = 2.0 ** -24, 2.0 ** -53
_ids = lambda cases: [c[0] for c in cases]


def gamma(k, u=U32):
    """k roundings of unit round-off u in a row: (1 + u)^k - 1 <= k u / (1 - k u)"""
    return k * u / (1.0 - k * u)


def guarded(shape, guard, dtype=F32):
    """-> (flat buffer of prod(shape) + guard NaNs on the device, its first prod(shape) elements viewed as `shape`)"""
    n = int(np.prod(shape))
    full = torch.full((n + guard,), NAN, device="cuda", dtype=dtype)
    return full, full[:n].view(shape)


def untouched(full, n, what):
    tail = full[n:].cpu()
    assert bool(torch.isnan(tail).all()), f"{what}: {int((~torch.isnan(tail)).sum())} elements of the guard zone behind the buffer were written"


def lib():
    from rnnpose_amd import _lib
    return _lib.load()


def refused(entry, args, text, buffers):
    """the call returns 1 with `text` in the error message and leaves every buffer (all NaN) as it was"""
    rc = getattr(lib(), entry)(*args)
    msg = lib().rnnpose_last_error()
    assert rc == 1 and text in msg, (entry, rc, msg)
    torch.cuda.synchronize()
    for b in buffers:
        assert bool(torch.isnan(b.cpu().float()).all()), (entry, text, "a refused call wrote a buffer")


def off(t, nbytes):
    return C.c_void_p(t.data_ptr() + nbytes)


# ================================================================================================== 1. stem: the tile walk
TH, TW = 8, 16                                              # output tile of stem_conv7x7_s2_kernel
MI355X_CUS, HOST_CUS = 256, 4
CAPS = [0, 8, 16, 24]
# (id, N, H, W).  Ho = ceil(H / 2), Wo = ceil(W / 2); tiles per image tpi = ceil(Ho / 8) * ceil(Wo / 16); chunk = ceil(N * tpi / 8).
STEM = [
    ("dn_20x16x32", 20, 16, 32),                            # tpi = 1, 20 tiles, chunks of 3: every step is an image step (dn = per); the last chunk is short (2)
    ("straddle_5x37x41", 5, 37, 41),                        # tpi = 3 x 2 = 6, ragged on both axes (19 x 21 outputs), chunks of 4 straddle images; dy > 0 at per >= 2
    ("dn_9x16x40", 9, 16, 40),                              # tpi = 1 x 2, 18 tiles, chunks of 3 start at odd tiles; per = 2: dn = 1 alone
    ("carry_17x3x33", 17, 3, 33),                           # tpi = 1 x 2, 34 tiles, chunks of 5; per = 3: dn = 1, dx = 1 and both carries in one step
    ("single_1x1x1", 1, 1, 1),                              # one output pixel; 7 XCDs have an empty chunk
    ("tiny_1x2x7", 1, 2, 7),                                # 1 x 4 outputs: the patch is wider than the image on both axes
    ("column_2x15x3", 2, 15, 3),                            # 8 x 2 outputs: a full tile height, two columns; 2 tiles, 6 empty chunks
    ("h6_2x6x35", 2, 6, 35),                                # H = 6 (even): three output rows, Wo = 18: a second tile with two columns
    ("w7_3x40x7", 3, 40, 7),                                # W = 7 (odd): tiles_x = 1, tiles_y = 3: a step of one tile is a row step (dy = 1, dx = 0)
    ("h8_w8_3x8x8", 3, 8, 8),                               # H = W = 8: 4 x 4 outputs, every texel of the image in one patch with all four borders
]


def stem_grid(ntiles, cap, cus):
    """gridDim.x of rnnpose_stem_conv7x7_s2_f16x3"""
    per = min((2 * cus) >> 3, (ntiles + 7) >> 3)
    if cap > 0:
        per = min(per, max(cap >> 3, 1))
    return 8 * max(per, 1)


def walk_model(N, H, W, grid):
    """The walk of stem_conv7x7_s2_kernel for gridDim.x = grid, restated: -> dict(per, chunk, dn, dy, dx, visits = [(block, t, n, ty, tx)]
    with (n, ty, tx) CARRIED from tile to tile as the kernel does, and the facts the table test asks for)."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    tiles_x, tiles_y = -(-Wo // TW), -(-Ho // TH)
    tpi = tiles_x * tiles_y
    ntiles = N * tpi
    per, chunk = grid >> 3, (ntiles + 7) >> 3
    dn = per // tpi
    dy = (per - dn * tpi) // tiles_x
    dx = per - dn * tpi - dy * tiles_x
    m = dict(per=per, chunk=chunk, ntiles=ntiles, tpi=tpi, dn=dn, dy=dy, dx=dx, visits=[], carry_x=0, carry_y=0, step_all=0, empty=0, short=0,
             straddle=0, longest=0)
    for xcd in range(8):
        t0, t_end = xcd * chunk, min((xcd + 1) * chunk, ntiles)
        m["empty"] += t0 >= ntiles
        m["short"] += 0 < t_end - t0 < chunk
        m["straddle"] += t_end > t0 and t0 // tpi != (t_end - 1) // tpi
    for block in range(grid):
        xcd = block & 7
        t_end = min((xcd + 1) * chunk, ntiles)
        t = xcd * chunk + (block >> 3)
        if t >= t_end:
            continue
        cn = t // tpi
        cy = (t - cn * tpi) // tiles_x
        cx = t - cn * tpi - cy * tiles_x
        nn, ny, nx = cn, cy, cx
        steps = 0
        while t < t_end:
            m["visits"].append((block, t, cn, cy, cx))
            steps += 1
            nx += dx; ny += dy; nn += dn
            c1 = nx >= tiles_x
            if c1:
                nx -= tiles_x; ny += 1
            c2 = ny >= tiles_y
            if c2:
                ny -= tiles_y; nn += 1
            if t + per < t_end:                             # (a step that is taken: its tile is computed)
                m["carry_x"] += c1
                m["carry_y"] += c2
                m["step_all"] += bool(dn > 0 and dx > 0 and c1 and c2)
            t += per
            cn, cy, cx = nn, ny, nx
        m["longest"] = max(m["longest"], steps)
    m["steps_taken"] = len(m["visits"]) - len({v[0] for v in m["visits"]})
    return m


def test_stem_table_reaches_the_walk_paths():
    """From the restated walk alone (no device).  The restatement itself: for every shape, cap and both devices' CU counts it visits
    every tile exactly once at the (n, ty, tx) that t decodes to.  Then, for the MI355X: at cap 8 (per = 1 on both tiers) the table
    holds dn > 0 with at least 16 images, chunks that straddle an image boundary (5x37x41; 17x3x33 with two tiles per image), empty
    chunks, a short last chunk and a workgroup that walks at least 3 tiles; at caps 16 and 24 (per = 2, 3) it holds a taken step with
    dn > 0, dx > 0 and both carries at once, and steps with dy > 0.  On the host-executed device per stays 1 at every cap."""
    models = {}
    for name, N, H, W in STEM:
        for cus in (MI355X_CUS, HOST_CUS):
            for cap in CAPS:
                ntiles = N * (-(-((H + 1) // 2) // TH)) * (-(-((W + 1) // 2) // TW))
                m = walk_model(N, H, W, stem_grid(ntiles, cap, cus))
                tiles_x = -(-((W + 1) // 2) // TW)
                want = sorted((t, t // m["tpi"], (t % m["tpi"]) // tiles_x, (t % m["tpi"]) % tiles_x) for t in range(ntiles))
                assert sorted(v[1:] for v in m["visits"]) == want, (name, cus, cap)
                models[name, cus, cap] = m
                if cus == HOST_CUS or cap == 8:
                    assert m["per"] == 1, (name, cus, cap)
    at = lambda cap: {name: models[name, MI355X_CUS, cap] for name, *_ in STEM}
    c8 = at(8)
    dn1 = [n for n, N, H, W in STEM if c8[n]["dn"] > 0 and c8[n]["steps_taken"] > 0]
    assert dn1 and all(N >= 16 for n, N, H, W in STEM if n in dn1), dn1
    assert c8["straddle_5x37x41"]["straddle"] >= 2 and c8["carry_17x3x33"]["straddle"] >= 4 and c8["carry_17x3x33"]["tpi"] == 2
    assert c8["straddle_5x37x41"]["carry_x"] > 0 and c8["straddle_5x37x41"]["carry_y"] > 0           # the carry into the next image, at per = 1
    assert any(m["empty"] > 0 and m["ntiles"] < 8 for m in c8.values())
    assert any(m["short"] > 0 for m in c8.values())
    assert sum(m["longest"] >= 3 for m in c8.values()) >= 4
    c16, c24 = at(16), at(24)
    assert c16["dn_20x16x32"]["per"] == 2 and c24["carry_17x3x33"]["per"] == 3
    assert c16["dn_20x16x32"]["dn"] == 2 and c16["dn_20x16x32"]["steps_taken"] > 0
    assert c16["dn_9x16x40"]["dn"] == 1 and c16["dn_9x16x40"]["dx"] == 0 and c16["dn_9x16x40"]["steps_taken"] > 0
    assert c24["carry_17x3x33"]["dn"] == 1 and c24["carry_17x3x33"]["dx"] == 1 and c24["carry_17x3x33"]["step_all"] > 0
    for m in (c16["straddle_5x37x41"], c24["straddle_5x37x41"], c8["w7_3x40x7"]):        # (one tile column: at per = 1 the step is a row step)
        assert m["dy"] > 0 and m["steps_taken"] > 0
    assert c24["straddle_5x37x41"]["dx"] > 0 and c24["straddle_5x37x41"]["carry_y"] > 0


# ================================================================================================== 2. stem: values, statistics, pack, refusals
STEM_GUARD = 16384                                          # floats behind `out` (one row of tiles of the widest table entry is 8 x 21 x 64 = 10752), doubles behind the records
_stem_cache = {}


def stem_inputs(name, N, H, W, normalize):
    img = syn.uniform("sme.img." + name, (N, 3, H, W), 9, 0.0, 255.0) if normalize else syn.normal("sme.x." + name, (N, 3, H, W), 9, std=0.7)
    wt = T(syn.normal("sme.w." + name, (64, 3, 7, 7), 9, std=0.1))
    bias = T(syn.uniform("sme.b." + name, (64,), 9, -0.5, 0.5))
    return T(img), wt, bias


def stem_geometry(H, W):
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    return Ho, Wo, -(-Ho // TH), -(-Wo // TW)


def stem_launch(ops, ps, img_dev, normalize, cap, stats=True):
    """one launch on NaN buffers with guard zones -> (out (N,Ho,Wo,64), records (N*tpi,64,2) or None), on the CPU"""
    from rnnpose_amd import _lib
    N, _, H, W = img_dev.shape
    Ho, Wo, ty, tx = stem_geometry(H, W)
    ofull, out = guarded((N, Ho, Wo, 64), STEM_GUARD)
    sfull, ts = guarded((N * ty * tx, 64, 2), STEM_GUARD, F64)
    try:
        _lib.call("rnnpose_stem_workgroups", cap)
        ops._launch("rnnpose_stem_conv7x7_s2_f16x3", ops._ptr(img_dev), N, H, W, int(normalize), ops._ptr(ps.w_hi), ops._ptr(ps.w_lo), ops._ptr(ps.bias),
                    ps.a_scale, ps.w_scale, ops._ptr(out), ops._ptr(ts if stats else None), ops._stream())
        torch.cuda.synchronize()
    finally:
        _lib.call("rnnpose_stem_workgroups", 0)
    what = f"stem {tuple(img_dev.shape)} cap {cap}"
    untouched(ofull, out.numel(), what + " out")
    untouched(sfull, ts.numel() if stats else 0, what + " tile_stats")
    return out.cpu(), (ts.cpu() if stats else None)


def stem_case(ops, name, N, H, W, normalize):
    """-> dict: the fp64 / fp32 references (computed once per (shape, normalize)) and the launches by cap"""
    key = (name, normalize)
    if key not in _stem_cache:
        img, wt, bias = stem_inputs(name, N, H, W, normalize)
        xin = (2 * (img.to(F64) / 255.0) - 1.0) if normalize else img.to(F64)
        ref64 = F.conv2d(xin, wt.to(F64), bias.to(F64), stride=2, padding=3).permute(0, 2, 3, 1)          # (zero padding of the NORMALISED tensor)
        ref32 = F.conv2d(xin.to(F32), wt, bias, stride=2, padding=3).permute(0, 2, 3, 1)
        _stem_cache[key] = dict(ps=ops.PackedStem(D(wt), D(bias)), img=D(img), ref64=ref64, err32=float((ref32.to(F64) - ref64).abs().max()), runs={})
    c = _stem_cache[key]
    return c


def stem_run(ops, c, normalize, cap):
    if cap not in c["runs"]:
        c["runs"][cap] = stem_launch(ops, c["ps"], c["img"], normalize, cap)
    return c["runs"][cap]


@pytest.mark.parametrize("cap", CAPS, ids=[f"cap{c}" for c in CAPS])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "raw"])
@pytest.mark.parametrize("name,N,H,W", STEM, ids=_ids(STEM))
def test_stem_values_vs_fp64_at_every_cap(ops, name, N, H, W, normalize, cap):
    """out == F.conv2d in fp64 (padding applied after the normalisation) within max(3 * err32, 2e-6), err32 being the error of the same
    convolution in fp32 on the CPU -- the gate of test_encoder_stem_kernel -- with no element left at its NaN pre-fill, nothing written
    behind the buffers, and output and tile records bit-identical to the uncapped launch."""
    c = stem_case(ops, name, N, H, W, normalize)
    out, ts = stem_run(ops, c, normalize, cap)
    err, err32 = float((out.to(F64) - c["ref64"]).abs().max()), c["err32"]
    nan = int(torch.isnan(out).sum())
    print(f"stem_mask_edges stem [{name}.{'normalize' if normalize else 'raw'}.cap{cap}] err_gpu {err:.3e} err_ref {err32:.3e} "
          f"err/bound {err / max(3 * err32, 2e-6):.3f} unwritten {nan}")
    assert nan == 0, f"{nan} of {out.numel()} outputs were never written"
    assert err <= max(3 * err32, 2e-6), (err, err32)
    assert not bool(torch.isnan(ts).any()), "tile records left unwritten"
    out0, ts0 = stem_run(ops, c, normalize, 0)
    assert torch.equal(out, out0) and torch.equal(ts, ts0), f"cap {cap} differs from the uncapped launch"


@pytest.mark.parametrize("name,N,H,W", STEM, ids=_ids(STEM))
def test_stem_tile_statistics_are_the_sums_of_the_stored_outputs(ops, name, N, H, W):
    """Every (sum, sum of squares) record against the fp64 sums of the kernel's OWN stored fp32 outputs of that tile; pixels of a ragged
    tile outside the image contribute nothing (they are not in the output at all).  The bound follows the summation order of the kernel
    (stem.hip, "Statistics"): a lane adds its 16 pixels of a column in fp32 groups of four, (a + b) + (c + d) -- every value passes
    two fp32 additions: relative gamma32(2) of sum|y|; a square passes at most three fp32 roundings (the product y1 * y1, the fused
    multiply-add, the pair addition): gamma32(3) of sum y^2.  Groups, the two lanes of a column and the four waves are added in fp64,
    8 additions in a row: gamma64(8), doubled for the fp64 sum of 128 values that this test forms itself.
        |sum - S| <= (gamma32(2) + 2 gamma64(8)) sum|y|,     |sumsq - Q| <= (gamma32(3) + 2 gamma64(8)) sum y^2.
    With tile_stats = NULL the output is the same and the statistics buffer of the launch keeps its NaN."""
    c = stem_case(ops, name, N, H, W, True)
    out, ts = stem_run(ops, c, True, 0)
    Ho, Wo, ty, tx = stem_geometry(H, W)
    y = torch.zeros(N, ty * TH, tx * TW, 64, dtype=F64)
    y[:, :Ho, :Wo] = out.to(F64)
    tiles = y.view(N, ty, TH, tx, TW, 64).permute(0, 1, 3, 2, 4, 5).reshape(N * ty * tx, TH * TW, 64)          # tile t = (n * tiles_y + ty) * tiles_x + tx
    s, sa, q = tiles.sum(1), tiles.abs().sum(1), (tiles * tiles).sum(1)
    bs, bq = (gamma(2) + 2 * gamma(8, U64)) * sa, (gamma(3) + 2 * gamma(8, U64)) * q
    es, eq = (ts[..., 0] - s).abs(), (ts[..., 1] - q).abs()
    rs, rq = float((es / bs.clamp(min=1e-300)).max()), float((eq / bq.clamp(min=1e-300)).max())
    print(f"stem_mask_edges stem_stats [{name}] err_sum {float(es.max()):.3e} err/bound {rs:.3f} err_sumsq {float(eq.max()):.3e} err/bound {rq:.3f}")
    assert bool((es <= bs).all()) and bool((eq <= bq).all()), (rs, rq)
    out_n, none = stem_launch(ops, c["ps"], c["img"], True, 0, stats=False)            # (stem_launch: the whole statistics buffer is guard zone)
    assert none is None and torch.equal(out_n, out)


def _pack_ref(w, w_scale):
    """stem_pack_kernel restated: element i = ((kk * 2 + ni) * 64 + ln) * 8 + j carries output channel 32 ni + (ln & 31) and tap kx = j of patch
    row r = 2 kk + (ln >> 5) = (c, ky) = (r / 7, r % 7); kx = 7 and row 21 are zero"""
    kk, ni, ln, j = np.meshgrid(np.arange(11), np.arange(2), np.arange(64), np.arange(8), indexing="ij")
    r, nn = 2 * kk + (ln >> 5), ni * 32 + (ln & 31)
    real = (r < 21) & (j < 7)
    v = np.where(real, w[nn, np.minimum(r, 20) // 7, np.minimum(r, 20) % 7, np.minimum(j, 6)] * np.float32(w_scale), np.float32(0)).astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return v.reshape(-1), hi.reshape(-1), lo.reshape(-1), real.reshape(-1)


@pytest.mark.parametrize("w_scale", [2048.0, 8192.0], ids=["scale2048", "scale8192"])
def test_stem_weight_pack_is_the_fragment_order(ops, w_scale):
    """rnnpose_stem_pack_weights_f16x3 against a numpy restatement of the fragment order (stem_pack_kernel), bit for bit; the kx = 7
    slots and row 21 are exactly zero; hi + lo reproduces v = w * w_scale to the residual of the split: hi = fp16(v) leaves at most
    2^-11 |v|, lo = fp16(v - hi) at most 2^-11 of that while lo is a normal fp16 and half a subnormal step, 2^-25, below:
    |hi + lo - v| <= max(2^-22 |v|, 2^-25).  Scale 2048 is what PackedStem picks for these weights (max |v| in [512, 1024)); 8192
    moves every value two binades up, still inside the fp16 range.  (Kernel and restatement agree bit for bit, so err / bound is a
    property of the seeded weights alone: 0.859 and 0.517.  The bound is sharp: a tie of the last rounding attains it.)"""
    w = syn.normal("sme.pack.w", (64, 3, 7, 7), 4, std=0.1)
    n = int(lib().rnnpose_stem_packed_halfs())
    assert n == 11 * 2 * 64 * 8
    hfull, hi = guarded((n,), 64, F16)
    lfull, lo = guarded((n,), 64, F16)
    ops._launch("rnnpose_stem_pack_weights_f16x3", ops._ptr(D(w)), w_scale, ops._ptr(hi), ops._ptr(lo), ops._stream())
    torch.cuda.synchronize()
    untouched(hfull, n, "pack hi")
    untouched(lfull, n, "pack lo")
    v, rhi, rlo, real = _pack_ref(w, w_scale)
    ghi, glo = hi.cpu().numpy(), lo.cpu().numpy()
    assert int(real.sum()) == 64 * 147
    assert np.array_equal(ghi[~real].view(np.int16), np.zeros(int((~real).sum()), np.int16)) and np.array_equal(glo[~real].view(np.int16), np.zeros(int((~real).sum()), np.int16))
    assert np.array_equal(ghi.view(np.int16), rhi.view(np.int16)) and np.array_equal(glo.view(np.int16), rlo.view(np.int16))
    assert float(np.abs(v).max()) < 65504.0 / 4
    v64 = v.astype(np.float64)
    err = np.abs(ghi.astype(np.float64) + glo.astype(np.float64) - v64)
    bound = np.maximum(2.0 ** -22 * np.abs(v64), 2.0 ** -25)
    print(f"stem_mask_edges stem_pack [scale{w_scale:g}] err {err.max():.3e} err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_stem_refusals_leave_every_buffer_alone(ops):
    """Null pointers, non-positive sizes or scales, misaligned out / bias: 1 and the entry's message, nothing launched."""
    name, N, H, W = "refuse", 1, 5, 6
    img, wt, bias = stem_inputs(name, N, H, W, True)
    ps = ops.PackedStem(D(wt), D(bias))
    b68 = torch.zeros(68, device="cuda")
    img_d = D(img)
    _, out = guarded((N, 3, 3, 64), 64)
    _, ts = guarded((1, 64, 2), 64, F64)
    P, S, Z = ops._ptr, ops._stream(), C.c_void_p(0)
    good = [P(img_d), N, H, W, 1, P(ps.w_hi), P(ps.w_lo), P(b68), ps.a_scale, ps.w_scale, P(out), P(ts), S]

    def sub(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    for i in (0, 5, 6, 7, 10):
        refused("rnnpose_stem_conv7x7_s2_f16x3", sub(**{f"a{i}": Z}), b"null pointer", [out, ts])
    for kw in (dict(a1=0), dict(a1=-3), dict(a2=0), dict(a3=-1), dict(a8=0.0), dict(a9=-1.0)):
        refused("rnnpose_stem_conv7x7_s2_f16x3", sub(**kw), b"bad size / scale", [out, ts])
    for kw in (dict(a10=off(out, 4)), dict(a10=off(out, 8)), dict(a7=off(b68, 4)), dict(a5=off(ps.w_hi, 8)), dict(a6=off(ps.w_lo, 2))):
        refused("rnnpose_stem_conv7x7_s2_f16x3", sub(**kw), b"must be 16-byte aligned", [out, ts])
    _, hi = guarded((11 * 2 * 64 * 8,), 64, F16)
    for a in ([Z, 1.0, P(hi), P(hi), S], [P(img_d), 1.0, Z, P(hi), S], [P(img_d), 1.0, P(hi), Z, S], [P(img_d), 0.0, P(hi), P(hi), S]):
        refused("rnnpose_stem_pack_weights_f16x3", a, b"null pointer / non-positive scale", [hi])
    assert getattr(lib(), "rnnpose_stem_conv7x7_s2_f16x3")(*good) == 0                  # the accepted call still runs
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(ts).any())


# (id, N, H, W): sizes whose 32-bit byte offsets do not fit
STEM_TOO_LARGE = [
    ("110_frames_480x640", 110, 480, 640),                  # output: 110 * 240 * 320 * 256 = 2 162 688 000 >= 2^31 (109 frames: 2 143 027 200, accepted)
    ("219_frames_480x640", 219, 480, 640),                  # the output offset would wrap modulo 2^32
    ("one_13400x13400", 1, 13400, 13400),                   # image: 3 * 13400^2 * 4 = 2 154 720 000 >= 2^31 (and the output with it: it is always the larger)
    ("overhang_109x482x640", 109, 482, 640),                # output 109 * 241 * 320 * 256 < 2^31, but the last tile row (241 = 30 x 8 + 1) computes offsets of 7 rows more
]


@pytest.mark.parametrize("name,N,H,W", STEM_TOO_LARGE, ids=_ids(STEM_TOO_LARGE))
def test_stem_refuses_sizes_beyond_its_32_bit_byte_offsets(ops, name, N, H, W):
    """stem_conv7x7_s2_kernel forms byte offsets into the image and the output in 32-bit integers: the entry refuses, before any launch
    and with a message that names the limit, every size at which the largest of them -- last image, last tile, overhang of a ragged
    tile included -- reaches 2^31.  Sizes only, on tiny dummy buffers that keep their NaN; the number of tiles is far below its own
    limit, so it is this check that answers.  (Accepted sizes near the limit would need gigabytes and are not run.)"""
    Ho, Wo, ty, tx = stem_geometry(H, W)
    assert N * ty * tx < 2 ** 31
    out_end = (((N - 1) * Ho + ty * TH - 1) * Wo + tx * TW) * 256
    in_end = (((N - 1) * 3 * H + 2 * (ty - 1) * TH - 3 + 2 * H + 20) * W + 2 * (tx - 1) * TW - 3 + 36) * 4 + 4
    assert out_end > 2 ** 31 or in_end > 2 ** 31
    wt, bias = T(syn.normal("sme.big.w", (64, 3, 7, 7), 9, std=0.1)), torch.zeros(64)
    ps = ops.PackedStem(D(wt), D(bias))
    _, img = guarded((3, 4, 4), 64)
    _, out = guarded((2, 2, 64), 64)
    _, ts = guarded((1, 64, 2), 64, F64)
    P = ops._ptr
    refused("rnnpose_stem_conv7x7_s2_f16x3", [P(img), N, H, W, 1, P(ps.w_hi), P(ps.w_lo), P(ps.bias), ps.a_scale, ps.w_scale, P(out), P(ts), ops._stream()],
            b"32-bit byte offsets", [img, out, ts])
    assert b"2^31" in lib().rnnpose_last_error()


# ================================================================================================== 3. mask head
# (id, B, h, w).  Workgroup = 32 consecutive low-resolution pixels of the flattened (B, h, w) list.
MASK = [
    ("one_pixel_1x1x1", 1, 1, 1),                           # every neighbour but the centre is outside; 31 padding rows re-read the pixel
    ("row_h1_31px", 1, 1, 31),                              # h = 1: the taps above and below are always outside; 31 = one short of a tile
    ("column_w1_32px", 1, 32, 1),                           # w = 1: left and right always outside; exactly one tile
    ("33px_3x11", 1, 3, 11),                                # a second tile with one pixel
    ("straddle_2x3x7", 2, 3, 7),                            # h w = 21: tile 0 holds image 0 and 11 pixels of image 1
    ("three_tiles_3x5x5", 3, 5, 5),                         # 75 pixels: tiles 0 and 1 straddle images, tile 2 holds 11 pixels
]
# (cs, co): the 256 input channels [co, co + 256) of a cs-channel row
WINDOWS = [(512, 256), (264, 8), (260, 0), (256, 0)]
MASK_GUARD = 4096
A_SCALE = 8.0                                               # ops.A_SCALE, written out: the bound below must not follow a changed constant
N_ADD = 52                                                  # fp32 additions a product passes on its way into a logit (see mask_bound)


def _taps(flow):
    """flow (B,h,w,2) fp32 -> (B,h,w,9,2) fp64: 8 * flow of the 3x3 neighbourhood, tap k = (k / 3 - 1, k % 3 - 1), zeros outside"""
    B, h, w, _ = flow.shape
    fp = F.pad(8.0 * flow.to(F64).permute(0, 3, 1, 2), (1, 1, 1, 1))
    return torch.stack([fp[:, :, k // 3:k // 3 + h, k % 3:k % 3 + w] for k in range(9)], -1).permute(0, 2, 3, 4, 1)


def _inside(B, h, w):
    return _taps(torch.ones(B, h, w, 2))[..., 0] != 0       # (B,h,w,9)


def mask_reference(xs, wt, bs, flow, dtype):
    """update.py:183-187 + CFNet.py:95-106 in `dtype`: logits 0.25 (W x + b) (B,h,w,9,8,8), softmax over the taps, weighted sum of the
    3x3 neighbourhood of 8 * flow -> ((B,2,8h,8w), logits)"""
    B, h, w, _ = xs.shape
    logits = (0.25 * (xs.to(dtype) @ wt.to(dtype).t() + bs.to(dtype))).view(B, h, w, 9, 8, 8)
    p = torch.softmax(logits, dim=3)
    up = torch.einsum("byxkij,byxkc->bcyixj", p, _taps(flow).to(dtype)).reshape(B, 2, 8 * h, 8 * w)
    return up, logits


def mask_bound(xs, wt, bs, flow, w_scale):
    """Per element 2 * delta * max_k |8 flow_k| (the neighbourhood's largest magnitude in the element's flow channel), delta being the
    largest error of the element's nine logits.  A perturbation of the logits by at most delta changes softmax(l) . f by at most
    sum_k p_k |f_k - o| delta <= 2 delta max|f|.  delta, with S = 0.25 sum_c |x_c| |w_c| of the logit (u = 2^-24):
      * the split.  a x = hi + lo + e with |e| <= 2^-22 |a x|, or 2^-25 where lo is a subnormal fp16; the same for s 0.25 w (the
        products with 0.25 and the power-of-two scales are exact).  The kernel adds hi hi + hi lo + lo hi: it drops lo lo, at most
        2^-11 2^-11 of a product, and inherits e_x (s w) and (a x) e_w: 3 * 2^-22 S + 2^-25 (sum_c |0.25 w_c| / a + sum_c |x_c| / s);
      * the accumulation.  Products of fp16 numbers are exact in fp32.  A tap's logit is a chain of 8 channel blocks x 3 products x 2
        MFMAs of K = 16 = 48 accumulations, and a product is at most 4 additions deep inside its MFMA (16 terms over 4 lane groups of 4
        elements): every term passes at most N_ADD = 52 fp32 additions, each allowed 2 u (a matrix core may truncate): 52 * 2^-23 S;
      * acc * out_scale + bias: two roundings, of at most S and S + |0.25 b|: 2^-23 (S + |0.25 b|);
      * the online softmax as an equivalent logit error: d = l - max rounds by u |d| <= 2 u (S + |0.25 b|)max; expf within 2 ulp:
        2^-22; per tap one multiplication by the scale and one addition on numerator and denominator, one product with the flow, and
        the final division: 9 * 3 + 1 roundings: 28 u.
    -> (bound (B,2,8h,8w), delta (B,h,w,8,8))"""
    x64, w64, b64 = xs.to(F64).abs(), 0.25 * wt.to(F64).abs(), 0.25 * bs.to(F64).abs()
    B, h, w, _ = xs.shape
    S = x64 @ w64.t()                                                                                       # (B,h,w,576)
    sub = 2.0 ** -25 * (w64.sum(1) / A_SCALE + x64.sum(-1, keepdim=True) / w_scale)
    lmax = (S + b64).amax(dim=(0, 1, 2, 3))
    delta = (3 * 2.0 ** -22 + N_ADD * 2.0 ** -23) * S + sub + 2.0 ** -23 * (S + b64) + 2 * U32 * lmax + 2.0 ** -22 + 28 * U32
    delta = delta.view(B, h, w, 9, 8, 8).amax(3)                                                            # (B,h,w,8,8)
    fmax = _taps(flow).abs().amax(3)                                                                        # (B,h,w,2)
    bound = 2.0 * torch.einsum("byxij,byxc->bcyixj", delta, fmax).reshape(B, 2, 8 * h, 8 * w)
    return bound, delta


def mask_launch(ops, pm, x, co, flow):
    """one launch through the C ABI on a NaN buffer with a guard zone -> (B,2,8h,8w) on the CPU"""
    B, h, w, cs = x.shape
    full, up = guarded((B, 2, 8 * h, 8 * w), MASK_GUARD)
    ops._launch("rnnpose_mask_upsample_f16x3", ops._ptr(x), cs, co, ops._ptr(pm.w_packed), 576, ops._ptr(pm.bias), pm.a_scale, pm.w_scale, ops._ptr(flow),
                B, h, w, ops._ptr(up), ops._stream())
    torch.cuda.synchronize()
    untouched(full, up.numel(), f"mask_upsample {tuple(x.shape)} co {co}")
    return up.cpu()


def mask_gate(case, got, ref64, ref32, bound):
    eg = (got.to(F64) - ref64).abs()
    nan = int(torch.isnan(got).sum())
    err_gpu, err_ref = float(eg[~torch.isnan(eg)].max()) if nan < eg.numel() else NAN, float((ref32.to(F64) - ref64).abs().max())
    ratio = float((eg / bound)[~torch.isnan(eg)].max()) if nan < eg.numel() else NAN
    print(f"stem_mask_edges mask_upsample [{case}] err_gpu {err_gpu:.3e} err_ref {err_ref:.3e} err/bound {ratio:.4f} unwritten {nan}")
    assert nan == 0, f"{case}: {nan} of {got.numel()} outputs were never written"
    bad = ~(eg <= bound)
    if bad.any():
        i = tuple(int(k) for k in torch.nonzero(bad)[0])
        raise AssertionError(f"mask_upsample [{case}]: {int(bad.sum())}/{bad.numel()} elements beyond the bound; first at {i}: got {float(got[i])!r} want "
                             f"{float(ref64[i])!r}, bound {float(bound[i]):.3e}")


def mask_inputs(key, B, h, w, cs, wmul=2.0, tap_bias=None):
    """x >= 0 in ALL cs channels (relu(mask.0) and its neighbours in the row), weights for logits of std `wmul`, bias U(-0.5, 0.5)
    [+ 4 * tap_bias(k) on every column of tap k: tap_bias is in logit units], flow N(0, 2)"""
    x = T(syn.normal("sme.mu.x." + key, (B, h, w, cs), 11)).clamp(min=0)
    wt = T(syn.normal("sme.mu.w." + key, (576, 256), 11, std=float(np.sqrt(2.0 / 256)) * 4.0)) * wmul
    bs = T(syn.uniform("sme.mu.b." + key, (576,), 11, -0.5, 0.5))
    if tap_bias is not None:
        bs = bs + 4.0 * torch.tensor([float(tap_bias(k)) for k in range(9)], dtype=F32).repeat_interleave(64)
    flow = T(syn.normal("sme.mu.f." + key, (B, h, w, 2), 11, std=2.0))
    return x, wt, bs, flow


@pytest.mark.parametrize("cs,co", WINDOWS, ids=[f"cs{a}_co{b}" for a, b in WINDOWS])
@pytest.mark.parametrize("name,B,h,w", MASK, ids=_ids(MASK))
def test_mask_upsample_vs_fp64_at_every_channel_window(ops, name, B, h, w, cs, co):
    """N(0,2) logits at every shape x channel window against the fp64 formula, within the derived bound of mask_bound; and, as
    test_mask_upsample_fused_equals_conv_plus_upsample does at (512, 256), equal to the 1x1 convolution kernel followed by the
    up-sampling kernel up to the online softmax's round-off.  The channels of the row outside the window hold data of the same scale:
    a kernel that ignored co, or took it for another, fails."""
    key = f"{name}.{cs}.{co}"
    x, wt, bs, flow = mask_inputs(key, B, h, w, cs)
    xs = x[..., co:co + 256]
    pm = ops.PackedMaskHead(D(wt.reshape(576, 256, 1, 1)), D(bs), post_scale=0.25)
    assert pm.a_scale == A_SCALE
    xd, fd = D(x), D(flow)
    got = mask_launch(ops, pm, xd, co, fd)
    ref64, l64 = mask_reference(xs, wt, bs, flow, F64)
    assert 1.0 < float(l64.std()) < 4.0
    bound, _ = mask_bound(xs, wt, bs, flow, pm.w_scale)
    mask_gate(key, got, ref64, mask_reference(xs, wt, bs, flow, F32)[0], bound)
    assert torch.equal(xd.cpu(), x) and torch.equal(fd.cpu(), flow)
    pc = ops.PackedConv(D(wt.reshape(576, 256, 1, 1)), D(bs), [256], post_scale=0.25)
    mask = torch.full((B, h, w, 576), NAN, device="cuda")
    ops.conv2d_nhwc(pc, [(xd, co)], (mask, 0), ops.EPI_LINEAR)
    want = ops.convex_upsample_nhwc(fd, mask).cpu()
    two = float((got - want).abs().max())
    print(f"stem_mask_edges mask_upsample.two_kernels [{key}] diff {two:.3e}")
    assert two <= 2e-6 * max(1.0, float(want.abs().max()))


# (id, weight multiplier = std of the weight part of the logits, tap bias in logit units or None)
REGIMES = [
    ("abs80", 40.0, None),                                  # |logit| around 80 and beyond: neighbouring taps differ by tens
    ("ascending_3", 0.25, lambda k: 3.0 * k),               # the running maximum moves at every tap, all nine taps keep weight
    ("descending_3", 0.25, lambda k: -3.0 * k),             # it never moves after the first
    ("ascending_120", 2.0, lambda k: 120.0 * (k - 4)),      # |logit| up to 480, steps of 120: exp(-|d|) underflows to 0 at every tap, the maximum moves
    ("descending_120", 2.0, lambda k: -120.0 * (k - 4)),    # ... and never moves: every later tap enters with weight exp(-120 k) = 0
]
REGIME_SHAPES = [MASK[4], MASK[5]]


@pytest.mark.parametrize("regime,wmul,tap_bias", REGIMES, ids=_ids(REGIMES))
@pytest.mark.parametrize("name,B,h,w", REGIME_SHAPES, ids=_ids(REGIME_SHAPES))
def test_mask_upsample_logit_regimes_vs_fp64(ops, name, B, h, w, regime, wmul, tap_bias):
    """Large and ordered logits, made by scaling weights and bias, at the two shapes whose tiles straddle images, window (264, 8):
    the same bound.  The regime itself is asserted on the fp64 logits."""
    cs, co = 264, 8
    key = f"{name}.{regime}"
    x, wt, bs, flow = mask_inputs(key, B, h, w, cs, wmul, tap_bias)
    xs = x[..., co:co + 256]
    pm = ops.PackedMaskHead(D(wt.reshape(576, 256, 1, 1)), D(bs), post_scale=0.25)
    got = mask_launch(ops, pm, D(x), co, D(flow))
    ref64, l64 = mask_reference(xs, wt, bs, flow, F64)
    bound, delta = mask_bound(xs, wt, bs, flow, pm.w_scale)
    step = l64[:, :, :, 1:] - l64[:, :, :, :-1]
    margin = 2 * float(delta.max())
    if regime == "abs80":
        assert float(l64.abs().max()) > 100.0 and 60.0 < float(l64.abs().amax(3).median()) < 110.0
    elif regime.startswith("ascending"):
        assert float(step.min()) > margin
    else:
        assert float(step.max()) < -margin
    if regime.endswith("120"):
        assert float(step.abs().min()) > 104.0 and float(l64.abs().max()) > 470.0                           # expf(-104) is 0 in fp32, subnormals included
    mask_gate(key, got, ref64, mask_reference(xs, wt, bs, flow, F32)[0], bound)


@pytest.mark.parametrize("name,B,h,w", MASK, ids=_ids(MASK))
def test_mask_upsample_equal_logits_give_the_mean_of_the_nine_taps(ops, name, B, h, w):
    """Zero weights and one bias for all 576 columns: every logit is equal, so the output is the mean of the nine taps of 8 * flow
    with the taps outside the map as zeros -- at borders and corners the divisor stays 9.  Bound: the kernel's denominator is exactly
    9 (exp(0) = 1, eight exact additions) and its numerator the nine taps added one after the other in fp32 (8 roundings), then one
    division: gamma32(9) * sum_k |f_k| / 9 per element."""
    cs, co = 264, 8
    x, _, _, flow = mask_inputs("mean." + name, B, h, w, cs)
    pm = ops.PackedMaskHead(torch.zeros(576, 256, 1, 1, device="cuda"), torch.full((576,), 1.5, device="cuda"), post_scale=0.25)
    got = mask_launch(ops, pm, D(x), co, D(flow))
    taps = _taps(flow)                                                                                      # (B,h,w,9,2)
    want = (taps.sum(3) / 9.0).permute(0, 3, 1, 2).repeat_interleave(8, 2).repeat_interleave(8, 3)
    bound = (gamma(9) * taps.abs().sum(3) / 9.0).permute(0, 3, 1, 2).repeat_interleave(8, 2).repeat_interleave(8, 3)
    eg = (got.to(F64) - want).abs()
    print(f"stem_mask_edges mask_upsample.mean9 [{name}] err_gpu {float(eg.max()):.3e} err/bound {float((eg / bound).max()):.3f}")
    assert bool((eg <= bound).all())


@pytest.mark.parametrize("name,B,h,w", MASK, ids=_ids(MASK))
def test_mask_upsample_one_tap_at_plus_60_gives_that_neighbour(ops, name, B, h, w):
    """Zero weights, a bias of +60 (in logit units) on ONE tap, the hot tap cycling through all nine: the other eight enter with
    e = exp(-60) = 8.8e-27 each.  Where the hot neighbour lies inside the map the output is 8 * its flow EXACTLY in fp32 (8 e |f| is
    far below half an ulp of any flow value here, the denominator 1 + 8 e rounds to 1); where it lies outside, the hot value is the
    padding zero and what remains is at most the eight others' e-weighted sum: |out| <= 8 e max|8 flow|."""
    cs, co = 264, 8
    x, _, _, flow = mask_inputs("hot." + name, B, h, w, cs)
    taps, inside = _taps(flow), _inside(B, h, w)
    assert float(flow.abs().min()) > 1e-12
    e60 = math.exp(-60.0)
    seen_in = seen_out = 0
    xd, fd = D(x), D(flow)
    for hot in range(9):
        bs = torch.zeros(576)
        bs[hot * 64:(hot + 1) * 64] = 240.0                                                                 # 0.25 * 240 = 60
        pm = ops.PackedMaskHead(torch.zeros(576, 256, 1, 1, device="cuda"), D(bs), post_scale=0.25)
        got = mask_launch(ops, pm, xd, co, fd)
        want = taps[:, :, :, hot].to(F32).permute(0, 3, 1, 2).repeat_interleave(8, 2).repeat_interleave(8, 3)
        ins = inside[:, :, :, hot][:, None].expand(B, 2, h, w).repeat_interleave(8, 2).repeat_interleave(8, 3)
        lim = (8 * e60 * 1.001 * taps.abs().amax(3)).permute(0, 3, 1, 2).repeat_interleave(8, 2).repeat_interleave(8, 3)
        assert torch.equal(got[ins], want[ins]), (name, hot)
        assert bool((got[~ins].to(F64).abs() <= lim[~ins]).all()), (name, hot, float(got[~ins].abs().max()))
        seen_in += int(ins.sum())
        seen_out += int((~ins).sum())
    assert seen_out > 0 and (seen_in > 0 or B * h * w == 1)


def test_mask_upsample_refusals_write_nothing(ops):
    """c_out != 576, a channel window outside the row or off a 16-byte boundary, misaligned pointers, h w >= 2^24 and B h w >= 2^31
    (sizes only, on the tiny buffers of the accepted call): 1 and the entry's message, the output keeps its NaN."""
    B, h, w, cs, co = 1, 2, 3, 264, 8
    x, wt, bs, flow = mask_inputs("refuse", B, h, w, cs)
    pm = ops.PackedMaskHead(D(wt.reshape(576, 256, 1, 1)), D(bs), post_scale=0.25)
    xd, fd = D(x), D(flow)
    _, up = guarded((B, 2, 8 * h, 8 * w), MASK_GUARD)
    P, S, Z = ops._ptr, ops._stream(), C.c_void_p(0)
    good = [P(xd), cs, co, P(pm.w_packed), 576, P(pm.bias), pm.a_scale, pm.w_scale, P(fd), B, h, w, P(up), S]

    def sub(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    E = "rnnpose_mask_upsample_f16x3"
    for i in (0, 3, 5, 8, 12):
        refused(E, sub(**{f"a{i}": Z}), b"null pointer", [up])
    for c_out in (575, 512, 64, 0):
        refused(E, sub(a4=c_out), b"c_out must be 576", [up])
    for kw in (dict(a2=12), dict(a1=252, a2=0), dict(a2=-4), dict(a2=6), dict(a1=266), dict(a1=262, a2=2)):
        refused(E, sub(**kw), b"must lie inside the row, 16-byte aligned", [up])
    for kw in (dict(a0=off(xd, 4)), dict(a3=off(pm.w_packed, 8)), dict(a8=off(fd, 4)), dict(a12=off(up, 4)), dict(a12=off(up, 8))):
        refused(E, sub(**kw), b"16-byte, flow 8-byte aligned", [up])
    for kw in (dict(a10=4096, a11=4096), dict(a9=32768, a10=256, a11=256), dict(a9=65536), dict(a9=0), dict(a10=65536, a11=1), dict(a11=0)):
        refused(E, sub(**kw), b"bad size", [up])
    for kw in (dict(a6=0.0), dict(a7=-1.0)):
        refused(E, sub(**kw), b"scales must be positive", [up])
    assert getattr(lib(), E)(*good) == 0                                                                    # the accepted call still runs
    torch.cuda.synchronize()
    assert not bool(torch.isnan(up).any())
