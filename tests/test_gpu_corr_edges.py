"""The correlation family -- csrc/corr_pyramid.hip (volume + pyramid: the fp32 MFMA kernel, the three fp16x3 kernels and the split
pre-pass), csrc/corr_lookup.hip + corr_lookup.cuh (the two window-lookup kernels), csrc/corr_alt.hip (the volume-free lookup) and
csrc/corr_convc1.hip (lookup + convc1 in one launch) -- against fp64 at their edges (run with -m gpu on an MI355X; every shape whose
test name does not contain `full_size` also runs on the host-executed kernels, tests/test_kernels_on_host.py).

tests/test_gpu_parity.py meets these kernels at one tile-order supertile, four levels, unit-variance inputs and random window centres.
Here every shape is in a table with the code path it is there for; inputs are seeded by rnnpose_amd.synthetic; references are plain
fp64 expressions on the CPU.

Gates.  err_gpu = |HIP - ref64|, err_ref = max|ref32 - ref64| where ref32 is the SAME formula evaluated in fp32 on the CPU (channels
summed in a fixed order, not through a library matrix product); a test passes iff err_gpu <= max(2 * err_ref, floor) at every element.
The fp16x3 volume kernels compute, by contract (include/rnnpose_hip.h "SPLIT TENSORS"; the header of corr_pyramid_h3_kernel),
sum_c (hi1 hi2 + hi1 lo2 + lo1 hi2) / (sqrt(C) a^2) of hi = fp16(a x), lo = fp16(a x - hi): that expression is built here in fp64 from
the fp32 inputs, err_model = |contract64 - ref64| per element, and the gate is err_gpu <= max(2 * (err_model + err_ref), floor) -- the
designed loss is allowed, anything beyond it (a flushed subnormal lo half, a dropped cross term) is not.  Floors: the project's 1e-5
on volume quantities at unit-variance inputs, times the product of the two input standard deviations; 16 * 2^-24 * max|level| for a
lookup of given levels (three roundings per weight, four products, three sums, doubled); 1e-4 for the on-the-fly lookup; the fused
lookup + convc1 keeps the bound of test_corr_lookup_convc1_fused_equals_the_two_kernels.  Layout, untouched memory, zero padding,
supertile geometry, kernel variants and the NCHW / NHWC forms are exact (torch.equal).  All errors are printed per case.
"""
import math
import os

import pytest
import torch

from rnnpose_amd import synthetic as syn
from test_gpu_parity import D, N, T, close, ops  # noqa: F401  (ops: the module-scoped build fixture)

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
NAN = float("nan")
VOL_FLOOR, ALT_FLOOR = 1e-5, 1e-4
TAIL = 64 + 128                                             # NaN floats behind offs[-1]: 64, and one level-0 row more, so that a row stored past the end shows here
A_SCALE = 8.0                                               # ops.A_SCALE, written out: the contract below must not follow a changed constant
_ids = lambda cases: [c[0] for c in cases]


def gate(kernel, case, got, ref64, err_ref, floor, err_model=None):
    """err_gpu <= max(2 * (err_model + err_ref), floor) at every element; prints the errors"""
    g, r = got.detach().cpu().to(F64), ref64.to(F64)
    assert g.shape == r.shape, f"{kernel} {case}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    eg = (g - r).abs()
    bound = torch.full_like(r, 2.0 * err_ref) if err_model is None else 2.0 * (err_model + err_ref)
    bound = bound.clamp(min=floor)
    err_gpu = float(eg.max()) if r.numel() else 0.0
    em = "" if err_model is None else f" err_model {float(err_model.max()):.3e}"
    print(f"corr_edges {kernel} [{case}] err_gpu {err_gpu:.3e} err_ref {err_ref:.3e}{em}")
    bad = ~(eg <= bound)                      # (NaN fails)
    if bad.any():
        i = tuple(int(k) for k in torch.nonzero(bad)[0])
        raise AssertionError(f"{kernel} [{case}]: {int(bad.sum())}/{bad.numel()} elements beyond the gate; first at {i}: got {float(g[i])!r} "
                             f"want {float(r[i])!r}, bound {float(bound[i]):.3e}, err_gpu {err_gpu:.3e}, err_ref {err_ref:.3e}{em}")


# ================================================================================================== references
def _pool(v):
    """(R, hl, wl) -> (R, hl // 2, wl // 2): 2x2 mean, floor cropping"""
    hl, wl = v.shape[-2] // 2, v.shape[-1] // 2
    v = v[:, :2 * hl, :2 * wl]
    return (((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + v[:, 1::2, 0::2]) + v[:, 1::2, 1::2]) * 0.25


def _chain(v, B, h, w, levels):
    out = [v.reshape(B * h * w, h, w)]
    for _ in range(1, levels):
        out.append(_pool(out[-1]))
    return out


def volume_levels(f1, f2, levels, dtype):
    """f1, f2 (B,C,h,w) fp32 -> [(B*h*w, h_l, w_l)]: f1^T f2 / sqrt(C), then chained 2x2 means.  The fp32 evaluation adds the channels
    one after the other (the order a library sgemm adds in depends on the CPU it runs on)."""
    B, C, h, w = f1.shape
    a, b = f1.reshape(B, C, h * w).to(dtype), f2.reshape(B, C, h * w).to(dtype)
    if dtype == F64:
        acc = torch.bmm(a.transpose(1, 2), b)
    else:
        acc = torch.zeros(B, h * w, h * w, dtype=dtype)
        for c in range(C):
            acc += a[:, c, :, None] * b[:, c, None, :]
    return _chain(acc / math.sqrt(C), B, h, w, levels)


def contract_levels(f1, f2, levels, a_scale=A_SCALE):
    """The fp16x3 contract in fp64: hi = fp16(a x) (round to nearest even, subnormals kept, clamped to +-65504), lo = fp16(a x - hi);
    sum_c (hi1 hi2 + hi1 lo2 + lo1 hi2) / (sqrt(C) a^2); the pooled levels are means of that."""
    B, C, h, w = f1.shape

    def halves(f):
        x = (f.reshape(B, C, h * w) * a_scale).clamp(-65504.0, 65504.0)             # fp32: a power-of-two scale is exact
        hi = x.to(torch.float16)
        lo = (x - hi.to(F32)).to(torch.float16)                                     # (the fp32 difference is exact)
        return hi.to(F64), lo.to(F64)
    h1, l1 = halves(f1)
    h2, l2 = halves(f2)
    acc = torch.bmm(h1.transpose(1, 2), h2) + torch.bmm(h1.transpose(1, 2), l2) + torch.bmm(l1.transpose(1, 2), h2)
    return _chain(acc / (math.sqrt(C) * a_scale * a_scale), B, h, w, levels)


def lookup_ref(lv, coords, dtype):
    """The direct formula.  lv: [(B*N, h_l, w_l)]; coords (B,2,h,w) fp32 -> (values (B,h,w,L*81) in `dtype`, `touched` (same shape, bool):
    at least one of the four taps lies inside the level).  Channel l*81 + i*9 + j = bilinear, zeros outside, at (cx / 2^l + i - 4,
    cy / 2^l + j - 4); a centre that is non-finite or not inside (-1e6, 1e6) at the level's scale gives zeros."""
    B, _, h, w = coords.shape
    P = B * h * w
    c = coords.permute(0, 2, 3, 1).reshape(P, 2)
    d = (torch.arange(9) - 4).to(dtype)
    rows = torch.arange(P)[:, None, None]
    vals, touched = [], []
    for l, m in enumerate(lv):
        hl, wl = m.shape[-2:]
        cl = c * (0.5 ** l)                                                         # fp32, exact
        sane = (torch.isfinite(cl) & (cl.abs() < 1.0e6)).all(1)
        cc = torch.where(sane[:, None], cl, torch.zeros_like(cl)).to(dtype)
        x, y = cc[:, 0, None, None] + d[None, :, None], cc[:, 1, None, None] + d[None, None, :]
        x0, y0 = torch.floor(x), torch.floor(y)
        fx, fy = x - x0, y - y0
        x0, y0 = x0.long(), y0.long()
        m = m.to(dtype)

        def tap(xi, yi):
            ok = (xi >= 0) & (xi < wl) & (yi >= 0) & (yi < hl) & sane[:, None, None]
            v = m[rows, yi.clamp(0, hl - 1), xi.clamp(0, wl - 1)]
            return torch.where(ok, v, torch.zeros_like(v)), ok
        (v00, k00), (v10, k10), (v01, k01), (v11, k11) = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
        vals.append((((1 - fx) * (1 - fy)) * v00 + (fx * (1 - fy)) * v10 + ((1 - fx) * fy) * v01 + (fx * fy) * v11).reshape(P, 81))
        touched.append((k00 | k10 | k01 | k11).reshape(P, 81))
    return torch.cat(vals, 1).view(B, h, w, -1), torch.cat(touched, 1).view(B, h, w, -1)


def coords_grid(B, h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=F32), torch.arange(w, dtype=F32), indexing="ij")
    return torch.stack([xs, ys], 0)[None].repeat(B, 1, 1, 1)


EPS = 2.0 ** -10


def centre_table(h, w):
    """The fixed window centres (cx, cy): footprint seams, windows one texel outside, level-0 patch seams, the `sane` threshold,
    non-finite and signed-zero centres."""
    t = [(-1.0, -1.0), (-0.5, 0.0), (w - 1.0, h - 1.0), (w - 0.5, h - 0.25), (float(w), float(h)),
         (-5.0, 3.0),                                                               # nine columns -9 .. -1: exact zeros at level 0
         (-4.5, -4.5), (w + 3.5, h + 3.5), (w + 4.0, 1.0),
         (12.0, 4.0),                                                               # integers down to level 2: (3, 1); (1.5, 0.5) at level 3
         (6.0, 2.0),                                                                # integers at levels 0 and 1 only
         (999999.0, 0.0), (1.0e6, 0.0), (-1.0e6, 1.0), (3.0e9, 3.0e9),
         (NAN, 1.0), (2.0, float("inf")), (-0.0, -0.0), (1e-30, 1e-30), (-1e-30, -1e-30), (1e-30, -1e-30)]
    if w > 16 and h > 8:
        t += [(16.0 - EPS, 8.0 - EPS), (16.0, 8.0)]                                 # the corner of four 8 x 16 patches of level 0
    return t


ZERO_L0 = 5                                                 # index of (-5, 3) in the table


def coord_rounds(name, B, h, w):
    """[(coords (B,2,h,w), {flat pixel: table index})]: the grid + U(-6, 6), row h // 2 of image 0 rounded to integers, and the table
    written over pixels spread evenly from the first to the last pixel of the tensor -- in as many rounds as a small map needs."""
    tab = centre_table(h, w)
    P = B * h * w
    per = min(len(tab), max(2, P // 2))
    rounds = []
    for r0 in range(0, len(tab), per):
        chunk = list(range(r0, min(r0 + per, len(tab))))
        c = coords_grid(B, h, w) + T(syn.uniform(f"ce.jit.{name}.{r0}", (B, 2, h, w), 17, -6.0, 6.0))
        c[0, :, h // 2, :] = torch.round(c[0, :, h // 2, :])
        flat = c.permute(0, 2, 3, 1).reshape(P, 2)
        where = {}
        for k, ti in enumerate(chunk):
            p = round(k * (P - 1) / max(1, len(chunk) - 1))
            flat[p, 0], flat[p, 1] = tab[ti]
            where[p] = ti
        rounds.append((flat.view(B, h, w, 2).permute(0, 3, 1, 2).contiguous(), where))
    return rounds


def synthetic_pyramid(ops, name, B, h, w, levels):
    """Independent random levels, level l of std l + 1 (every image, pixel and level differs at the scale of the data) -> (the flat
    buffer with level 0 blocked j-patch-major BY HAND and NaN in its padding cells, [(B*N, h_l, w_l)])."""
    n = h * w
    lv = [T(syn.normal(f"ce.lv{l}.{name}", (B * n, h >> l, w >> l), 23, std=float(l + 1))) for l in range(levels)]
    npy, npx = -(-h // 8), -(-w // 16)
    p = torch.full((B, n, npy * 8, npx * 16), NAN)
    p[:, :, :h, :w] = lv[0].view(B, n, h, w)
    blocked = p.view(B, n, npy, 8, npx, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1)             # [b][patch row][patch col][i][8][16]
    flat = torch.cat([blocked] + [m.reshape(-1) for m in lv[1:]])
    offs, hl, wl = ops.pyramid_layout(B, h, w, levels)
    assert flat.numel() == offs[-1] and hl == [h >> l for l in range(levels)] and wl == [w >> l for l in range(levels)]
    return flat, lv


# ================================================================================================== A. volume and pyramid
# (id, B, C, h, w, levels)
PYRAMID = [
    ("one_pixel", 1, 64, 1, 1, 1),                          # N = 1: one partial i-tile, one partial patch, levels = 1
    ("thin_3x50_l2", 1, 32, 3, 50, 2),                      # h < 8; w not a multiple of 16; N % 4 != 0 (unaligned template); C = 32: one k-slab of the h3 kernel, two of the DMA kernel
    ("row_patch_17x33", 2, 32, 17, 33, 4),                  # one-row and one-column patches; N = 561 = 4 i-tiles + 49 rows; 90 tiles (the XCD remap's remainder branch)
    ("wide_8x129", 1, 32, 8, 129, 4),                       # one patch row, 9 patch columns, level 3 is 1 x 16; N = 1032 = 8 * 128 + 8
    ("odd_slabs_9x21_l3", 3, 96, 9, 21, 3),                 # C = 96 (three 32-slabs, six 16-slabs), B odd, pooled levels drop a row and a column
    ("aligned_16x16_c16", 1, 16, 16, 16, 4),                # fp32 entry only (C = 16: its minimum; the fp16x3 entries refuse it); aligned template, level 3 = 2 x 2
    ("full_size_default_supertile_ragged_48x56", 1, 32, 48, 56, 4),     # n_it = 21 -> two supertiles of 11 at the shipped limit of 20 (one phantom i-tile), n_patch = 24 -> 2 x 12; 29 MB
]
PYRAMID_BY_NAME = {c[0]: c for c in PYRAMID}
ENTRIES = ["f32", "f16x3", "nhwc", "split"]                 # ops.corr_pyramid "f32" / "f16x3", ops.corr_pyramid_nhwc, ops.corr_pyramid_split
# (id, std of fmap1, std of fmap2) on row_patch_17x33.  All three fp16x3 entries take these raw features: the pre-pass of the two
# fp32-source entries and ops.split_hl for the split entry write the same halves.
REGIMES = [
    ("std_1e-2", 1e-2, 1e-2),                               # a x ~ 0.08: lo ~ 4e-5 < 6.1e-5, the smallest normal fp16 -- most lo halves subnormal
    ("std_1e-3", 1e-3, 1e-3),                               # a x ~ 0.008: every lo half subnormal (a few multiples of 2^-24)
    ("std_30_vs_0.03", 30.0, 0.03),                         # mixed: normal lo halves on one side, subnormal ones on the other
]
_vol_cache = {}


def _volume_case(name, s1=1.0, s2=1.0):
    """inputs and references of a case, computed once and shared (never modified)"""
    key = (name, s1, s2)
    if key not in _vol_cache:
        _, B, C, h, w, levels = PYRAMID_BY_NAME[name]
        f1 = T(syn.normal(f"ce.f1.{name}.{s1}", (B, C, h, w), 31, std=s1))
        f2 = T(syn.normal(f"ce.f2.{name}.{s2}", (B, C, h, w), 31, std=s2))
        r64, r32 = volume_levels(f1, f2, levels, F64), volume_levels(f1, f2, levels, F32)
        err_ref = [float((a.to(F64) - b).abs().max()) for a, b in zip(r32, r64)]
        model = [(a - b).abs() for a, b in zip(contract_levels(f1, f2, levels), r64)] if C % 32 == 0 else None
        _vol_cache[key] = (f1, f2, r64, err_ref, model)
    return _vol_cache[key]


def _restore_corr_switches(ops):
    from rnnpose_amd import _lib
    ops.corr_variant(int(os.environ.get("RNNPOSE_CORR_VARIANT", ops.CORR_VARIANT_DEFAULT)))
    _lib.call("rnnpose_corr_supertile", 20)


def _build(ops, entry, f1, f2, levels, out):
    if entry in ("f32", "f16x3"):
        return ops.corr_pyramid(D(f1), D(f2), levels, out=out, precision=entry)
    n1, n2 = D(f1).permute(0, 2, 3, 1).contiguous(), D(f2).permute(0, 2, 3, 1).contiguous()
    if entry == "nhwc":
        return ops.corr_pyramid_nhwc(n1, n2, levels, out=out, a_scale=A_SCALE)
    return ops.corr_pyramid_split(ops.SplitTensor(ops.split_hl(n1, a_scale=A_SCALE), A_SCALE), ops.SplitTensor(ops.split_hl(n2, a_scale=A_SCALE), A_SCALE),
                                  levels, out=out)


def _build_checked(ops, entry, f1, f2, levels, what):
    """check 1: every cell below offs[-1] is written, nothing beyond it, and the call returns the storage it was handed"""
    B, _, h, w = f1.shape
    offs, hl, wl = ops.pyramid_layout(B, h, w, levels)
    full = torch.full((offs[-1] + TAIL,), NAN, device="cuda")
    out = full[:offs[-1]]
    buf, _ = _build(ops, entry, f1, f2, levels, out)
    assert buf.data_ptr() == out.data_ptr() and buf.numel() == offs[-1], what + ": the call did not write the buffer it was handed"
    fc = full.cpu()
    assert bool(torch.isnan(fc[offs[-1]:]).all()), what + ": wrote beyond offs[-1]"
    fin = torch.isfinite(fc[:offs[-1]])
    assert bool(fin.all()), what + f": {int((~fin).sum())} cells never written, first at {int(torch.nonzero(~fin)[0])}"
    return fc[:offs[-1]], offs, hl, wl


def _level0(buf, offs, B, h, w, what):
    """check 2 + the dense level 0: rows >= h and columns >= w of the border patches are exactly 0.0"""
    n, npy, npx = h * w, -(-h // 8), -(-w // 16)
    assert offs[1] == B * npy * npx * n * 128
    v = buf[:offs[1]].view(B, npy, npx, n, 8, 16)
    Y = (torch.arange(npy)[:, None] * 8 + torch.arange(8)[None, :])[:, None, None, :, None]       # (npy,1,1,8,1)
    X = (torch.arange(npx)[:, None] * 16 + torch.arange(16)[None, :])[None, :, None, None, :]     # (1,npx,1,1,16)
    pad = ((Y >= h) | (X >= w)).expand(npy, npx, n, 8, 16)
    assert bool((v[:, pad] == 0).all()), what + ": padding cells of level 0 are not zero"
    return v.permute(0, 3, 1, 4, 2, 5).reshape(B * n, npy * 8, npx * 16)[:, :h, :w]


def _levels_of(buf, offs, hl, wl, B, h, w, what):
    return [_level0(buf, offs, B, h, w, what)] + [buf[offs[l]:offs[l + 1]].view(B * h * w, hl[l], wl[l]) for l in range(1, len(hl))]


def _pyramid_entry(ops, name, entry, s1=1.0, s2=1.0):
    _, B, C, h, w, levels = PYRAMID_BY_NAME[name]
    f1, f2, r64, err_ref, model = _volume_case(name, s1, s2)
    floor = VOL_FLOOR * s1 * s2
    variants = (0,) if entry == "f32" else (0, 1, 2)
    first = None
    try:
        for v in variants:
            ops.corr_variant(v)
            what = f"{name} {entry} variant {v}"
            buf, offs, hl, wl = _build_checked(ops, entry, f1, f2, levels, what)
            for l, got in enumerate(_levels_of(buf, offs, hl, wl, B, h, w, what)):
                gate(f"corr_pyramid.{entry}.v{v}", f"{name}.s{s1:g}x{s2:g}.level{l}", got, r64[l], err_ref[l], floor,
                     None if entry == "f32" else model[l])
            if first is None:
                first = buf
            assert torch.equal(buf, first), what + ": differs from variant 0"
    finally:
        _restore_corr_switches(ops)
    return first


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", [c[0] for c in PYRAMID])
def test_corr_pyramid_entries_vs_fp64(ops, name, entry):
    """checks 1-3 of every entry point (the fp16x3 ones under rnnpose_corr_variant 0, 1 and 2: bit-identical)"""
    C = PYRAMID_BY_NAME[name][2]
    if entry != "f32" and C % 32:
        _, B, C, h, w, levels = PYRAMID_BY_NAME[name]
        f1, f2 = _volume_case(name)[:2]
        offs, _, _ = ops.pyramid_layout(B, h, w, levels)
        out = torch.full((offs[-1],), NAN, device="cuda")
        with pytest.raises(RuntimeError, match="C must be a positive multiple of 32"):
            _build(ops, entry, f1, f2, levels, out)
        assert bool(torch.isnan(out).all()), "a refused call wrote to the pyramid"
        return
    _pyramid_entry(ops, name, entry)


@pytest.mark.parametrize("regime,s1,s2", REGIMES, ids=_ids(REGIMES))
def test_corr_pyramid_f16x3_value_regimes(ops, regime, s1, s2):
    """check 4: features whose lo halves are fp16-subnormal at a_scale 8, and mixed magnitudes.  The gate allows the contract's own loss
    (err_model) and no more: a kernel (or a matrix instruction) that flushed subnormal halves would lose 2^-11 of every product."""
    bufs = [_pyramid_entry(ops, "row_patch_17x33", entry, s1, s2) for entry in ("f16x3", "nhwc", "split")]
    assert torch.equal(bufs[0], bufs[1]) and torch.equal(bufs[0], bufs[2]), "the three fp16x3 entries differ"
    model = _volume_case("row_patch_17x33", s1, s2)[4]
    r64 = _volume_case("row_patch_17x33", s1, s2)[2]
    print(f"corr_edges corr_pyramid.regime [{regime}] max|ref| {float(r64[0].abs().max()):.3e} err_model {float(model[0].max()):.3e}")


_super_base = {}


@pytest.mark.parametrize("limit", [1, 2, 3])
@pytest.mark.parametrize("name", ["row_patch_17x33", "wide_8x129"])
def test_corr_pyramid_supertile_geometry(ops, name, limit):
    """check 5: tile-order supertiles of at most 1, 2 and 3 i-tiles x patches (ragged splits with phantom tiles in both directions: 5
    i-tiles at limit 2 are 3 supertiles of 2, 9 patches at limit 2 are 5 of 2): every kernel variant of every fp16x3 entry writes the
    buffer of the shipped limit (20), bit for bit, padding included, every cell, and nothing beyond it."""
    from rnnpose_amd import _lib
    _, B, C, h, w, levels = PYRAMID_BY_NAME[name]
    f1, f2 = _volume_case(name)[:2]
    try:
        if name not in _super_base:
            _lib.call("rnnpose_corr_supertile", 20)
            ops.corr_variant(0)
            _super_base[name] = _build_checked(ops, "f16x3", f1, f2, levels, name + " limit 20")[0]
        base = _super_base[name]
        _lib.call("rnnpose_corr_supertile", limit)
        for v in (0, 1, 2):
            ops.corr_variant(v)
            for entry in ("f16x3", "nhwc", "split"):
                what = f"{name} {entry} variant {v} supertile limit {limit}"
                buf = _build_checked(ops, entry, f1, f2, levels, what)[0]
                assert torch.equal(buf, base), what + f": {int((buf != base).sum())} cells differ from the limit-20 buffer"
    finally:
        _restore_corr_switches(ops)


def test_corr_pyramid_refusals_write_nothing(ops):
    """check 6: each refused call returns its documented error and leaves the pyramid untouched"""
    from rnnpose_amd import _lib
    lib = _lib.load()
    B, h, w = 1, 16, 16
    pyr = torch.full((4 * h * w * h * w,), NAN, device="cuda")
    f = {c: D(syn.normal(f"ce.refuse.{c}", (B, h, w, c), 3)) for c in (24, 32, 48)}
    ws = torch.empty(4 * B * h * w * 48, device="cuda", dtype=torch.float16)
    p, st = ops._ptr, ops._stream

    def refused(rc, text):
        msg = lib.rnnpose_last_error().decode()
        assert rc == 1 and text in msg, (rc, msg)
        assert bool(torch.isnan(pyr).all()), text + ": a refused call wrote to the pyramid"
    refused(lib.rnnpose_corr_pyramid_f32(p(f[32]), p(f[32]), B, 32, h, w, 5, p(pyr), st()), "levels must be 1..4")
    refused(lib.rnnpose_corr_pyramid_split(p(f[32]), p(f[32]), B, 32, h, w, 5, A_SCALE, p(pyr), st()), "levels must be 1..4")
    refused(lib.rnnpose_corr_pyramid_f16x3(p(f[32]), p(f[32]), 1, B, 32, h, w, 5, A_SCALE, p(ws), ws.numel() * 2, p(pyr), st()), "levels must be 1..4")
    small = "feature map too small for the requested number of levels"
    refused(lib.rnnpose_corr_pyramid_f32(p(f[32]), p(f[32]), B, 32, 7, 16, 4, p(pyr), st()), small)
    refused(lib.rnnpose_corr_pyramid_split(p(f[32]), p(f[32]), B, 32, 7, 16, 4, A_SCALE, p(pyr), st()), small)
    refused(lib.rnnpose_corr_pyramid_f32(p(f[24]), p(f[24]), B, 24, h, w, 4, p(pyr), st()), "C must be a positive multiple of 16")
    refused(lib.rnnpose_corr_pyramid_f16x3(p(f[48]), p(f[48]), 1, B, 48, h, w, 4, A_SCALE, p(ws), ws.numel() * 2, p(pyr), st()),
            "C must be a positive multiple of 32")
    refused(lib.rnnpose_corr_pyramid_split(p(f[48]), p(f[48]), B, 48, h, w, 4, A_SCALE, p(pyr), st()), "C must be a positive multiple of 32")
    # the Python front end: the same texts as exceptions, and the split entry's own test on the two scales
    x = D(syn.normal("ce.refuse.nchw", (B, 32, h, w), 3))
    out = pyr[:ops.pyramid_layout(B, h, w, 4)[0][-1]]
    with pytest.raises(RuntimeError, match="levels must be 1..4"):
        ops.corr_pyramid(x, x, 5, out=out)
    with pytest.raises(RuntimeError, match=small):
        ops.corr_pyramid(x[:, :, :7], x[:, :, :7], 4, out=out, precision="f16x3")
    s = ops.split_hl(f[32], a_scale=A_SCALE)
    with pytest.raises(ValueError, match="same shape and scale"):
        ops.corr_pyramid_split(ops.SplitTensor(s, 8.0), ops.SplitTensor(s, 4.0), 4, out=out)
    assert bool(torch.isnan(pyr).all())


# ================================================================================================== B. window lookup on synthetic pyramids
# (id, B, h, w, levels, image ranges of the `part` entry)
LOOKUP = [
    ("min_2x2_l1", 1, 2, 2, 1, [(0, 1)]),                   # N = 4 < the 16 pixels of a wave: slots 4..15 repeat pixel 3; levels = 1
    ("l2_5x7", 1, 5, 7, 2, [(0, 1)]),                       # levels = 2; N = 35: the last wave has 3 pixels
    ("l3_9x21", 2, 9, 21, 3, [(0, 2), (1, 2)]),             # levels = 3; level 2 is 2 x 5
    ("seams_17x19", 3, 17, 19, 4, [(1, 3), (2, 3), (0, 1)]),    # N = 323 (not a multiple of 16): a wave's 16 pixels straddle two images; 17 rows: a one-row patch
    ("patches_16x33", 2, 16, 33, 4, [(0, 2), (1, 2)]),      # three patch columns, the last one column wide; the minimum h for 4 levels
]
SENTINEL = -7.0


def _check_lookup_values(kernel, case, got, lv, coords, where, err_scale=None, floors=None):
    """got (B,h,w,L*81) on the CPU against the direct formula: finite, exact zeros where no tap is inside, the gate per level"""
    r64, touched = lookup_ref(lv, coords, F64)
    r32, _ = lookup_ref(lv, coords, F32)
    assert bool(torch.isfinite(got).all()), f"{kernel} [{case}]: non-finite outputs"
    assert bool((got[~touched] == 0).all()), f"{kernel} [{case}]: a window tap wholly outside its level (or a centre that is not sane) is not exactly 0"
    B, h, w, _ = got.shape
    flat = got.view(B * h * w, -1)
    for p, ti in where.items():
        if ti == ZERO_L0:
            assert bool((flat[p, :81] == 0).all()), f"{kernel} [{case}]: the centre (-5, 3) must give zeros at level 0"
    for l in range(len(lv)):
        sl = slice(l * 81, (l + 1) * 81)
        floor = floors[l] if floors is not None else 16.0 * 2.0 ** -24 * float(lv[l].abs().max())
        gate(kernel, f"{case}.level{l}", got[..., sl], r64[..., sl], float((r32[..., sl].to(F64) - r64[..., sl]).abs().max()), floor)
    return r64


@pytest.mark.parametrize("name,B,h,w,levels,parts", LOOKUP, ids=_ids(LOOKUP))
def test_corr_lookup_on_synthetic_pyramids_vs_fp64(ops, name, B, h, w, levels, parts):
    from rnnpose_amd import _lib
    flat, lv = synthetic_pyramid(ops, name, B, h, w, levels)
    buf = D(flat)
    seen = set()
    try:
        for ri, (coords, where) in enumerate(coord_rounds(name, B, h, w)):
            seen |= set(where.values())
            cd = D(coords)
            got = {}
            for v in (1, 0):
                _lib.call("rnnpose_corr_lookup_variant", v)
                nchw = ops.corr_lookup(buf, cd, levels)
                nhwc = ops.corr_lookup_nhwc(buf, cd, out=torch.full((B, h, w, levels * 81), NAN, device="cuda"), levels=levels)
                assert tuple(nchw.shape) == (B, levels * 81, h, w)
                assert bool(torch.isfinite(nhwc).all()), f"{name} variant {v}: non-finite outputs (a NaN centre, or a padding cell of level 0, reached the arithmetic)"
                assert torch.equal(nchw.permute(0, 2, 3, 1), nhwc), f"{name} variant {v}: NCHW is not a permutation of NHWC"
                for b0, b1 in parts:
                    whole = torch.full((B, h, w, levels * 81), SENTINEL, device="cuda")
                    ops.corr_lookup_nhwc_part(buf, cd[b0:b1].contiguous(), whole[b0:b1], B, b0, b1, levels)
                    assert torch.equal(whole[b0:b1], nhwc[b0:b1]), f"{name} variant {v}: part [{b0},{b1}) differs from the whole batch"
                    rest = torch.cat([whole[:b0], whole[b1:]])
                    assert bool((rest == SENTINEL).all()), f"{name} variant {v}: part [{b0},{b1}) wrote rows of other images"
                got[v] = nhwc.cpu()
            assert torch.equal(got[0], got[1]), f"{name}: the two lookup kernels differ"
            _check_lookup_values("corr_lookup", f"{name}.round{ri}", got[1], lv, coords, where)
    finally:
        _lib.call("rnnpose_corr_lookup_variant", 1)
    assert seen == set(range(len(centre_table(h, w))))
    assert bool(torch.equal(buf.cpu().nan_to_num(123.0), flat.nan_to_num(123.0))), "the lookup changed the pyramid"


# ================================================================================================== C. on-the-fly lookup
# (id, B, C, h, w, levels)
ALT = [
    ("c4_5x7_l2", 1, 4, 5, 7, 2),                           # C = 4: one float4, lanes 1..63 idle
    ("c260_9x21_l3", 2, 260, 9, 21, 3),                     # C = 260 > 256: the two-float4 kernel with one live lane in the second
    ("c512_16x16_l4", 1, 512, 16, 16, 4),                   # the largest C; level 3 is 2 x 2
    ("c32_17x19_l4", 3, 32, 17, 19, 4),                     # N = 323, odd sizes: floor cropping at every level
]
ALT_CS, ALT_CO = 344, 12                                    # a (levels * 81)-channel slice at offset 12 of 344-channel rows


@pytest.mark.parametrize("name,B,C,h,w,levels", ALT, ids=_ids(ALT))
def test_corr_alt_lookup_vs_fp64(ops, name, B, C, h, w, levels):
    """ops.fmap_pyramid + rnnpose_corr_alt_lookup_f32 with a channel stride and offset: the volume of part A (pooling is linear), the
    centre table and gate of part B; err_ref = fp32 dot products in channel order, then the fp32 bilinear formula."""
    f1, f2 = T(syn.normal("ce.alt1." + name, (B, C, h, w), 41)), T(syn.normal("ce.alt2." + name, (B, C, h, w), 41))
    v64, v32 = volume_levels(f1, f2, levels, F64), volume_levels(f1, f2, levels, F32)
    n1, n2 = D(f1).permute(0, 2, 3, 1).contiguous(), D(f2).permute(0, 2, 3, 1).contiguous()
    pooled = ops.fmap_pyramid(n2, levels)
    nch = levels * 81
    for ri, (coords, where) in enumerate(coord_rounds(name, B, h, w)):
        out = torch.full((B, h, w, ALT_CS), SENTINEL, device="cuda")
        ops._launch("rnnpose_corr_alt_lookup_f32", ops._ptr(n1), ops._ptr(n2), ops._ptr(pooled), ops._ptr(D(coords)), B, h, w, C, levels, 4,
                    ops._ptr(out), ALT_CS, ALT_CO, ops._stream())
        oc = out.cpu()
        assert bool((oc[..., :ALT_CO] == SENTINEL).all()) and bool((oc[..., ALT_CO + nch:] == SENTINEL).all()), name + ": channels around the slice"
        got = oc[..., ALT_CO:ALT_CO + nch].contiguous()
        r64, touched = lookup_ref(v64, coords, F64)
        r32, _ = lookup_ref(v32, coords, F32)
        assert bool(torch.isfinite(got).all()) and bool((got[~touched] == 0).all()), name
        for l in range(levels):
            sl = slice(l * 81, (l + 1) * 81)
            gate("corr_alt_lookup", f"{name}.round{ri}.level{l}", got[..., sl], r64[..., sl], float((r32[..., sl].to(F64) - r64[..., sl]).abs().max()), ALT_FLOOR)
        if ri == 0:         # the front end (offset 0, stride = the slice) writes the same values
            assert torch.equal(ops.corr_alt_lookup(n1, n2, pooled, D(coords), levels).cpu(), got)


@pytest.mark.parametrize("C,radius,text", [(516, 4, "at most 512"), (6, 4, "multiple of 4"), (32, 3, "radius must be 4")], ids=["c516", "c6", "radius3"])
def test_corr_alt_lookup_refusals(ops, C, radius, text):
    B, h, w = 1, 4, 4
    f = D(syn.normal("ce.alt.refuse", (B, h, w, C), 3))
    out = torch.full((B, h, w, 2 * 81), NAN, device="cuda")
    with pytest.raises(RuntimeError, match=text):
        ops.corr_alt_lookup(f, f, torch.zeros(B * 2 * 2 * C + 4, device="cuda"), D(coords_grid(B, h, w)), 2, radius, out=out)
    assert bool(torch.isnan(out).all()), "a refused call wrote its output"


# ================================================================================================== D. lookup + convc1 in one launch
# (id, B_total, b0, b1, h, w)
FUSED = [
    ("16x16_b1to3_of_3", 3, 1, 3, 16, 16),                  # 512 pixels: 16 full 32-pixel tiles, the range starts inside the pyramid
    ("17x19_b0to2_of_2", 2, 0, 2, 17, 19),                  # 646 pixels: a ragged last tile, a tile that straddles two images, a one-row patch
    ("16x33_b2to3_of_4", 4, 2, 3, 16, 33),                  # one image of four, 528 pixels, three patch columns
]
FUSED_CS, FUSED_CO = 272, 8


def _split_window(shape, co, c):
    """fp16 elements of a split tensor (..., Cs) that hold channels [co, co + c): (..., Cs // 8, 2, 8)"""
    m = torch.zeros(tuple(shape[:-1]) + (shape[-1] // 8, 2, 8), dtype=torch.bool)
    assert co % 8 == 0 and c % 8 == 0
    m[..., co // 8:(co + c) // 8, :, :] = True
    return m


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
@pytest.mark.parametrize("name,Bt,b0,b1,h,w", FUSED, ids=_ids(FUSED))
def test_corr_lookup_convc1_vs_fp64(ops, name, Bt, b0, b1, h, w, split):
    """the fp64 lookup of part B followed by an fp64 1x1 convolution + ReLU, at the bound of
    test_corr_lookup_convc1_fused_equals_the_two_kernels (2e-5 of the output magnitude: the convolution is fp16x3)"""
    nb, n = b1 - b0, h * w
    flat, lv = synthetic_pyramid(ops, name, Bt, h, w, 4)
    sub = [m[b0 * n:b1 * n] for m in lv]
    wt = T(syn.normal("ce.c1w", (256, 324), 7, std=math.sqrt(2.0 / 324)))
    bs = T(syn.uniform("ce.c1b", (256,), 7, -0.3, 0.3))
    pc = ops.PackedConv1x1(D(wt.view(256, 324, 1, 1)), D(bs))
    buf = D(flat)
    for ri, (coords, where) in enumerate(coord_rounds(name, nb, h, w)):
        r64, _ = lookup_ref(sub, coords, F64)
        y64 = torch.relu(r64 @ wt.to(F64).t() + bs.to(F64))
        dst = torch.full((nb, h, w, FUSED_CS), SENTINEL, device="cuda")
        ops.corr_lookup_convc1(pc, buf, D(coords), (dst, FUSED_CO), Bt, b0, b1, relu=True, dst_split=split)
        dc = dst.cpu()
        if split:
            keep = ~_split_window(dc.shape, FUSED_CO, 256)
            raw = dc.contiguous().view(torch.float16).view(keep.shape)
            sent = torch.full(tuple(dc.shape), SENTINEL).view(torch.float16).view(keep.shape)
            assert torch.equal(raw[keep].view(torch.int16), sent[keep].view(torch.int16)), name + ": split store outside its channel window"
            got = ops.unsplit_hl(dst).cpu()[..., FUSED_CO:FUSED_CO + 256]
        else:
            assert bool((dc[..., :FUSED_CO] == SENTINEL).all()) and bool((dc[..., FUSED_CO + 256:] == SENTINEL).all()), name + ": channels around the slice"
            got = dc[..., FUSED_CO:FUSED_CO + 256]
        assert bool(torch.isfinite(got).all()), name
        bound = 2e-5 * max(1.0, float(y64.abs().max()))
        err = float((got.to(F64) - y64).abs().max())
        print(f"corr_edges corr_lookup_convc1 [{name}.{'split' if split else 'fp32'}.round{ri}] err_gpu {err:.3e} bound {bound:.3e}")
        assert err < bound, (name, err, bound)
