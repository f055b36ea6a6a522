"""The zoom-crop kernels (csrc/zoom_crop.hip: vertex splat, mask bounding box, window parameters, fused affine_grid + grid_sample, plain
and indexed) against fp64 references (tests/zoom_ref.py, oracle/zoom_oracle.py) at their edges: crop windows that hang over every
border, shear / rotation / flips, non-finite theta, the 64 x 4-pixel workgroup tile edges, grid-only launches, the empty-mask window,
block boundaries of the per-image kernels, odd mask shapes and the values that decide `> 0`, round-half-even, cross-block collisions
and degenerate depth in the splat -- and one small end-to-end chain.

Tolerances of the fused crop are not constants: every case measures torch's own fp32 CPU F.affine_grid / F.grid_sample (the
functions the reference calls) against the same fp64 reference on the same inputs, and the kernel may be 4 x that plus four fp32 ulps
at the operand magnitude (2^-22 (|th0| + |th1| + |th2|) per theta row for the grid, 2^-22 max|x| for the crop).  The crop is compared
with the fp64 sampler evaluated ON THE KERNEL'S OWN GRID, which separates the sampler's error from the grid's.  Each case prints its
measured `kernel error / torch error`.  Window parameters keep the tolerances of tests/test_zoom.py.

Out of scope: a degenerate window (crop_h == 0: singular in the reference too), and the fp32-vs-fp64 window arithmetic of the
reference under different numpy versions (the oracle's statement of it, float64 between the fp32 rounding points, is the expectation).

Every case is small enough for the host-executed kernels (tests/test_kernels_on_host.py runs the whole module)."""
import numpy as np
import pytest
import torch

import zoom_ref as zr
from oracle import zoom_oracle as zo

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
SENTINEL = [INT_MAX, INT_MAX, -1, -1]
TH_TOL = dict(rtol=2e-6, atol=1e-7)             # tests/test_zoom.py
KC_TOL = dict(rtol=1e-5, atol=1e-3)


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def npy(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from rnnpose_amd import build, ops as _ops
    build.build()
    return _ops


# ================================================================================================ 1. the fused crop
def both(ops, x_src, index, theta, size, want_grid=False):
    """Run the plain kernel on the gathered input and the indexed kernel on the S sources; they must agree bit for bit.  -> plain result"""
    x = np.ascontiguousarray(x_src[index])
    a = ops.zoom_crop(D(x), D(theta), size, want_grid=want_grid)
    b = ops.zoom_crop(D(x_src), D(theta), size, want_grid=want_grid, src_index=list(index))
    a, b = (a, b) if want_grid else ((a,), (b,))
    a, b = [npy(t) for t in a], [npy(t) for t in b]
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True), "indexed kernel differs from the plain one on the gathered input"
    return a if want_grid else a[0]


def sources(B, C, H, W, seed, integer=False):
    """(x_src (2,C,H,W), index (B,)): two DIFFERENT sources and a non-monotone index, so the source offset s*C*H*W matters"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (2, C, H, W)).astype(np.float32) if integer else rng.standard_normal((2, C, H, W)).astype(np.float32)
    return x, np.array([1, 0, 1, 1, 0][:B])


IDENT = np.float32([[1, 0, 0], [0, 1, 0]])


def test_identity_theta_full_size_returns_the_image_bit_for_bit(ops):
    x, idx = sources(3, 3, 8, 16, 1)
    out = both(ops, x, idx, np.tile(IDENT, (3, 1, 1)), (8, 16))
    assert np.array_equal(out, x[idx])


def test_identity_theta_half_size_is_the_exact_2x2_block_mean(ops):
    x, idx = sources(3, 2, 8, 8, 2, integer=True)
    out = both(ops, x, idx, np.tile(IDENT, (3, 1, 1)), (4, 4))
    want = x[idx].reshape(3, 2, 4, 2, 4, 2).mean((3, 5))
    assert np.array_equal(out, want.astype(np.float32))


def test_pixels_with_four_taps_outside_are_exactly_zero(ops):
    """scale-3 window on a 5 x 6 image (most of the crop is outside), and a window entirely outside (translation 5)"""
    x, idx = sources(3, 3, 5, 6, 3)
    x += 10.0                                                          # no zero anywhere inside
    theta = np.float32([[[3, 0, 0], [0, 3, 0]], [[3, 0, 0.5], [0, -3, -0.25]], [[1, 0, 5], [0, 1, 0]]])
    out, grid = both(ops, x, idx, theta, (9, 70), want_grid=True)
    ix, iy = zr.unnormalise(grid, 5, 6)
    m = 1e-3                                                           # px: well clear of the fp32 rounding of ix
    outside = (ix < -1 - m) | (ix > 6 + m) | (iy < -1 - m) | (iy > 5 + m)
    inside = (ix > m) & (ix < 5 - m) & (iy > m) & (iy < 4 - m)
    assert 0.5 < outside[:2].mean() < 0.95 and inside[:2].sum() > 20
    assert (out.transpose(0, 2, 3, 1)[outside] == 0).all()
    assert (out.transpose(0, 2, 3, 1)[inside] > 1).all()               # (and the inside is not zero: the window did land on the image)
    assert outside[2].all() and (out[2] == 0).all()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e30, -1e30])
@pytest.mark.parametrize("slot", [0, 1, 2, 4, 5])
def test_non_finite_and_huge_theta_give_a_finite_all_zero_crop(ops, bad, slot):
    """The kernel's documented choice (the `sane` guard): no tap is read, the crop is zeros.  torch on the CPU returns NaN for NaN / inf
    and 0 for 1e30; image 1 of the batch keeps an ordinary theta and must be untouched by its neighbour."""
    x, idx = sources(2, 3, 7, 5, 4)
    theta = np.stack([IDENT, IDENT]).copy()
    theta[0].reshape(-1)[slot] = bad
    out = both(ops, x, idx, theta, (4, 64))            # (even sizes: no base coordinate is 0, so 1e30 * base is huge in every pixel)
    assert np.isfinite(out).all() and (out[0] == 0).all()
    want = zr.grid_sample64(x[idx][1:], zr.affine_grid64(theta[1:], 4, 64).astype(np.float32))
    assert np.abs(out[1] - want[0]).max() < 1e-5 and np.abs(out[1]).max() > 0.5


def _rot(deg, s):
    a = np.deg2rad(deg)
    return [[s * np.cos(a), -s * np.sin(a), 0.1], [s * np.sin(a), s * np.cos(a), -0.05]]


THETAS = {
    "shear": [[1.3, 0.2, -0.4], [-0.3, 0.9, 0.5]],
    "rot30": _rot(30, 0.8),
    "hflip": [[-1, 0, 0], [0, 1, 0]],
    "vflip_rot": _rot(200, 1.1),
    "left": [[0.5, 0, -0.8], [0, 0.45, 0.05]],
    "right": [[0.5, 0, 0.8], [0, 0.45, -0.05]],
    "top": [[0.45, 0, 0.05], [0, 0.5, -0.8]],
    "bottom": [[0.45, 0, -0.05], [0, 0.5, 0.8]],
    "corner": [[0.6, 0, 0.7], [0, 0.6, 0.7]],
}
_TN = list(THETAS)
CROPS = [(1, 1), (3, 63), (4, 64), (5, 65), (9, 70), (2, 130)]
IMAGES = [(1, 1), (2, 3), (13, 21), (7, 5)]
# every crop size with every image size; theta, C and B cycle with co-prime periods so that each value meets each tile shape
GENERAL = [(_TN[i % 9], CROPS[i % 6], IMAGES[(i // 6) % 4], (1, 3, 33)[(i + i // 6) % 3], (1, 3)[(i + i // 3) % 2]) for i in range(24)]
GENERAL += [(n, (5, 65), (13, 21), 3, 1) for n in _TN]            # every theta on the image large enough for four distinct borders


def _thetas(name, B):
    i = _TN.index(name)
    return np.float32([THETAS[_TN[(i + 4 * b) % 9]] for b in range(B)])


def _gid(c):
    return f"{c[0]}-{c[1][0]}x{c[1][1]}-from{c[2][0]}x{c[2][1]}-C{c[3]}-B{c[4]}"


def test_case_list_reaches_the_padding_branches():
    """From the fp64 reference alone: at least a quarter of all output pixels of GENERAL have one to three taps outside the image."""
    part = total = 0
    for name, (hc, wc), (H, W), C, B in GENERAL:
        n = zr.taps_outside(zr.affine_grid64(_thetas(name, B), hc, wc), H, W)
        part += int(((n >= 1) & (n <= 3)).sum())
        total += n.size
    print(f"padded-tap pixels: {part} of {total} = {part / total:.3f}")
    assert part >= 0.25 * total


@pytest.mark.parametrize("case", GENERAL, ids=_gid)
def test_crop_and_grid_vs_fp64(ops, case):
    name, (hc, wc), (H, W), C, B = case
    theta = _thetas(name, B)
    x, idx = sources(B, C, H, W, seed=hc * 1000 + wc + H)
    out, grid = both(ops, x, idx, theta, (hc, wc), want_grid=True)
    assert np.array_equal(both(ops, x, idx, theta, (hc, wc)), out)                       # want_grid does not change the crop
    g_only = ops.zoom_crop(None, D(theta), (hc, wc), want_grid=True)
    assert g_only[0] is None and np.array_equal(npy(g_only[1]), grid)                    # grid-only launch (in = None, C = 0): the same grid
    # the grid, per image and theta row
    g64 = zr.affine_grid64(theta, hc, wc)
    e_k = np.abs(grid - g64).max((1, 2))                                                 # (B, 2)
    e_t = np.abs(zr.torch_affine_grid(theta, C, hc, wc) - g64).max((1, 2))
    bound = 4 * e_t + 2.0 ** -22 * np.abs(theta.astype(np.float64)).sum(2)
    print(f"grid   kernel {e_k.max():.3e} torch {e_t.max():.3e} ratio {e_k.max() / max(e_t.max(), 1e-30):.2f} bound {bound.min():.3e}")
    assert (e_k <= bound).all(), (e_k, bound)
    # the crop, on the kernel's own grid
    xg = x[idx]
    c64 = zr.grid_sample64(xg, grid)
    e_k = np.abs(out - c64).max()
    e_t = np.abs(zr.torch_grid_sample(xg, grid) - c64).max()
    bound = 4 * e_t + 2.0 ** -22 * np.abs(xg).max()
    n = zr.taps_outside(grid, H, W)
    print(f"crop   kernel {e_k:.3e} torch {e_t:.3e} ratio {e_k / max(e_t, 1e-30):.2f} bound {bound:.3e} padded {((n >= 1) & (n <= 3)).mean():.2f}")
    assert e_k <= bound, (e_k, bound)


# ================================================================================================ 2. mask_bbox
def expect_bbox(depth):
    bb = zo.mask_bbox(depth)
    bb[~(depth > 0).any((1, 2, 3))] = SENTINEL
    return bb.tolist()


def _offset_on_lane_63(H, W):
    """flat index inside the first 16-row group that thread 64 k + 63 of the 256-thread block reads first, k as large as the group allows"""
    n = min(H, 16) * W
    o = min(n, 256) - 1
    o -= (o - 63) % 64
    return o if o >= 0 else None


def mask_cases(H, W):
    """name -> list of (y, x) foreground pixels"""
    c = {"none": [], "corner00": [(0, 0)], "corner0W": [(0, W - 1)], "cornerH0": [(H - 1, 0)], "last": [(H - 1, W - 1)],
         "full": [(y, x) for y in range(H) for x in range(W)]}
    o = _offset_on_lane_63(H, W)
    if o is not None:
        c["lane63"] = [(o // W, o % W)]
    if H > 16:
        c["two_groups"] = [(1, W - 1), (H - 1, 0)]                       # different workgroups: joined by the atomics alone
    if min(H, 16) * W > 130:
        c["two_waves"] = [(1 // W, 1 % W), (130 // W, 130 % W)]          # threads 1 and 130 of one workgroup
    return c


MASK_SIZES = [(1, 1), (1, 300), (15, 63), (16, 64), (17, 65), (33, 7), (50, 70)]
BACKGROUND = np.float32([0.0, -0.0, -1.0, np.nan, -np.inf, -1e-40])         # none of them is `> 0`
FOREGROUND = np.float32([1.0, 1e-40, np.inf, 3.5])                          # a denormal and +inf count


@pytest.mark.parametrize("H,W", MASK_SIZES)
def test_mask_bbox_shapes_pixels_and_comparison_values(ops, H, W):
    cases = mask_cases(H, W)
    depth = np.empty((len(cases), 1, H, W), np.float32)
    depth[:] = BACKGROUND[np.arange(H * W) % len(BACKGROUND)].reshape(H, W)
    for b, pix in enumerate(cases.values()):
        for k, (y, x) in enumerate(pix):
            depth[b, 0, y, x] = FOREGROUND[(k + b) % len(FOREGROUND)]
    assert depth[1, 0, 0, 0] == np.float32(1e-40) and depth[1, 0, 0, 0] > 0           # the corner pixel IS the denormal
    got = npy(ops.mask_bbox(D(depth))).tolist()
    want = expect_bbox(depth)
    assert want[0] == SENTINEL
    for name, g, w in zip(cases, got, want):
        assert g == w, (name, g, w)


def test_mask_bbox_empty_image_between_two_others_keeps_its_sentinel(ops):
    depth = np.zeros((3, 1, 17, 65), np.float32)
    depth[0, 0, 16, 64] = 1.0
    depth[1] = -1.0
    depth[2, 0, 3:9, 60:65] = np.inf
    assert npy(ops.mask_bbox(D(depth))).tolist() == [[64, 16, 64, 16], SENTINEL, [60, 3, 64, 8]] == expect_bbox(depth)


def test_mask_bbox_65_images_cross_the_init_block(ops):
    """bbox_init_kernel: 4 B = 260 > 256 threads.  A different single pixel per image, every fifth image empty."""
    B, H, W = 65, 17, 65
    depth = np.full((B, 1, H, W), -0.0, np.float32)
    for b in range(B):
        if b % 5 != 2:
            depth[b, 0, (7 * b) % H, (11 * b + 3) % W] = 0.5 + b
    got = npy(ops.mask_bbox(D(depth))).tolist()
    assert got == expect_bbox(depth)
    assert got[62] == SENTINEL and got[64] == [(11 * 64 + 3) % W, (7 * 64) % H] * 2


# ================================================================================================ 3. zoom_crop_params
def regime(r, i, H, W):
    """-> (box [x0,y0,x1,y1] or None = empty mask, centre (cx, cy) in pixels): where the projected model origin lies against the box.
    The four `max` terms of the window height, ratio*(x1-cx), ratio*(cx-x0), cy-y0, y1-cy, each win in one of 1..4."""
    j = (i // 7) % 5                                     # a little variation between images of the same regime
    bx, by = W // 2 + j, H // 2 - j
    if r == 0:
        return [bx - 9, by - 6, bx + 8, by + 7], (bx + 0.3, by - 0.4)                  # centre inside the box
    if r == 1:
        return [bx, by - 3, bx + 12, by + 3], (bx - 6.5 - j, by + 0.25)                # centre left of the box: the `right` term wins
    if r == 2:
        return [bx - 12, by - 3, bx, by + 3], (bx + 5.5 + j, by - 0.25)                # right of it: `left` wins
    if r == 3:
        return [bx - 3, by - 10, bx + 3, by], (bx + 0.5, by + 7.25 + j)                # below it: `up` wins
    if r == 4:
        return [bx - 3, by, bx + 3, by + 10], (bx - 0.5, by - 6.75 - j)                # above it: `down` wins
    if r == 5:
        return [2, 3, 12 + j, 11], (-0.35 * W - j, 1.2 * H)                            # centre outside the image
    return None, (0.55 * W + j, 0.45 * H)                                              # empty mask


def params_batch(B, H, W, skew=True):
    """bbox_kernel (B,4) int32 with the sentinel for empty masks, bbox_oracle (zeros there), K (B,3,3) per image, T (B,4,4)"""
    bk, bo = np.zeros((B, 4), np.int32), np.zeros((B, 4), np.int64)
    K, T = np.zeros((B, 3, 3), np.float32), np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    wins = []
    for i in range(B):
        box, (cx, cy) = regime(i % 7, i, H, W)
        fx, fy, sk = 60.0 + 3 * (i % 4), 58.0 + 2 * (i % 3), (0.0, 1.5, -0.75)[i % 3] if skew else 0.0
        px, py, tz = W / 2 - 0.5 + (i % 2), H / 2 + 0.25, 0.6 + 0.05 * (i % 5)
        ty = (cy - py) * tz / fy
        tx = ((cx - px) * tz - sk * ty) / fx
        K[i], T[i, :3, 3] = [[fx, sk, px], [0, fy, py], [0, 0, 1]], [tx, ty, tz]
        bk[i], bo[i] = (SENTINEL, 0) if box is None else (box, box)
        # which term of the max wins, from the fp32 inputs the kernel sees
        c = K[i].astype(np.float64) @ T[i, :3, 3].astype(np.float64)
        u, v = c[0] / c[2], c[1] / c[2]
        terms = [H / W * (bo[i, 2] - u), H / W * (u - bo[i, 0]), v - bo[i, 1], bo[i, 3] - v]
        wins.append(int(np.argmax(terms)))
    return bk, bo, K, T, wins


PARAM_CASES = [(1, (48, 64), (24, 40), 0.4), (64, (48, 64), (128, 160), 0.0), (65, (64, 48), (2, 2), 1.0), (130, (48, 64), (240, 240), 0.4),
               (65, (33, 70), (24, 40), 0.0), (7, (64, 48), (128, 160), 0.4)]


@pytest.fixture(scope="module")
def params_runs(ops):
    """every PARAM_CASES entry, run once: (inputs, oracle outputs, kernel outputs), shared by the oracle and the property test"""
    runs = {}
    for B, (H, W), (hc, wc), margin in PARAM_CASES:
        bk, bo, K, T, wins = params_batch(B, H, W)
        th_o, kc_o = zo.zoom_params(bo, K, T, H, W, hc, wc, margin)
        th, kc = ops.zoom_crop_params(D(bk), D(K), D(T), (H, W), (hc, wc), margin)
        runs[(B, H, W, hc, wc, margin)] = (bk, bo, K, T, wins, th_o, kc_o, npy(th), npy(kc))
    return runs


def test_params_regimes_are_what_they_claim():
    _, bo, K, T, wins = params_batch(130, 48, 64)
    assert [wins[i] for i in range(1, 5)] == [0, 1, 2, 3]                              # each term of the max wins somewhere
    assert len({i % 7 for i in (63, 64, 65, 129)}) == 4                                # the block-boundary images differ in regime
    c = np.einsum("bij,bj->bi", K, T[:, :3, 3])
    assert (c[5::7, 0] / c[5::7, 2] < 0).all() and (c[5::7, 1] / c[5::7, 2] > 48).all()
    assert (K[:, 0, 1] != 0).any() and len({tuple(k.ravel()) for k in K}) > 8          # skew, per-image K


@pytest.mark.parametrize("case", PARAM_CASES, ids=lambda c: f"B{c[0]}-{c[1][0]}x{c[1][1]}-to{c[2][0]}x{c[2][1]}-m{c[3]}")
def test_params_vs_oracle_every_row_the_empty_mask_included(params_runs, case):
    B, (H, W), (hc, wc), margin = case
    bk, bo, K, T, wins, th_o, kc_o, th, kc = params_runs[(B, H, W, hc, wc, margin)]
    assert np.isfinite(th).all() and np.isfinite(kc).all()
    for i in range(B):
        np.testing.assert_allclose(th[i], th_o[i], err_msg=f"theta of image {i} (regime {i % 7})", **TH_TOL)
        np.testing.assert_allclose(kc[i], kc_o[i], err_msg=f"K_crop of image {i} (regime {i % 7})", **KC_TOL)
    assert (th[:, 0, 1] == 0).all() and (th[:, 1, 0] == 0).all()
    if B >= 7:
        assert (bk[6] == SENTINEL).all() and abs(th[6, 0, 0]) < 10                     # the empty-mask row: no INT_MAX arithmetic


def test_params_empty_mask_window_quoted_in_the_issue(ops):
    K = np.float32([[[500, 0, 320], [0, 500, 240], [0, 0, 1]]])
    T = np.eye(4, dtype=np.float32)[None].copy()
    T[0, :3, 3] = [0.05, -0.02, 0.8]
    bb = ops.mask_bbox(D(np.zeros((1, 1, 480, 640), np.float32)))
    assert npy(bb).tolist() == [SENTINEL]
    th, kc = ops.zoom_crop_params(bb, D(K), D(T), (480, 640), (240, 240), 0.4)
    th_o, kc_o = zo.zoom_params(np.zeros((1, 4), np.int64), K, T, 480, 640, 240, 240)
    assert abs(float(th_o[0, 0, 0]) - 1.5367) < 1e-4
    np.testing.assert_allclose(npy(th), th_o, **TH_TOL)
    np.testing.assert_allclose(npy(kc), kc_o, **KC_TOL)


@pytest.mark.parametrize("case", PARAM_CASES, ids=lambda c: f"B{c[0]}-{c[1][0]}x{c[1][1]}-to{c[2][0]}x{c[2][1]}-m{c[3]}")
def test_params_K_crop_and_theta_describe_the_same_window(params_runs, case):
    """On the kernel's outputs alone: a camera-frame point projected with K_crop lands on a crop pixel; theta's window, read with the
    align_corners=False conventions of affine_grid / grid_sample, assigns that crop pixel an image pixel; with the reference's
    half-pixel / scale inconsistency between the two conventions taken out (zoom_ref's docstring derives it) that is the pixel K
    projects the point to.
    Tolerance 2^-19 M px, M = the largest pixel magnitude involved (image size, window corners, the projected point): the two paths
    hold 8 + 4 fp32 rounding points (window corners, a / 1/a / -o/a, two products and a sum per K_crop entry, its storage; the
    normalised corners and the two theta entries), each <= 2^-24 M here -- 12 * 2^-24, doubled for the fp64 evaluation of the
    quotients below: 2^-19."""
    B, (H, W), (hc, wc), margin = case
    _, _, K, T, _, _, _, th, kc = params_runs[(B, H, W, hc, wc, margin)]
    rng = np.random.default_rng(B)
    for i in range(B):
        X = T[i, :3, 3].astype(np.float64) + rng.uniform(-0.08, 0.08, (5, 3))
        p, q = X @ K[i].astype(np.float64).T, X @ kc[i].astype(np.float64).T
        u, v, ju, jv = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        for got, want, a, s, N in ((zr.crop_to_image_px(ju, th[i, 0, 0], th[i, 0, 2], wc, W), u, th[i, 0, 0], th[i, 0, 2], W),
                                   (zr.crop_to_image_px(jv, th[i, 1, 1], th[i, 1, 2], hc, H), v, th[i, 1, 1], th[i, 1, 2], H)):
            corners = [(s - a + 1) * N / 2, (s + a + 1) * N / 2]
            M = max(N, np.abs(corners).max(), np.abs(want).max())
            assert np.abs(got - want).max() <= 2.0 ** -19 * M, (i, i % 7, got, want)


# ================================================================================================ 4. the splat
def splat(verts_list, T, K, size):
    from rnnpose_amd import zoom
    return npy(zoom.render_pointcloud([D(np.float32(v)) for v in verts_list], D(np.float32(T)), D(np.float32(K)), size))[:, 0]


def KP2(cx, cy, f=64.0):
    return np.float32([[f, 0, cx], [0, f, cy], [0, 0, 1]])


EYE = np.eye(4, dtype=np.float32)


def test_splat_rounds_half_to_even(ops):
    """f = 64, integer principal point, Z = 1: x / z is exact, so the vertices sit at EXACTLY k + 0.5 pixels, k = 0..5 -> 0 2 2 4 4 6"""
    H, W, K = 9, 10, KP2(4, 3)
    k = np.arange(6)
    vx = np.stack([(k + 0.5 - 4) / 64, np.full(6, (7 - 3) / 64), np.ones(6)], 1)            # along x in row 7
    vy = np.stack([np.full(6, (8 - 4) / 64), (k + 0.5 - 3) / 64, np.ones(6)], 1)            # along y in column 8
    got = splat([np.concatenate([vx, vy])], EYE[None], K[None], (H, W))[0]
    want = np.zeros((H, W), np.float32)
    want[7, [0, 2, 4, 6]] = 1
    want[[0, 2, 4, 6], 8] = 1
    assert np.array_equal(got, want)
    assert np.array_equal(got, zo.render_pointcloud(np.float32(np.concatenate([vx, vy])), EYE, K, H, W))


@pytest.mark.parametrize("last_is_behind", [False, True])
def test_splat_collision_across_blocks_highest_index_wins(ops, last_is_behind):
    """600 vertices = three 256-thread blocks; 3, 300 and 599 sit on the optical axis (one pixel) at different depths"""
    H, W, K = 24, 40, KP2(17, 9)
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.uniform(-0.3, 0.3, (600, 2)), rng.uniform(0.8, 1.6, (600, 1))], 1).astype(np.float32)
    v[[3, 300, 599]] = [[0, 0, 1.25], [0, 0, 2.5], [0, 0, -0.75 if last_is_behind else 0.5]]
    got = splat([v], EYE[None], K[None], (H, W))
    want = zo.render_pointcloud(v, EYE, K, H, W)
    assert np.array_equal(got[0], want)
    assert got[0, 9, 17] == (-0.75 if last_is_behind else 0.5)
    bb = npy(ops.mask_bbox(D(got[:, None]))).tolist()
    assert bb == zo.mask_bbox(want[None, None]).tolist()
    assert (want[9, 17] > 0) != last_is_behind                                              # a negative owner is not foreground


@pytest.mark.parametrize("zero_last", [False, True])
def test_splat_zero_depth_vertices_land_on_pixel_0(ops, zero_last):
    """Z == 0 exactly with X > 0, < 0, == 0: +inf, -inf and NaN pixel coordinates -> pixel (0, 0) (the reference's .long() of a
    non-finite value, clamped).  Their depth, 0, overwrites an earlier vertex of pixel (0, 0) and is overwritten by a later one."""
    H, W, K = 6, 8, KP2(4, 3)
    origin = np.float32([[-4 / 64, -3 / 64, 1.0]])                                          # projects to pixel (0, 0), depth 1
    degenerate = np.float32([[1, 0, 0], [-1, 0, 0], [0, 0, 0], [0.5, -2, 0]])
    v = np.concatenate([origin, degenerate] if zero_last else [degenerate, origin])
    got = splat([v], EYE[None], K[None], (H, W))[0]
    assert np.array_equal(got, zo.render_pointcloud(v, EYE, K, H, W))
    assert got[0, 0] == (0.0 if zero_last else 1.0) and np.count_nonzero(got) == (0 if zero_last else 1)


def _uneven():
    rng = np.random.default_rng(11)
    H, W = 31, 45
    counts = (1, 700, 257)
    verts = [rng.uniform(-0.25, 0.25, (n, 3)).astype(np.float32) for n in counts]
    from rnnpose_amd import synthetic as syn
    T = syn.se3_exp_np(rng.normal(0, 0.5, (3, 6))).astype(np.float32)
    T[:, :3, 3] = [[0.02, -0.01, 0.9], [-0.05, 0.03, 0.7], [0.3, 0.2, 0.8]]                # (image 2: partly off-screen -> border clamps)
    K = np.float32([[[50, 0.5, 22], [0, 48, 15], [0, 0, 1]], [[61, 0, 20.5], [0, 63, 16.25], [0, 0, 1]], [[40, -1, 30], [0, 45, 10], [0, 0, 1]]])
    return verts, T, K, H, W


def test_splat_uneven_batch_per_image_K_and_T(ops):
    verts, T, K, H, W = _uneven()
    got = splat(verts, T, K, (H, W))
    for b in range(3):
        assert np.array_equal(got[b], zo.render_pointcloud(verts[b], T[b], K[b], H, W)), b
    assert all((got[b] > 0).sum() >= min(len(verts[b]), 40) // 2 for b in range(3))
    for perm in ([2, 0, 1], [1, 2, 0]):                                                     # an image does not depend on its neighbours
        assert np.array_equal(splat([verts[p] for p in perm], T[perm], K[perm], (H, W)), got[perm])


def test_splat_tiny_image_where_most_vertices_clamp(ops):
    H, W = 5, 7
    rng = np.random.default_rng(13)
    v = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    v[:, 2] = rng.uniform(0.5, 1.5, 300)
    v[::17, 2] *= -1
    K = np.float32([[30, 0, 3.25], [0, 28, 2.5], [0, 0, 1]])
    got = splat([v], EYE[None], K[None], (H, W))[0]
    want = zo.render_pointcloud(v, EYE, K, H, W)
    assert np.array_equal(got, want)
    u, w = 30.0 * v[:, 0] / v[:, 2] + 3.25, 28.0 * v[:, 1] / v[:, 2] + 2.5
    assert ((u < -0.5) | (u > W - 0.5) | (w < -0.5) | (w > H - 0.5)).mean() > 0.6           # most vertices clamp to a border
    assert (want[0] != 0).all() and (want[:, 0] != 0).all() and (want[:, -1] != 0).all()     # ... e.g. the whole top, left and right borders


def test_splat_all_behind_the_camera_gives_the_zero_box_window(ops):
    from rnnpose_amd import zoom
    H, W = 24, 40
    rng = np.random.default_rng(17)
    v = rng.uniform(-0.2, 0.2, (300, 3)).astype(np.float32)
    T = EYE[None].copy()
    T[0, :3, 3] = [0.03, -0.02, -0.9]
    K = KP2(19.5, 11.5, 60.0)[None]
    depth = zoom.render_pointcloud([D(v)], D(T), D(K), (H, W))
    d = npy(depth)
    assert np.array_equal(d[0, 0], zo.render_pointcloud(v, T[0], K[0], H, W)) and (d < 0).any() and not (d > 0).any()
    grids, kc, th = zoom.gen_zoom_crop_grids(depth, D(K), D(T), [1, 3, 12, 20])
    th_o, kc_o = zo.zoom_params(np.zeros((1, 4), np.int64), K, T, H, W, 12, 20)
    np.testing.assert_allclose(npy(th), th_o, **TH_TOL)
    np.testing.assert_allclose(npy(kc), kc_o, **KC_TOL)
    assert np.abs(npy(grids) - zr.affine_grid64(npy(th), 12, 20)).max() <= 2.0 ** -22 * np.abs(npy(th)).sum(2).max()


# ================================================================================================ 5. the chain
def test_chain_splat_bbox_params_crop_vs_oracle_chain(ops):
    """48 x 64 -> 24 x 40, B = 3, image 1 with an empty foreground.  Every stage against the oracle's, at the tolerances above; the
    final crop also against the ORACLE's chain end to end, where the theta tolerance becomes a sampling shift: |d ix| <= W/2 (tol(th0) +
    tol(th2)) px (|base| <= 1), times the largest step between neighbouring pixels of the image."""
    from rnnpose_amd import zoom
    H, W, hc, wc, C = 48, 64, 24, 40, 3
    rng = np.random.default_rng(23)
    verts = [rng.uniform(-0.12, 0.12, (n, 3)).astype(np.float32) for n in (400, 90, 700)]
    T = np.tile(EYE, (3, 1, 1))
    T[:, :3, 3] = [[0.05, -0.03, 0.8], [0.0, 0.02, -0.7], [-0.1, 0.06, 0.9]]
    K = np.float32([[[70, 0, 31.5], [0, 70, 23.5], [0, 0, 1]], [[64, 0.5, 30], [0, 66, 25], [0, 0, 1]], [[75, -0.5, 33], [0, 72, 22], [0, 0, 1]]])
    x = rng.standard_normal((3, C, H, W)).astype(np.float32)
    depth = zoom.render_pointcloud([D(v) for v in verts], D(T), D(K), (H, W))
    d = npy(depth)
    for b in range(3):
        assert np.array_equal(d[b, 0], zo.render_pointcloud(verts[b], T[b], K[b], H, W))
    bb = npy(ops.mask_bbox(depth))
    assert bb.tolist() == expect_bbox(d) and bb[1].tolist() == SENTINEL and bb[0, 2] > bb[0, 0]
    grids, kc, th = zoom.gen_zoom_crop_grids(depth, D(K), D(T), [3, C, hc, wc])
    out = npy(zoom.zoom_crop(D(x), th, (hc, wc)))
    grids, kc, th = npy(grids), npy(kc), npy(th)
    th_o, kc_o = zo.zoom_params(zo.mask_bbox(d), K, T, H, W, hc, wc)
    np.testing.assert_allclose(th, th_o, **TH_TOL)
    np.testing.assert_allclose(kc, kc_o, **KC_TOL)
    g64 = zr.affine_grid64(th, hc, wc)
    e_t = np.abs(zr.torch_affine_grid(th, C, hc, wc) - g64).max((1, 2))
    assert (np.abs(grids - g64).max((1, 2)) <= 4 * e_t + 2.0 ** -22 * np.abs(th.astype(np.float64)).sum(2)).all()
    c64 = zr.grid_sample64(x, grids)
    crop_bound = 4 * np.abs(zr.torch_grid_sample(x, grids) - c64).max() + 2.0 ** -22 * np.abs(x).max()
    assert np.abs(out - c64).max() <= crop_bound
    # end to end against the oracle's own chain
    want = zr.grid_sample64(x, zr.affine_grid64(th_o, hc, wc))
    tol = TH_TOL["rtol"] * np.abs(th_o.astype(np.float64)) + TH_TOL["atol"]
    shift = max(W / 2 * (tol[:, 0, 0] + tol[:, 0, 2]).max(), H / 2 * (tol[:, 1, 1] + tol[:, 1, 2]).max()) + \
        max(W, H) / 2 * np.abs(grids - g64).max()
    step = max(np.abs(np.diff(x, axis=2)).max(), np.abs(np.diff(x, axis=3)).max(), np.abs(x).max())
    assert np.abs(out - want).max() <= crop_bound + 2 * shift * step                        # (a shift in x and one in y)
    assert np.abs(out).max() > 1
