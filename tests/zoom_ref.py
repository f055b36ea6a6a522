"""TEST INFRASTRUCTURE ONLY -- fp64 references for the zoom-crop kernels (csrc/zoom_crop.hip), the parts oracle/zoom_oracle.py
does not already provide.  `zo.affine_grid` and `zo.grid_sample` compute in fp64 and CAST to fp32 at the end (they restate torch's
fp32 functions); an error bound measured against them would contain their own rounding.  Here the same two operations stay in fp64:

  affine_grid64(theta, hc, wc)   F.affine_grid(theta, (B, C, hc, wc), align_corners=False) of the fp32 theta, exact to fp64 rounding
  grid_sample64(x, grid)         F.grid_sample(x, grid) bilinear / zeros / align_corners=False of the fp32 x and grid, likewise
  taps_outside(grid, H, W)       how many of a pixel's four bilinear taps lie outside the image (0 ... 4): the padding branches
  torch_affine_grid / torch_grid_sample   torch's own fp32 CPU functions (what the reference calls): they set the error scale
  crop_to_image_px(...)          the pixel relation between K_crop and theta, derived below

tests/test_zoom_ref.py ties the first two to torch's CPU functions and to oracle/zoom_oracle.py.

K_crop against theta (the property test of zoom_crop_params).  The reference builds both from ONE window [w1, w2] (pixels, per axis; n
= crop size along it, N = image size, c = w2 - w1) through two conventions (PoseRefiner.py:167-203):
  * intrinsics: crop pixel j in [0, n-1] <-> image pixel u = w1 + j c / (n - 1)          (getAffineTransform on [0, n-1]);
  * theta: the window in normalised coordinates, g = 2 w / N - 1, handed to affine_grid / grid_sample with align_corners=False, where
    crop pixel j sits at s = (2 j + 1) / n - 1 and a normalised g is the image pixel i = ((g + 1) N - 1) / 2 = w - 1/2.  So crop
    pixel j samples i(j) = w1 + (j + 1/2) c / n - 1/2.
The two disagree by  u(j) - i(j) = 1/2 + (c / n) (j / (n - 1) - 1/2):  half a pixel at the crop centre j = (n - 1) / 2 (pixel CENTRES
at integers for K, at half-integers for the window), plus a scale mismatch c / n against c / (n - 1) that grows to +-c / (2 n) at the
crop's borders.  That inconsistency is the reference's and is part of the expected value."""
import numpy as np
import torch
import torch.nn.functional as F


def affine_grid64(theta, hc, wc):
    """theta (B,2,3) -> (B,hc,wc,2) float64"""
    th = np.asarray(theta).astype(np.float64)
    xs = (2.0 * np.arange(wc, dtype=np.float64) + 1.0) / wc - 1.0
    ys = (2.0 * np.arange(hc, dtype=np.float64) + 1.0) / hc - 1.0
    bx, by = np.meshgrid(xs, ys)
    gx = th[:, 0, 0, None, None] * bx + th[:, 0, 1, None, None] * by + th[:, 0, 2, None, None]
    gy = th[:, 1, 0, None, None] * bx + th[:, 1, 1, None, None] * by + th[:, 1, 2, None, None]
    return np.stack([gx, gy], -1)


def unnormalise(grid, H, W):
    """grid (...,2) -> (ix, iy) float64 source pixel coordinates, align_corners=False"""
    g = np.asarray(grid).astype(np.float64)
    return ((g[..., 0] + 1.0) * W - 1.0) / 2.0, ((g[..., 1] + 1.0) * H - 1.0) / 2.0


def grid_sample64(x, grid):
    """x (B,C,H,W), grid (B,hc,wc,2), finite -> (B,C,hc,wc) float64, no cast"""
    x = np.asarray(x).astype(np.float64)
    B, C, H, W = x.shape
    ix, iy = unnormalise(grid, H, W)
    x0, y0 = np.floor(ix), np.floor(iy)
    out = np.zeros((B, C) + ix.shape[1:], np.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            w = (1.0 - np.abs(ix - xx)) * (1.0 - np.abs(iy - yy))
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            xc, yc = np.clip(xx, 0, W - 1).astype(np.int64), np.clip(yy, 0, H - 1).astype(np.int64)
            for b in range(B):
                out[b] += x[b][:, yc[b], xc[b]] * (w[b] * ok[b])[None]
    return out


def taps_outside(grid, H, W):
    """grid (B,hc,wc,2) -> (B,hc,wc) int: number of the four bilinear taps that fall outside the H x W image"""
    ix, iy = unnormalise(grid, H, W)
    x0, y0 = np.floor(ix), np.floor(iy)
    n = np.zeros(ix.shape, np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            n += ~((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H))
    return n


def torch_affine_grid(theta, C, hc, wc):
    th = torch.from_numpy(np.ascontiguousarray(theta, dtype=np.float32))
    return F.affine_grid(th, [th.shape[0], C, hc, wc], align_corners=False).numpy()


def torch_grid_sample(x, grid):
    return F.grid_sample(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float32)),
                         mode="bilinear", padding_mode="zeros", align_corners=False).numpy()


def crop_to_image_px(j, th_scale, th_shift, n, N):
    """Crop pixel coordinate j (continuous, K_crop's convention) along one axis -> the image pixel coordinate in K's convention that
    the window of theta assigns to it: the sampler's pixel i(j) plus the offset derived in the module docstring.  th_scale / th_shift
    are that axis's theta entries (th[0], th[2] for x; th[4], th[5] for y), n the crop size, N the image size along it."""
    j = np.asarray(j, np.float64)
    g = float(th_scale) * ((2.0 * j + 1.0) / n - 1.0) + float(th_shift)
    i = ((g + 1.0) * N - 1.0) / 2.0
    c = float(th_scale) * N                                       # window extent in pixels: th_scale = (g(w2) - g(w1)) / 2 = c / N
    return i + 0.5 + (c / n) * (j / (n - 1.0) - 0.5)
