"""tests/zoom_ref.py (the uncast fp64 affine_grid / grid_sample behind tests/test_gpu_zoom_edges.py) tied to torch's own CPU
F.affine_grid / F.grid_sample -- the functions the reference calls -- and to oracle/zoom_oracle.py.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import zoom_ref as zr
from oracle import zoom_oracle as zo

SHEAR = np.float32([[1.3, 0.2, -0.4], [-0.3, 0.9, 0.5]])
THETAS = np.stack([SHEAR, np.float32([[-1, 0, 0], [0, 1, 0]]), np.float32([[0.6, 0, 0.7], [0, 0.6, 0.7]])])


def test_affine_grid64_vs_torch_float64_and_float32_and_oracle():
    for hc, wc in ((1, 1), (5, 65), (9, 70)):
        g = zr.affine_grid64(THETAS, hc, wc)
        assert g.dtype == np.float64
        t64 = F.affine_grid(torch.from_numpy(THETAS).double(), [3, 1, hc, wc], align_corners=False).numpy()
        np.testing.assert_allclose(g, t64, rtol=0, atol=1e-14)                  # torch's own fp64 evaluation
        assert np.abs(zr.torch_affine_grid(THETAS, 1, hc, wc) - g).max() < 1e-6    # a few fp32 ulps at |grid| <= 2.5
        assert np.abs(zo.affine_grid(THETAS, hc, wc) - g).max() <= 2.0 ** -23    # the oracle = this, cast: half an ulp at |grid| < 4


def test_grid_sample64_vs_torch_float64_and_float32_and_oracle():
    rng = np.random.default_rng(5)
    for (H, W), (hc, wc) in (((13, 21), (9, 70)), ((2, 3), (5, 65)), ((1, 1), (4, 64)), ((7, 5), (3, 63))):
        x = rng.standard_normal((3, 2, H, W)).astype(np.float32)
        grid = zr.affine_grid64(THETAS, hc, wc).astype(np.float32)
        got = zr.grid_sample64(x, grid)
        assert got.dtype == np.float64
        t64 = F.grid_sample(torch.from_numpy(x).double(), torch.from_numpy(grid).double(), mode="bilinear", padding_mode="zeros",
                            align_corners=False).numpy()
        np.testing.assert_allclose(got, t64, rtol=0, atol=1e-13)
        assert np.abs(zr.torch_grid_sample(x, grid) - got).max() < 2e-5        # the bound tests/test_zoom.py holds the oracle to
        assert np.array_equal(zo.grid_sample(x, grid), got.astype(np.float32))    # the oracle = this, cast
        # the padding census agrees with the samples: 4 taps outside <=> the fp64 sample of an all-ones image is 0
        ones = zr.grid_sample64(np.ones((3, 1, H, W), np.float32), grid)[:, 0]
        assert np.array_equal(zr.taps_outside(grid, H, W) == 4, ones == 0)
        assert (np.abs(ones - 1)[zr.taps_outside(grid, H, W) == 0] < 1e-12).all()      # (an outside tap of weight 0 also gives 1)


def test_reference_quoted_in_the_issue_the_scale_of_torch_fp32():
    """13 x 21 unit-variance image, the shear theta: torch's fp32 CPU path is a few 1e-6 from fp64 while a large share of the output is
    zero padded -- the scale every bound of test_gpu_zoom_edges.py is a multiple of."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 1, 13, 21)).astype(np.float32)
    grid = zr.torch_affine_grid(SHEAR[None], 1, 9, 70)
    err = np.abs(zr.torch_grid_sample(x, grid) - zr.grid_sample64(x, grid)).max()
    assert 0 < err < 1e-5
    assert 0.2 < (zr.taps_outside(grid, 13, 21) > 0).mean() < 0.8


def test_crop_to_image_px_is_the_oracles_two_conventions():
    """K_crop and theta of zo.zoom_params describe one window through two conventions; crop_to_image_px holds the offset between them:
    K_crop^-1 (crop pixel) == crop_to_image_px(crop pixel) for the oracle's own outputs."""
    K = np.float32([[[500, 0.7, 320], [0, 480, 240], [0, 0, 1]]])
    T = np.eye(4, dtype=np.float32)[None].copy()
    T[0, :3, 3] = [0.05, -0.02, 0.8]
    H, W = 480, 640
    for (hc, wc), box in (((240, 240), [300, 200, 420, 260]), ((128, 160), [0, 0, 0, 0]), ((2, 2), [100, 50, 130, 400])):
        theta, Kc = zo.zoom_params(np.int64([box]), K, T, H, W, hc, wc)
        M = K[0].astype(np.float64) @ np.linalg.inv(Kc[0].astype(np.float64))          # crop pixel -> image pixel, K's convention
        for j, n, N, a, s, row in ((np.linspace(-3, wc + 2, 7), wc, W, theta[0, 0, 0], theta[0, 0, 2], 0),
                                   (np.linspace(-3, hc + 2, 7), hc, H, theta[0, 1, 1], theta[0, 1, 2], 1)):
            want = M[row, row] * j + M[row, 2]
            np.testing.assert_allclose(zr.crop_to_image_px(j, a, s, n, N), want, rtol=0, atol=2.0 ** -19 * 1024)
    theta, _ = zo.zoom_params(np.int64([[0, 0, 0, 0]]), np.float32([[[500, 0, 320], [0, 500, 240], [0, 0, 1]]]), T, 480, 640, 240, 240)
    assert abs(theta[0, 0, 0] - 1.5367) < 1e-4                                  # the empty-mask window quoted in the issue
