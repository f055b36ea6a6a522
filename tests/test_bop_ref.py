"""tests/bop_ref.py -- the fp64 restatement of the BOP pose-error functions that the device kernels are held to -- against closed
forms and hand-counted images.  CPU only."""
import numpy as np
import pytest

import bop_ref as br

K = np.array([[100.0, 0.0, 5.0], [0.0, 100.0, 3.0], [0.0, 0.0, 1.0]], np.float32)
H, W = 6, 10


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def pose(t, R=None):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R[:3, :3]
    T[:3, 3] = t
    return T


def rect(c0, c1, depth, empty=0.0):
    """rows 1..4, columns c0..c1-1 at `depth`, `empty` elsewhere"""
    d = np.full((H, W), empty, np.float32)
    d[1:5, c0:c1] = depth
    return d


IDENT = np.eye(4)[None, :3]
PLANE = np.array([[x, y, 0.0] for x in (-0.05, 0.0, 0.05) for y in (-0.03, 0.02)], np.float32)


def test_equal_poses_give_zero():
    T = pose([0.01, -0.02, 0.8], rot_z(0.3))[None, :3]
    assert np.array_equal(br.sym_dist(PLANE, IDENT, T, T, K), np.zeros((1, 2)))
    d = rect(2, 6, 1.0)[None]
    err, counts, _ = br.vsd(d, d, d, [0], K, 0.1, br.DELTA, br.TAUS)
    assert np.array_equal(err, np.zeros((1, 10))) and counts[0, 0] == counts[0, 1] == 16 and not counts[0, 2:].any()


@pytest.mark.parametrize("t", [0.01, -0.025])
def test_a_translation_along_x_of_a_planar_model(t):
    Z = 0.8
    gt, est = pose([0.0, 0.0, Z])[None, :3], pose([t, 0.0, Z])[None, :3]
    got = br.sym_dist(PLANE, IDENT, est, gt, K)
    assert np.allclose(got[0], [abs(t), 100.0 * abs(t) / Z], rtol=1e-12, atol=0)


def test_a_symmetry_of_the_list_is_found_and_a_missing_one_is_not():
    Sk = rot_z(np.pi)
    gt = pose([0.02, 0.01, 0.9], rot_z(0.4))
    est = gt @ Sk
    syms = np.stack([np.eye(4), rot_z(np.pi / 2), Sk])[:, :3]
    a = br.sym_dist_all(PLANE, syms, est[None, :3], gt[None, :3], K)
    assert a[0].argmin(0).tolist() == [2, 2]
    assert np.all(br.sym_dist(PLANE, syms, est[None, :3], gt[None, :3], K) < 1e-12)
    without = br.sym_dist(PLANE, syms[:2], est[None, :3], gt[None, :3], K)
    assert without[0, 0] > 0.05 and without[0, 1] > 5.0          # the far corners are 2 x 0.058 m apart


@pytest.mark.parametrize("empty", [0.0, -1.0, np.nan])
def test_shifted_rectangles_counted_by_hand(empty):
    """gt: columns 2-5, est: the same 4 x 4 rectangle 2 columns to the right and 0.1 deeper; nothing observed.  16 + 16 pixels, 8
    shared; on those e = 0.1 * ray with ray in [1, 1.002]."""
    gt, est = rect(2, 6, 1.0, empty)[None], rect(4, 8, 1.1, empty)[None]
    obs = np.zeros((1, H, W), np.float32)
    err, counts, near = br.vsd(est, gt, obs, [0], K, 0.0, br.DELTA, (0.05, 0.2))
    assert counts.tolist() == [[24, 8, 8, 0]] and near == 0
    assert err.tolist() == [[(8 + 24 - 8) / 24, (0 + 24 - 8) / 24]]
    err, counts, _ = br.vsd(est, gt, obs, [0], K, 0.5, br.DELTA, (0.1, 0.3))       # normalised: e = 0.2 * ray
    assert counts.tolist() == [[24, 8, 8, 0]]
    err, counts, _ = br.vsd(est, gt, obs, [0], K, -2.0, br.DELTA, (0.05, 0.15))    # a diameter <= 0 leaves e = 0.1 * ray
    assert counts.tolist() == [[24, 8, 8, 0]]


def test_an_observed_surface_in_front_hides_the_ground_truth():
    """obs 0.1 in front of gt on its columns 2-3 (more than delta = 0.015): vis_gt keeps columns 4-5 only; est (columns 4-7) is
    unobserved, hence visible.  With obs only 0.01 in front nothing is hidden."""
    gt, est = rect(2, 6, 1.0)[None], rect(4, 8, 1.0)[None]
    obs = rect(2, 4, 0.9)[None]
    err, counts, _ = br.vsd(est, gt, obs, [0], K, 0.0, br.DELTA, (0.05,))
    assert counts.tolist() == [[16, 8, 0]] and err.tolist() == [[0.5]]
    err, counts, _ = br.vsd(est, gt, rect(2, 4, 0.99)[None], [0], K, 0.0, br.DELTA, (0.05,))
    assert counts.tolist() == [[24, 8, 0]]


@pytest.mark.parametrize("missing", [0.0, -3.0, np.nan, np.inf])
def test_a_missing_observed_depth_counts_as_visible(missing):
    gt = rect(2, 6, 1.0)[None]
    obs = np.full((1, H, W), 0.5, np.float32)          # in front of everything ...
    obs[0, 1:5, 2:4] = missing                         # ... except where nothing was measured
    err, counts, _ = br.vsd(gt, gt, obs, [0], K, 0.0, br.DELTA, (0.05,))
    assert counts.tolist() == [[8, 8, 0]] and err.tolist() == [[0.0]]


def test_vis_est_takes_the_pixels_where_the_ground_truth_is_visible():
    """est 0.1 BEHIND the observed surface (not visible on its own), gt on the surface: est is counted where gt is visible."""
    gt, est = rect(2, 6, 1.0)[None], rect(2, 6, 1.1)[None]
    err, counts, _ = br.vsd(est, gt, gt.copy(), [0], K, 0.0, br.DELTA, (0.05, 0.2))
    assert counts.tolist() == [[16, 16, 16, 0]] and err.tolist() == [[1.0, 0.0]]


def test_an_empty_union_gives_one():
    z = np.zeros((2, H, W), np.float32)
    err, counts, _ = br.vsd(z, z, z[:1], [0, 0], K, 0.1, br.DELTA, br.TAUS)
    assert np.array_equal(err, np.ones((2, 10))) and not counts.any()
    hidden = rect(2, 6, 1.0)[None]                     # both models wholly behind the observed surface
    err, counts, _ = br.vsd(hidden, hidden, np.full((1, H, W), 0.5, np.float32), [0], K, 0.1, br.DELTA, (0.05,))
    assert err.tolist() == [[1.0]] and not counts.any()


def test_source_index_and_per_sample_intrinsics():
    gt = np.stack([rect(2, 6, 1.0), rect(2, 6, 1.0)])
    obs = np.stack([np.zeros((H, W), np.float32), np.full((H, W), 0.5, np.float32)])
    _, counts, _ = br.vsd(gt, gt, obs, [1, 0], K, 0.0, br.DELTA, (0.05,))
    assert counts.tolist() == [[0, 0, 0], [16, 16, 0]]


def test_recalls_count_strict_comparisons():
    vs = np.array([[0.0] * 10, [0.05] * 5 + [0.6] * 5])
    r = br.recalls(vs, [0.0, 0.021], [0.0, 12.0], [0.1, 0.1], 640)
    assert r[0].tolist() == [1.0, 1.0, 1.0]
    # 0.05 is below the 9 thetas above it (strict); 0.021 is below 0.25 ... 0.5 x 0.1 (6 of 10); 12 px is below 15 ... 50 (8)
    assert np.allclose(r[1], [5 * 9 / 100, 0.6, 0.8], rtol=0, atol=1e-15)
    assert br.recalls(vs[1:], [0.021], [12.0], [0.1], 320)[0, 2] == 0.6         # half the width halves the pixel thresholds
