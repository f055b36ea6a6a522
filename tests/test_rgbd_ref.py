"""tests/rgbd_ref.py, the numpy restatement the depth-aware LM kernels are checked against (tests/test_gpu_rgbd.py), checked itself: the
Jacobian and residual against finite differences of exp(xi) G, the hole-aware sampling rule on hand-made frames, the gate at exactly
representable boundaries and the scale against its formula.  CPU only."""
import numpy as np

import rgbd_ref as rr
from rnnpose_amd import synthetic as syn

IDENT_THETA = np.array([[1, 0, 0], [0, 1, 0]], np.float32)            # crop == frame when both have one size


def _one_pixel_scene(dz=0.0, depth=1.25, H=4, W=4, obs_value=None):
    """a 4 x 4 crop that IS the frame (theta = identity, K_obs = K), every target on its own pixel centre: ix = x, iy = y exactly"""
    K = np.array([[[6.0, 0, 1.5], [0, 5.0, 2.0], [0, 0, 1]]], np.float32)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    target = np.stack([xs, ys], -1)[None].astype(np.float32)
    dep = np.full((1, H, W), depth, np.float32)
    G = np.eye(4, dtype=np.float32)[None].copy()
    G[0, 2, 3] = dz
    obs = np.full((1, H, W), depth if obs_value is None else obs_value, np.float32)
    return dict(target=target, weight=np.ones((1, H, W), np.float32), depth=dep, K=K, G=G, obs_depth=obs, src_index=None,
                theta=IDENT_THETA[None], K_obs=K)


def test_identity_crop_maps_pixel_centres_onto_themselves():
    for f in (np.float32, np.float64):
        ix, iy = rr.obs_position(np.arange(4.0), np.arange(4.0)[::-1], 4, 4, IDENT_THETA, 4, 4, f)
        assert np.array_equal(ix, np.arange(4.0)) and np.array_equal(iy, np.arange(4.0)[::-1]) and ix.dtype == f
    # a crop of the frame's right half at twice the resolution: crop 8 wide over frame columns 4..8 of 8
    ix, _ = rr.obs_position(np.array([0.0, 7.0]), np.zeros(2), 8, 8, np.array([[0.5, 0, 0.5], [0, 1, 0]], np.float32), 8, 8)
    assert np.allclose(ix, [3.75, 7.25])


def test_jt_and_r3_against_finite_differences_of_the_left_increment():
    rng = np.random.RandomState(3)
    h = 1e-6
    for _ in range(5):
        X = rng.uniform(-1, 1, 3) + [0, 0, 2.0]
        Y = X + rng.normal(0, 0.05, 3)
        JT = rr.jt_matrix(X)
        grad = np.zeros(6)
        for i in range(6):
            e = np.zeros((1, 6))
            e[0, i] = h
            Xp = syn.se3_exp_np(e)[0] @ np.append(X, 1.0)
            Xm = syn.se3_exp_np(-e)[0] @ np.append(X, 1.0)
            assert np.allclose((Xp - Xm)[:3] / (2 * h), JT[:, i], atol=1e-8), i          # d(exp(xi) X)/d xi_i at 0
            grad[i] = (0.5 * np.sum((Y - Xp[:3]) ** 2) - 0.5 * np.sum((Y - Xm[:3]) ** 2)) / (2 * h)
        assert np.allclose(JT.T @ (Y - X), -grad, atol=1e-8)                              # b = J_T^T r3 is the descent direction of |r3|^2 / 2


def test_depth_sums_are_omega_jt_jt_and_omega_jt_r3_per_pixel():
    s = _one_pixel_scene(dz=0.03125)
    s["weight"][:] = 0
    s["weight"][0, 1, 2] = 0.75
    for f in (np.float32, np.float64):
        H1, b1, d1, terms = rr.normal_eq(**s, depth_weight=2.0, depth_gate=0.0625, f=f, want_terms=True)
        H0, b0, d0 = rr.normal_eq(**s, depth_weight=0.0, depth_gate=0.0625, f=f)
        t = terms[0]
        X, Yp = t["X1"][1, 2].astype(np.float64), t["Yp"][1, 2].astype(np.float64)
        Zc = X[2]
        omega = 2.0 * 6.0 * 5.0 / Zc ** 2                                                 # depth_weight fx fy / Zc^2
        assert np.isclose(float(t["omega"][1, 2]), omega, rtol=1e-6)
        JT = rr.jt_matrix(X)
        assert np.allclose(H1[0] - H0[0], 0.75 * omega * JT.T @ JT, rtol=1e-6, atol=1e-9)
        assert np.allclose(b1[0] - b0[0], 0.75 * omega * JT.T @ (Yp - X), rtol=1e-5, atol=1e-9)
        assert np.allclose(Yp - X, [0, 0, -0.03125], atol=1e-5)                           # the observation sits at the un-displaced depth
        assert d1[0, 0] == 16 and d0[0, 0] == 16                                          # the count ignores weights and depth_weight
        assert np.isclose(d1[0, 1], 0.75 * omega * np.sum((Yp - X) ** 2), rtol=1e-5) and d0[0, 1] == 0.0


def test_omega_is_zero_under_the_tiny_clamp():
    s = _one_pixel_scene(dz=-1.24, obs_value=0.015)                                      # Z1 = 0.01001: clamped region (Zc <= 0.02)
    _, _, _, terms = rr.normal_eq(**s, want_terms=True)
    assert terms[0]["tiny"].all() and not terms[0]["omega"].any() and not terms[0]["active"].any()      # (and v fails: Z1 < 0.1)


def _frame(fill=1.0):
    return np.full((4, 4), fill, np.float32)


def _sample(obs, ix, iy, tol=0.015625):
    out = {}
    for f in (np.float32, np.float64):
        zo, mode, _ = rr.sample_depth(obs, np.array([ix], f), np.array([iy], f), tol, f)
        out[f] = (float(zo[0]), int(mode[0]))
    assert out[np.float32] == out[np.float64]
    return out[np.float32]


def test_sampling_rule_on_hand_made_frames():
    obs = _frame()
    obs[1, 1], obs[1, 2], obs[2, 1], obs[2, 2] = 1.0, 1.5, 2.0, 2.5
    assert _sample(obs, 1.25, 1.5, tol=2.0) == (0.375 * 1.0 + 0.125 * 1.5 + 0.375 * 2.0 + 0.125 * 2.5, 1)      # plain bilinear, nw ne sw se
    # a hole at one tap: the nearest tap if it is present ...
    for hole in (0.0, -1.0, np.nan, np.inf):
        o = obs.copy()
        o[1, 2] = hole
        assert _sample(o, 1.25, 1.25, tol=2.0) == (1.0, 2)                                 # nearest = (1,1), present
        assert _sample(o, 1.75, 1.25, tol=2.0)[1] == 0                                     # nearest = (2,1) in x,y = the hole itself
    # a step edge: above the tolerance -> nearest, at the tolerance -> bilinear (inclusive)
    o = _frame(1.0)
    o[:, 2:] = 1.0 + 0.015625
    assert _sample(o, 1.25, 1.0) == (1.0 + 0.25 * 0.015625, 1)
    o[:, 2:] = 1.0 + 0.015625 + 2.0 ** -20
    assert _sample(o, 1.25, 1.0) == (1.0, 2) and _sample(o, 1.75, 1.0) == (float(o[1, 2]), 2)
    # ties of the nearest tap go up: floor(ix + 0.5)
    assert _sample(o, 1.5, 1.0) == (float(o[1, 2]), 2)
    # out of frame: taps beyond the border are missing; just inside, the nearest tap still serves
    o = _frame(1.0)
    assert _sample(o, 3.25, 1.0) == (1.0, 2) and _sample(o, -0.25, 1.0) == (1.0, 2)
    assert _sample(o, 3.75, 1.0)[1] == 0 and _sample(o, -0.75, 1.0)[1] == 0 and _sample(o, 1.0, 4.5)[1] == 0
    assert _sample(o, 3.0, 3.0) == (1.0, 2)                                                # the last pixel itself: its east / south taps are outside
    # positions that are no positions
    for bad in (np.nan, np.inf, -np.inf, 1.0e8, -3.0e9):
        assert _sample(o, bad, 1.0)[1] == 0 and _sample(o, 1.0, bad)[1] == 0


def test_gate_is_inclusive_at_representable_boundaries():
    for gap, gate, want in ((0.0625, 0.0625, True), (0.0625 + 2.0 ** -20, 0.0625, False), (0.0625 - 2.0 ** -20, 0.0625, True), (0.0, 0.0, True),
                            (-0.0625, 0.0625, True), (-0.0625 - 2.0 ** -20, 0.0625, False)):
        s = _one_pixel_scene(obs_value=1.25 + gap)                                        # Z1 = fp32(depth + 1e-5): set it to 1.25 exactly
        s["depth"][:] = np.float32(1.25) - np.float32(1e-5)
        for f in (np.float32,):
            _, _, ds, terms = rr.normal_eq(**s, depth_gate=gate, f=f, want_terms=True)
            z1 = terms[0]["X1"][..., 2]
            assert np.all(z1 == np.float32(1.25))                                         # (IEEE single: fp32(1.25 - 1e-5) + fp32(1e-5) == 1.25)
            assert bool(terms[0]["active"].all()) == want and ds[0, 0] == (16 if want else 0), (gap, gate)


def test_invalid_pixels_and_missing_depth_never_enter():
    s = _one_pixel_scene()
    s["depth"][0, 0, 0] = 0.0                                                             # background: v fails
    s["obs_depth"][0, 3, 3] = np.nan
    Hm, bv, ds, terms = rr.normal_eq(**s, want_terms=True)
    assert np.isfinite(Hm).all() and np.isfinite(bv).all() and ds[0, 0] == 14
    assert not terms[0]["active"][0, 0] and not terms[0]["active"][3, 3]
