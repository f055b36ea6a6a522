"""The fp64 restatement of the grouped (multi-view) LM step, tests/views_ref.py, against first principles (CPU):
the group system is the Gauss-Newton system of the stacked re-projections differentiated numerically with respect to a rig-frame
increment, and the adjoint identity exp(Ad(E) delta) = E exp(delta) E^-1 that the pose update rests on."""
import numpy as np

import views_ref as vr

H, W = 12, 16


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return vr.se3_exp(np.concatenate([np.zeros(3), a * np.deg2rad(deg)]))[:3, :3]


def _rig():
    """five views: a group of three cameras (0, +80, -40 degrees about axes near y, up to 1 m apart) and a group of two"""
    E = np.tile(np.eye(4), (5, 1, 1))
    for v, (axis, deg, t) in enumerate([((0, 1, 0), 0.0, (0, 0, 0)), ((0.1, 1, 0), 80.0, (-1.0, 0.05, 0.7)), ((0, 1, 0.2), -40.0, (0.6, -0.1, 0.3)),
                                        ((1, 0, 0), 25.0, (0.0, 0.4, 0.1)), ((0, 0, 1), -60.0, (0.2, 0.0, -0.05))]):
        E[v, :3, :3] = _rot(axis, deg)
        E[v, :3, 3] = t
    return E, [0, 3, 5]                                                 # (fp64: rigid to rounding, as the identity needs)


def _scene(seed=0):
    rng = np.random.default_rng(seed)
    B = 5
    depth = (1.0 + 0.3 * rng.random((B, 1, H, W))).astype(np.float32)               # all depths in [1, 1.3]: no validity mask flips
    K = np.tile(np.array([[20.0, 0, 7.6], [0, 21.0, 5.7], [0, 0, 1]], np.float32), (B, 1, 1))
    G = np.stack([vr.se3_exp(0.02 * rng.standard_normal(6)) for _ in range(B)]).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    target = (np.stack([xs, ys], -1)[None] + rng.uniform(-2, 2, (B, H, W, 2))).astype(np.float32)
    weight = rng.random((B, H, W)).astype(np.float32)
    return target, weight, depth, K, G


def _reproject(depth, K, Gv):
    """(H,W,2) re-projections of one view under the relative pose Gv, fp64, the unclamped form of rgbd_ref.pixel_terms"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    K = K.astype(np.float64)
    Z0 = depth.astype(np.float64) + np.float64(np.float32(1e-5))
    P0 = np.stack([Z0 * (xs - K[0, 2]) / K[0, 0], Z0 * (ys - K[1, 2]) / K[1, 1], Z0], -1)
    P1 = P0 @ Gv[:3, :3].T + Gv[:3, 3]
    assert P1[..., 2].min() > 0.5
    return np.stack([K[0, 0] * P1[..., 0] / P1[..., 2] + K[0, 2], K[1, 1] * P1[..., 1] / P1[..., 2] + K[1, 2]], -1)


def test_group_system_is_the_gauss_newton_system_of_the_stacked_reprojections():
    target, weight, depth, K, G = _scene()
    E, starts = _rig()
    Hm, bv = vr.view_systems(target, weight, depth, K, G)
    Hg, bg = vr.group_system(Hm, bv, E, starts)
    h = 1e-6
    for g in range(len(starts) - 1):
        views = range(starts[g], starts[g + 1])

        def stacked(delta):
            out = []
            for v in views:
                Ev = E[v]
                Gv = Ev @ vr.se3_exp(delta) @ vr.rigid_inverse(Ev) @ G[v].astype(np.float64)
                out.append(_reproject(depth[v, 0], K[v], Gv).reshape(-1))
            return np.concatenate(out)
        J = np.stack([(stacked(h * np.eye(6)[k]) - stacked(-h * np.eye(6)[k])) / (2 * h) for k in range(6)], -1)      # (n, 6)
        w = np.concatenate([np.repeat(weight[v].astype(np.float64).reshape(-1), 2) for v in views])
        r = np.concatenate([target[v].astype(np.float64).reshape(-1) for v in views]) - stacked(np.zeros(6))
        wantH, wantb = J.T @ (w[:, None] * J), J.T @ (w * r)
        eH, eb = np.abs(Hg[g] - wantH).max(), np.abs(bg[g] - wantb).max()
        print(f"group {g}: |Hg - J^T W J| {eH:.3e} of {np.abs(wantH).max():.3e}; |bg - J^T W r| {eb:.3e} of {np.abs(wantb).max():.3e}")
        assert eH <= 1e-6 * np.abs(wantH).max() and eb <= 1e-6 * np.abs(wantb).max()
    # a wrong adjoint (the transpose convention) is far outside the tolerance
    bad, _ = vr.group_system(Hm, bv, np.stack([vr.rigid_inverse(e) for e in E]), starts)
    assert np.abs(bad[0] - Hg[0]).max() > 1e-2 * np.abs(Hg[0]).max()


def test_adjoint_identity():
    rng = np.random.default_rng(1)
    E, _ = _rig()
    for e in E:
        for scale in (1e-8, 1e-3, 0.06, 1.0):
            delta = scale * rng.standard_normal(6)
            lhs, rhs = vr.se3_exp(vr.adjoint(e) @ delta), e @ vr.se3_exp(delta) @ vr.rigid_inverse(e)
            assert np.abs(lhs - rhs).max() <= 1e-12, (scale, np.abs(lhs - rhs).max())


def test_solve_and_increment_restatements():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((2, 12, 6))
    Hg, bg = 50.0 * np.einsum("bki,bkj->bij", A, A), rng.standard_normal((2, 6))
    xi, info = vr.solve(Hg, bg)
    for g in range(2):
        Hd = Hg[g] + 100.0 * np.eye(6) + 1e-4 * np.diag(np.diag(Hg[g]))
        assert np.abs(Hd @ xi[g] - bg[g]).max() < 1e-10 and info[g] == 0
    _, info = vr.solve(-Hg - 200.0 * np.eye(6), bg)
    assert (info == 1).all()
    E, starts = _rig()
    G = np.tile(np.eye(4), (5, 1, 1))
    out = vr.apply_increment(G, E, xi, starts)
    for v in range(5):
        assert np.abs(out[v] - vr.se3_exp(vr.adjoint(E[v]) @ xi[0 if v < 3 else 1])).max() < 1e-6
