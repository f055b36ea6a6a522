"""numpy restatement of the grouped (multi-view) LM step (include/rnnpose_hip.h: rnnpose_lm_step_views_io_f32).

Views of one object form a group; view v has the camera-from-rig transform E_v = (R, t).  A rig-frame left increment delta (translation
first) acts in view v as xi_v = Ad(E_v) delta with Ad(E) = [[R, [t]x R], [0, R]].  Group system Hg = sum_v Ad_v^T Hm_v Ad_v,
bg = sum_v Ad_v^T bv_v over the views in ascending order; the damped solve of the ungrouped step; G_v <- (E_v exp(delta) E_v^-1) G_v.
Everything is fp64 here.  The per-view systems are those of tests/rgbd_ref.normal_eq (the depth term on or off).
"""
import numpy as np

import rgbd_ref as rr


def skew(t):
    t = np.asarray(t, np.float64)
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def adjoint(E):
    """E (4,4) -> Ad(E) (6,6) fp64, twist order (translation, rotation)"""
    E = np.asarray(E, np.float64)
    R, t = E[:3, :3], E[:3, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = R
    Ad[:3, 3:] = skew(t) @ R
    Ad[3:, 3:] = R
    return Ad


def group_system(Hm, bv, E, group_start, absolute=False):
    """Hm (B,6,6), bv (B,6), E (B,4,4), group_start (n_groups + 1) -> Hg (n_groups,6,6), bg (n_groups,6) fp64.
    absolute: the same sums over |Ad|, |Hm|, |bv| (the scale of the rounding bound)."""
    Hm, bv, E = np.asarray(Hm, np.float64), np.asarray(bv, np.float64), np.asarray(E, np.float64)
    ng = len(group_start) - 1
    Hg, bg = np.zeros((ng, 6, 6)), np.zeros((ng, 6))
    for g in range(ng):
        for v in range(int(group_start[g]), int(group_start[g + 1])):
            Ad = adjoint(E[v])
            if absolute:
                Hg[g] += np.abs(Ad).T @ np.abs(Hm[v]) @ np.abs(Ad)
                bg[g] += np.abs(Ad).T @ np.abs(bv[v])
            else:
                Hg[g] += Ad.T @ Hm[v] @ Ad
                bg[g] += Ad.T @ bv[v]
    return Hg, bg


def se3_exp(xi):
    """xi (6,) (translation, rotation) -> (4,4) fp64, closed form with series near zero"""
    xi = np.asarray(xi, np.float64)
    v, w = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    W = skew(w)
    if th < 1e-6:
        A, Bc, Cc = 1.0 - th * th / 6, 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        A, Bc, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + A * W + Bc * W @ W
    out[:3, 3] = (np.eye(3) + Bc * W + Cc * W @ W) @ v
    return out


def rigid_inverse(E):
    E = np.asarray(E, np.float64)
    out = np.eye(4)
    out[:3, :3] = E[:3, :3].T
    out[:3, 3] = -E[:3, :3].T @ E[:3, 3]
    return out


def solve(Hg, bg, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    """the damped solve of every LM step, fp64 -> xi (n_groups,6), info (n_groups,) (0, or the order of the first non-positive minor)"""
    Hg, bg = np.asarray(Hg, np.float64), np.asarray(bg, np.float64)
    xi, info = np.zeros((len(Hg), 6)), np.zeros(len(Hg), np.int64)
    for g in range(len(Hg)):
        Hd = Hg[g] + ep_lambda * np.eye(6) + lm_lambda * np.diag(np.diag(Hg[g]))
        for k in range(1, 7):
            if not np.linalg.det(Hd[:k, :k]) > 0 and info[g] == 0:
                info[g] = k
        if info[g] == 0 and np.isfinite(Hd).all() and np.isfinite(bg[g]).all():
            x = np.linalg.solve(Hd, bg[g])
            xi[g] = np.clip(np.where(np.isnan(x), 0.0, x), -max_update, max_update)
    return xi, info


def apply_increment(G, E, xi, group_start=None):
    """G (B,4,4), E (B,4,4), xi (n_groups,6) [or (B,6) without group_start] -> (E_v exp(xi_g) E_v^-1) G_v, fp64"""
    G, E, xi = np.asarray(G, np.float64).reshape(-1, 4, 4), np.asarray(E, np.float64).reshape(-1, 4, 4), np.asarray(xi, np.float64)
    B = len(G)
    group_start = list(range(B + 1)) if group_start is None else [int(v) for v in group_start]
    out = np.zeros_like(G)
    for g in range(len(group_start) - 1):
        D = se3_exp(xi[g])
        for v in range(group_start[g], group_start[g + 1]):
            out[v] = E[v] @ D @ rigid_inverse(E[v]) @ G[v]
    return out


def view_systems(target, weight, depth, K, G, rgbd=None, f=np.float64):
    """The per-view undamped systems: rgbd_ref.normal_eq with the depth term on (rgbd = dict(obs_depth, src_index, theta, K_obs,
    depth_weight, depth_gate, edge_tol)) or off (None: an empty observed frame) -> Hm (B,6,6), bv (B,6)."""
    B = np.asarray(weight).shape[0]
    if rgbd is None:
        rgbd = dict(obs_depth=np.zeros((B, 2, 2), np.float32), src_index=None, theta=np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (B, 1, 1)),
                    K_obs=np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)), depth_weight=0.0)
    Hm, bv, _ = rr.normal_eq(target, weight, depth, K, G, f=f, **rgbd)
    return Hm, bv
