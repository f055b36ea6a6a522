"""numpy restatement of the depth-aware normal equations (include/rnnpose_hip.h: rnnpose_lm_normal_eq_rgbd_f64).

Evaluated in float32 it performs the per-pixel operations of csrc/lm.hip in the kernel's order (IEEE single operations, no contraction),
so every per-pixel value and every decision is the kernel's; evaluated in float64 it is the value both approximate.  The sums are fp64
in both.  Inputs are the fp32 arrays the kernel reads; `target` is absolute, (B,H,W,2) crop pixel-index coordinates.
"""
import numpy as np

MIN_DEPTH_VALID = 0.1
MIN_DEPTH_PROJ = 0.01
EPS_DEPTH = 1e-5


def obs_position(tx, ty, H, W, theta, Ho, Wo, f=np.float32):
    """crop coordinates (tx, ty) -> (ix, iy) in the observed frame; theta (6,)"""
    th = np.asarray(theta, np.float32).reshape(6).astype(f)
    tx, ty = np.asarray(tx).astype(f), np.asarray(ty).astype(f)
    bx = (f(2) * tx + f(1)) / f(W) - f(1)
    by = (f(2) * ty + f(1)) / f(H) - f(1)
    gx = th[0] * bx + th[1] * by + th[2]
    gy = th[3] * bx + th[4] * by + th[5]
    ix = ((gx + f(1)) * f(Wo) - f(1)) * f(0.5)
    iy = ((gy + f(1)) * f(Ho) - f(1)) * f(0.5)
    return ix, iy


def sample_depth(obs, ix, iy, edge_tol, f=np.float32):
    """obs (Ho,Wo) fp32, ix / iy arrays in `f` -> (zo, mode, corner): mode 0 = no depth, 1 = bilinear, 2 = nearest tap; corner = (x0, y0,
    east, south), the decisions that pick the taps."""
    obs = np.asarray(obs, np.float32)
    Ho, Wo = obs.shape
    tol = f(np.float32(edge_tol))
    with np.errstate(invalid="ignore", over="ignore"):
        sane = (np.abs(ix) < f(1.0e8)) & (np.abs(iy) < f(1.0e8))
        fx0, fy0 = np.floor(np.where(sane, ix, f(0))), np.floor(np.where(sane, iy, f(0)))
        x0 = np.where(sane, fx0, -10).astype(np.int64)
        y0 = np.where(sane, fy0, -10).astype(np.int64)
        ixs, iys = np.where(sane, ix, f(0)), np.where(sane, iy, f(0))
        east = np.floor(ixs + f(0.5)) != fx0
        south = np.floor(iys + f(0.5)) != fy0
        z, p = [], []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):                 # nw, ne, sw, se
            xx, yy = x0 + dx, y0 + dy
            inside = (xx >= 0) & (xx < Wo) & (yy >= 0) & (yy < Ho)
            v = obs[np.clip(yy, 0, Ho - 1), np.clip(xx, 0, Wo - 1)]
            p.append(inside & (v > 0) & np.isfinite(v))
            z.append(np.where(p[-1], v, np.float32(1.0)).astype(f))      # (a placeholder where the tap is missing: never used)
        all4 = p[0] & p[1] & p[2] & p[3]
        zmax = np.maximum(np.maximum(z[0], z[1]), np.maximum(z[2], z[3]))
        zmin = np.minimum(np.minimum(z[0], z[1]), np.minimum(z[2], z[3]))
        smooth = all4 & ((zmax - zmin) <= tol)
        fx1, fy1 = fx0 + f(1), fy0 + f(1)
        w00, w10 = (fx1 - ixs) * (fy1 - iys), (ixs - fx0) * (fy1 - iys)
        w01, w11 = (fx1 - ixs) * (iys - fy0), (ixs - fx0) * (iys - fy0)
        zb = f(0) + z[0] * w00
        zb = zb + z[1] * w10
        zb = zb + z[2] * w01
        zb = zb + z[3] * w11
        zn = np.where(south, np.where(east, z[3], z[2]), np.where(east, z[1], z[0]))
        pn = np.where(south, np.where(east, p[3], p[2]), np.where(east, p[1], p[0]))
    mode = np.where(smooth, 1, np.where(pn, 2, 0))
    zo = np.where(smooth, zb, zn).astype(f)
    return zo, mode, (x0, y0, east, south)


def pixel_terms(target, depth, K, G, obs, theta, K_obs, depth_weight, depth_gate, edge_tol, f=np.float32):
    """One image: target (H,W,2), depth (H,W), K, K_obs (3,3), G (4,4), obs (Ho,Wo), theta (2,3) -> dict of per-pixel arrays in `f`
    (J0, J1 (H,W,6), r2 (H,W,2), X1 (H,W,3), Yp (H,W,3), omega) and the decisions (valid, tiny, mode, corner, active)."""
    H, W = depth.shape
    K, G, K_obs = (np.asarray(a, np.float32).astype(f) for a in (K, G, K_obs))
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = xs.astype(f), ys.astype(f)
    tx, ty = np.asarray(target, np.float32)[..., 0].astype(f), np.asarray(target, np.float32)[..., 1].astype(f)
    with np.errstate(all="ignore"):
        Z0 = np.asarray(depth, np.float32).astype(f) + f(np.float32(EPS_DEPTH))
        X0 = Z0 * (x - cx) / fx
        Y0 = Z0 * (y - cy) / fy
        X1 = G[0, 0] * X0 + G[0, 1] * Y0 + G[0, 2] * Z0 + G[0, 3]
        Y1 = G[1, 0] * X0 + G[1, 1] * Y0 + G[1, 2] * Z0 + G[1, 3]
        Z1 = G[2, 0] * X0 + G[2, 1] * Y0 + G[2, 2] * Z0 + G[2, 3]
        Zc = np.maximum(Z1, f(np.float32(MIN_DEPTH_PROJ)))
        u = fx * (X1 / Zc) + cx
        v = fy * (Y1 / Zc) + cy
        valid = (Z0 > f(np.float32(MIN_DEPTH_VALID))) & (Z1 > f(np.float32(MIN_DEPTH_VALID)))
        tiny = Zc <= f(np.float32(MIN_DEPTH_PROJ)) + f(np.float32(0.01))
        zi1 = np.where(tiny, f(0), f(1) / Zc)
        zi2 = np.where(tiny, f(0), f(1) / (Zc * Zc))
        a, c = fx * zi1, -fx * X1 * zi2
        d, e = fy * zi1, -fy * Y1 * zi2
        D = np.float64
        a, c, d, e, X, Y, Z = (q.astype(D) for q in (a, c, d, e, X1, Y1, Z1))
        zero = np.zeros_like(a)
        J0 = np.stack([a, zero, c, c * Y, a * Z + c * (-X), a * (-Y)], -1)
        J1 = np.stack([zero, d, e, d * (-Z) + e * Y, e * (-X), d * X], -1)
        r2 = np.stack([tx.astype(D) - u.astype(D), ty.astype(D) - v.astype(D)], -1)
        # the depth term
        Ho, Wo = obs.shape
        ix, iy = obs_position(tx, ty, H, W, theta, Ho, Wo, f)
        zo, mode, corner = sample_depth(obs, ix, iy, edge_tol, f)
        Yx = zo * (ix - K_obs[0, 2]) / K_obs[0, 0]
        Yy = zo * (iy - K_obs[1, 2]) / K_obs[1, 1]
        gap = np.abs(zo - Z1)
        active = (mode > 0) & valid & (gap <= f(np.float32(depth_gate)))
        omega = f(np.float32(depth_weight)) * (fx * fy) * zi2
    return dict(J0=J0, J1=J1, r2=r2, X1=np.stack([X1, Y1, Z1], -1), Yp=np.stack([Yx, Yy, zo], -1), omega=omega, valid=valid, tiny=tiny,
                mode=mode, corner=corner, active=active, gap=gap, ix=ix, iy=iy, zo=zo)


def jt_matrix(X):
    """J_T = [I | -[X]x] of one point (3,) -> (3,6) fp64"""
    X, Y, Z = (float(q) for q in X)
    return np.array([[1, 0, 0, 0, Z, -Y], [0, 1, 0, -Z, 0, X], [0, 0, 1, Y, -X, 0]], np.float64)


def normal_eq(target, weight, depth, K, G, obs_depth, src_index, theta, K_obs, depth_weight=1.0, depth_gate=0.05, edge_tol=0.02,
              f=np.float32, want_terms=False):
    """target (B,H,W,2), weight (B,H,W), depth (B,1,H,W) or (B,H,W), K / K_obs (B,3,3), G (B,4,4) or (B,1,4,4), obs_depth (S,Ho,Wo),
    src_index B integers or None, theta (B,2,3) -> Hm (B,6,6), bv (B,6), dstats (B,2) fp64 [, list of pixel_terms]."""
    target, weight, depth = (np.asarray(a, np.float32) for a in (target, weight, depth))
    B = weight.shape[0]
    depth = depth.reshape(B, depth.shape[-2], depth.shape[-1])
    G = np.asarray(G, np.float32).reshape(B, 4, 4)
    Hm, bv, ds, terms = np.zeros((B, 6, 6)), np.zeros((B, 6)), np.zeros((B, 2)), []
    for b in range(B):
        s = b if src_index is None else int(src_index[b])
        t = pixel_terms(target[b], depth[b], K[b], G[b], np.asarray(obs_depth, np.float32)[s], theta[b], K_obs[b], depth_weight,
                        depth_gate, edge_tol, f)
        vw = np.where(t["valid"], weight[b].astype(np.float64), 0.0)
        with np.errstate(all="ignore"):
            Hm[b] = np.einsum("hw,hwi,hwj->ij", vw, t["J0"], t["J0"]) + np.einsum("hw,hwi,hwj->ij", vw, t["J1"], t["J1"])
            bv[b] = np.einsum("hw,hwi,hw->i", vw, t["J0"], t["r2"][..., 0]) + np.einsum("hw,hwi,hw->i", vw, t["J1"], t["r2"][..., 1])
            s3 = vw * t["omega"].astype(np.float64)
            on = t["active"] & (s3 != 0.0)
            X = t["X1"].astype(np.float64)[on]                          # (n,3): only the active pixels enter (a missing measurement adds nothing)
            r3 = t["Yp"].astype(np.float64)[on] - X
            sw = s3[on]
            n = X.shape[0]
            JT = np.zeros((n, 3, 6))
            JT[:, 0, 0] = JT[:, 1, 1] = JT[:, 2, 2] = 1.0
            JT[:, 0, 4], JT[:, 0, 5] = X[:, 2], -X[:, 1]
            JT[:, 1, 3], JT[:, 1, 5] = -X[:, 2], X[:, 0]
            JT[:, 2, 3], JT[:, 2, 4] = X[:, 1], -X[:, 0]
            Hm[b] += np.einsum("n,nki,nkj->ij", sw, JT, JT)
            bv[b] += np.einsum("n,nki,nk->i", sw, JT, r3)
            ds[b] = [float(t["active"].sum()), float((sw * (r3 * r3).sum(-1)).sum())]
        terms.append(t)
    return (Hm, bv, ds, terms) if want_terms else (Hm, bv, ds)


def decisions(terms):
    """the discrete decisions of every image, for the fp32 == fp64 precondition of the GPU tests"""
    return [(t["valid"], t["tiny"], t["mode"], t["corner"][0], t["corner"][1], t["corner"][2], t["corner"][3], t["active"]) for t in terms]
