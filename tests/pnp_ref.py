"""fp64 numpy restatement of the pose initialiser: the descriptor matcher, the P3P RANSAC hypothesis loop with
the library's `rnd` rule, and the Gauss-Newton polish.  Written from the specification (include/rnnpose_hip.h), not from the kernels:
the quartic is solved by numpy's companion-matrix eigenvalues and the pose by Kabsch's SVD, where the kernels use Ferrari's
factorisation and a frame alignment.  tests/test_pnp_ref.py checks this file on its own; the GPU and host tests compare against it."""
from __future__ import annotations

import numpy as np

MIN_Z = 1e-6


# ---- matcher ----------------------------------------------------------------------------------------------------------------------
def roi_pixels(bbox, H, W, step):
    """-> (u, v) int arrays of the box's participating pixels in ascending linear index v W + u (empty arrays for an empty box)."""
    x0, y0, x1, y1 = max(int(bbox[0]), 0), max(int(bbox[1]), 0), min(int(bbox[2]), W - 1), min(int(bbox[3]), H - 1)
    if x1 < x0 or y1 < y0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    vv, uu = np.meshgrid(np.arange(y0, y1 + 1, step), np.arange(x0, x1 + 1, step), indexing="ij")
    return uu.reshape(-1).astype(np.int64), vv.reshape(-1).astype(np.int64)


def similarities(desc3d, desc2d_img, u, v):
    """(P,D) x the pixels (u, v) of one (D,H,W) map -> (P,N) fp64."""
    return np.asarray(desc3d, np.float64) @ np.asarray(desc2d_img, np.float64)[:, v, u]


def match_object(desc3d, points, desc2d_img, bbox, step, min_sim, mutual, pixel_center, M):
    """One object.  -> dict: X, x, sim, point_idx (compacted, at most M rows), count, and the full record S (P,N), u, v, fwd (P), bwd (N)."""
    D, H, W = desc2d_img.shape
    u, v = roi_pixels(bbox, H, W, step)
    P = desc3d.shape[0]
    out = dict(u=u, v=v, S=None, fwd=None, bwd=None, X=np.zeros((0, 3)), x=np.zeros((0, 2)), sim=np.zeros(0), point_idx=np.zeros(0, np.int64),
               count=0, total=0)
    if u.size == 0 or P == 0:
        return out
    S = similarities(desc3d, desc2d_img, u, v)
    fwd = S.argmax(1)                 # numpy's argmax returns the FIRST maximum: the lowest linear pixel index / point index
    bwd = S.argmax(0)
    keep = S[np.arange(P), fwd] >= min_sim
    if mutual:
        keep &= bwd[fwd] == np.arange(P)
    idx = np.nonzero(keep)[0]
    out.update(S=S, fwd=fwd, bwd=bwd, total=int(idx.size))
    idx = idx[:M]
    out.update(X=np.asarray(points, np.float64)[idx], x=np.stack([u[fwd[idx]] + pixel_center, v[fwd[idx]] + pixel_center], 1).astype(np.float64),
               sim=S[idx, fwd[idx]], point_idx=idx, count=int(idx.size))
    return out


def match(desc3d, points, pt_off, desc2d, src_index, bbox, step, min_sim, mutual, pixel_center, M):
    """The batch: a list of match_object records (an index outside [0, S) gives count 0)."""
    res = []
    for b in range(len(src_index)):
        s = int(src_index[b])
        a, e = int(pt_off[b]), int(pt_off[b + 1])
        if not 0 <= s < desc2d.shape[0]:
            res.append(match_object(desc3d[a:a], points[a:a], desc2d[0], bbox[b], step, min_sim, mutual, pixel_center, M))
        else:
            res.append(match_object(desc3d[a:e], points[a:e], desc2d[s], bbox[b], step, min_sim, mutual, pixel_center, M))
    return res


# ---- P3P --------------------------------------------------------------------------------------------------------------------------
def kabsch(P, Q):
    """Proper rotation and translation with Q ~ R P + t (rows are points)."""
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - qc).T @ (P - pc))
    d = np.sign(np.linalg.det(U @ Vt))
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    return R, qc - R @ pc


def p3p(Xw, xn):
    """Xw (3,3) model points, xn (3,2) normalised image points -> list of (R, t): every P3P solution with the three depths > 0.
    Grunert: s2 = u s1, s3 = v s1, u = N(v) / D(v), v a root of a quartic formed with numpy's polynomial arithmetic."""
    Xw, xn = np.asarray(Xw, np.float64), np.asarray(xn, np.float64)
    j = np.concatenate([xn, np.ones((3, 1))], 1)
    j /= np.linalg.norm(j, axis=1, keepdims=True)
    a2, b2, c2 = ((Xw[1] - Xw[2]) ** 2).sum(), ((Xw[0] - Xw[2]) ** 2).sum(), ((Xw[0] - Xw[1]) ** 2).sum()
    n = np.cross(Xw[1] - Xw[0], Xw[2] - Xw[0])
    if not (n @ n > 1e-20 * c2 * b2):
        return []
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    q, cr = (a2 - c2) / b2, c2 / b2
    N = np.poly1d([q - 1.0, -2.0 * q * cb, q + 1.0])
    D = np.poly1d([-2.0 * ca, 2.0 * cg])
    Wp = np.poly1d([1.0, -2.0 * cb, 1.0])
    quartic = D * D + N * N - N * D * float(2.0 * cg) - Wp * D * D * float(cr)      # (poly1d first: a numpy scalar on the left would broadcast)
    sols = []
    for root in np.roots(quartic.coeffs):
        if abs(root.imag) > 1e-6 * (1.0 + abs(root.real)):
            continue
        v = float(root.real)
        if v <= 0 or Wp(v) <= 0 or abs(D(v)) < 1e-12:
            continue
        u = N(v) / D(v)
        if u <= 0:
            continue
        s = np.array([1.0, u, v]) * np.sqrt(b2 / Wp(v))
        for _ in range(4):                                  # Newton on the three distance equations
            f = np.array([s[1] ** 2 + s[2] ** 2 - 2 * s[1] * s[2] * ca - a2, s[0] ** 2 + s[2] ** 2 - 2 * s[0] * s[2] * cb - b2,
                          s[0] ** 2 + s[1] ** 2 - 2 * s[0] * s[1] * cg - c2])
            J = 2.0 * np.array([[0.0, s[1] - s[2] * ca, s[2] - s[1] * ca], [s[0] - s[2] * cb, 0.0, s[2] - s[0] * cb],
                                [s[0] - s[1] * cg, s[1] - s[0] * cg, 0.0]])
            try:
                d = np.linalg.solve(J, f)
            except np.linalg.LinAlgError:
                break
            if not np.all(np.isfinite(d)) or np.any(np.abs(d) > 0.5 * s):
                break
            s = s - d
        if np.any(s <= 0):
            continue
        R, t = kabsch(Xw, s[:, None] * j)
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and np.all((Xw @ R.T + t)[:, 2] > 0):
            sols.append((R, t))
    return sols


# ---- scoring, polish --------------------------------------------------------------------------------------------------------------
def project(R, t, K, X):
    Xc = np.asarray(X, np.float64) @ R.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
    return uv, Xc


def residuals2(R, t, K, X, x):
    """-> r^2 per correspondence, +inf for a point at Z <= 1e-6 (an outlier)."""
    uv, Xc = project(R, t, K, X)
    r2 = ((uv - np.asarray(x, np.float64)) ** 2).sum(1)
    return np.where(Xc[:, 2] > MIN_Z, r2, np.inf)


def score(R, t, K, X, x, tau):
    """-> MSAC cost sum min(r^2, tau^2), inliers #{r^2 < tau^2}, the inlier mask."""
    r2 = residuals2(R, t, K, X, x)
    return float(np.minimum(r2, tau * tau).sum()), int((r2 < tau * tau).sum()), r2 < tau * tau


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """xi = (translation, rotation) -> (E, V v): the SE(3) exponential."""
    v, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.linalg.norm(w)
    Wx = skew(w)
    if th < 1e-8:
        A, B, C = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        A, B, C = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + A * Wx + B * Wx @ Wx, (np.eye(3) + B * Wx + C * Wx @ Wx) @ v


def left_update(xi, R, t):
    E, tv = se3_exp(xi)
    return E @ R, E @ t + tv


def jacobian(R, t, K, X, x):
    """-> r (N,2) = proj(R X + t) - x and J (N,2,6) with respect to a LEFT increment exp(xi), xi = (translation, rotation):
    J = J_proj [I | -[X1]x]."""
    uv, Xc = project(R, t, K, X)
    N = Xc.shape[0]
    iz = 1.0 / Xc[:, 2]
    Jp = np.zeros((N, 2, 3))
    Jp[:, 0, 0], Jp[:, 0, 2] = K[0, 0] * iz, -K[0, 0] * Xc[:, 0] * iz * iz
    Jp[:, 1, 1], Jp[:, 1, 2] = K[1, 1] * iz, -K[1, 1] * Xc[:, 1] * iz * iz
    JT = np.zeros((N, 3, 6))
    JT[:, :, :3] = np.eye(3)
    for i in range(N):
        JT[i, :, 3:] = -skew(Xc[i])
    return uv - np.asarray(x, np.float64), Jp @ JT


def polish(R, t, K, X, x, tau, n_polish, margins=None):
    """n_polish Gauss-Newton steps, the inlier set re-selected with tau before every step -> (R, t), or None (no inlier, a system that
    is not positive definite, a pose that is not finite).  margins: a list that receives the smallest | |r| - tau | of every inlier
    decision taken on the way and of the one the final pose's mask will take (nothing where no residual is finite)."""
    def note(r2):
        if margins is not None and np.isfinite(r2).any():
            margins.append(float(np.abs(np.sqrt(r2[np.isfinite(r2)]) - tau).min()))
        return r2
    for _ in range(n_polish):
        m = note(residuals2(R, t, K, X, x)) < tau * tau
        if not m.any():
            return None
        r, J = jacobian(R, t, K, X[m], x[m])
        J2, r2 = J.reshape(-1, 6), r.reshape(-1)
        H, g = J2.T @ J2, J2.T @ r2
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return None
        if np.any(np.diag(L) ** 2 <= 1e-13 * np.diag(H)):
            return None
        xi = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        R, t = left_update(xi, R, t)
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return None
    note(residuals2(R, t, K, X, x))
    return R, t


def pose_matrix(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def hypotheses(X, x, count, K, rnd, tau, min_count=4):
    """One object: X (M,3), x (M,2), rnd (Hyp,3) uint32; count is clamped to [0, M] as the kernels clamp it.  Hypothesis h samples the
    correspondences rnd[h] % count; its cheapest P3P solution is its candidate.
    -> cost (Hyp), inliers (Hyp), poses (list of (4,4) or None)."""
    Hyp, count = rnd.shape[0], max(0, min(int(count), len(X)))
    X, x, Kd = np.asarray(X, np.float64)[:count], np.asarray(x, np.float64)[:count], np.asarray(K, np.float64)
    cost, inl, poses = np.full(Hyp, np.inf), np.zeros(Hyp, np.int64), [None] * Hyp
    if count < min_count or count < 3:
        return cost, inl, poses
    for h in range(Hyp):
        i = [int(r) % count for r in rnd[h]]
        if len(set(i)) < 3:
            continue
        xn = np.stack([(x[i, 0] - Kd[0, 2]) / Kd[0, 0], (x[i, 1] - Kd[1, 2]) / Kd[1, 1]], 1)
        for R, t in p3p(X[i], xn):
            c, n, _ = score(R, t, Kd, X, x, tau)
            if c < cost[h]:
                cost[h], inl[h], poses[h] = c, n, pose_matrix(R, t)
    return cost, inl, poses


def ransac_object(X, x, count, K, rnd, tau, n_polish, min_count):
    """One object (the arguments of `hypotheses`).  -> dict cost (Hyp), inliers (Hyp), best, T (4,4) or None, inlier_mask (count),
    n_inliers, final_cost, info, and r2_final (the squared residuals under the final pose)."""
    cost, inl, poses = hypotheses(X, x, count, K, rnd, tau, min_count)
    count = max(0, min(int(count), len(X)))
    X, x, Kd = np.asarray(X, np.float64)[:count], np.asarray(x, np.float64)[:count], np.asarray(K, np.float64)
    out = dict(cost=cost, inliers=inl, best=-1, T=None, inlier_mask=np.zeros(count, bool), n_inliers=0, final_cost=np.inf, info=-1, r2_final=None)
    if not np.isfinite(cost).any():
        return out
    best = int(np.argmin(cost))              # the first minimum: the lowest h on a tie
    out["best"] = best
    pose = polish(poses[best][:3, :3], poses[best][:3, 3], Kd, X, x, tau, n_polish)
    if pose is None:
        return out
    c, n, m = score(*pose, Kd, X, x, tau)
    out.update(T=pose_matrix(*pose), inlier_mask=m, n_inliers=n, final_cost=c, info=0, r2_final=residuals2(*pose, Kd, X, x))
    return out


def ransac(X, x, count, K, rnd, tau, n_polish, min_count=4):
    return [ransac_object(X[b], x[b], count[b], K[b], rnd[b], tau, n_polish, min_count) for b in range(len(count))]


def fallback_pose(K, bbox, diameter, size, pixel_center):
    """The box-centre start: rotation = identity, t = K^-1 (box centre, 1) z with z = f diameter / max(box width, box height),
    f = (fx + fy) / 2.  The box [xmin, ymin, xmax, ymax] (inclusive pixels; pixel u covers the ray through u + pixel_center) is clamped
    to the image of `size` = (H, W); an empty box counts as the whole image."""
    K = np.asarray(K, np.float64)
    H, W = size
    x0, y0, x1, y1 = max(int(bbox[0]), 0), max(int(bbox[1]), 0), min(int(bbox[2]), W - 1), min(int(bbox[3]), H - 1)
    if x1 < x0 or y1 < y0:
        x0, y0, x1, y1 = 0, 0, W - 1, H - 1
    centre = np.array([(x0 + x1) / 2.0 + pixel_center, (y0 + y1) / 2.0 + pixel_center, 1.0])
    z = (K[0, 0] + K[1, 1]) / 2.0 * diameter / max(x1 - x0 + 1, y1 - y0 + 1)
    T = np.eye(4)
    T[:3, 3] = np.linalg.inv(K) @ centre * z
    return T


# ---- the P3P test distribution (numpy seed 0) -------------------------------------------------------------------------------------
P3P_K = np.array([[572.4, 0.0, 325.3], [0.0, 572.4, 242.0], [0.0, 0.0, 1.0]])


def p3p_scenes(n_scenes=100, n_triples=200, M=64, seed=0):
    """-> X (n,M,3) fp32, x (n,M,2) fp32 (noise-free projections rounded to fp32 -- the residual of that rounding is part of the data),
    rnd (n,n_triples,3) uint32, poses (n,4,4) fp64: M points uniform in a +-0.1 m cube, R = exp(w), w ~ N(0,1)^3,
    t = (U(-.15,.15), U(-.1,.1), U(.6,1.2))."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.1, 0.1, (n_scenes, M, 3)).astype(np.float32).astype(np.float64)
    w = rng.normal(0.0, 1.0, (n_scenes, 3))
    t = np.stack([rng.uniform(-0.15, 0.15, n_scenes), rng.uniform(-0.1, 0.1, n_scenes), rng.uniform(0.6, 1.2, n_scenes)], 1)
    rnd = rng.integers(0, 2 ** 32, (n_scenes, n_triples, 3), dtype=np.uint64).astype(np.uint32)
    poses = np.tile(np.eye(4), (n_scenes, 1, 1))
    xs = np.zeros((n_scenes, M, 2))
    for s in range(n_scenes):
        R, _ = se3_exp(np.concatenate([np.zeros(3), w[s]]))
        poses[s, :3, :3], poses[s, :3, 3] = R, t[s]
        xs[s] = project(R, t[s], P3P_K, X[s])[0]
    return X.astype(np.float32), xs.astype(np.float32), rnd, poses
