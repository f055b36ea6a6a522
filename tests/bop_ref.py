"""The BOP pose-error functions -- VSD, MSSD, MSPD -- and their recalls restated in fp64 numpy from the definitions in
include/rnnpose_hip.h: the yardstick of tests/test_gpu_bop.py.  tests/test_bop_ref.py ties it to closed forms.  The reference has no
code for these metrics and bop_toolkit is absent: parity with the toolkit is unpinned.

Conventions: every input is taken as given (the tests pass fp32 arrays) and converted to fp64 first; a pose is (3,4) [R|t]; K is
(3,3) row-major, proj(X) = (fx X/Z + cx, fy Y/Z + cy)."""
import numpy as np

TAUS = (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5)
THETAS = TAUS
THETAS_PX = (5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 45.0, 50.0)
DELTA = 0.015


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _k(K, B):
    K = _f64(K)
    return np.broadcast_to(K, (B, 3, 3)) if K.ndim == 2 else K


def _apply(T, x):
    """T (3,4), x (P,3) -> (P,3)"""
    return x @ T[:, :3].T + T[:, 3]


def _proj(K, X):
    return np.stack([K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2], K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]], 1)


def sym_dist_all(model, sym, pose_est, pose_gt, K):
    """-> (B,S,2): per symmetry, the max over the model points of the 3-D distance and of the distance of the projections."""
    model, sym, pe, pg = _f64(model), _f64(sym), _f64(pose_est), _f64(pose_gt)
    B, S = pe.shape[0], sym.shape[0]
    K = _k(K, B)
    out = np.empty((B, S, 2))
    for b in range(B):
        xe = _apply(pe[b], model)
        ue = _proj(K[b], xe)
        for s in range(S):
            Tgs = np.concatenate([pg[b][:, :3] @ sym[s][:, :3], (pg[b][:, :3] @ sym[s][:, 3] + pg[b][:, 3])[:, None]], 1)
            xg = _apply(Tgs, model)
            out[b, s, 0] = np.sqrt(((xe - xg) ** 2).sum(1)).max()
            out[b, s, 1] = np.sqrt(((ue - _proj(K[b], xg)) ** 2).sum(1)).max()
    return out


def sym_dist(model, sym, pose_est, pose_gt, K):
    """-> (B,2) [MSSD, MSPD]: min over the symmetries of sym_dist_all."""
    return sym_dist_all(model, sym, pose_est, pose_gt, K).min(1)


def vsd(depth_est, depth_gt, depth_obs, src_index, K, diameter, delta, taus):
    """depth_est / depth_gt (B,H,W), depth_obs (S,H,W), src_index (B) ints, K (3,3) or (B,3,3), diameter a number or (B), delta,
    taus (NT) -> err (B,NT) fp64, counts (B,2+NT) int64 [#union, #inter, n_tau...], near: how many comparisons (a pixel against
    delta, an inter pixel against a tau) have their value within a relative 1e-9 of the threshold -- where the last bits of the
    arithmetic could decide."""
    de, dg, dobs = _f64(depth_est), _f64(depth_gt), _f64(depth_obs)
    B, H, W = de.shape
    K = _k(K, B)
    diam = np.broadcast_to(_f64(diameter).reshape(-1), (B,))
    taus = [float(t) for t in taus]
    NT = len(taus)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    err, counts, near = np.empty((B, NT)), np.zeros((B, 2 + NT), np.int64), 0
    for b in range(B):
        fx, fy, cx, cy = K[b, 0, 0], K[b, 1, 1], K[b, 0, 2], K[b, 1, 2]
        ray = np.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1.0)
        o = dobs[int(src_index[b])]
        with np.errstate(invalid="ignore", over="ignore"):
            empty_e, empty_g = ~(de[b] > 0), ~(dg[b] > 0)
            missing = ~(o > 0) | ~np.isfinite(o)
            dist_e, dist_g, dist_o = de[b] * ray, dg[b] * ray, o * ray
            ce, cg = dist_e - dist_o, dist_g - dist_o
            vis_g = ~empty_g & (missing | (cg <= delta))
            vis_e = (~empty_e & (missing | (ce <= delta))) | (vis_g & ~empty_e)
            inter, union = vis_g & vis_e, vis_g | vis_e
            e = np.abs(dist_g - dist_e)
            if diam[b] > 0:
                e = e / diam[b]
            for c, em in ((ce, empty_e), (cg, empty_g)):
                near += int((~em & ~missing & (np.abs(c - delta) <= 1e-9 * abs(delta))).sum())
            counts[b, 0], counts[b, 1] = union.sum(), inter.sum()
            for t, tau in enumerate(taus):
                counts[b, 2 + t] = (inter & (e >= tau)).sum()
                near += int((inter & (np.abs(e - tau) <= 1e-9 * abs(tau))).sum())
        nu, ni = int(counts[b, 0]), int(counts[b, 1])
        for t in range(NT):
            err[b, t] = 1.0 if nu == 0 else float(int(counts[b, 2 + t]) + nu - ni) / float(nu)
    return err, counts, near


def recalls(vsd_err, mssd, mspd, diameters, width, vsd_thetas=THETAS, mssd_thetas=THETAS, mspd_thetas=THETAS_PX):
    """-> (B,3) [AR_VSD, AR_MSSD, AR_MSPD], counted one comparison at a time."""
    vsd_err = _f64(vsd_err)
    B = vsd_err.shape[0]
    d = np.broadcast_to(_f64(diameters).reshape(-1), (B,))
    out = np.zeros((B, 3))
    for b in range(B):
        hits = [float(x) < float(th) for x in vsd_err[b].reshape(-1) for th in vsd_thetas]
        out[b, 0] = sum(hits) / len(hits)
        out[b, 1] = sum(float(mssd[b]) < float(th) * d[b] for th in mssd_thetas) / len(mssd_thetas)
        out[b, 2] = sum(float(mspd[b]) < float(th) * (float(width) / 640.0) for th in mspd_thetas) / len(mspd_thetas)
    return out
