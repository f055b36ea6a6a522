"""fp64 numpy restatement of the pose confidence (include/rnnpose_hip.h: rnnpose_pose_score_f64): the per-pixel
classification, the ten statistics and the score.  Written from the definitions, vectorised over a window, sums by numpy's pairwise
np.sum -- an order of its own, so the kernel's sums are held to it by a rounding bound and its counts exactly."""
import numpy as np

COLUMNS = ("n_rend", "n_out", "n_occ", "n_cons", "n_viol", "n_hole", "n_desc", "sum_cos", "sum_abs_dd", "n_bad")
NORM_EPS = 1e-12


def classify(rend_depth, rend_desc, window, desc2d, depth_obs, s, tol):
    """One pose.  rend_depth (h,w), rend_desc (D,h,w), window (x0, y0), desc2d (S,D,H,W), depth_obs (S,H,W) or None, s its frame.
    -> dict of (h,w) boolean masks rend / out / occ / cons / viol / hole / desc / bad and fp64 maps cos (0 off `desc`), add (|dd|, 0 off
    `cons`)."""
    z = np.asarray(rend_depth, np.float64)
    a = np.asarray(rend_desc, np.float64)
    h, w = z.shape
    S, D, H, W = desc2d.shape
    none = np.zeros((h, w), bool)
    m = dict(rend=none.copy(), out=none.copy(), occ=none.copy(), cons=none.copy(), viol=none.copy(), hole=none.copy(), desc=none.copy(),
             bad=none.copy(), cos=np.zeros((h, w)), add=np.zeros((h, w)))
    if not 0 <= s < S:
        return m
    with np.errstate(invalid="ignore"):
        m["rend"] = np.isfinite(z) & (z > 0)
    y, x = np.mgrid[0:h, 0:w]
    u, v = x + int(window[0]), y + int(window[1])
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    m["out"] = m["rend"] & ~inside
    live = m["rend"] & inside
    uc, vc = np.clip(u, 0, W - 1), np.clip(v, 0, H - 1)
    if depth_obs is None:
        m["hole"] = live.copy()
    else:
        d = np.asarray(depth_obs[s], np.float64)[vc, uc]
        with np.errstate(invalid="ignore"):
            valid = np.isfinite(d) & (d > 0)
            dd = np.where(valid & live, d - np.where(m["rend"], z, 0.0), 0.0)
        m["occ"] = live & valid & (dd < -tol)
        m["cons"] = live & valid & (np.abs(dd) <= tol)
        m["viol"] = live & valid & (dd > tol)
        m["hole"] = live & ~valid
        m["add"] = np.where(m["cons"], np.abs(dd), 0.0)
    cmp = live & ~m["occ"]
    g = np.asarray(desc2d[s], np.float64)[:, vc, uc]                       # (D,h,w)
    fin = np.isfinite(a).all(0) & np.isfinite(g).all(0)
    m["bad"] = cmp & ~fin
    m["desc"] = cmp & fin
    a0, g0 = np.where(m["desc"][None], a, 0.0), np.where(m["desc"][None], g, 0.0)
    dot = np.sum(a0 * g0, 0)
    na, ng = np.sqrt(np.sum(a0 * a0, 0)), np.sqrt(np.sum(g0 * g0, 0))
    m["cos"] = np.where(m["desc"], dot / (np.maximum(na, NORM_EPS) * np.maximum(ng, NORM_EPS)), 0.0)
    return m


def score_of(stats):
    """The score of one statistics row."""
    st = dict(zip(COLUMNS, stats))
    if not st["n_desc"] > 0:
        return 0.0
    den = st["n_cons"] + st["n_viol"]
    return max(st["sum_cos"] / st["n_desc"], 0.0) * (st["n_cons"] / den if den > 0 else 1.0)


def pose_score(rend_depth, rend_desc, window, desc2d, depth_obs, src_index, tol):
    """rend_depth (B,h,w), rend_desc (B,D,h,w), window (B,2), desc2d (S,D,H,W), depth_obs (S,H,W) or None, src_index (B)
    -> stats (B,10) fp64, score (B) fp64."""
    B = len(src_index)
    stats, score = np.zeros((B, len(COLUMNS))), np.zeros(B)
    for b in range(B):
        m = classify(rend_depth[b], rend_desc[b], window[b], desc2d, depth_obs, int(src_index[b]), float(tol))
        stats[b] = [np.sum(m[k]) for k in ("rend", "out", "occ", "cons", "viol", "hole", "desc")] + [np.sum(m["cos"]), np.sum(m["add"]), np.sum(m["bad"])]
        score[b] = score_of(stats[b])
    return stats, score
