"""fp64 numpy restatement of the object onboarding kernels (csrc/model_prep.cuh), written from their contract in
include/rnnpose_hip.h: the same association d2 = (dx dx + dy dy) + dz dz on values converted from fp32, the same tie rules (diameter:
the lowest i, then the lowest j; FPS: the lowest index) and the same rule for points that are not finite (they take part in nothing).
numpy has no fma contraction, so the bits are the kernels' bits."""
import numpy as np


def _finite(p):
    return np.isfinite(p).all(1)


def _d2(a, b):
    """a (...,3), b (...,3) fp64 -> squared distances in the kernels' association"""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def diameter(points):
    """points (P,3) fp32 -> d2 (fp64), diameter (fp64), pair (i, j), bounds (2,3) fp32"""
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    ok = _finite(p32)
    keep = np.nonzero(ok)[0]
    bounds = np.stack([np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)])
    if keep.size:
        bounds = np.stack([p32[keep].min(0), p32[keep].max(0)])
    if keep.size < 2:
        return 0.0, 0.0, (-1, -1), bounds
    p = p32[keep].astype(np.float64)
    best, pair = -1.0, (-1, -1)
    for a in range(len(p) - 1):                         # ascending i; strict >: the lowest i, and argmax's first maximum the lowest j
        d = _d2(p[a], p[a + 1:])
        j = int(np.argmax(d))
        if d[j] > best:
            best, pair = float(d[j]), (int(keep[a]), int(keep[a + 1 + j]))
    return best, float(np.sqrt(best)), pair, bounds


def fps(points, n, start=-1, want_margin=False):
    """points (P,3) fp32 -> idx (n) int32, dist2 (n) fp64 [, the smallest relative margin between the best and the runner-up running
    distance over the picks that had a runner-up]"""
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    P = p32.shape[0]
    idx, dist2 = np.full(n, -1, np.int32), np.full(n, -1.0, np.float64)
    margin = np.inf
    if start < -1 or start >= P:
        return (idx, dist2, margin) if want_margin else (idx, dist2)
    ok = _finite(p32)
    p = np.where(ok[:, None], p32, 0).astype(np.float64)
    run = np.where(ok, _d2(p, np.zeros(3)) if start < 0 else np.inf, -2.0)
    for k in range(n):
        if k == 0 and start >= 0:
            pick = start if run[start] >= 0 else -1
        else:
            cand = run >= 0
            pick = int(np.argmax(np.where(cand, run, -3.0))) if cand.any() else -1      # (argmax: the first maximum = the lowest index)
            if want_margin and pick >= 0 and cand.sum() > 1:
                top = np.sort(run[cand])[-2:]
                if top[1] > 0 and np.isfinite(top[1]):
                    margin = min(margin, (top[1] - top[0]) / top[1])
        if pick < 0:
            break
        idx[k], dist2[k] = pick, run[pick]
        upd = run >= 0
        run[upd] = np.minimum(run[upd], _d2(p[upd], p[pick]))
        run[pick] = -1.0
    return (idx, dist2, margin) if want_margin else (idx, dist2)


def fragments(verts, n):
    """fragmentation_fps restated: the picks by `fps` from the origin, every vertex to its nearest centre (fp64, the first minimum)
    -> centers (n,3) fp32, center_inds (n), vert_frag_ids (P)"""
    v = np.asarray(verts, np.float32)
    idx, _ = fps(v, n, -1)
    c = v[idx].astype(np.float64)
    ids = np.array([int(np.argmin(_d2(c, q))) for q in v.astype(np.float64)], np.int64)
    return v[idx], idx, ids
