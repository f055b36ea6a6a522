"""fp64 numpy restatement of the top-K distinct RANSAC hypotheses, on top of tests/pnp_ref.py: the extent and
the corner distance, the greedy selection, the per-slot polish and dup_of.  Written from the specification (include/rnnpose_hip.h).

The selection takes the hypotheses' costs, inlier counts and candidate poses as ARGUMENTS, so a GPU test can hand it the device's
cost array (held to this file's at 1e-6 relative by an assertion of its own): near-ties in cost then cannot reorder the comparison.
It walks the hypotheses once in ascending (cost, h) and records every distance it DECIDES on; the smallest |d - sep| of those is
returned, so that a test can first assert that no decision is close enough to the threshold for rounding to flip it.
tests/test_pnp_topk_ref.py checks this file on its own."""
from __future__ import annotations

import numpy as np

import pnp_ref as pr
from pnp_ref import hypotheses, pose_matrix          # (this module's users reach them here)


def extent(X, count):
    """-> lo (3), hi (3), diag of the first `count` points (count 0: an empty box, diag = inf)."""
    P = np.asarray(X, np.float64)[:max(int(count), 0)]
    if P.shape[0] == 0:
        return np.full(3, np.inf), np.full(3, -np.inf), np.inf
    lo, hi = P.min(0), P.max(0)
    return lo, hi, float(np.linalg.norm(hi - lo))


def corners(lo, hi):
    return np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]] for c in range(8)], np.float64)


def distance(P, Q, lo, hi):
    """max over the 8 corners c of [lo, hi] of |P c - Q c|; P, Q: (4,4) or (3,4) matrices.  NaN when any corner's displacement is."""
    P, Q, C = np.asarray(P, np.float64), np.asarray(Q, np.float64), corners(lo, hi)
    a, b = C @ P[:3, :3].T + P[:3, 3], C @ Q[:3, :3].T + Q[:3, 3]
    return float(np.max(np.sqrt(((a - b) ** 2).sum(1))))


def select(cost, inliers, poses, lo, hi, sep, Kt, min_inliers=0):
    """The greedy rule.  Slot 0: the cheapest hypothesis (cost < inf; the lowest h on a tie).  Slot k >= 1: the cheapest remaining one
    (lowest h on a tie) with a finite cost, inliers >= min_inliers and distance > sep to the candidate pose of EVERY earlier slot.
    -> (hyp: list of at most Kt hypothesis indices, margin: the smallest |d - sep| over every distance decided on, inf if none)."""
    cost = np.asarray(cost, np.float64)
    order = np.lexsort((np.arange(len(cost)), cost))          # ascending cost, ascending h within equal costs (NaN last)
    chosen, margin = [], np.inf
    for h in order:
        if len(chosen) >= Kt:
            break
        h = int(h)
        if not cost[h] < np.inf or poses[h] is None:
            continue
        if chosen:
            if not np.isfinite(cost[h]) or inliers[h] < min_inliers:
                continue
            d = np.array([distance(poses[h], poses[j], lo, hi) for j in chosen])
            with np.errstate(invalid="ignore"):
                margin = min(margin, float(np.nanmin(np.abs(d - sep)))) if np.isfinite(d).any() else margin
                if not np.all(d > sep):
                    continue
        chosen.append(h)
    return chosen, margin


def topk_object(X, x, count, K, rnd, tau, n_polish, min_count, Kt, sep_frac, min_inliers=0, hyps=None, cost=None, inliers=None):
    """One object.  hyps: (cost, inliers, poses) of `hypotheses` computed before (None: computed here); cost / inliers: arrays that
    REPLACE the restatement's in the selection (the device's).
    -> dict: cost, inliers, poses (the restatement's own), lo, hi, diag, sep, hyp (Kt, -1 padded), n_found, T (Kt: (4,4) or None),
    inlier_mask (Kt, count), n_inliers, final_cost, info, dup_of (Kt each), select_margin, dup_margin (distances, absolute) and
    tau_margin (pixels)."""
    count = max(0, min(int(count), len(X)))
    c0, i0, poses = hypotheses(X, x, count, K, rnd, tau, min_count) if hyps is None else hyps
    lo, hi, diag = extent(X, count)
    sep = sep_frac * diag
    chosen, smargin = select(c0 if cost is None else cost, i0 if inliers is None else inliers, poses, lo, hi, sep, Kt, min_inliers)
    Xd, xd, Kd = np.asarray(X, np.float64)[:count], np.asarray(x, np.float64)[:count], np.asarray(K, np.float64)
    out = dict(cost=c0, inliers=i0, poses=poses, lo=lo, hi=hi, diag=diag, sep=sep, hyp=np.full(Kt, -1, np.int64), n_found=len(chosen), T=[None] * Kt,
               inlier_mask=np.zeros((Kt, count), bool), n_inliers=np.zeros(Kt, np.int64), final_cost=np.full(Kt, np.inf),
               info=np.full(Kt, -1, np.int64), dup_of=np.full(Kt, -1, np.int64), select_margin=smargin, dup_margin=np.inf, tau_margin=np.inf)
    for k, h in enumerate(chosen):
        out["hyp"][k] = h
        tm = []
        pose = pr.polish(poses[h][:3, :3], poses[h][:3, 3], Kd, Xd, xd, tau, n_polish, margins=tm)
        out["tau_margin"] = min([out["tau_margin"]] + tm)
        if pose is None:
            continue
        c, n, m = pr.score(*pose, Kd, Xd, xd, tau)
        out["T"][k] = pose_matrix(*pose)
        out["inlier_mask"][k], out["n_inliers"][k], out["final_cost"][k], out["info"][k] = m, n, c, 0
        for j in range(k):
            if out["info"][j] != 0:
                continue
            d = distance(out["T"][k], out["T"][j], lo, hi)
            out["dup_margin"] = min(out["dup_margin"], abs(d - sep))
            if not d > sep:
                out["dup_of"][k] = j
                break
    return out


def topk(X, x, count, K, rnd, tau, n_polish, min_count=4, Kt=4, sep_frac=0.1, min_inliers=0, hyps=None, cost=None, inliers=None):
    B = len(count)
    pick = lambda a, b: None if a is None else a[b]
    return [topk_object(X[b], x[b], count[b], K[b], rnd[b], tau, n_polish, min_count, Kt, sep_frac, min_inliers, pick(hyps, b), pick(cost, b),
                        pick(inliers, b)) for b in range(B)]


def two_mode_case(counts, Hyp, seed, shares=(0.45, 0.35), noise=0.5, M=None):
    """Planted two-mode data of pnp_ref.p3p_scenes's distribution: per object, points uniform in a +-0.1 m cube; a share of the
    correspondences projects under a WRONG pose A, a share under the TRUE pose B (both drawn as p3p_scenes draws its poses), the rest is
    uniform in a 120 x 120 px box about the projected origin; Gaussian pixel noise on A and B; everything rounded to fp32.  A count of 4
    is 2 + 2.  -> X (B,M,3) fp32, x (B,M,2) fp32, counts int32, K (B,3,3) fp32, rnd (B,Hyp,3) uint64, poses_a, poses_b (B,4,4) fp64,
    label (B,M) int (0 = A, 1 = B, 2 = random, -1 = behind count)."""
    rng = np.random.default_rng(seed)
    B, M = len(counts), int(M or max(counts))
    X, x = np.zeros((B, M, 3), np.float32), np.zeros((B, M, 2), np.float32)
    K = np.tile(pr.P3P_K, (B, 1, 1)).astype(np.float32)
    Ta, Tb, label = np.tile(np.eye(4), (B, 1, 1)), np.tile(np.eye(4), (B, 1, 1)), np.full((B, M), -1, np.int64)

    def draw():
        R, _ = pr.se3_exp(np.concatenate([np.zeros(3), rng.normal(0, 1, 3)]))
        return R, np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)])
    for b, n in enumerate(counts):
        Xb = rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32).astype(np.float64)
        (Ra, ta), (Rb, tb) = draw(), draw()
        na, nb = (2, 2) if n == 4 else (int(round(shares[0] * n)), int(round(shares[1] * n)))
        perm = rng.permutation(n)
        lab = np.full(n, 2, np.int64)
        lab[perm[:na]], lab[perm[na:na + nb]] = 0, 1
        c = pr.project(Rb, tb, pr.P3P_K, np.zeros((1, 3)))[0][0]
        uv = c + rng.uniform(-60, 60, (n, 2))
        uv[lab == 0] = pr.project(Ra, ta, pr.P3P_K, Xb[lab == 0])[0] + rng.normal(0, noise, (na, 2))
        uv[lab == 1] = pr.project(Rb, tb, pr.P3P_K, Xb[lab == 1])[0] + rng.normal(0, noise, (nb, 2))
        X[b, :n], x[b, :n], label[b, :n] = Xb, uv, lab
        Ta[b], Tb[b] = pose_matrix(Ra, ta), pose_matrix(Rb, tb)
    rnd = rng.integers(0, 2 ** 32, (B, Hyp, 3), dtype=np.uint64)
    return X, x, np.array(counts, np.int32), K, rnd, Ta, Tb, label
