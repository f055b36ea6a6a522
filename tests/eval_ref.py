"""The LINEMOD metric kernels of csrc/eval_metrics.hip -- nn_search<2|3>, transform_points, pose_metrics -- restated in plain numpy: the
yardstick of tests/test_gpu_eval_edges.py.  tests/test_eval_ref.py ties the restatements to oracle/eval_oracle.py, to a literal double
loop and to the `eval_metric` golden fixture.

nn_idx_serial is the reference's serial loop (thirdparty/nn/src/nearest_neighborhood.cu:48-81) as a statement about values: the fp32
distance `(dx*dx + dy*dy) + dz*dz` with every product and every sum rounded to fp32, a candidate taken only if `d < best` with best
starting at FLT_MAX, ascending index.  Hence: the FIRST minimum wins; a NaN, an inf or a distance of exactly FLT_MAX is never taken; a
query that takes nothing keeps index 0.  (oracle/eval_oracle.py:nn_idx is np.argmin, which picks a NaN: the two differ there.)

pose_metrics_ref computes the fp64 terms in the operation order of the kernel and of oracle/eval_oracle.py, sums them exactly
(math.fsum) and returns, next to the five columns, the error each column of ANOTHER fp64 evaluation of the same formulas may show.

ERROR BOUNDS (u = 2^-53; derived, not tuned; `gamma(n) = n u` stands for n u / (1 - n u), the difference is below 1e-13 of the bound).
They hold for any fp64 evaluation of the formulas, in any association and with or without fma, so they do not lean on the kernel's
operation order -- with ONE exception that is said where it is used (the fp32 points of ADD-S).

 * transformed point, row r:  p_r = T_r0 x + T_r1 y + T_r2 z + T_r3.  An inner product of 4 terms evaluated in fp64 is within
   gamma(4) M_r of the exact value, M_r = |T_r0 x| + |T_r1 y| + |T_r2 z| + |T_r3| (Higham, Accuracy and Stability, (3.5); an fma only
   removes roundings).  Two evaluations differ by at most  dP_r = 8 u M_r.
 * ADD term  d = |pp - pg|:  s_r = pp_r - pg_r differs by at most  E_r = dPp_r + dPg_r + 2 u |s_r|  (one rounding of the subtraction on
   each side).  | |s| - |s'| | <= |s - s'| <= |E|_2.  The norm's own arithmetic: three squares and two adds are within gamma(3) of the
   sum of squares (relative), the square root halves that and adds its own rounding, 2.5 u per side, 5 u between two: taken as 6 u d.
       tau_add_i = |E_i|_2 + 6 u d_i
 * a mean of P non-negative terms:  a recursive or tree sum in any order is within (P - 1) u sum(d) (Higham (4.4), all terms >= 0 so
   sum|d| = sum d); the division by P adds u; math.fsum on this side is exact up to one rounding and one division, 2 u:
       bound(mean) = mean(tau) + (P + 2) u mean(d)
 * ADD-S term:  a, g are fp32 POINTS.  Here the derivation assumes that both sides hold the SAME fp32 points and the same index: the
   points are `float(T_r0 x + T_r1 y + T_r2 z + T_r3)` with IEEE fp64 products and sums in the written order (the file compiles with fp
   contraction off), which has one value; the index is exact by the tests of nn_search.  That is what pins transform_points_kernel's
   rounding: fp64 points in the search, or another association, move an ADD-S mean at the 1e-8 relative scale, 1e7 bounds away.
   dx = a_x - g_x is one rounding (u |dx|, 2 u between two sides, which moves the norm by at most 2 u d), the norm as above 5 u:
       tau_adds_i = 8 u d_i        (7 u, taken as 8)
 * projection term:  q_r = K_r0 p_0 + K_r1 p_1 + K_r2 p_2 with p uncertain by dP:  dq_r = sum_c |K_rc| dP_c + 6 u sum_c |K_rc p_c|
   (gamma(3) per side).  pixel = q_0 / q_2:  dpix = dq_0 / |q_2| + |q_0| dq_2 / q_2^2 + 2 u |q_0 / q_2|  (first order in dq_2 / q_2,
   which is below 1e-13 for every finite case here; one rounding of the division per side).  e = pix_p - pix_g:
   de = dpix_p + dpix_g + 2 u |e|.  The term |e|_2:  tau_proj_i = |de_i|_2 + 6 u |e_i|.  The per-term error therefore scales with
   u max|pixel coordinate| and is ABSOLUTE: a projection error of 1e-3 px at pixel 600 carries 600 u, not 1e-3 u.
 * translation:  differences of fp32 values in fp64 (one rounding each), the norm 2.5 u, the factor 100 one rounding; two sides:
       bound = 8 u value
 * rotation, cosine domain:  the nine products of fp32 entries are exact in fp64 (24 + 24 bits), so the trace differs from the exact
   one only by its eight additions: gamma(8) S, S = sum |products| (<= 3 (1 + 2^-23)^2 for rotations: "at most 8 u" per unit of S).
   This side sums exactly (one rounding, u |tr|).  c = (tr - 1) / 2: the subtraction rounds once per side, the halving is exact:
       bound(c) = (8 u S + u |tr| + 2 u |tr - 1|) / 2
   The kernel reports an angle.  acos is held to 4 ulp (the OpenCL bound the device library documents), the conversion to degrees is a
   product with a rounded constant, 2 u: the reported angle is within  dA = 6 u theta  of 180/pi acos(c_kernel).  Tests take the cosine of
   the reported angle (numpy, 1 ulp, |d cos| <= sin(theta) d theta) and compare with c:
       bound(cos) = bound(c) + sin(theta) 6 u theta_rad + 2 u
   and as an angle only where sin(theta) is away from 0: by the mean value theorem |acos a - acos b| <= |a - b| / sqrt(1 - m^2) with
   m = max(|a|, |b|) <= |c| + bound(c):
       bound(theta_deg) = 180/pi bound(c) / sqrt(1 - (|c| + bound(c))^2) + 6 u theta_deg         where that root is >= SIN_MIN
   Where the trace is exact (all products in {0, +-1}: axis-aligned rotations), bound(c) is 0 and the angle is compared directly.
"""
import math

import numpy as np

F32 = np.float32
FLT_MAX = np.float32(np.finfo(np.float32).max)
U = 2.0 ** -53
K_LM = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float32)      # the LINEMOD camera
SIN_MIN = 0.1          # the angle is compared as an angle where sqrt(1 - (|c| + bound)^2) >= SIN_MIN: theta in about [5.8, 174.2] degrees


# ---------------------------------------------------------------------------------------------------------------- nearest neighbour
def _dist_f32(ref, que, form="serial"):
    """(n2, n1) fp32 squared distances.  form: "serial" -- every product and sum rounded to fp32; "fma_all" -- what full contraction
    makes of the expression: fma(dz, dz, fma(dx, dx, dy*dy)); "fma_last" -- only the last add contracted: fma(dz, dz, dx*dx + dy*dy)
    (dim 2 has one add: fma(dx, dx, dy*dy) and fma(dy, dy, dx*dx)).  An fma is emulated in fp64: the product of two fp32 values is exact
    there, the sum is rounded to fp64 and then to fp32 (a double rounding; exact for the lattice clouds, whose sums fit 53 bits)."""
    ref, que = np.asarray(ref, F32), np.asarray(que, F32)
    dim = ref.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        dx = ref[None, :, 0] - que[:, None, 0]
        dy = ref[None, :, 1] - que[:, None, 1]
        dz = ref[None, :, 2] - que[:, None, 2] if dim == 3 else None
        fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
        if form == "serial":
            d = dx * dx + dy * dy
            return d + dz * dz if dim == 3 else d
        if form == "fma_all":
            d = fma(dx, dx, dy * dy)
            return fma(dz, dz, d) if dim == 3 else d
        if form == "fma_last":
            return fma(dz, dz, dx * dx + dy * dy) if dim == 3 else fma(dy, dy, dx * dx)
    raise ValueError(form)


def _first_taken(d, exclude_self):
    d = np.array(d, F32)
    if exclude_self:
        n = min(d.shape)                               # p1i == p2i on GLOBAL indices, whatever pn1 and pn2
        d[np.arange(n), np.arange(n)] = np.inf
    d = np.where(d < FLT_MAX, d, F32(np.inf))          # `d < best` from FLT_MAX: NaN, inf and FLT_MAX itself are never taken
    return np.argmin(d, axis=1).astype(np.int32)       # first minimum; a row of inf only -> 0


def nn_idx_serial(ref, que, exclude_self=False):
    """ref (n1, D), que (n2, D), D in {2, 3} -> (n2,) int32: the index the reference's serial loop ends with."""
    return _first_taken(_dist_f32(ref, que, "serial"), exclude_self)


def nn_idx_contracted(ref, que, exclude_self=False, form="fma_all"):
    """the same loop over a contracted distance (form "fma_all" or "fma_last"): only to show that a planted cloud is sensitive"""
    assert form in ("fma_all", "fma_last")
    return _first_taken(_dist_f32(ref, que, form), exclude_self)


def nn_idx_loop(ref, que, exclude_self=False):
    """the loop itself, literally (sizes <= 40 in the tests)"""
    ref, que = np.asarray(ref, F32), np.asarray(que, F32)
    out = np.zeros(que.shape[0], np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for p2i in range(que.shape[0]):
            best, best_i = FLT_MAX, 0
            for p1i in range(ref.shape[0]):
                if exclude_self and p1i == p2i:
                    continue
                dx, dy = F32(ref[p1i, 0] - que[p2i, 0]), F32(ref[p1i, 1] - que[p2i, 1])
                d = F32(F32(dx * dx) + F32(dy * dy))
                if ref.shape[1] == 3:
                    dz = F32(ref[p1i, 2] - que[p2i, 2])
                    d = F32(d + F32(dz * dz))
                if d < best:
                    best, best_i = d, p1i
            out[p2i] = best_i
    return out


def contraction_cloud(dim, seed=3):
    """A cloud on which fp contraction changes the winner.  Queries sit on an integer lattice (8 x 8 x 8 in [-4, 4)^3, 16 x 16 in
    [-8, 8)^2); query i has two reference points, i and i + Q, at offsets v and a cyclic permutation of v (dim 2: (a, b) and (b, a)),
    the components k 2^-20 with |k| < 2^18.  lattice + offset has at most 3 + 20 = 23 significant bits: the points are exact fp32
    values and ref - que gives v back exactly, so both candidates have the same exact squared length and only the ROUNDING of the partial
    sums -- taken in a different association for the two -- decides; every other reference point is more than 0.56 away, these two
    less than 0.44.   -> ref (2Q, dim), que (Q, dim) fp32."""
    from rnnpose_amd import synthetic as syn
    side = 8 if dim == 3 else 16
    g = np.arange(side, dtype=np.float64) - side // 2
    que = np.stack(np.meshgrid(*([g] * dim), indexing="ij"), -1).reshape(-1, dim)
    Q = que.shape[0]
    k = np.floor(syn.uniform(f"contraction{dim}", (Q, dim), seed, -2.0 ** 18 + 1, 2.0 ** 18).astype(np.float64))
    v = k * 2.0 ** -20
    w = np.roll(v, 1, axis=1)
    ref = np.concatenate([que + v, que + w], 0)
    ref32, que32 = ref.astype(F32), que.astype(F32)
    assert np.array_equal(ref32.astype(np.float64), ref) and np.array_equal((ref32[:Q] - que32).astype(np.float64), v)
    return ref32, que32


# ---------------------------------------------------------------------------------------------------------------- pose metrics
def _apply(T, m):
    """T (3,4), m (P,3) fp64 -> points (P,3) in the kernel's order ((T0 x + T1 y) + T2 z) + T3, and M = the sum of the magnitudes"""
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3] for r in range(3)], 1)
        M = np.stack([np.abs(T[r, 0] * x) + np.abs(T[r, 1] * y) + np.abs(T[r, 2] * z) + np.abs(T[r, 3]) for r in range(3)], 1)
    return p, M


def _project(K, p, dP):
    """pixel (P,2) = (K p)_{0,1} / (K p)_2 and its uncertainty (see the module docstring)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.stack([K[r, 0] * p[:, 0] + K[r, 1] * p[:, 1] + K[r, 2] * p[:, 2] for r in range(3)], 1)
        dq = np.stack([np.abs(K[r, 0]) * dP[:, 0] + np.abs(K[r, 1]) * dP[:, 1] + np.abs(K[r, 2]) * dP[:, 2]
                       + 6 * U * (np.abs(K[r, 0] * p[:, 0]) + np.abs(K[r, 1] * p[:, 1]) + np.abs(K[r, 2] * p[:, 2])) for r in range(3)], 1)
        pix = q[:, :2] / q[:, 2:]
        dpix = dq[:, :2] / np.abs(q[:, 2:]) + np.abs(q[:, :2]) * dq[:, 2:] / q[:, 2:] ** 2 + 2 * U * np.abs(pix)
    return pix, dpix


def _fmean(v):
    v = np.asarray(v, np.float64)
    if not np.isfinite(v).all():                       # math.fsum refuses inf - inf; the class (nan / inf) is what numpy's sum gives
        with np.errstate(invalid="ignore"):
            return float(np.sum(v)) / len(v)
    return math.fsum(v.tolist()) / len(v)


def _norm(v):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((v * v).sum(1)) if v.shape[1] != 3 else np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def pose_metrics_ref(model, pose_pred, pose_gt, K, symmetric, swap_direction=False):
    """model (P,3), pose_pred / pose_gt (B,3,4), K (3,3) (fp32 arrays, as the kernel gets them) -> dict
         cols (B,5) fp64 [ADD, ADD-S or -1, proj2d px, trans cm, rot deg]      bound (B,5): |another fp64 evaluation - cols| (the angle's
         entry is NaN where it may only be compared as a cosine)      cos_raw, cos (B): (tr - 1) / 2 before / after the clamp at tr = 3
         c_bound (B): bound(c), the error another evaluation's cosine may have      cos_bound (B): bound(cos) of the module docstring, for
         cos(reported angle) against `cos`.
    swap_direction: ADD-S as the nearest TARGET point of every PREDICTED point -- the direction the kernel must NOT implement."""
    m = np.asarray(model, F32).astype(np.float64)
    Kd = np.asarray(K, F32).astype(np.float64)
    pp_all, pg_all = np.asarray(pose_pred, F32).astype(np.float64), np.asarray(pose_gt, F32).astype(np.float64)
    B, P = pp_all.shape[0], m.shape[0]
    cols, bound = np.empty((B, 5)), np.empty((B, 5))
    cos_raw, cos_c, cos_bound, c_bound = np.empty(B), np.empty(B), np.empty(B), np.empty(B)
    for b in range(B):
        Tp, Tg = pp_all[b], pg_all[b]
        xp, Mp = _apply(Tp, m)
        xg, Mg = _apply(Tg, m)
        dPp, dPg = 8 * U * Mp, 8 * U * Mg
        with np.errstate(invalid="ignore", over="ignore"):
            s = xp - xg
            d = _norm(s)
            tau = _norm(dPp + dPg + 2 * U * np.abs(s)) + 6 * U * d
        cols[b, 0] = _fmean(d)
        bound[b, 0] = _fmean(tau) + (P + 2) * U * cols[b, 0]
        if symmetric:
            a32, g32 = xp.astype(F32), xg.astype(F32)                         # transform_points_kernel's store
            if swap_direction:
                idx = nn_idx_serial(g32, a32)
                da = a32.astype(np.float64) - g32.astype(np.float64)[idx]
            else:
                idx = nn_idx_serial(a32, g32)                                 # ref = predicted points, queries = target points
                da = a32.astype(np.float64)[idx] - g32.astype(np.float64)
            ds = _norm(da)
            cols[b, 1] = _fmean(ds)
            bound[b, 1] = (8 + P + 2) * U * cols[b, 1]
        else:
            cols[b, 1], bound[b, 1] = -1.0, 0.0
        up, dup = _project(Kd, xp, dPp)
        ug, dug = _project(Kd, xg, dPg)
        with np.errstate(invalid="ignore", over="ignore"):
            e = up - ug
            en = _norm(e)
            taup = _norm(dup + dug + 2 * U * np.abs(e)) + 6 * U * en
        cols[b, 2] = _fmean(en)
        bound[b, 2] = _fmean(taup) + (P + 2) * U * cols[b, 2]
        t = Tp[:, 3] - Tg[:, 3]
        with np.errstate(invalid="ignore", over="ignore"):
            cols[b, 3] = np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) * 100.0
        bound[b, 3] = 8 * U * cols[b, 3]
        prods = (Tp[:, :3] * Tg[:, :3]).reshape(-1)                            # exact: fp32 x fp32 in fp64
        if np.isfinite(prods).all():
            tr, S = math.fsum(prods.tolist()), math.fsum(np.abs(prods).tolist())
        else:
            tr, S = float("nan"), float("nan")
        exact = bool(np.isin(prods, (0.0, 1.0, -1.0)).all())
        c0 = (tr - 1.0) / 2.0
        c1 = (min(tr, 3.0) - 1.0) / 2.0 if tr == tr else c0
        cb = 0.0 if exact else (8 * U * S + U * abs(tr) + 2 * U * abs(tr - 1.0)) / 2.0
        cos_raw[b], cos_c[b], c_bound[b] = c0, c1, cb
        with np.errstate(invalid="ignore"):
            th = float(np.arccos(c1))                                          # NaN for c1 < -1 (and for a NaN pose), as the reference
        cols[b, 4] = np.rad2deg(th)
        cos_bound[b] = cb + (math.sin(th) * 6 * U * th + 2 * U if th == th else float("nan"))
        root = 1.0 - (abs(c1) + cb) ** 2
        if exact and th == th:
            bound[b, 4] = 6 * U * cols[b, 4]
        elif th == th and root > 0 and math.sqrt(root) >= SIN_MIN:
            bound[b, 4] = math.degrees(cb) / math.sqrt(root) + 6 * U * cols[b, 4]
        else:
            bound[b, 4] = float("nan")
    return {"cols": cols, "bound": bound, "cos_raw": cos_raw, "cos": cos_c, "cos_bound": cos_bound, "c_bound": c_bound}


def flags(cols, diameter, symmetric):
    """the evaluator's five decisions, strict `<` (a NaN misses)   [add, add2, add5, proj2d, cmd5] = distributed.METRICS order"""
    cols = np.asarray(cols, np.float64)
    d = cols[:, 1] if symmetric else cols[:, 0]
    with np.errstate(invalid="ignore"):
        return np.stack([d < 0.1 * diameter, d < 0.02 * diameter, d < 0.05 * diameter, cols[:, 2] < 5.0,
                         (cols[:, 3] < 5.0) & (cols[:, 4] < 5.0)], 1)


# ---------------------------------------------------------------------------------------------------------------- planted rotations
def _trace_exact(Rp, Rg):
    return math.fsum((np.asarray(Rp, F32).astype(np.float64) * np.asarray(Rg, F32).astype(np.float64)).reshape(-1).tolist())


def rotation_with_trace(kind, seed=0, tries=4000):
    """Seeded search for fp32 rotation pairs whose ROUNDED entries put the trace outside [-1, 3] -- by parts in 1e8, the scale of fp32
    rounding, seven orders above what the order of an fp64 summation can move (8 u S, about 3e-15):
      "above3":  Rp = Rg = float(R): the trace is the squared Frobenius norm, > 3 + 1e-9
      "below-1": Rp = float(R), Rg = Rp with its second and third column negated (exactly R Rx(180 deg)): trace < -1 - 1e-9
    -> (Rp, Rg) (3,3) fp32.  The tests assert the precondition again, against bound(c)."""
    from rnnpose_amd import synthetic as syn
    for n in range(tries):
        w = syn.normal(f"planted_rot_{kind}", (3,), seed + 7919 * n, std=1.0).astype(np.float64)
        R = syn.se3_exp_np(np.concatenate([np.zeros(3), w])[None])[0, :3, :3].astype(F32)
        Rg = R.copy() if kind == "above3" else (R * np.array([1, -1, -1], F32)[None, :])
        tr = _trace_exact(R, Rg)
        if (kind == "above3" and tr > 3.0 + 1e-9) or (kind == "below-1" and tr < -1.0 - 1e-9):
            return R, Rg
    raise RuntimeError(f"no {kind} rotation in {tries} draws")


def pose_pair(name, B, scales, seed=0, depth=0.9):
    """B ground-truth poses in front of the camera and predictions that are off by scales[b % len(scales)] metres (and as many radians
    over a tenth of a metre of lever) -> pred, gt (B,3,4) fp32"""
    from rnnpose_amd import synthetic as syn
    gt = syn.se3_exp_np(syn.normal(name + "gt", (B, 6), seed, std=0.3) * np.array([[1 / 3, 1 / 3, 1 / 3, 1, 1, 1]]))      # |t| < 0.35 per axis: depth > 0.5
    gt[:, 2, 3] += depth
    sc = np.asarray([scales[b % len(scales)] for b in range(B)], np.float64)[:, None]
    d = syn.normal(name + "d", (B, 6), seed + 1, std=1.0).astype(np.float64) * sc * np.array([[1, 1, 1, 5, 5, 5]])
    pred = syn.se3_exp_np(d) @ gt
    return pred[:, :3].astype(F32), gt[:, :3].astype(F32)


def clustered_case():
    """A deliberately asymmetric model -- 40 points in a tight cluster, 24 spread over the object -- under 3 poses that are centimetres
    off: many target points share one nearest predicted point in one direction and not in the other."""
    from rnnpose_amd import synthetic as syn
    model = np.concatenate([syn.uniform("cluster", (40, 3), 5, 0.060, 0.064), syn.uniform("spread", (24, 3), 5, -0.08, 0.08)], 0)
    pred, gt = pose_pair("clustered", 3, (0.01, 0.02, 0.04), seed=5)
    return model, pred, gt


def flt_max_point(dim):
    """-> an fp32 point whose squared distance from the origin, in the loop's arithmetic, is EXACTLY FLT_MAX: `d < best` from FLT_MAX does
    not take it (a loop that starts from infinity would).  A search over a from 1.25e19 upwards with b next to sqrt(FLT_MAX - a^2)."""
    a = F32(1.25e19)
    with np.errstate(over="ignore"):
        for _ in range(4096):
            a = np.nextafter(a, F32(np.inf))
            X = F32(a * a)
            b = np.nextafter(F32(np.sqrt(float(FLT_MAX) - float(X))), F32(0))
            for _ in range(3):
                if F32(X + F32(b * b)) == FLT_MAX:
                    p = np.zeros(dim, F32)
                    p[0], p[1] = a, b
                    return p
                b = np.nextafter(b, F32(np.inf))
    raise RuntimeError("no point at a squared distance of FLT_MAX")
