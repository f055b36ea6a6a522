"""TEST INFRASTRUCTURE ONLY -- an fp64 RAY CASTER as the reference of the mesh rasteriser (rnnpose_amd/csrc/raster.hip), independent of
the screen-space edge-function algorithm the kernel and oracle/raster_oracle.py share.

For pixel (x, y) the ray is ((x + pc - cx) / fx, (y + pc - cy) / fy, 1) in camera space; it is intersected with every triangle after T by
Moeller-Trumbore in float64.  The ray's z component is 1, so the ray parameter of a hit IS its camera z; the hit with the smallest
positive z wins, on exactly equal z the lower face index.  The 3-D barycentrics of the hit point are by construction the
perspective-correct weights (what the kernel gets from BarycentricPerspectiveCorrection of its screen-space weights), and
z = sum w_i z_i.  Faces with any vertex at Z <= near are dropped whole, faces whose doubled screen area is <= 1e-8 px^2 are dropped (both
as documented in include/rnnpose_hip.h).  `perspective=False` returns the SCREEN-space weights of the projected 2-D triangle and
z = sum w_i z_i with them (render_depth's depth_perspective_correct=False path).

Work is vectorised over (face, pixel) pairs: every face is paired with the pixels of its projected bounding box grown by 2 px (a ray
outside that box cannot meet the face), clamped to the image.

THE CERTAINTY MASK.  fp32 and fp64 may legitimately disagree only where a pixel centre lies within rounding distance of a projected edge
or where two surfaces are within rounding distance in depth.  With d_f(p) the signed distance in pixels of centre p to the boundary of
the projected face f (positive inside) and

    delta_f = 32 * 2^-24 * max(H, W, largest |screen coordinate| of f)  px        tau(z) = 32 * 2^-24 * z

(a projected coordinate is O(W); the ~8 fp32 roundings of the projection X' = r.v + t, x = fx X' / Z + cx and of the edge function each
cost at most one ulp of that, 2^-24 * coordinate relative to the edge length after the division by the doubled area; 32 is a 4x margin),
face f SURELY covers p when d_f >= delta_f and is a BOUNDARY face of p when |d_f| < delta_f.  With z_s(p) the nearest surely covering
depth, the CANDIDATES of p are the surely-covering and boundary faces with z_f(p) <= z_s(p) + tau(z_s(p)) (z_f: the ray's intersection
with the face's plane, defined on both sides of the edge).  A pixel is CERTAIN when it has no candidate (a certain miss) or exactly one,
which surely covers it: no face that could be the nearest hit has the centre within delta of its boundary, and no second covering face
is within tau of the winner.  This is the conservative form: two faces that share the edge in question are both counted (the exemption
the continuity of depth and attributes across a shared edge would allow is not used), which only enlarges the uncertain share -- and
that share is capped by the tests.  At an UNCERTAIN pixel the kernel must still reproduce one of the candidates (or "no surface" when
no face surely covers it): `candidates` lists them with their weights.

Nearest-vertex depth (the argmax of the weights) needs more: it is certain where the pixel is certain and the two largest weights differ
by at least 2 * delta_f / a_f + 64 * 2^-24, a_f the smallest altitude of the projected face in pixels: a weight changes by at most 1 / a_f
per pixel of displacement, the difference of two by at most twice that, and the perspective division adds a few relative roundings.
(a_f <= every edge length, so this excludes no less than delta / (edge length).)
"""
import numpy as np

EPS = 2.0 ** -24
MARGIN = 32.0


def _camera(verts, T, K):
    v = np.asarray(verts, np.float64)
    T = np.asarray(T, np.float64)
    K = np.asarray(K, np.float64)
    return v @ T[:3, :3].T + T[:3, 3], K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def _pairs(x0, x1, y0, y1, budget=1 << 21):
    """chunks of (face position, px, py) over the inclusive integer boxes"""
    n = (x1 - x0 + 1) * (y1 - y0 + 1)
    lo = 0
    while lo < n.size:
        hi, tot = lo, 0
        while hi < n.size and (hi == lo or tot + n[hi] <= budget):
            tot += n[hi]
            hi += 1
        nn, w = n[lo:hi], (x1 - x0 + 1)[lo:hi]
        k = np.arange(tot) - np.repeat(np.cumsum(nn) - nn, nn)
        ww = np.repeat(w, nn)
        yield np.repeat(np.arange(lo, hi), nn), np.repeat(x0[lo:hi], nn) + k % ww, np.repeat(y0[lo:hi], nn) + k // ww
        lo = hi


def raycast(verts, faces, T, K, H, W, near=0.1, pixel_center=0.5, perspective=True):
    """-> dict: face (H,W) int64 (-1 = miss), z (H,W) (-1 = miss), w (H,W,3), vz (H,W) (0 = miss), certain (H,W) bool, vd_certain (H,W) bool,
    miss_ok (H,W) bool (no face surely covers the pixel), candidates = dict(pix, face, z, w) over the candidate pairs of every pixel,
    cam_z (P,), and per face delta (F,) and alt (F,): delta_f and the smallest projected altitude a_f of the docstring above, in px"""
    faces = np.asarray(faces, np.int64)
    Xc, fx, fy, cx, cy = _camera(verts, T, K)
    if not (np.isfinite(Xc).all()):
        keep = np.isfinite(Xc[faces]).all((1, 2))
    else:
        keep = np.ones(len(faces), bool)
    Z = Xc[:, 2]
    keep &= np.all(np.nan_to_num(Z[faces], nan=-1.0) > near, 1)
    with np.errstate(all="ignore"):
        sx = fx * Xc[:, 0] / Z + cx
        sy = fy * Xc[:, 1] / Z + cy
        tx, ty = sx[faces], sy[faces]                                           # (F,3)
        area = (tx[:, 1] - tx[:, 0]) * (ty[:, 2] - ty[:, 0]) - (tx[:, 2] - tx[:, 0]) * (ty[:, 1] - ty[:, 0])
        keep &= np.nan_to_num(np.abs(area), nan=0.0) > 1e-8
        pc = float(pixel_center)
        big = np.maximum(np.abs(tx).max(1), np.abs(ty).max(1))
        delta = MARGIN * EPS * np.maximum(float(max(H, W)), big)
        grow = 2.0 + delta
        bx0 = np.clip(np.floor(tx.min(1) - pc - grow), 0, W)
        bx1 = np.clip(np.ceil(tx.max(1) - pc + grow), -1, W - 1)
        by0 = np.clip(np.floor(ty.min(1) - pc - grow), 0, H)
        by1 = np.clip(np.ceil(ty.max(1) - pc + grow), -1, H - 1)
    keep &= (bx0 <= bx1) & (by0 <= by1)
    ids = np.nonzero(keep)[0]
    P = H * W
    acc = {k: [] for k in ("pix", "face", "z", "w", "d", "inside")}
    for fpos, px, py in _pairs(bx0[ids].astype(np.int64), bx1[ids].astype(np.int64), by0[ids].astype(np.int64), by1[ids].astype(np.int64)):
        f = ids[fpos]
        qx, qy = px + pc, py + pc
        # signed distance to the boundary of the projected triangle (positive inside, either winding)
        s = np.sign(area[f])
        d = np.full(f.shape, np.inf)
        e = []
        for i in range(3):
            ax, ay = tx[f, (i + 1) % 3], ty[f, (i + 1) % 3]
            bx, by = tx[f, (i + 2) % 3], ty[f, (i + 2) % 3]
            cr = (bx - ax) * (qy - ay) - (by - ay) * (qx - ax)
            e.append(cr)
            d = np.minimum(d, s * cr / np.hypot(bx - ax, by - ay))
        v0, v1, v2 = Xc[faces[f, 0]], Xc[faces[f, 1]], Xc[faces[f, 2]]
        if perspective:                                                         # Moeller-Trumbore, origin 0, direction D
            D = np.stack([(qx - cx) / fx, (qy - cy) / fy, np.ones_like(qx)], 1)
            e1, e2 = v1 - v0, v2 - v0
            pv = np.cross(D, e2)
            det = np.einsum("ij,ij->i", e1, pv)
            with np.errstate(all="ignore"):
                u = np.einsum("ij,ij->i", -v0, pv) / det
                qv = np.cross(-v0, e1)
                v = np.einsum("ij,ij->i", D, qv) / det
                z = np.einsum("ij,ij->i", e2, qv) / det
            w = np.stack([1.0 - u - v, u, v], 1)
            inside = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
        else:
            w = np.stack(e, 1) / area[f][:, None]
            z = (w * np.stack([v0[:, 2], v1[:, 2], v2[:, 2]], 1)).sum(1)
            inside = (w >= 0).all(1)
        k = (d > -delta[f]) & np.isfinite(z) & (z > 0)
        acc["pix"].append((py * W + px)[k]); acc["face"].append(f[k]); acc["z"].append(z[k]); acc["w"].append(w[k])
        acc["d"].append(d[k]); acc["inside"].append(inside[k])
    cat = lambda k, dt, shape=(0,): np.concatenate(acc[k]) if acc[k] else np.zeros(shape, dt)
    pix, fid, z, d, inside = cat("pix", np.int64), cat("face", np.int64), cat("z", float), cat("d", float), cat("inside", bool)
    w = cat("w", float, (0, 3))
    # the ray caster's own winner: nearest inside hit, lower face index on exactly equal z
    best_f = np.full(P, -1, np.int64)
    best_z = np.full(P, -1.0)
    best_w = np.zeros((P, 3))
    sel = np.nonzero(inside)[0]
    order = sel[np.lexsort((fid[sel], z[sel], pix[sel]))]
    first = order[np.concatenate([[True], pix[order][1:] != pix[order][:-1]])] if order.size else order
    best_f[pix[first]], best_z[pix[first]], best_w[pix[first]] = fid[first], z[first], w[first]
    hit = best_f >= 0
    fz = Z[faces[np.clip(best_f, 0, None)]]
    vz = np.where(hit, np.take_along_axis(fz, best_w.argmax(1)[:, None], 1)[:, 0], 0.0)
    # certainty
    sure = d >= delta[fid]
    zs = np.full(P, np.inf)
    np.minimum.at(zs, pix[sure], z[sure])
    cand = z <= zs[pix] * (1.0 + MARGIN * EPS)
    ncand = np.bincount(pix[cand], minlength=P)
    nbnd = np.bincount(pix[cand & ~sure], minlength=P)
    certain = (ncand == 0) | ((ncand == 1) & (nbnd == 0))
    assert np.all(hit[certain] == (ncand[certain] == 1))                        # the two notions of coverage agree away from edges
    one = cand & certain[pix]
    assert np.array_equal(best_f[pix[one]], fid[one])
    # nearest-vertex depth
    ws = np.sort(best_w, 1)
    bf = np.clip(best_f, 0, None)
    with np.errstate(all="ignore"):
        edge = np.sqrt((tx - np.roll(tx, 1, 1)) ** 2 + (ty - np.roll(ty, 1, 1)) ** 2).max(1)
        alt_f = np.abs(area) / edge                                             # (F,) smallest projected altitude of every face, px
        alt = alt_f[bf]
        gap = 2.0 * delta[bf] / alt + 64.0 * EPS
    vd_certain = certain & (~hit | (ws[:, 2] - ws[:, 1] >= gap))
    r = lambda a: a.reshape((H, W) + a.shape[1:])
    return dict(face=r(best_f), z=r(best_z), w=r(best_w), vz=r(vz), hit=r(hit), certain=r(certain), vd_certain=r(vd_certain),
                miss_ok=r(~np.isfinite(zs)), candidates=dict(pix=pix[cand], face=fid[cand], z=z[cand], w=w[cand]),
                cam_z=Z, delta=delta, alt=alt_f)


def interpolate(face, w, faces, attr):
    """-> (C,H,W) attribute map of the winners, 0 where empty"""
    f = np.asarray(faces)[np.clip(face, 0, None)]
    a = np.asarray(attr, np.float64)[f]                                         # (H,W,3,C)
    return np.moveaxis((a * w[..., None]).sum(2) * (face >= 0)[..., None], -1, 0)
