"""GPU tests of the pose initialiser: the descriptor matcher rnnpose_desc_match_f32, the P3P RANSAC
rnnpose_pnp_ransac_f64 and the plumbing above them (ops, torch.ops.rnnpose, DescriptorPoseInitializer, HipEpoch), against the fp64
numpy restatement tests/pnp_ref.py.

Matcher bounds: a similarity of two unit 32-vectors accumulated in fp32 is within 32 * 2^-24 * sum|a||b| <= 1.9e-6 of its fp64 value,
so the fp64 similarity of a chosen index is >= the fp64 maximum - 4e-6 and the returned value within 2e-6 of fp64 at that index; where
the fp64 top-two gap exceeds 4e-6 the index must equal the restatement's -- the inputs are built so that it does everywhere, which
is asserted on the restatement.  RANSAC: fp64 against fp64, 1e-6 relative, for at least 99 % of the hypotheses (near-double roots).

tests/test_pose_init_on_host.py runs the small cases of this module on the host-executed kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

import pnp_ref as pr

pytestmark = pytest.mark.gpu

H, W, S, D = 64, 96, 2, 32
GAP = 4e-6


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from rnnpose_amd import build, ops as _ops
    build.build()
    return _ops


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def npy(t):
    return t.detach().cpu().numpy()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def guarded(shape, dtype, fill, guard=64):
    """A tensor of `shape` inside a larger buffer filled with `fill`: -> (whole buffer, the view, its guard zones as a function)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype).cuda()
    view = buf[guard:guard + n].view(*shape)
    return buf, view, lambda: torch.cat([buf[:guard], buf[guard + n:]])


CANARY = {torch.float32: -777.0, torch.int32: -777}


def match_outputs(B, M):
    spec = [((B, M, 3), torch.float32), ((B, M, 2), torch.float32), ((B, M), torch.float32), ((B, M), torch.int32), ((B,), torch.int32)]
    g = [guarded(s, dt, CANARY[dt]) for s, dt in spec]
    return tuple(v for _, v, _ in g), [z for _, _, z in g]


def assert_untouched(views, zones, counts=None):
    for v, z in zip(views, zones):
        assert bool((z() == CANARY[v.dtype]).all()), "a guard zone was written"
    if counts is not None:
        for v in views[:4]:
            for b, c in enumerate(counts):
                assert bool((v[b, int(c):] == CANARY[v.dtype]).all()), "a row behind count was written"


# ---- matcher -------------------------------------------------------------------------------------------------------------------------
def matcher_case(P, roi, step, seed):
    """B = 3 objects over S = 2 frames: object 0 (P points) has the box under test in frame 0; object 1 (17 points) a box partly outside
    frame 1 -- or, at step 2, an EMPTY box; object 2 (P points) shares frame 0 with object 0 through another, clipped box.  Every pixel
    descriptor is a noisy copy of a random point descriptor of the frame's first object, so mutual matches exist."""
    rng = np.random.default_rng(seed)
    counts = [P, 17, P]
    off = np.concatenate([[0], np.cumsum(counts)])
    d3 = unit(rng.normal(size=(off[-1], D))).astype(np.float32)
    pts = rng.uniform(-0.1, 0.1, (off[-1], 3)).astype(np.float32)
    d2 = np.zeros((S, D, H, W), np.float32)
    for s, b in ((0, 0), (1, 1)):
        src = d3[off[b]:off[b + 1]][rng.integers(0, counts[b], H * W)]
        d2[s] = unit(src + 0.25 * rng.normal(size=src.shape)).T.reshape(D, H, W)
    rh, rw = roi                                                             # (rows x columns, as the image is 64 x 96)
    x0, y0 = (W - rw) // 2 - 1, (H - rh) // 3
    boxes = np.array([[x0, y0, x0 + rw - 1, y0 + rh - 1], [5, 5, 4, 4] if step == 2 else [W - 9, -6, W + 20, 11], [-3, H - 20, 30, H + 5]], np.int32)
    return dict(d3=d3, pts=pts, off=off, d2=d2, boxes=boxes, src=[0, 1, 0], counts=counts)


def margins_hold(c, step, thresholds):
    """The restatement's own margins on a case: every top-two gap above 4e-6 in both directions, no forward maximum near a threshold."""
    for r in pr.match(c["d3"], c["pts"], c["off"], c["d2"], c["src"], c["boxes"], step, -2.0, False, 0.5, max(c["counts"])):
        if r["S"] is None:
            continue
        rows, cols = np.sort(r["S"], 1)[:, ::-1], np.sort(r["S"], 0)[::-1]
        if any(np.abs(rows[:, 0] - t).min() <= GAP for t in thresholds) or (rows.shape[1] > 1 and (rows[:, 0] - rows[:, 1]).min() <= GAP) or \
                (cols.shape[0] > 1 and (cols[0] - cols[1]).min() <= GAP):
            return False
    return True


def check_match(c, got, ref, min_sim, mutual, M):
    X, x, sim, pidx, count = [npy(t) for t in got]
    for b, r in enumerate(ref):
        n = int(count[b])
        assert n == min(r["total"], M) == r["count"], (b, n, r["total"])
        if r["S"] is None:
            continue
        Sb, Pn = r["S"], r["S"].shape[0]
        # the restatement's own margins: no forward maximum near min_sim, top-two gaps above 4e-6 in both directions
        top = np.sort(Sb, 1)[:, ::-1]
        assert np.abs(top[:, 0] - min_sim).min() > GAP
        if Sb.shape[1] > 1:
            assert (top[:, 0] - top[:, 1]).min() > GAP
        if Pn > 1:
            col = np.sort(Sb, 0)[::-1]
            assert (col[0] - col[1]).min() > GAP
        idx = pidx[b, :n]
        assert np.array_equal(idx, r["point_idx"]) and np.all(np.diff(idx) > 0)
        assert np.array_equal(X[b, :n], c["pts"][c["off"][b]:c["off"][b + 1]][idx])
        assert np.array_equal(x[b, :n], r["x"].astype(np.float32))
        # bounds that hold whatever the gaps: chosen pixel within 4e-6 of the row maximum, returned similarity within 2e-6 of fp64 there
        lin = {(int(u), int(v)): j for j, (u, v) in enumerate(zip(r["u"], r["v"]))}
        j = np.array([lin[(int(px[0] - 0.5), int(px[1] - 0.5))] for px in x[b, :n]], np.int64)
        assert np.all(Sb[idx, j] >= Sb[idx].max(1) - GAP)
        assert np.abs(sim[b, :n].astype(np.float64) - Sb[idx, j]).max(initial=0.0) <= 2e-6
        if mutual:      # kept: the point is its pixel's best within 4e-6; dropped (but above min_sim): it is not the best by more than 4e-6
            assert np.all(Sb[idx, j] >= Sb[:, j].max(0) - GAP)
            dropped = np.setdiff1d(np.nonzero(Sb.max(1) >= min_sim)[0], r["point_idx"]) if r["total"] <= M else np.zeros(0, np.int64)
            for i in dropped if Pn > 1 else ():
                jj = r["fwd"][i]
                assert np.delete(Sb[:, jj], i).max() >= Sb[i, jj] - GAP


@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("roi", [(1, 1), (7, 5), (37, 70), (H, W)])
@pytest.mark.parametrize("P", [1, 33, 642])
def test_matcher_against_fp64(ops, P, roi, step):
    for attempt in range(50):          # the inputs are BUILT so that the fp64 gaps exceed 4e-6 everywhere: the first seed for which they do
        c = matcher_case(P, roi, step, seed=100 * P + 10 * roi[0] + step + 10000 * attempt)
        if margins_hold(c, step, (-2.0, 0.35)):
            break
    M = max(c["counts"])
    for min_sim, mutual in ((-2.0, False), (0.35, True)):
        out, zones = match_outputs(3, M)
        got = ops.desc_match(dev(c["d3"]), dev(c["pts"]), c["off"].tolist(), dev(c["d2"]), c["src"], dev(c["boxes"], np.int32), step=step,
                             min_sim=min_sim, mutual=mutual, pixel_center=0.5, out=out)
        torch.cuda.synchronize()
        ref = pr.match(c["d3"], c["pts"], c["off"], c["d2"], c["src"], c["boxes"], step, min_sim, mutual, 0.5, M)
        check_match(c, got, ref, min_sim, mutual, M)
        assert_untouched(out, zones, npy(got[4]))
        if not mutual and step != 2:
            assert npy(got[4]).tolist() == c["counts"]          # min_sim = -2 keeps every point of an object with a non-empty box
        if step == 2:
            assert int(got[4][1]) == 0                           # the empty box


def test_matcher_duplicates_zero_descriptors_and_capacity(ops):
    """Planted exact duplicates resolve to the lower index in both directions; zero descriptors (rendered background) never pass
    min_sim > 0; M smaller than the survivors keeps the first M in ascending point index."""
    rng = np.random.default_rng(7)
    P = 40
    d3 = unit(rng.normal(size=(P, D))).astype(np.float32)
    d3[23] = d3[4]                                                            # two identical points
    d2 = np.zeros((1, D, H, W), np.float32)                                   # background: zeros
    spots = rng.permutation(H * W)[:P + 1]
    for i, s in enumerate(spots[:P]):
        d2[0, :, s // W, s % W] = d3[i]
    lo, hi = sorted((int(spots[9]), int(spots[P])))
    d2[0, :, lo // W, lo % W] = d3[9]
    d2[0, :, hi // W, hi % W] = d3[9]                                         # two identical pixels (and point 9's own spot)
    d2[0, :, spots[9] // W, spots[9] % W] = d3[9]
    pts = rng.uniform(-0.1, 0.1, (P, 3)).astype(np.float32)
    box = np.array([[0, 0, W - 1, H - 1]], np.int32)
    args = (dev(d3), dev(pts), [0, P], dev(d2), [0], dev(box, np.int32))
    X, x, sim, pidx, count = [npy(t) for t in ops.desc_match(*args, step=1, min_sim=0.5, mutual=False)]
    assert int(count[0]) == P and np.array_equal(pidx[0], np.arange(P))
    assert x[0, 9].tolist() == [lo % W + 0.5, lo // W + 0.5]                  # the lower linear pixel index of the two identical pixels
    assert np.array_equal(x[0, 23], x[0, 4]) and np.abs(sim[0] - 1.0).max() < 2e-6
    ref = pr.match(d3, pts, [0, P], d2, [0], box, 1, 0.5, True, 0.5, P)[0]
    X, x, sim, pidx, count = [npy(t) for t in ops.desc_match(*args, step=1, min_sim=0.5, mutual=True)]
    assert pidx[0, :int(count[0])].tolist() == ref["point_idx"].tolist() == [i for i in range(P) if i != 23]      # pixel of 4 / 23: the lower point
    # zero descriptors: points that match only background have similarity 0 and never pass a positive threshold
    d2z = d2.copy()
    for i in (3, 11):
        s = spots[i]
        d2z[0, :, s // W, s % W] = 0.0
    args_z = (dev(d3), dev(pts), [0, P], dev(d2z), [0], dev(box, np.int32))
    pidx, count = [npy(t) for t in ops.desc_match(*args_z, step=1, min_sim=0.9, mutual=False)[3:]]
    assert pidx[0, :int(count[0])].tolist() == [i for i in range(P) if i not in (3, 11)]
    pidx, count = [npy(t) for t in ops.desc_match(dev(d3), dev(pts), [0, P], dev(np.zeros_like(d2)), [0], dev(box, np.int32), step=1, min_sim=1e-30, mutual=False)[3:]]
    assert int(count[0]) == 0
    # capacity
    out, zones = match_outputs(1, 5)
    got = ops.desc_match(*args, step=1, min_sim=0.5, mutual=False, M=5, out=out)
    assert int(got[4][0]) == 5 and npy(got[3])[0].tolist() == [0, 1, 2, 3, 4]
    assert_untouched(out, zones)


def test_matcher_reruns_and_batch_independence(ops):
    c = matcher_case(33, (30, 37), 2, seed=5)
    c["boxes"][1] = [W - 9, -6, W + 20, 11]
    a = (dev(c["d3"]), dev(c["pts"]), c["off"].tolist(), dev(c["d2"]), c["src"], dev(c["boxes"], np.int32))
    kw = dict(step=2, min_sim=0.35, mutual=True, pixel_center=0.25)
    one = ops.desc_match(*a, **kw)
    two = ops.desc_match(*a, **kw)
    assert all(torch.equal(p, q) for p, q in zip(one, two)) and int(one[4].sum()) > 10
    M = one[0].shape[1]
    for b in range(3):                                                        # every object alone == the object in the batch
        lo, hi = int(c["off"][b]), int(c["off"][b + 1])
        alone = ops.desc_match(dev(c["d3"][lo:hi]), dev(c["pts"][lo:hi]), [0, hi - lo], dev(c["d2"]), [c["src"][b]], dev(c["boxes"][b:b + 1], np.int32),
                               M=M, **kw)
        assert all(torch.equal(p[0], q[b]) for p, q in zip(alone, one))
    with pytest.raises(ValueError):
        ops.desc_match(*a[:4], [0, 2, 0], a[5], **kw)                         # index outside [0, S): refused on the host
    with pytest.raises(ValueError):
        ops.desc_match(a[0], a[1], [0, 40, 30, 67], a[3], a[4], a[5], **kw)   # offsets not ascending
    with pytest.raises(ValueError):
        ops.desc_match(a[0][:, :16].contiguous(), *a[1:], **kw)               # D != 32


def test_matcher_bad_arguments_return_1_and_write_nothing(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    c = matcher_case(33, (7, 5), 1, seed=6)
    d3, pts, off, d2, src, box = dev(c["d3"]), dev(c["pts"]), dev(c["off"], np.int32), dev(c["d2"]), dev(c["src"], np.int32), dev(c["boxes"], np.int32)
    total, M = int(c["off"][-1]), 33
    n = int(lib.rnnpose_desc_match_workspace_bytes(total, 3, H, W, 1))
    assert n == 8 * (total + 3 * H * W) and lib.rnnpose_desc_match_workspace_bytes(total, 3, H, W, 0) == 0
    assert lib.rnnpose_desc_match_workspace_bytes(total, 3, H, W, 3) == 8 * (total + 3 * 22 * 32)
    ws = torch.zeros(n // 8, dtype=torch.int64).cuda()
    out, zones = match_outputs(3, M)
    good = dict(desc3d=ptr(d3), points=ptr(pts), pt_off=ptr(off), total=total, maxp=33, desc2d=ptr(d2), S=S, D=D, H=H, W=W, src=ptr(src), bbox=ptr(box),
                B=3, step=1, min_sim=0.3, mutual=1, pc=0.5, M=M, ws=ptr(ws), n=n, X=ptr(out[0]), x=ptr(out[1]), sim=ptr(out[2]), idx=ptr(out[3]),
                count=ptr(out[4]), stream=None)
    bad = [dict(desc3d=None), dict(points=None), dict(pt_off=None), dict(desc2d=None), dict(src=None), dict(bbox=None), dict(ws=None), dict(X=None),
           dict(x=None), dict(sim=None), dict(idx=None), dict(count=None), dict(D=16), dict(D=64), dict(B=0), dict(S=0), dict(H=0), dict(W=-1),
           dict(total=0), dict(maxp=0), dict(maxp=total + 1), dict(M=0), dict(step=0), dict(mutual=2), dict(n=n - 8), dict(desc3d=C.c_void_p(d3.data_ptr() + 4))]
    for change in bad:
        assert lib.rnnpose_desc_match_f32(*dict(good, **change).values()) == 1, change
        assert len(lib.rnnpose_last_error()) > 0
    torch.cuda.synchronize()
    assert_untouched(out, zones, [0, 0, 0])
    assert not bool(ws.any())
    assert lib.rnnpose_desc_match_f32(*good.values()) == 0
    torch.cuda.synchronize()
    assert int(out[4].sum()) > 0
    # an index outside [0, S) handed straight to the library: count = 0, nothing else written, the call returns 0
    out, zones = match_outputs(3, M)
    src2 = dev([0, 7, -1], np.int32)
    assert lib.rnnpose_desc_match_f32(*dict(good, src=ptr(src2), X=ptr(out[0]), x=ptr(out[1]), sim=ptr(out[2]), idx=ptr(out[3]), count=ptr(out[4])).values()) == 0
    torch.cuda.synchronize()
    assert npy(out[4])[1:].tolist() == [0, 0] and int(out[4][0]) > 0
    assert_untouched(out, zones, npy(out[4]))


# ---- P3P per hypothesis ----------------------------------------------------------------------------------------------------------------
def test_p3p_hypotheses_on_noise_free_data(ops):
    """100 scenes x 200 random triples (tests/pnp_ref.p3p_scenes, numpy seed 0), noise-free up to the fp32 rounding of the inputs: of
    the hypotheses with three distinct indices, at least 99 % must have a best candidate that reprojects all 64 points within 1e-3 px
    (cost < 64e-6 and 64 inliers at tau = 1).  The CPU figure of the same arithmetic (csrc/pnp_math.cuh behind a shim) on these inputs:
    0.87 % missed, all of them from the fp32 rounding of the image points (none with fp64 image points)."""
    X, x, rnd, _ = pr.p3p_scenes()
    B, Hyp = rnd.shape[:2]
    K = np.tile(pr.P3P_K, (B, 1, 1))
    count = torch.full((B,), 64, dtype=torch.int32).cuda()
    out = ops.pnp_ransac(dev(X), dev(x), count, dev(K), dev(rnd.astype(np.int64), np.int64), tau=1.0, n_polish=0)
    cost, inl = npy(out[1]), npy(out[2])
    i = rnd % 64
    distinct = (i[..., 0] != i[..., 1]) & (i[..., 0] != i[..., 2]) & (i[..., 1] != i[..., 2])
    assert np.isinf(cost[~distinct]).all() and (inl[~distinct] == 0).all() and (~distinct).sum() > 100
    good = (cost < 64e-6) & (inl == 64)
    share = 1.0 - good[distinct].mean()
    print(f"P3P: {distinct.sum()} hypotheses with distinct indices, {100 * share:.2f} % without a pose that reprojects all points within 1e-3 px")
    assert share <= 0.01
    assert (npy(out[7]) == 0).all() and (npy(out[5]) == 64).all()           # every scene: the best hypothesis has all 64 inliers
    again = ops.pnp_ransac(dev(X), dev(x), count, dev(K), dev(rnd.astype(np.int64), np.int64), tau=1.0, n_polish=0)
    assert all(torch.equal(p, q) for p, q in zip(out, again))


# ---- RANSAC against the restatement -----------------------------------------------------------------------------------------------------
RANSAC_SEED = 0
TAU = 4.0


def ransac_case(seed):
    """B = 3 objects with 4, 57 and 300 correspondences, half of them inliers with 0.5 px Gaussian noise, half outliers uniform in a
    120 x 120 px box; everything rounded to fp32 first; Hyp = 256."""
    rng = np.random.default_rng(seed)
    counts, M, Hyp = [4, 57, 300], 300, 256
    X, x = np.zeros((3, M, 3), np.float32), np.zeros((3, M, 2), np.float32)
    K = np.tile(pr.P3P_K, (3, 1, 1)).astype(np.float32)
    for b, n in enumerate(counts):
        Xb = rng.uniform(-0.1, 0.1, (n, 3))
        R, _ = pr.se3_exp(np.concatenate([np.zeros(3), rng.normal(0, 1, 3)]))
        t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)])
        uv = pr.project(R, t, pr.P3P_K, Xb)[0] + rng.normal(0, 0.5, (n, 2))
        out = rng.permutation(n)[:n // 2]
        c = pr.project(R, t, pr.P3P_K, np.zeros((1, 3)))[0][0]
        uv[out] = c + rng.uniform(-60, 60, (len(out), 2))
        X[b, :n], x[b, :n] = Xb, uv
    rnd = rng.integers(0, 2 ** 32, (3, Hyp, 3), dtype=np.uint64)
    return X, x, np.array(counts, np.int32), K, rnd


@pytest.fixture(scope="module")
def ransac_ref():
    X, x, counts, K, rnd = ransac_case(RANSAC_SEED)
    ref = pr.ransac(X, x, counts, K.astype(np.float64), rnd, TAU, 4)
    for r in ref:                      # the pinned seed: no residual of the final pose within 1e-3 px of tau
        assert r["info"] == 0 and np.abs(np.sqrt(r["r2_final"][np.isfinite(r["r2_final"])]) - TAU).min() > 1e-3
    return (X, x, counts, K, rnd), ref


def test_ransac_against_the_restatement(ops, ransac_ref):
    (X, x, counts, K, rnd), ref = ransac_ref
    Tc = torch.full((3, 4, 4), -777.0).cuda()
    T, cost, inl, best, mask, n_inl, fcost, info = [npy(t) for t in ops.pnp_ransac(dev(X), dev(x), dev(counts, np.int32), dev(K),
                                                                                   dev(rnd.astype(np.int64), np.int64), tau=TAU, n_polish=4, T=Tc)]
    for b, r in enumerate(ref):
        n = int(counts[b])
        fin = np.isfinite(r["cost"])
        assert np.array_equal(np.isfinite(cost[b]), fin) or np.mean(np.isfinite(cost[b]) != fin) <= 0.01
        both = fin & np.isfinite(cost[b])
        close = both.copy()
        close[both] = np.abs(cost[b][both] - r["cost"][both]) <= 1e-6 * np.abs(r["cost"][both])
        agree = close | (~fin & ~np.isfinite(cost[b]))
        print(f"object {b}: {fin.sum()} hypotheses with a pose, cost agrees on {agree.mean() * 100:.2f} %")
        assert agree.mean() >= 0.99
        assert np.array_equal(inl[b][close], r["inliers"][close]) and (inl[b][~np.isfinite(cost[b])] == 0).all()
        i = rnd[b] % np.uint64(n)
        repeated = (i[:, 0] == i[:, 1]) | (i[:, 0] == i[:, 2]) | (i[:, 1] == i[:, 2])
        assert np.isinf(cost[b][repeated]).all()
        two = np.sort(r["cost"])[:2]
        if two[1] - two[0] > 1e-6 * two[0]:
            assert best[b] == r["best"]
        assert info[b] == 0 and np.array_equal(mask[b, :n].astype(bool), r["inlier_mask"]) and not mask[b, n:].any()
        assert n_inl[b] == r["n_inliers"] and abs(fcost[b] - r["final_cost"]) <= 1e-6 * r["final_cost"]
        assert np.abs(T[b, :3, :3] - r["T"][:3, :3]).max() <= 1e-6 and np.abs(T[b, :3, 3] - r["T"][:3, 3]).max() <= 1e-6
        assert T[b, 3].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_ransac_edge_cases(ops, ransac_ref):
    (X, x, counts, K, rnd), _ = ransac_ref
    a = (dev(X), dev(x))
    rw = dev(rnd.astype(np.int64), np.int64)
    # count 0 and 3 (below min_count) -> info -1, T untouched; a count beyond M is clamped to M
    Tc = torch.full((3, 4, 4), -777.0).cuda()
    out = ops.pnp_ransac(*a, dev([0, 3, 100000], np.int32), dev(K), rw, tau=TAU, n_polish=2, T=Tc)
    T, cost, inl, best, mask, n_inl, fcost, info = [npy(t) for t in out]
    assert info.tolist() == [-1, -1, 0] and (T[:2] == -777.0).all() and np.isfinite(T[2]).all()
    assert np.isinf(cost[:2]).all() and (inl[:2] == 0).all() and best[:2].tolist() == [-1, -1] and n_inl[:2].tolist() == [0, 0]
    assert np.isinf(fcost[:2]).all() and not mask[:2].any()
    # all-collinear points: info -1 or a finite pose, never NaN
    line = np.zeros_like(X)
    line[:] = np.linspace(-0.1, 0.1, X.shape[1])[None, :, None] * np.array([1.0, 0.4, -0.3])
    xl = np.stack([pr.project(np.eye(3), np.array([0.0, 0.0, 0.8]), pr.P3P_K, line[b].astype(np.float64))[0] for b in range(3)]).astype(np.float32)
    Tc = torch.full((3, 4, 4), -777.0).cuda()
    T, cost, _, _, _, _, fcost, info = [npy(t) for t in ops.pnp_ransac(dev(line), dev(xl), dev(counts, np.int32), dev(K), rw, tau=TAU, n_polish=4, T=Tc)]
    assert not np.isnan(cost).any() and not np.isnan(T).any() and not np.isnan(fcost).any()
    for b in range(3):
        assert (info[b] == -1 and (T[b] == -777.0).all()) or (info[b] == 0 and np.isfinite(T[b]).all())
    # reruns are bit-identical
    cnt = dev(counts, np.int32)
    one = ops.pnp_ransac(*a, cnt, dev(K), rw, tau=TAU, n_polish=4)
    two = ops.pnp_ransac(*a, cnt, dev(K), rw, tau=TAU, n_polish=4)
    assert all(torch.equal(p, q) for p, q in zip(one, two))
    for bad in (dict(tau=0.0), dict(tau=float("nan")), dict(n_polish=-1), dict(min_count=3)):
        with pytest.raises(ValueError):
            ops.pnp_ransac(*a, cnt, dev(K), rw, **bad)
    with pytest.raises(ValueError):
        ops.pnp_ransac(*a, cnt, dev(K), rw[:2])


def test_torch_ops_equal_ops_and_have_fake_kernels(ops, ransac_ref):
    """torch.ops.rnnpose.desc_match / pnp_ransac: the dispatcher operators give what ops gives, and their fake kernels its shapes and dtypes."""
    import rnnpose_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    c = matcher_case(33, (30, 37), 2, seed=5)
    a = (dev(c["d3"]), dev(c["pts"]), torch.tensor(c["off"]), dev(c["d2"]), torch.tensor(c["src"]), dev(c["boxes"], np.int32))
    want = ops.desc_match(a[0], a[1], c["off"].tolist(), a[3], c["src"], a[5], step=2, min_sim=0.35, mutual=True, pixel_center=0.25, M=a[1].shape[0])
    got = torch.ops.rnnpose.desc_match(*a, 2, 0.35, True, 0.25, 0)
    assert all(torch.equal(p, q) for p, q in zip(got, want)) and int(got[4].sum()) > 10
    (X, x, counts, K, rnd), _ = ransac_ref
    b = (dev(X), dev(x), dev(counts, np.int32), dev(K), dev(rnd.astype(np.int64), np.int64))
    want2 = ops.pnp_ransac(*b, tau=TAU, n_polish=4)
    got2 = torch.ops.rnnpose.pnp_ransac(*b, TAU, 4, 4)
    assert all(torch.equal(p, q) for p, q in zip(got2, want2))
    with FakeTensorMode():
        e = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="cuda", dtype=dtype)
        f = torch.ops.rnnpose.desc_match(e(83, 32), e(83, 3), e(4, dtype=torch.int64), e(2, 32, H, W), e(3, dtype=torch.int64), e(3, 4, dtype=torch.int32))
        assert [(tuple(t.shape), t.dtype) for t in f] == [(tuple(t.shape), t.dtype) for t in got]
        f = torch.ops.rnnpose.pnp_ransac(e(3, 300, 3), e(3, 300, 2), e(3, dtype=torch.int32), e(3, 3, 3), e(3, 256, 3, dtype=torch.int64))
        assert [(tuple(t.shape), t.dtype) for t in f] == [(tuple(t.shape), t.dtype) for t in got2]


def test_ransac_bad_arguments_return_1_and_write_nothing(ops, ransac_ref):
    from rnnpose_amd import _lib
    lib = _lib.load()
    (X, x, counts, K, rnd), _ = ransac_ref
    B, M, Hyp = 3, X.shape[1], rnd.shape[1]
    Xd, xd, cd, Kd, rd = dev(X), dev(x), dev(counts, np.int32), dev(K), ops.random_words(dev(rnd.astype(np.int64), np.int64))
    n = int(lib.rnnpose_pnp_ransac_workspace_bytes(B, Hyp))
    assert n == B * Hyp * 392 and lib.rnnpose_pnp_ransac_workspace_bytes(0, Hyp) == 0
    ws = torch.zeros(n // 8, dtype=torch.int64).cuda()
    outs = dict(T=torch.full((B, 4, 4), -777.0).cuda(), cost=torch.full((B, Hyp), -777.0, dtype=torch.float64).cuda(),
                inl=torch.full((B, Hyp), -777, dtype=torch.int32).cuda(), best=torch.full((B,), -777, dtype=torch.int32).cuda(),
                mask=torch.full((B, M), 77, dtype=torch.uint8).cuda(), n_inl=torch.full((B,), -777, dtype=torch.int32).cuda(),
                fcost=torch.full((B,), -777.0, dtype=torch.float64).cuda(), info=torch.full((B,), -777, dtype=torch.int32).cuda())
    good = dict(X=ptr(Xd), x=ptr(xd), count=ptr(cd), M=M, K=ptr(Kd), rnd=ptr(rd), B=B, Hyp=Hyp, tau=TAU, n_polish=2, min_count=4, ws=ptr(ws), n=n,
                **{k: ptr(v) for k, v in outs.items()}, stream=None)
    bad = [dict(X=None), dict(x=None), dict(count=None), dict(K=None), dict(rnd=None), dict(ws=None)] + [{k: None} for k in outs] + \
          [dict(B=0), dict(M=0), dict(Hyp=0), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(n_polish=-1), dict(n_polish=65), dict(min_count=3),
           dict(n=n - 8)]
    for change in bad:
        assert lib.rnnpose_pnp_ransac_f64(*dict(good, **change).values()) == 1, change
    torch.cuda.synchronize()
    assert all(bool((v == (77 if v.dtype == torch.uint8 else -777)).all()) for v in outs.values()) and not bool(ws.any())
    assert lib.rnnpose_pnp_ransac_f64(*good.values()) == 0
    torch.cuda.synchronize()
    assert npy(outs["info"]).tolist() == [0, 0, 0]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(ops):
    from oracle import rnnpose_oracle as orc
    from rnnpose_amd import eval_epoch as ee, synthetic as syn
    from rnnpose_amd.pose_refiner import default_config
    torch.manual_seed(0)
    models = ee.synthetic_models(sub=3)
    cfg = default_config(RENDER_ITER_COUNT=1, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=(240, 320), zoom_crop_size=(128, 128))
    hip = ee.HipEpoch(models, cfg=cfg, init="descriptors")
    Tt = lambda v: torch.from_numpy(v)
    hip.refiner.cf_net.update_block.load_state_dict({k: Tt(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
    hip.refiner.image_fea_enc.fnet.load_state_dict({k: Tt(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
    items = ee.synthetic_scenes(models, 1, 3, image_size=(240, 320), renderer=hip.renderer)
    names = [it.class_name for it in items]
    Tg = dev(np.stack([it.pose_gt for it in items]))
    K = dev(np.stack([it.K for it in items]))
    depth = hip.renderer.render_zbuf(names, Tg, K, (240, 320))
    boxes = npy(ops.mask_bbox(depth.float().contiguous())) + np.array([-8, -8, 8, 8], np.int32)
    for it, bb in zip(items, boxes):
        it.bbox = bb
    return hip, models, items, boxes


def check_scene_match(r, idx, xk, simk, Xk, pts, min_sim, pixel_center):
    """The kernel's matches of ONE object (idx, xk, simk, Xk: its compacted rows) against the restatement's record r on a map whose gaps
    nobody built (mutual matching): the bounds of the grid test.  A point is CLEAR when its fp64 row maximum is below min_sim by more
    than 4e-6 (both sides drop it), or when it is above by more than 4e-6 and the top-two gaps of its row and of its best pixel's
    column exceed 4e-6: there the kept set and the pixel must EQUAL the restatement's.  Whatever the gaps: the chosen pixel within 4e-6
    of the row maximum, the point within 4e-6 of its pixel's column maximum, the similarity within 2e-6 of fp64.  With every point
    clear the matches are identical.  -> (identical, number of points that are not clear)."""
    Sb, fwd = r["S"], r["fwd"]
    P = Sb.shape[0]
    rows = np.sort(Sb, 1)[:, ::-1]
    rowmax, rowgap = rows[:, 0], rows[:, 0] - rows[:, 1]
    col = np.sort(Sb[:, fwd], 0)[::-1]                       # the column of every point's best pixel
    clear = (rowmax < min_sim - GAP) | ((rowmax > min_sim + GAP) & (rowgap > GAP) & (col[0] - col[1] > GAP))
    kept, kept_ref = np.zeros(P, bool), np.zeros(P, bool)
    kept[idx], kept_ref[r["point_idx"]] = True, True
    assert r["total"] == r["count"] and np.array_equal(kept[clear], kept_ref[clear])
    assert np.all(np.diff(idx) > 0) and np.array_equal(Xk, pts[idx])
    lin = {(int(u), int(v)): j for j, (u, v) in enumerate(zip(r["u"], r["v"]))}
    j = np.array([lin[(int(round(px[0] - pixel_center)), int(round(px[1] - pixel_center)))] for px in xk], np.int64)
    assert np.all(Sb[idx, j] >= rowmax[idx] - GAP) and np.all(Sb[idx, j] >= Sb[:, j].max(0) - GAP) and np.all(Sb[idx, j] >= min_sim - GAP)
    sure = rowgap[idx] > GAP
    assert np.array_equal(j[sure], fwd[idx][sure])
    assert np.abs(simk.astype(np.float64) - Sb[idx, j]).max(initial=0.0) <= 2e-6
    same = np.array_equal(idx, r["point_idx"]) and np.array_equal(xk, r["x"].astype(np.float32))
    unclear = int((~clear).sum())
    assert abs(len(idx) - r["count"]) <= unclear and (same or unclear > 0)
    return same, unclear


def test_end_to_end_initial_poses_from_the_rendered_descriptors(ops, scene):
    """Matching the rendered descriptor map back against the models returns the poses it was rendered at.  The matcher on the rendered
    map -- 642 points per object, boxes clamped to the image, step 2, the path HipEpoch takes -- is held to the restatement on the same
    map by check_scene_match; RANSAC and polish to the restatement run on the RESTATEMENT's matches wherever the two are identical (the
    kernel's own where a point is not clear) with the same random words: best equal, T within 1e-5; and every object's ADD against
    pose_gt is below 0.1 diameter, the project's LINEMOD criterion (evaluator.py).  The observed values are printed for the record."""
    import dataclasses
    hip, models, items, boxes = scene
    assert hip.init.pixel_center == hip.renderer.pixel_center
    T0 = npy(hip.initial_poses(items))
    rec = hip.last_init_info
    assert rec["info"].tolist() == [0, 0, 0] and not rec["fallback"].any() and rec["rows"].tolist() == [0, 1, 2]
    names = [it.class_name for it in items]
    g2 = items[0].geofea_2d.cuda()[None]
    X, x, sim, pidx, count = [npy(t) for t in hip.init.match(names, g2, [0, 0, 0], dev(boxes, np.int32))]
    rnd = npy(hip.init.random_words(3)).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum([models[n].verts.shape[0] for n in names])])
    d3 = np.concatenate([npy(models[n].geofea_3d[0]) for n in names])
    pts = np.concatenate([models[n].verts for n in names])
    mref = pr.match(d3, pts, off, npy(g2), [0, 0, 0], boxes, hip.init.step, hip.init.min_sim, hip.init.mutual, hip.init.pixel_center, 642)
    Xr, xr, cr = X.astype(np.float64), x.astype(np.float64), count.copy()
    for b in range(3):
        n, r = int(count[b]), mref[b]
        same, unclear = check_scene_match(r, pidx[b, :n], x[b, :n], sim[b, :n], X[b, :n], pts[off[b]:off[b + 1]], hip.init.min_sim, hip.init.pixel_center)
        print(f"object {b} ({names[b]}): {n} matches of {off[b + 1] - off[b]} points in {r['u'].size} box pixels, {unclear} points not clear, "
              f"identical to the restatement's: {same}")
        if same:                                             # the reference then runs on the restatement's own matches
            Xr[b, :n], xr[b, :n], cr[b] = r["X"], r["x"], r["count"]
    K = np.stack([it.K for it in items]).astype(np.float64)
    ref = pr.ransac(Xr, xr, cr, K, rnd, hip.init.tau, hip.init.n_polish)
    _, cost, _, best, _, n_inl, _, _ = [npy(t) for t in ops.pnp_ransac(dev(X), dev(x), dev(count, np.int32), dev(K), dev(rnd.astype(np.int64), np.int64),
                                                                      hip.init.tau, hip.init.n_polish)]
    for b, it in enumerate(items):
        assert best[b] == ref[b]["best"] and np.abs(T0[b] - ref[b]["T"]).max() <= 1e-5
        v = models[it.class_name].verts.astype(np.float64)
        add = np.linalg.norm((v @ T0[b, :3, :3].T + T0[b, :3, 3]) - (v @ it.pose_gt[:3, :3].T.astype(np.float64) + it.pose_gt[:3, 3]), axis=1).mean()
        print(f"object {b}: {count[b]} matches, {n_inl[b]} inliers, ADD {add * 1e3:.3f} mm = {add / models[it.class_name].diameter:.4f} diameter")
        assert add < 0.1 * models[it.class_name].diameter
    # refine_frame on items without a pose == refine_frame on the same items with pose_init = initial_poses(items)
    bare = [dataclasses.replace(it, pose_init=None) for it in items]
    given = [dataclasses.replace(it, pose_init=T0[b].copy(), bbox=None) for b, it in enumerate(items)]
    hip.last_init_info = None
    p_given = hip.refine_frame(given)
    assert hip.last_init_info is None                                           # with every pose_init given, nothing new runs
    p_bare = hip.refine_frame(bare)
    assert torch.equal(p_bare, p_given) and hip.last_init_info["rows"].tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        hip.refine_frame([bare[0], dataclasses.replace(bare[1], bbox=None), bare[2]])
    # an empty box: the box-centre fallback, reported, not raised
    empty = [bare[0], dataclasses.replace(bare[1], bbox=np.array([30, 30, 20, 20], np.int32)), bare[2]]
    Te = npy(hip.initial_poses(empty))
    rec = hip.last_init_info
    assert rec["info"].tolist() == [0, -1, 0] and rec["fallback"].tolist() == [False, True, False] and rec["count"][1] == 0
    assert np.array_equal(Te[0], T0[0]) and np.array_equal(Te[2], T0[2])        # the others do not depend on it
    want = pr.fallback_pose(items[1].K, [30, 30, 20, 20], models[names[1]].diameter, (240, 320), hip.init.pixel_center)     # = the whole image
    assert np.abs(Te[1] - want).max() <= 1e-6 and np.array_equal(Te[1, :3, :3], np.eye(3, dtype=np.float32)) and 0.2 < Te[1, 2, 3] < 0.3
    # a box on the background, partly outside the image: no match passes min_sim, the fallback sits at the centre of the CLAMPED box
    corner = np.array([-4, -6, 9, 7], np.int32)
    Tc = npy(hip.initial_poses([bare[0], bare[1], dataclasses.replace(bare[2], bbox=corner)]))
    rec = hip.last_init_info
    assert rec["info"].tolist() == [0, 0, -1] and rec["fallback"].tolist() == [False, False, True] and rec["count"][2] < 4
    want = pr.fallback_pose(items[2].K, corner, models[names[2]].diameter, (240, 320), hip.init.pixel_center)
    assert np.abs(Tc[2] - want).max() <= 1e-6 * max(1.0, np.abs(want).max()) and np.array_equal(Tc[:2], T0[:2])


def test_end_to_end_class_batches_and_multi_view_groups(ops, scene):
    """The other two callers of the start poses: `refine` (one class per batch) on an item without a pose == the same item with
    pose_init = initial_poses; a multi-view group (two views through the same camera, E = I) whose views bring no pose: only the FIRST
    view is initialised (one row in the record), the second is tied to it by the rig, and the result equals the run with that pose given."""
    import dataclasses
    hip, models, items, boxes = scene
    T0 = npy(hip.initial_poses(items))
    whole = hip.last_init_info
    bare = [dataclasses.replace(it, pose_init=None) for it in items]
    given = [dataclasses.replace(it, pose_init=T0[b].copy(), bbox=None) for b, it in enumerate(items)]
    assert torch.equal(hip.refine(bare[1].class_name, [bare[1]]), hip.refine(given[1].class_name, [given[1]]))
    with pytest.raises(ValueError):
        hip.refine(bare[1].class_name, [dataclasses.replace(bare[1], bbox=None)])
    eye = np.eye(4, dtype=np.float32)
    views = lambda src: [dataclasses.replace(src[0], object_id="a", cam_from_rig=eye), dataclasses.replace(src[2], object_id="c", cam_from_rig=eye),
                         dataclasses.replace(src[0], object_id="a", cam_from_rig=eye)]
    hip.last_init_info = None
    p_bare = hip.refine_frame(views(bare))
    rec = hip.last_init_info                                      # rows of the CALLER's batch: the first view of "a" and the only view of "c"
    assert rec["rows"].tolist() == [0, 1] and rec["info"].tolist() == [0, 0]
    assert rec["count"].tolist() == whole["count"][[0, 2]].tolist() and rec["n_inliers"].tolist() == whole["n_inliers"][[0, 2]].tolist()      # each row's record is its own object's
    p_given = hip.refine_frame(views(given))
    assert torch.equal(p_bare, p_given) and torch.equal(p_bare[0], p_bare[2])
