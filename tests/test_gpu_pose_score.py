"""GPU tests of the pose confidence: the kernel pair behind rnnpose_pose_score_f64 and the plumbing above it
(ops.pose_score, torch.ops.rnnpose.pose_score, pose_score.PoseScorer, HipEpoch.score_poses / select_poses / score=) against the fp64
numpy restatement tests/score_ref.py.

Bounds.  The classification is exact in fp64 on both sides (fp32 inputs, one subtraction, comparisons), so the eight counts are EQUAL.
Every term of sum_cos carries about 40 fp64 roundings (3 x 32 products and sums, two roots, a product, a quotient): < 5e-15; any
summation order of n terms of magnitude <= 1 adds at most n u sum|term| <= 1.2e-16 n^2, 7e-13 n at the largest window (n <= 6144):
sums within 1e-12 * max(n, 1) absolute, the score within 1e-12.

tests/test_pose_score_on_host.py runs every case of this module except the end-to-end and torch_ops ones on the host-executed kernels."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import score_ref as sr

pytestmark = pytest.mark.gpu

H, W, S, D = 40, 56, 2, 32
COL = {k: j for j, k in enumerate(sr.COLUMNS)}
COUNTS = [0, 1, 2, 3, 4, 5, 6, 9]
CANARY = -777.0
WINDOWS = [(1, 1), (7, 5), (37, 70), (64, 96)]
PLACEMENTS = ["inside", "top_left", "bottom_right", "outside"]


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


def guarded(n, guard=64):
    """n doubles inside a larger buffer filled with the canary -> (the view, its guard zones as a function)"""
    buf = torch.full((n + 2 * guard,), CANARY, dtype=torch.float64).cuda()
    return buf[guard:guard + n], lambda: torch.cat([buf[:guard], buf[guard + n:]])


def corners(h, w, placement):
    """window corners (x0, y0) of the three poses"""
    if placement == "inside":                     # (as far inside as the window fits: 37x70 and 64x96 are wider than the frame)
        x0, y0 = (W - w) // 2, (H - h) // 2
        return [[x0, y0], [x0 + 1, y0 - 1 if h < H else y0 + 1], [max(x0 - 2, 0) if w < W else x0 - 2, y0 + 2]]
    if placement == "top_left":                   # negative x0 / y0
        return [[-(w // 2) - 1, -(h // 2) - 1], [-(w // 3) - 1, 2], [3, -(h // 2) - 2]]
    if placement == "bottom_right":
        return [[W - (w + 1) // 2, H - (h + 1) // 2], [W - 1 - w // 3, 1], [2, H - 1 - h // 4]]
    return [[W + 3, 2], [-w - 1, 5], [2, H]]      # fully outside: right of, left of, below the frame


@functools.lru_cache(maxsize=None)
def grid_case(h, w, placement):
    """B = 3 poses over S = 2 frames (poses 0 and 2 share frame 0): random descriptors, not normalised; about 30 % of the rendered
    depths empty (-1, 0, NaN, +Inf), about 20 % of the observed depths holes (0, negative, NaN, Inf).  With its restatement, computed
    once for the tests that share the case."""
    rng = np.random.default_rng(1000 * h + 10 * w + PLACEMENTS.index(placement))
    B = 3
    z = rng.uniform(0.4, 0.6, (B, h, w)).astype(np.float32)
    empty = rng.random(z.shape) < 0.3
    z[empty] = rng.choice(np.array([-1.0, 0.0, np.nan, np.inf], np.float32), int(empty.sum()))
    if h * w == 1:
        z[:] = [[[0.5]], [[0.45]], [[-1.0]]]                                  # one lane: two rendered pixels and an empty one
    a = (rng.normal(size=(B, D, h, w)) * rng.uniform(0.1, 4.0, (B, 1, h, w))).astype(np.float32)
    g = (rng.normal(size=(S, D, H, W)) * rng.uniform(0.1, 4.0, (S, 1, H, W))).astype(np.float32)
    if h * w > 1:                                                             # a few non-finite channels on either side: n_bad
        a[rng.random(a.shape) < 0.002] = np.nan
        g[rng.random(g.shape) < 0.002] = np.inf
    d = rng.uniform(0.4, 0.6, (S, H, W)).astype(np.float32)
    holes = rng.random(d.shape) < 0.2
    d[holes] = rng.choice(np.array([0.0, -0.3, np.nan, np.inf], np.float32), int(holes.sum()))
    window = np.array(corners(h, w, placement), np.int32)
    src = [0, 1, 0]
    c = dict(z=z, a=a, g=g, d=d, window=window, src=src, tol=0.03)
    c["ref"] = {False: sr.pose_score(z, a, window, g, None, src, c["tol"]), True: sr.pose_score(z, a, window, g, d, src, c["tol"])}
    return c


def raw_call(lib, c, with_depth, tol=None, rows=None):
    """rnnpose_pose_score_f64 straight from the library on guarded outputs and a guarded workspace -> stats, score (numpy), after the
    canaries around all three were checked.  rows: the poses to score (None: all)."""
    rows = list(range(len(c["src"]))) if rows is None else rows
    B, (h, w) = len(rows), c["z"].shape[1:]
    n = int(lib.rnnpose_pose_score_workspace_bytes(B, h, w))
    assert n == B * -(-h * w // 256) * 10 * 8
    ws, ws_zone = guarded(n // 8)
    stats, st_zone = guarded(B * 10)
    score, sc_zone = guarded(B)
    t = [dev(c["z"][rows]), dev(c["a"][rows]), dev(c["window"][rows], np.int32), dev(c["g"]), dev(c["d"]) if with_depth else None,
         dev(np.asarray(c["src"])[rows], np.int32)]
    r = lib.rnnpose_pose_score_f64(*[ptr(x) for x in t], B, S, D, h, w, H, W, float(c["tol"] if tol is None else tol), ptr(ws), n, ptr(stats),
                                   ptr(score), None)
    torch.cuda.synchronize()
    assert r == 0
    for zone in (ws_zone, st_zone, sc_zone):
        assert bool((zone() == CANARY).all()), "a guard zone was written"
    assert bool((ws != CANARY).all()), "a used workspace row was not written"
    return npy(stats).reshape(B, 10).copy(), npy(score).copy()


def check(got, ref, tag=""):
    (stats, score), (rstats, rscore) = got, ref
    print(f"{tag}: counts {stats[:, COUNTS].astype(np.int64).tolist()}  max |sum_cos err| {np.abs(stats[:, 7] - rstats[:, 7]).max():.3e}  "
          f"max |sum_dd err| {np.abs(stats[:, 8] - rstats[:, 8]).max():.3e}  max |score err| {np.abs(score - rscore).max():.3e}")
    assert np.array_equal(stats[:, COUNTS], rstats[:, COUNTS]), (stats[:, COUNTS], rstats[:, COUNTS])
    assert np.all(np.abs(stats[:, 7] - rstats[:, 7]) <= 1e-12 * np.maximum(rstats[:, COL["n_desc"]], 1.0))
    assert np.all(np.abs(stats[:, 8] - rstats[:, 8]) <= 1e-12 * np.maximum(rstats[:, COL["n_cons"]], 1.0))
    assert np.all(np.abs(score - rscore) <= 1e-12)


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("window", WINDOWS)
def test_pose_score_against_fp64(ops, window, placement, with_depth):
    from rnnpose_amd import _lib
    c = grid_case(*window, placement)
    rstats = c["ref"][with_depth][0]
    if placement == "outside":                                    # what the placement is there to show, asserted on the restatement
        assert np.array_equal(rstats[:, COL["n_out"]], rstats[:, COL["n_rend"]]) and rstats[:, COL["n_rend"]].any() and not rstats[:, COL["n_desc"]].any()
    elif window != (1, 1):
        assert rstats[:, COL["n_desc"]].all() and (placement == "inside" or rstats[:, COL["n_out"]].all())
        assert not with_depth or min(window) < 7 or all(rstats[:, COL[k]].all() for k in ("n_occ", "n_cons", "n_viol", "n_hole"))
    got = raw_call(_lib.load(), c, with_depth)
    check(got, c["ref"][with_depth], f"{window} {placement} depth={with_depth}")
    st, sc = ops.pose_score(dev(c["z"]), dev(c["a"]), dev(c["window"], np.int32), dev(c["g"]), c["src"], dev(c["d"]) if with_depth else None, c["tol"])
    assert st.dtype == sc.dtype == torch.float64 and np.array_equal(npy(st), got[0]) and np.array_equal(npy(sc), got[1])


# ---- planted boundaries ------------------------------------------------------------------------------------------------------------------
def planted():
    """A 2 x 8 window inside frame 1, z = 0.5, tol = 0.125: row 0 = the four depth boundaries, a zero rendered descriptor, a zero frame
    descriptor, a NaN channel on either side; row 1 empty.  Pose 1: a window without a rendered pixel."""
    up, down = np.nextafter(np.float32(0.625), np.float32(np.inf)), np.nextafter(np.float32(0.375), np.float32(0))
    x0, y0 = 11, 7
    e = np.zeros(D, np.float32)
    e[5] = 3.0                                                     # |e|^2 = 9: the cosine with itself is exactly 1
    z = np.full((2, 2, 8), -1.0, np.float32)
    z[0, 0] = 0.5
    a = np.zeros((2, D, 2, 8), np.float32)
    a[0, :, 0, :] = e[:, None]
    g = np.zeros((S, D, H, W), np.float32)
    g[1, :, y0, x0:x0 + 8] = e[:, None]
    d = np.full((S, H, W), 0.5, np.float32)
    d[1, y0, x0:x0 + 4] = [0.625, up, 0.375, down]
    a[0, :, 0, 4] = 0.0
    g[1, :, y0, x0 + 5] = 0.0
    a[0, 9, 0, 6] = np.nan
    g[1, 30, y0, x0 + 7] = np.nan
    return dict(z=z, a=a, g=g, d=d, window=np.array([[x0, y0], [x0, y0]], np.int32), src=[1, 1], tol=0.125)


def test_planted_boundaries(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    c = planted()
    ref = sr.pose_score(c["z"], c["a"], c["window"], c["g"], c["d"], c["src"], c["tol"])
    #                      n_rend n_out n_occ n_cons n_viol n_hole n_desc sum_cos sum|dd| n_bad
    want = np.array([[8, 0, 1, 6, 1, 0, 5, 3.0, 0.25, 2], [0] * 10], np.float64)
    assert np.array_equal(ref[0], want) and ref[1].tolist() == [(3.0 / 5.0) * (6.0 / 7.0), 0.0]        # the restatement first
    stats, score = raw_call(lib, c, True)
    assert np.array_equal(stats, want) and score.tolist() == ref[1].tolist()
    # tol = 0 is valid: equal depths are consistent, one ulp either way is not
    c0 = dict(c, tol=0.0)
    c0["d"] = c["d"].copy()
    c0["d"][1, 7, 11:15] = [0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.5, np.nextafter(np.float32(0.5), np.float32(0))]
    ref0 = sr.pose_score(c0["z"], c0["a"], c0["window"], c0["g"], c0["d"], c0["src"], 0.0)
    assert ref0[0][0].tolist() == [8, 0, 1, 6, 1, 0, 5, 3.0, 0.0, 2]
    stats0, score0 = raw_call(lib, c0, True)
    assert np.array_equal(stats0, ref0[0]) and np.array_equal(score0, ref0[1])
    # without the observed depth every inside pixel is a hole and is compared: the occluded pixel's descriptor joins in
    refn = sr.pose_score(c["z"], c["a"], c["window"], c["g"], None, c["src"], c["tol"])
    assert refn[0][0].tolist() == [8, 0, 0, 0, 0, 8, 6, 4.0, 0.0, 2] and refn[1].tolist() == [4.0 / 6.0, 0.0]
    statsn, scoren = raw_call(lib, c, False)
    assert np.array_equal(statsn, refn[0]) and np.array_equal(scoren, refn[1])
    # every observed depth behind the surface: all compared pixels violated, the depth factor is 0 -- not the 1 of "no depth evidence"
    cv = dict(c, d=np.full_like(c["d"], 5.0))
    refv = sr.pose_score(cv["z"], cv["a"], cv["window"], cv["g"], cv["d"], cv["src"], cv["tol"])
    assert refv[0][0].tolist() == [8, 0, 0, 0, 8, 0, 6, 4.0, 0.0, 2] and refv[1].tolist() == [0.0, 0.0]
    statsv, scorev = raw_call(lib, cv, True)
    assert np.array_equal(statsv, refv[0]) and np.array_equal(scorev, refv[1])
    # an index outside [0, S) handed straight to the library: a zero row and score 0, the other pose untouched by it
    stats, score = raw_call(lib, dict(c, src=[1, 7], window=np.array([[11, 7], [0, 0]], np.int32), z=np.full_like(c["z"], 0.5)), True)
    assert stats[0, 0] == 16 and not stats[1].any() and score[1] == 0.0
    stats, score = raw_call(lib, dict(c, src=[-1, 1]), True)
    assert not stats.any() and not score.any()


# ---- determinism -------------------------------------------------------------------------------------------------------------------------
def test_reruns_and_batch_independence(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    c = grid_case(37, 70, "top_left")
    a = (dev(c["z"]), dev(c["a"]), dev(c["window"], np.int32), dev(c["g"]), c["src"], dev(c["d"]), c["tol"])
    one, two = ops.pose_score(*a), ops.pose_score(*a)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and float(one[1].sum()) > 0
    for with_depth in (False, True):
        whole = raw_call(lib, c, with_depth)
        for b in range(3):                                                     # every pose alone == the pose in the batch, bit for bit
            alone = raw_call(lib, c, with_depth, rows=[b])
            assert np.array_equal(alone[0][0], whole[0][b]) and alone[1][0] == whole[1][b]


def test_flat_grid_of_257_poses(ops):
    """B = 257 poses with 7 x 5 windows, more poses than a workgroup has threads: the grid is flat over B x chunks, and a row that read
    another pose's chunk would differ.  Every row equals the pose's single-pose result, bit for bit, and the restatement within the bounds."""
    from rnnpose_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(257)
    B, h, w = 257, 7, 5
    base = grid_case(7, 5, "inside")
    z = rng.uniform(0.4, 0.6, (B, h, w)).astype(np.float32)
    z[rng.random(z.shape) < 0.3] = -1.0
    c = dict(base, z=z, a=rng.normal(size=(B, D, h, w)).astype(np.float32), src=rng.integers(0, S, B).tolist(),
             window=np.stack([rng.integers(-3, W - 2, B), rng.integers(-3, H - 2, B)], 1).astype(np.int32))
    whole = raw_call(lib, c, True)
    check(whole, sr.pose_score(c["z"], c["a"], c["window"], c["g"], c["d"], c["src"], c["tol"]), "257 poses")
    assert len({tuple(r) for r in whole[0]}) > 200                             # (the rows are different poses)
    for b in range(B):
        alone = raw_call(lib, c, True, rows=[b])
        assert np.array_equal(alone[0][0], whole[0][b]) and alone[1][0] == whole[1][b], b


# ---- bad arguments -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_1_and_write_nothing(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    c = grid_case(7, 5, "inside")
    B, h, w = 3, 7, 5
    n = int(lib.rnnpose_pose_score_workspace_bytes(B, h, w))
    assert n == 3 * 1 * 80 and lib.rnnpose_pose_score_workspace_bytes(2, 37, 70) == 2 * 11 * 80
    assert lib.rnnpose_pose_score_workspace_bytes(0, h, w) == 0 and lib.rnnpose_pose_score_workspace_bytes(B, 0, w) == 0 and \
        lib.rnnpose_pose_score_workspace_bytes(B, h, -1) == 0
    t = dict(z=dev(c["z"]), a=dev(c["a"]), win=dev(c["window"], np.int32), g=dev(c["g"]), d=dev(c["d"]), src=dev(c["src"], np.int32))
    ws = torch.full((n // 8,), CANARY, dtype=torch.float64).cuda()
    stats = torch.full((B, 10), CANARY, dtype=torch.float64).cuda()
    score = torch.full((B,), CANARY, dtype=torch.float64).cuda()
    good = dict(z=ptr(t["z"]), a=ptr(t["a"]), win=ptr(t["win"]), g=ptr(t["g"]), d=ptr(t["d"]), src=ptr(t["src"]), B=B, S=S, D=D, h=h, w=w, H=H, W=W,
                tol=0.03, ws=ptr(ws), n=n, stats=ptr(stats), score=ptr(score), stream=None)
    bad = [dict(z=None), dict(a=None), dict(win=None), dict(g=None), dict(src=None), dict(ws=None), dict(stats=None), dict(score=None),
           dict(D=16), dict(D=64), dict(D=0), dict(B=0), dict(B=-1), dict(h=0), dict(w=0), dict(h=-7), dict(H=0), dict(W=0), dict(W=-56), dict(S=0),
           dict(S=-1), dict(tol=-1e-9), dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=-float("inf")), dict(n=n - 8), dict(n=0)]
    for change in bad:
        assert lib.rnnpose_pose_score_f64(*dict(good, **change).values()) == 1, change
        assert len(lib.rnnpose_last_error()) > 0
    torch.cuda.synchronize()
    assert all(bool((v == CANARY).all()) for v in (ws, stats, score))
    for change in (dict(), dict(d=None), dict(tol=0.0), dict(n=n + 8)):          # ... and these are fine (depth_obs may be NULL)
        assert lib.rnnpose_pose_score_f64(*dict(good, **change).values()) == 0, change
    torch.cuda.synchronize()
    assert np.array_equal(npy(stats)[:, COUNTS], c["ref"][True][0][:, COUNTS])


def test_ops_pose_score_refuses_bad_inputs(ops):
    c = grid_case(7, 5, "inside")
    z, a, win, g, d = dev(c["z"]), dev(c["a"]), dev(c["window"], np.int32), dev(c["g"]), dev(c["d"])
    ok = ops.pose_score(z, a, win, g, c["src"], d, 0.03)
    assert np.array_equal(npy(ok[0])[:, COUNTS], c["ref"][True][0][:, COUNTS])
    assert torch.equal(ops.pose_score(z[:, None], a, c["window"].tolist(), g, ops.SourceIndex(c["src"], S, z.device), d, 0.03)[0], ok[0])   # (B,1,h,w), host window
    assert torch.equal(ops.pose_score(z[:2], a[:2], win[:2], g, None, d, 0.03)[0], ok[0][:2])                 # src_index None: pose b reads frame b
    refused = [
        lambda: ops.pose_score(z.double(), a, win, g, c["src"], d),                    # dtypes
        lambda: ops.pose_score(z, a.half(), win, g, c["src"], d),
        lambda: ops.pose_score(z, a, win.long(), g, c["src"], d),
        lambda: ops.pose_score(z, a, win, g.double(), c["src"], d),
        lambda: ops.pose_score(z, a, win, g, c["src"], d.double()),
        lambda: ops.pose_score(z, a, win, g, torch.tensor([0.0, 1.0, 0.0]), d),
        lambda: ops.pose_score(z[:, :6].contiguous(), a, win, g, c["src"], d),         # shapes
        lambda: ops.pose_score(z[:2], a, win, g, c["src"], d),
        lambda: ops.pose_score(z, a[:, :16].contiguous(), win, g, c["src"], d),
        lambda: ops.pose_score(z, a, win[:2], g, c["src"], d),
        lambda: ops.pose_score(z, a, dev(np.zeros((3, 3)), np.int32), g, c["src"], d),
        lambda: ops.pose_score(z, a, win, g[:, :16].contiguous(), c["src"], d),
        lambda: ops.pose_score(z, a, win, g[0], c["src"], d),
        lambda: ops.pose_score(z, a, win, g, c["src"], d[:, :H - 1].contiguous()),
        lambda: ops.pose_score(z, a, win, g, c["src"], d[:1]),
        lambda: ops.pose_score(z, a, win, g, [0, 1], d),
        lambda: ops.pose_score(z, a.transpose(2, 3), win, g, c["src"], d),             # contiguity
        lambda: ops.pose_score(z, a, win, g[:, :, :, ::2], c["src"], d),
        lambda: ops.pose_score(z, a, win, g, [0, 2, 0], d),                            # index range
        lambda: ops.pose_score(z, a, win, g, [0, -1, 0], d),
        lambda: ops.pose_score(z, a, win, g, None, d),                                 # (3 poses, 2 frames)
        lambda: ops.pose_score(z, a, win, g, c["src"], d, -0.01),                      # depth_tol
        lambda: ops.pose_score(z, a, win, g, c["src"], d, float("nan")),
        lambda: ops.pose_score(z, a, win, g, c["src"], d, float("inf")),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")


def test_torch_ops_equal_ops_and_have_a_fake_kernel(ops):
    """torch.ops.rnnpose.pose_score gives what ops.pose_score gives, its fake kernel the shapes and dtypes; and ops.pose_score refuses a
    tensor on another device (checked here, on the GPU only: the host-executed tier has one device)."""
    import rnnpose_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    c = grid_case(37, 70, "bottom_right")
    z, a, win, g, d = dev(c["z"]), dev(c["a"]), dev(c["window"], np.int32), dev(c["g"]), dev(c["d"])
    src = torch.tensor(c["src"])
    for depth in (None, d):
        want = ops.pose_score(z, a, win, g, c["src"], depth, 0.03)
        got = torch.ops.rnnpose.pose_score(z, a, win.long(), g, src, depth, 0.03)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and float(got[1].sum()) > 0
    with pytest.raises(ValueError):
        torch.ops.rnnpose.pose_score(z, a, win, g, torch.tensor([0, 5, 0]), d, 0.03)
    for k in (0, 1, 3, 4):                                                       # (a window on the host is taken as host values and copied)
        args = [z, a, win, g, d]
        args[k] = args[k].cpu()
        with pytest.raises(ValueError):
            ops.pose_score(*args[:4], c["src"], args[4])
    with FakeTensorMode():
        e = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="cuda", dtype=dtype)
        f = torch.ops.rnnpose.pose_score(e(3, 37, 70), e(3, 32, 37, 70), e(3, 2, dtype=torch.int32), e(2, 32, H, W), e(3, dtype=torch.int64), e(2, H, W))
        assert [(tuple(t.shape), t.dtype, t.device.type) for t in f] == [(tuple(t.shape), t.dtype, "cuda") for t in got]
        f = torch.ops.rnnpose.pose_score(e(3, 37, 70), e(3, 32, 37, 70), e(3, 2, dtype=torch.int32), e(2, 32, H, W), e(3, dtype=torch.int64))
        assert [tuple(t.shape) for t in f] == [(3, 10), (3,)]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
SIZE = (240, 320)


@pytest.fixture(scope="module")
def scene(ops):
    from oracle import rnnpose_oracle as orc
    from rnnpose_amd import eval_epoch as ee, synthetic as syn
    from rnnpose_amd.pose_refiner import default_config
    models = ee.synthetic_models(sub=3)
    cfg = default_config(RENDER_ITER_COUNT=1, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=SIZE, zoom_crop_size=(128, 128))
    Tt = lambda v: torch.from_numpy(v)

    def epoch(**kw):                                              # the same weights every time: two epochs refine alike
        torch.manual_seed(0)
        hip = ee.HipEpoch(models, cfg=cfg, **kw)
        hip.refiner.cf_net.update_block.load_state_dict({k: Tt(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
        hip.refiner.image_fea_enc.fnet.load_state_dict({k: Tt(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
        return hip
    hip = epoch()
    items = ee.synthetic_scenes(models, 1, 3, image_size=SIZE, renderer=hip.renderer)
    assert all(it.depth is not None for it in items)
    return hip, models, items, epoch


def restate(scorer, items, poses, with_depth):
    """The restatement on PoseScorer.render's own tensors -> (stats, score), record of the derived quantities."""
    names = [it.class_name for it in items]
    K = np.stack([it.K for it in items])
    rd, ra, win, clipped = scorer.render(names, poses, K, SIZE)
    g = npy(items[0].geofea_2d)[None].astype(np.float32)
    d = npy(items[0].depth)[None].astype(np.float32) if with_depth else None
    stats, score = sr.pose_score(npy(rd)[:, 0], npy(ra), npy(win), g, d, [0] * len(items), scorer.depth_tol)
    c = lambda k: stats[:, COL[k]]
    rec = dict(visible_fraction=np.where(c("n_rend") > 0, c("n_desc") / np.maximum(c("n_rend"), 1), 0.0),
               depth_factor=np.where(c("n_cons") + c("n_viol") > 0, c("n_cons") / np.maximum(c("n_cons") + c("n_viol"), 1), 1.0), clipped=clipped,
               window=npy(win))
    return (stats, score), rec


def variants(models, items):
    """gt and the four wrong poses of the ranking: shifted 0.5 diameter along the camera's x, rotated 60 degrees about the camera's z-axis
    through the object's centre (the models are centred), pulled 0.3 diameter towards the camera, pushed 0.3 diameter away."""
    gt = np.stack([it.pose_gt for it in items]).astype(np.float64)
    diam = np.array([models[it.class_name].diameter for it in items])
    ang = np.deg2rad(60.0)
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    out = dict(gt=gt, shifted=gt.copy(), rotated=gt.copy(), pulled=gt.copy(), pushed=gt.copy())
    out["shifted"][:, 0, 3] += 0.5 * diam
    out["rotated"][:, :3, :3] = Rz @ gt[:, :3, :3]
    out["pulled"][:, 2, 3] -= 0.3 * diam
    out["pushed"][:, 2, 3] += 0.3 * diam
    return {k: v.astype(np.float32) for k, v in out.items()}


def test_end_to_end_score_poses_equals_the_restatement_and_ranks(ops, scene):
    import dataclasses
    hip, models, items, _ = scene
    var = variants(models, items)
    bare = [dataclasses.replace(it, depth=None) for it in items]
    ref, got = {}, {}
    for with_depth, batch in ((False, bare), (True, items)):
        for name, poses in var.items():
            score = hip.score_poses(batch, poses)
            rec = hip.last_score_info
            scorer = hip._default_scorer
            ref[name, with_depth] = restate(scorer, items, poses, with_depth)
            (rstats, rscore), rrec = ref[name, with_depth]
            stats = np.stack([rec[k] for k in sr.COLUMNS], 1)
            check((stats, npy(score)), (rstats, rscore), f"{name} depth={with_depth}")
            assert score.dtype == torch.float64 and score.shape == (3,) and np.array_equal(rec["window"], rrec["window"]) and not rec["clipped"].any()
            assert np.allclose(rec["visible_fraction"], rrec["visible_fraction"], rtol=0, atol=1e-15)
            assert np.allclose(rec["depth_factor"], rrec["depth_factor"], rtol=0, atol=1e-15)
            assert np.all((rec["n_cons"] + rec["n_viol"] + rec["n_occ"] > 0) == with_depth)
            got[name, with_depth] = (npy(score), rec)
            print(f"{name:8s} depth={with_depth}: score {npy(score).round(4).tolist()}  visible {rec['visible_fraction'].round(3).tolist()}  "
                  f"depth_factor {rec['depth_factor'].round(3).tolist()}  window {rec['window_size']}")
    # rankings: on the restatement FIRST (a scene that does not discriminate is not a kernel error), then on the device
    for with_depth in (False, True):
        for wrong in ("shifted", "rotated"):
            assert np.all(ref["gt", with_depth][0][1] > ref[wrong, with_depth][0][1]), (wrong, with_depth)
            assert np.all(got["gt", with_depth][0] > got[wrong, with_depth][0]), (wrong, with_depth)
    for side, (pose, key, low) in (("ref", ("pulled", "depth_factor", True)), ("ref", ("pushed", "visible_fraction", True)),
                                   ("got", ("pulled", "depth_factor", True)), ("got", ("pushed", "visible_fraction", True))):
        rec = ref[pose, True][1] if side == "ref" else got[pose, True][1]
        assert np.all(rec[key] < 0.5), (side, pose, key, rec[key])
    for rec in (ref["gt", True][1], got["gt", True][1]):
        assert np.all(rec["depth_factor"] > 0.9) and np.all(rec["visible_fraction"] > 0.9)


def test_end_to_end_select_poses(ops, scene):
    hip, models, items, _ = scene
    var = variants(models, items)
    cand = torch.as_tensor(np.stack([var["shifted"], var["gt"], var["rotated"]], 1)).cuda()          # (B,3,4,4)
    poses, index, scores = hip.select_poses(items, cand)
    assert index.tolist() == [1, 1, 1] and torch.equal(poses, cand[:, 1]) and scores.shape == (3, 3) and scores.dtype == torch.float64
    assert hip.last_score_info["n_rend"].shape == (3, 3) and hip.last_score_info["window"].shape == (3, 3, 2)
    for n, name in enumerate(("shifted", "gt", "rotated")):                    # one call over B * N == a call per hypothesis
        assert float((scores[:, n] - hip.score_poses(items, var[name])).abs().max()) <= 1e-12        # (another shared window: other chunks)
    same = torch.as_tensor(np.stack([var["gt"], var["gt"], var["shifted"]], 1)).cuda()                 # a tie goes to the lowest index
    assert hip.select_poses(items, same)[1].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        hip.select_poses(items, cand[:2])


def test_end_to_end_refine_frame_with_scores_equals_without(ops, scene):
    from rnnpose_amd import eval_epoch as ee
    from rnnpose_amd.pose_score import PoseScorer
    hip, models, items, epoch = scene
    plain = hip.refine_frame(items)
    assert hip.last_scores is None and hip.scorer is None
    on = epoch(score=True)
    scored = on.refine_frame(items)
    assert torch.equal(scored, plain)
    assert isinstance(on.scorer, PoseScorer) and on.last_scores.shape == (3,) and on.last_scores.dtype == torch.float64
    assert torch.equal(on.last_scores, on.score_poses(items, scored)) and torch.equal(on.last_scores, hip.score_poses(items, plain))
    # (the refiner's weights are random numbers here: what it returns is no better than its start, and the scores say so)
    assert float(on.last_scores.min()) >= 0.0 and float(on.last_scores.max()) <= 1.0
    one = on.refine(items[1].class_name, [items[1]])                            # the class-batch caller fills it too
    assert on.last_scores.shape == (1,) and torch.equal(on.last_scores, on.score_poses([items[1]], one))
    assert torch.equal(one, hip.refine(items[1].class_name, [items[1]])) and hip.last_scores is None
    # a multi-view group (two views through the same camera, E = I, regrouped inside refine_frame): scored view by view, in the caller's order
    import dataclasses
    eye = np.eye(4, dtype=np.float32)
    views = [dataclasses.replace(items[0], object_id="a", cam_from_rig=eye), dataclasses.replace(items[2], object_id="c", cam_from_rig=eye),
             dataclasses.replace(items[0], object_id="a", cam_from_rig=eye)]
    pv = on.refine_frame(views)
    assert torch.equal(pv, hip.refine_frame(views)) and torch.equal(pv[0], pv[2]) and on.last_scores.shape == (3,)
    assert torch.equal(on.last_scores, on.score_poses(views, pv)) and float(on.last_scores[0]) == float(on.last_scores[2])
    own = PoseScorer(on.renderer, models, device="cuda", depth_tol=0.05)        # a ready-made scorer
    assert ee.HipEpoch(models, cfg=hip.cfg, refiner=hip.refiner, score=own).scorer is own


def test_end_to_end_max_window_clips_and_still_equals_the_restatement(ops, scene):
    from rnnpose_amd.pose_score import PoseScorer
    hip, models, items, _ = scene
    gt = np.stack([it.pose_gt for it in items]).astype(np.float32)
    full = hip.score_poses(items, gt)
    box = hip.last_score_info["window_size"]
    assert min(box) > 24 and box[0] % 8 == 0 and box[1] % 8 == 0
    small = PoseScorer(hip.renderer, models, device="cuda", max_window=24)
    score = hip.score_poses(items, gt, scorer=small)
    rec = hip.last_score_info
    assert rec["clipped"].all() and rec["window_size"] == (24, 24) and np.all(rec["n_rend"] <= 24 * 24) and np.all(rec["n_rend"] > 200)
    (rstats, rscore), rrec = restate(small, items, gt, True)
    check((np.stack([rec[k] for k in sr.COLUMNS], 1), npy(score)), (rstats, rscore), "max_window=24")
    assert np.array_equal(rec["window"], rrec["window"]) and rrec["clipped"].all()
    assert np.all(npy(score) > 0.9) and np.all(npy(full) > 0.9)                 # the centre of the object still matches its frame
    # a pose behind the camera's near plane: the whole frame as far as the window allows, flagged, nothing rendered, score 0
    behind = gt.copy()
    behind[0, 2, 3] = -0.5
    score = hip.score_poses(items, behind)
    rec = hip.last_score_info
    assert rec["clipped"].tolist() == [True, False, False] and rec["window_size"] == SIZE and rec["window"][0].tolist() == [0, 0]
    assert float(score[0]) == 0.0 and float(score[1]) > 0.9
