"""GPU tests of object onboarding: the kernels behind rnnpose_point_diameter_f64 and rnnpose_fps_f64 against the
fp64 numpy restatement tests/model_prep_ref.py, and the plumbing above them (ops.point_diameter / ops.farthest_points, the torch ops,
model_prep.build_class_model / fragments, DescriptorPoseInitializer(point_subset=)).

Bounds.  Both sides convert fp32 to fp64 and evaluate d2 = (dx dx + dy dy) + dz dz without contraction, so every squared distance has
the same bits on both sides; maxima, minima and the tie rules are comparisons.  Hence d2, pair, idx and dist2 are compared EXACTLY, the
bounds bit for bit, and the diameter within 1 ulp of numpy.sqrt(d2) (both roots are correctly rounded; the ulp is the issue's allowance).
Random sets for FPS are used only where the restatement's best and runner-up running distances differ by a relative 1e-9 at every
pick (asserted on the CPU first); exact ties are the lattice cases' business.

tests/test_model_prep_on_host.py runs every case of this module except the end-to-end and torch_ops ones on the host-executed kernels."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import model_prep_ref as mr

pytestmark = pytest.mark.gpu

TILE, THREADS, REG = 256, 1024, 8          # csrc/model_prep.cuh: kTile, kFpsThreads, kFpsReg
CANARY = -777
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def guarded(n, dtype, guard=64):
    """n elements inside a larger buffer filled with the canary -> (the view, its guard zones as a function)"""
    buf = torch.full((n + 2 * guard,), CANARY, dtype=dtype).cuda()
    return buf[guard:guard + n], lambda: torch.cat([buf[:guard], buf[guard + n:]])


def pack(sets):
    """point sets -> (points on the device: at least one row, total, pt_off on the device)"""
    sets = [np.asarray(s, np.float32).reshape(-1, 3) for s in sets]
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    pts = np.concatenate(sets + [np.zeros((1, 3), np.float32)])
    return dev(pts), int(off[-1]), dev(off, np.int32)


def raw_diameter(lib, sets):
    """rnnpose_point_diameter_f64 straight from the library on guarded outputs and a guarded workspace -> d2, diameter, pair, bounds"""
    B = len(sets)
    pts, total, off = pack(sets)
    n = int(lib.rnnpose_point_diameter_workspace_bytes(total, B))
    nt = max(1, -(-total // TILE))
    assert n == B * (nt * (nt + 1) // 2) * 16
    ws, z0 = guarded(n // 8, torch.float64)
    d2, z1 = guarded(B, torch.float64)
    dm, z2 = guarded(B, torch.float64)
    pair, z3 = guarded(2 * B, torch.int32)
    bnd, z4 = guarded(6 * B, torch.float32)
    r = lib.rnnpose_point_diameter_f64(ptr(pts), ptr(off), total, B, ptr(ws), n, ptr(d2), ptr(dm), ptr(pair), ptr(bnd), None)
    torch.cuda.synchronize()
    assert r == 0
    for zone in (z0, z1, z2, z3, z4):
        assert bool((zone() == CANARY).all()), "a guard zone was written"
    return npy(d2).copy(), npy(dm).copy(), npy(pair).reshape(B, 2).copy(), npy(bnd).reshape(B, 2, 3).copy()


def raw_fps(lib, sets, n, start):
    """rnnpose_fps_f64 straight from the library on guarded buffers -> idx (B,n), dist2 (B,n)"""
    B = len(sets)
    pts, total, off = pack(sets)
    nb = int(lib.rnnpose_fps_workspace_bytes(total, B))
    assert nb == max(total, 1) * 8
    ws, z0 = guarded(nb // 8, torch.float64)
    idx, z1 = guarded(B * n, torch.int32)
    d2, z2 = guarded(B * n, torch.float64)
    st = dev(np.array(np.broadcast_to(np.asarray(start, np.int32), (B,))), np.int32)
    r = lib.rnnpose_fps_f64(ptr(pts), ptr(off), total, B, n, ptr(st), ptr(ws), nb, ptr(idx), ptr(d2), None)
    torch.cuda.synchronize()
    assert r == 0
    for zone in (z0, z1, z2):
        assert bool((zone() == CANARY).all()), "a guard zone was written"
    return npy(idx).reshape(B, n).copy(), npy(d2).reshape(B, n).copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_diameter(got, b, pts, tag=""):
    d2, dm, pair, bnd = got
    rd2, rdm, rpair, rbnd = mr.diameter(pts)
    print(f"{tag}: d2 {d2[b]!r} (ref {rd2!r}) pair {pair[b].tolist()} (ref {list(rpair)}) diameter {dm[b]!r}")
    assert d2[b] == rd2 and tuple(pair[b].tolist()) == rpair
    assert abs(dm[b] - np.sqrt(rd2)) <= np.spacing(np.sqrt(rd2))
    assert np.array_equal(bits(bnd[b]), bits(rbnd))


@functools.lru_cache(maxsize=None)
def cloud(P, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((P, 3)) * scale).astype(np.float32)


# ---- diameter ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("P", [0, 1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_diameter_against_fp64(ops, P, scale):
    from rnnpose_amd import _lib
    pts = cloud(P, 100 + P, scale)
    got = raw_diameter(_lib.load(), [pts])
    check_diameter(got, 0, pts, f"P={P} scale={scale}")
    if P < 2:
        assert got[0][0] == 0.0 and got[1][0] == 0.0 and got[2][0].tolist() == [-1, -1]
    o = ops.point_diameter(dev(pts).reshape(-1, 3))
    assert all(np.array_equal(npy(a).reshape(-1), np.asarray(b).reshape(-1)) for a, b in zip(o, got))


def test_diameter_batch_equals_single(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    sets = [cloud(2 * TILE + 37, 1), cloud(0, 2), cloud(TILE + 5, 3, 1e-2)]
    whole = raw_diameter(lib, sets)
    for b, s in enumerate(sets):
        check_diameter(whole, b, s, f"object {b}")
        alone = raw_diameter(lib, [s])
        assert all(w[b].tobytes() == a[0].tobytes() for w, a in zip(whole, alone)), b
    # offsets that do not fit the array: the object counts as empty, the others are untouched by it
    pts, total, off = pack(sets)
    bad = dev(np.array([0, total + 1, total + 1, total], np.int32), np.int32)
    d2, dm, pair, bnd = ops.point_diameter(pts[:total], bad)
    assert npy(d2).tolist() == [0.0, 0.0, 0.0] and npy(pair).tolist() == [[-1, -1]] * 3 and bool(torch.isinf(bnd).all())


def test_diameter_ties_go_to_the_lowest_pair(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    cube = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    r = mr.diameter(cube)
    assert r[0] == 3.0 and r[2] == (0, 7)                                         # the restatement first
    tied = [(i, j) for i in range(8) for j in range(i + 1, 8) if ((cube[i] - cube[j]) ** 2).sum() == 3.0]
    assert tied == [(0, 7), (1, 6), (2, 5), (3, 4)]
    got = raw_diameter(lib, [cube])
    assert got[0][0] == 3.0 and got[2][0].tolist() == [0, 7]
    perm = np.random.default_rng(5).permutation(8)
    inv = np.argsort(perm)                                                        # cube row c sits at inv[c] of cube[perm]
    want = min(tuple(sorted((int(inv[i]), int(inv[j])))) for i, j in tied)
    got = raw_diameter(lib, [cube[perm]])
    assert want != (0, 7) and got[0][0] == 3.0 and tuple(got[2][0].tolist()) == want == mr.diameter(cube[perm])[2]
    # one i with two farthest j: an equilateral triangle (all three distances 2) -> the lowest j, within a tile and across tiles
    tri = np.eye(3, dtype=np.float32)
    assert mr.diameter(tri)[2] == (0, 1) and raw_diameter(lib, [tri])[2][0].tolist() == [0, 1]
    spread = (cloud(2 * TILE + 9, 10, 1e-3) + np.float32(1 / 3)).astype(np.float32)
    spread[[5, TILE + 5, 2 * TILE + 5]] = tri
    got = raw_diameter(lib, [spread])
    assert got[0][0] == 2.0 and got[2][0].tolist() == [5, TILE + 5] and mr.diameter(spread)[2] == (5, TILE + 5)
    # ties across tiles: the cube's corners spread over three tiles of far smaller points
    big = np.concatenate([cloud(2 * TILE + 9, 9, 1e-3) + 0.5]).astype(np.float32)
    at = [3, 200, TILE + 1, TILE + 77, 2 * TILE - 1, 2 * TILE, 2 * TILE + 3, 2 * TILE + 8]
    big[at] = cube
    got = raw_diameter(lib, [big])
    assert got[0][0] == 3.0 and got[2][0].tolist() == [at[0], at[7]] and mr.diameter(big)[2] == (at[0], at[7])


def test_diameter_ignores_points_that_are_not_finite(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    clean = cloud(TILE + 40, 11)
    dirty = np.insert(clean, [0, 17, TILE + 3, len(clean)], 0.0, axis=0)
    where = [0, 18, TILE + 5, len(dirty) - 1]
    dirty[where[0]] = [np.nan, 9e9, 0.0]
    dirty[where[1]] = [1e30, np.inf, 0.0]
    dirty[where[2]] = [0.0, 0.0, -np.inf]
    dirty[where[3]] = [1e30, 1e30, np.nan]
    keep = np.setdiff1d(np.arange(len(dirty)), where)
    assert np.array_equal(dirty[keep], clean)
    a, b = raw_diameter(lib, [clean]), raw_diameter(lib, [dirty])
    check_diameter(b, 0, dirty, "with NaN / inf")
    assert b[0][0] == a[0][0] and bits(b[1])[0] == bits(a[1])[0] and keep[a[2][0]].tolist() == b[2][0].tolist()
    assert np.array_equal(bits(a[3]), bits(b[3]))
    one = raw_diameter(lib, [np.array([[np.nan, 0, 0], [1, 2, 3], [np.inf, 0, 0]], np.float32)])      # one finite point: no pair, its bounds
    assert one[0][0] == 0.0 and one[2][0].tolist() == [-1, -1] and one[3][0].tolist() == [[1, 2, 3], [1, 2, 3]]
    none = raw_diameter(lib, [np.full((5, 3), np.nan, np.float32)])
    assert none[2][0].tolist() == [-1, -1] and none[3][0].tolist() == [[np.inf] * 3, [-np.inf] * 3]


# ---- farthest-point sampling ---------------------------------------------------------------------------------------------------------------
def check_fps(got, b, pts, n, start, tag=""):
    idx, d2 = got
    ridx, rd2 = mr.fps(pts, n, start)
    print(f"{tag}: idx {idx[b][:8].tolist()} dist2 {d2[b][:4].tolist()}")
    assert np.array_equal(idx[b], ridx), (idx[b], ridx)
    assert np.array_equal(bits(d2[b]), bits(rd2))


def lattice():
    g = np.arange(-2, 3, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)        # 125 integer points: exact arithmetic, ties at every pick


@pytest.mark.parametrize("start", [-1, 0, 62, 124])
def test_fps_lattice_ties(ops, start):
    from rnnpose_amd import _lib
    pts = lattice()
    got = raw_fps(_lib.load(), [pts], 40, start)
    check_fps(got, 0, pts, 40, start, f"lattice start={start}")
    assert got[0][0, 0] == (0 if start < 0 else start)                            # the eight corners tie at 12: the lowest index
    assert got[1][0, 0] == (12.0 if start < 0 else np.inf) and len(set(got[0][0].tolist())) == 40
    o = ops.farthest_points(dev(pts), 40, None, start)
    assert np.array_equal(npy(o[0]), got[0]) and np.array_equal(bits(npy(o[1])), bits(got[1]))


def test_fps_duplicates_come_last_and_short_objects_are_padded(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    base = lattice()[::9]                                                          # 14 distinct points
    pts = np.concatenate([base, base[[3, 3, 7]], base[:2]])                        # five duplicates behind them
    n = len(pts) + 4
    for start in (-1, 5):
        got = raw_fps(lib, [pts], n, start)
        check_fps(got, 0, pts, n, start, f"duplicates start={start}")
        idx, d2 = got[0][0], got[1][0]
        first = idx[:14]
        assert len({tuple(pts[i]) for i in first}) == 14                           # every distinct location once, then the duplicates
        dup = idx[14:19]
        assert np.all(d2[14:19] == 0.0) and dup.tolist() == sorted(dup.tolist()) and len(set(idx[:19].tolist())) == 19
        assert idx[19:].tolist() == [-1] * 4 and d2[19:].tolist() == [-1.0] * 4    # P < n: the padding
    # duplicates one workgroup width apart: both copies sit in ONE thread's slice, which must keep the first of equal distances
    base = np.random.default_rng(8).integers(-30, 31, (THREADS, 3)).astype(np.float32)
    twice = np.concatenate([base, base, base[:1]])
    got = raw_fps(lib, [twice], 8, -1)
    check_fps(got, 0, twice, 8, -1, "duplicates a workgroup apart")
    assert np.all(got[0][0] < THREADS)
    empty = raw_fps(lib, [pts], 3, 99)                                             # a start outside the object
    assert empty[0].tolist() == [[-1] * 3] and empty[1].tolist() == [[-1.0] * 3]
    nan = pts.copy()
    nan[[0, 4]] = np.nan                                                           # points that are not finite are never picked
    got = raw_fps(lib, [nan], n, -1)
    check_fps(got, 0, nan, n, -1, "with NaN")
    assert not {0, 4} & set(got[0][0].tolist()) and (got[0][0] >= 0).sum() == len(pts) - 2
    assert raw_fps(lib, [nan], 2, 4)[0].tolist() == [[-1, -1]]                     # a start that is not finite: nothing to pick


@pytest.mark.parametrize("P", [THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1, THREADS * REG, THREADS * REG + 1])
def test_fps_at_the_workgroup_edges(ops, P):
    """n = 8 at P around the workgroup size and at the step from the register-resident slice to the one in memory"""
    from rnnpose_amd import _lib
    g = np.random.default_rng(P).integers(-40, 41, (P, 3)).astype(np.float32)      # a lattice: exact, with ties
    for start in (-1, P - 1):
        got = raw_fps(_lib.load(), [g], 8, start)
        check_fps(got, 0, g, 8, start, f"P={P} start={start}")


def test_fps_batch_equals_single_and_reruns(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    sets = [lattice(), np.zeros((0, 3), np.float32), cloud(THREADS + 3, 21)]
    starts = [-1, -1, 7]
    whole = raw_fps(lib, sets, 12, starts)
    again = raw_fps(lib, sets, 12, starts)
    assert np.array_equal(whole[0], again[0]) and np.array_equal(bits(whole[1]), bits(again[1]))
    assert whole[0][1].tolist() == [-1] * 12
    for b, (s, st) in enumerate(zip(sets, starts)):
        alone = raw_fps(lib, [s], 12, st)
        assert np.array_equal(alone[0][0], whole[0][b]) and np.array_equal(bits(alone[1][0]), bits(whole[1][b])), b


@pytest.mark.parametrize("P,n,scale", [(300, 64, 1.0), (THREADS + 200, 48, 1e-3), (THREADS * REG + 77, 24, 1e3)])
def test_fps_random_points_with_a_margin(ops, P, n, scale):
    from rnnpose_amd import _lib
    pts = cloud(P, 7 * P, scale)
    for start in (-1, 11):
        margin = mr.fps(pts, n, start, want_margin=True)[2]
        print(f"P={P} start={start}: smallest relative margin {margin:.3e}")
        assert margin >= 1e-9                                                       # the set qualifies (on the CPU, first)
        check_fps(raw_fps(_lib.load(), [pts], n, start), 0, pts, n, start, f"random P={P}")


# ---- pinned to the reference ---------------------------------------------------------------------------------------------------------------
def test_fragments_reproduce_the_reference(ops):
    from rnnpose_amd import model_prep
    g = np.load(os.path.join(GOLDEN, "fps_fragments.npz"))
    verts = np.random.default_rng(0).standard_normal((300, 3)).astype(np.float32)
    assert float(g["pick_margin"]) >= 1e-5 and float(g["assign_margin"]) >= 1e-5
    assert np.array_equal(mr.fps(verts, 64)[0], g["center_inds"])                  # the restatement, on the CPU
    centers, inds, ids = model_prep.fragments(dev(verts), 64)
    assert npy(inds).shape == (64,) and npy(ids).shape == (300,)
    assert np.array_equal(npy(inds), g["center_inds"]) and np.array_equal(npy(ids), g["vertex_frag_ids"])
    assert np.array_equal(npy(centers), verts[g["center_inds"]])


# ---- bad arguments -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_1_and_write_nothing(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    sets = [cloud(TILE + 9, 31), cloud(40, 32)]
    pts, total, off = pack(sets)
    B, n = 2, 6
    nd, nf = int(lib.rnnpose_point_diameter_workspace_bytes(total, B)), int(lib.rnnpose_fps_workspace_bytes(total, B))
    assert nd == 2 * 3 * 16 and nf == total * 8
    for f in (lib.rnnpose_point_diameter_workspace_bytes, lib.rnnpose_fps_workspace_bytes):
        assert f(total, 0) == 0 and f(-1, B) == 0 and f(0, 1) > 0
    assert lib.rnnpose_point_diameter_workspace_bytes((1 << 20) + 1, 1) == 0
    full = lambda m, dt: torch.full((m,), CANARY, dtype=dt).cuda()
    ws = full(max(nd, nf) // 8 + 8, torch.float64)
    d2, dm, pair, bnd = full(B, torch.float64), full(B, torch.float64), full(2 * B, torch.int32), full(6 * B, torch.float32)
    idx, dist2, st = full(B * n, torch.int32), full(B * n, torch.float64), dev([-1, -1], np.int32)
    good = dict(p=ptr(pts), off=ptr(off), total=total, B=B, ws=ptr(ws), n=nd, d2=ptr(d2), dm=ptr(dm), pair=ptr(pair), bnd=ptr(bnd), stream=None)
    bad = [dict(p=None), dict(off=None), dict(ws=None), dict(d2=None), dict(dm=None), dict(pair=None), dict(bnd=None), dict(B=0), dict(B=-2),
           dict(total=-1), dict(n=nd - 8), dict(n=0), dict(total=(1 << 20) + 1)]
    for change in bad:
        assert lib.rnnpose_point_diameter_f64(*dict(good, **change).values()) == 1, change
        assert len(lib.rnnpose_last_error()) > 0
    goodf = dict(p=ptr(pts), off=ptr(off), total=total, B=B, n=n, st=ptr(st), ws=ptr(ws), nb=nf, idx=ptr(idx), dist2=ptr(dist2), stream=None)
    badf = [dict(p=None), dict(off=None), dict(st=None), dict(ws=None), dict(idx=None), dict(dist2=None), dict(n=0), dict(n=-3), dict(B=0),
            dict(B=-1), dict(total=-1), dict(nb=nf - 8), dict(nb=0)]
    for change in badf:
        assert lib.rnnpose_fps_f64(*dict(goodf, **change).values()) == 1, change
        assert len(lib.rnnpose_last_error()) > 0
    torch.cuda.synchronize()
    assert all(bool((v == CANARY).all()) for v in (ws, d2, dm, pair, bnd, idx, dist2))
    assert lib.rnnpose_point_diameter_f64(*good.values()) == 0 and lib.rnnpose_fps_f64(*goodf.values()) == 0      # ... and these are fine
    torch.cuda.synchronize()
    assert npy(d2)[0] == mr.diameter(sets[0])[0] and np.array_equal(npy(idx).reshape(B, n)[1], mr.fps(sets[1], n)[0])


def test_ops_wrappers_refuse_bad_inputs(ops):
    pts = dev(cloud(50, 41))
    ok = ops.point_diameter(pts, [0, 20, 50])
    assert npy(ok[0]).tolist() == [mr.diameter(cloud(50, 41)[:20])[0], mr.diameter(cloud(50, 41)[20:])[0]]
    assert np.array_equal(npy(ops.farthest_points(pts, 5, [0, 20, 50], [-1, 3])[0][1]), mr.fps(cloud(50, 41)[20:], 5, 3)[0])
    i32 = lambda v: dev(v, np.int32)
    refused = [
        lambda: ops.point_diameter(pts.double()),                                   # dtype (the device: with the torch ops, below)
        lambda: ops.farthest_points(pts.half(), 4),
        lambda: ops.point_diameter(pts, i32([0, 50]).long()),
        lambda: ops.farthest_points(pts, 4, None, i32([0]).long()),
        lambda: ops.point_diameter(pts[:, :2]),                                     # shape, contiguity
        lambda: ops.point_diameter(pts[::2]),
        lambda: ops.farthest_points(pts.t(), 4),
        lambda: ops.point_diameter(pts, [0, 30, 20, 50]),                           # offsets that decrease, leave the array, are too few
        lambda: ops.farthest_points(pts, 4, [0, 30, 20, 50]),
        lambda: ops.point_diameter(pts, [0, 51]),
        lambda: ops.point_diameter(pts, [-1, 50]),
        lambda: ops.farthest_points(pts, 4, [50]),
        lambda: ops.farthest_points(pts, 0),                                        # n, start
        lambda: ops.farthest_points(pts, 4, None, -2),
        lambda: ops.farthest_points(pts, 4, [0, 20, 50], [0]),
        lambda: ops.farthest_points(pts, 4, [0, 20, 50], i32([0, 0, 0])),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")


# ---- torch ops -----------------------------------------------------------------------------------------------------------------------------
def test_torch_ops_equal_ops_and_have_fake_kernels(ops):
    """torch.ops.rnnpose.point_diameter / farthest_points give what the ops wrappers give, their fake kernels the shapes and dtypes; and
    the wrappers refuse a tensor on the CPU."""
    import rnnpose_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    pts = dev(np.concatenate([cloud(TILE + 9, 51), lattice()]))
    off = [0, TILE + 9, TILE + 9 + 125]
    want = ops.point_diameter(pts, off)
    got = torch.ops.rnnpose.point_diameter(pts, torch.tensor(off))
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and float(got[1].min()) > 0
    assert torch.equal(torch.ops.rnnpose.point_diameter(pts)[0], ops.point_diameter(pts)[0])
    wantf = ops.farthest_points(pts, 9, off, [-1, 4])
    gotf = torch.ops.rnnpose.farthest_points(pts, 9, torch.tensor(off), torch.tensor([-1, 4]))
    assert all(torch.equal(a, b) for a, b in zip(gotf, wantf)) and int(gotf[0][1, 0]) == 4
    assert torch.equal(torch.ops.rnnpose.farthest_points(pts, 9)[0], ops.farthest_points(pts, 9)[0])
    with pytest.raises(ValueError):
        torch.ops.rnnpose.point_diameter(pts, torch.tensor([0, 400, 300]))
    for call in (lambda: ops.point_diameter(pts.cpu()), lambda: ops.farthest_points(pts.cpu(), 4)):      # (here: the host tier has one device)
        with pytest.raises(ValueError):
            call()
            pytest.fail("a CPU tensor was accepted")
    with FakeTensorMode():
        e = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="cuda", dtype=dtype)
        f = torch.ops.rnnpose.point_diameter(e(390, 3), e(3, dtype=torch.int64))
        assert [(tuple(t.shape), t.dtype, t.device.type) for t in f] == [(tuple(t.shape), t.dtype, "cuda") for t in got]
        f = torch.ops.rnnpose.farthest_points(e(390, 3), 9, e(3, dtype=torch.int64), e(2, dtype=torch.int64))
        assert [(tuple(t.shape), t.dtype, t.device.type) for t in f] == [(tuple(t.shape), t.dtype, "cuda") for t in gotf]
        assert [tuple(t.shape) for t in torch.ops.rnnpose.farthest_points(e(390, 3), 5)] == [(1, 5), (1, 5)]


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def write_ply(path, verts, colors, faces):
    """binary_little_endian, uchar colours, faces as lists (triangles and quads)"""
    head = (f"ply\nformat binary_little_endian 1.0\ncomment written by the test\nelement vertex {len(verts)}\nproperty float x\nproperty float y\n"
            f"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face {len(faces)}\n"
            "property list uchar int vertex_indices\nend_header\n")
    rec = np.zeros(len(verts), np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    rec["p"], rec["c"] = verts, colors
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(rec.tobytes())
        for f in faces:
            fh.write(np.uint8(len(f)).tobytes() + np.asarray(f, "<i4").tobytes())


def make_net(name):
    import desc3d_fp64 as R
    from rnnpose_amd.descriptor3d import KPSuperpoint3Dv2
    cfg = R.DESC if name == "desc" else R.CTX
    net = KPSuperpoint3Dv2(dict(cfg))
    w = R.make_weights({k: tuple(v.shape) for k, v in net.state_dict().items()}, cfg, R.SEEDS[name])
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    return net.cuda().eval()


def test_end_to_end_from_a_ply_file_to_matches_on_a_subset(ops, tmp_path):
    from rnnpose_amd import eval_epoch as ee, model_prep
    from rnnpose_amd.descriptor3d import class_features
    from rnnpose_amd.pose_init import DescriptorPoseInitializer
    from rnnpose_amd.rasterizer import MeshRenderer
    verts, faces = ee._ellipsoid(3, (0.06, 0.045, 0.035))                          # 642 vertices
    verts = verts.astype(np.float32)
    colors = np.random.default_rng(3).integers(0, 256, (len(verts), 3)).astype(np.uint8)
    # one quad in place of two triangles that share an edge: (a, b, c) and (a, c, d) -> (a, b, c, d)
    a, b, c = [int(v) for v in faces[0]]
    mate = next(k for k in range(1, len(faces)) if {a, c} <= set(faces[k].tolist()))
    d = next(int(v) for v in faces[mate] if int(v) not in (a, c))
    rest = [f.tolist() for k, f in enumerate(faces) if k not in (0, mate)]
    path = str(tmp_path / "object.ply")
    write_ply(path, verts, colors, [[a, b, c, d]] + rest)
    desc, ctx = make_net("desc"), make_net("ctx")
    limits = [40, 40, 40, 40]
    cm = model_prep.build_class_model("thing", path, desc, ctx, limits, n_eval_points=100)
    assert isinstance(cm, ee.ClassModel) and cm.name == "thing" and cm.symmetries is None
    assert np.array_equal(bits(cm.verts), bits(verts))                            # bit for bit
    assert cm.faces.shape == (len(faces), 3) and cm.faces[:2].tolist() == [[a, b, c], [a, c, d]] and cm.faces[2:].tolist() == rest
    assert np.array_equal(cm.colors, colors.astype(np.float32) / np.float32(255))
    dd = verts.astype(np.float64)[:, None] - verts.astype(np.float64)[None]
    brute = np.sqrt(((dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]).max())
    assert cm.diameter == brute
    fea, geo = class_features(dev(verts), desc, ctx, limits)
    assert torch.equal(cm.fea_3d, fea) and torch.equal(cm.geofea_3d, geo) and tuple(geo.shape) == (1, len(verts), 32)
    assert np.array_equal(cm.eval_points, verts[mr.fps(verts, 100)[0]])
    assert model_prep.build_class_model("bare", path).fea_3d is None and model_prep.build_class_model("bare", path).eval_points is None
    scaled = model_prep.build_class_model("mm", path, scale=1000.0)
    assert np.array_equal(scaled.verts, verts * np.float32(1000.0)) and scaled.diameter == mr.diameter(verts * np.float32(1000.0))[1]

    # one rendered frame, matched against the 64-point subset and against a hand-built 64-row table
    models = {"thing": cm}
    renderer = MeshRenderer({"thing": dict(verts=cm.verts, faces=cm.faces, colors=cm.colors)}, device="cuda")
    item = ee.synthetic_scenes(models, 1, 1, image_size=(240, 320), renderer=renderer)[0]
    g2 = item.geofea_2d.cuda()[None].contiguous()
    box = np.array([[0, 0, 319, 239]], np.int32)
    sub = mr.fps(verts, 64)[0]
    hand = ee.ClassModel("thing", verts[sub], np.zeros((1, 3), np.int32), cm.colors[sub], None, cm.geofea_3d[:, torch.as_tensor(sub).long().cuda()], cm.diameter)
    init = DescriptorPoseInitializer(models, "cuda", point_subset=64)
    got = init.match(["thing"], g2, [0], box)
    want = DescriptorPoseInitializer({"thing": hand}, "cuda").match(["thing"], g2, [0], box)
    n = int(got[4][0])
    print(f"{n} matches on the 64-point subset")
    assert n > 0 and all(torch.equal(g, w) for g, w in zip(got, want))            # X, x, sim, point_idx, count
    assert np.array_equal(npy(init.subset_index["thing"]), sub)
    back = npy(init.subset_index["thing"])[npy(got[3][0, :n])]
    assert np.array_equal(verts[back], npy(got[0][0, :n]))
    plain, today = DescriptorPoseInitializer(models, "cuda", point_subset=None), DescriptorPoseInitializer(models, "cuda")
    full = plain.match(["thing"], g2, [0], box)
    assert all(torch.equal(g, w) for g, w in zip(full, today.match(["thing"], g2, [0], box))) and int(full[4][0]) > 0
    roomy = DescriptorPoseInitializer(models, "cuda", point_subset=len(verts))      # a class with at most N vertices: today's path
    assert all(torch.equal(g, w) for g, w in zip(full, roomy.match(["thing"], g2, [0], box))) and roomy.subset_index["thing"] is None
