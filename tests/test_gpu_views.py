"""The grouped (multi-view) LM step (csrc/lm.hip: lm_views_tail_kernel behind lm_eq_kernel<., false>; rnnpose_lm_step_views_io_f32;
DESIGN.md section 19) against the fp64 restatement tests/views_ref.py: the per-view systems bit-identical to the ungrouped entries, the
group system within the fp64 rounding bound of its sum, the solve, the pose update, the degenerate case == the ungrouped steps, the
coupling of a view without data to the views with data, output views / workspace slots, bad arguments and the dispatcher operator (run
with -m gpu on an MI355X; everything but the dispatcher test also runs on the host-executed kernels, tests/test_views_on_host.py).

Scenes are those of tests/test_gpu_rgbd.py (`_scene`): the arithmetic checks need no geometric consistency between the views of a group,
only the coupling test builds one rigid body seen by three cameras."""
import ctypes as C

import numpy as np
import pytest
import torch

import views_ref as vr
from rnnpose_amd import synthetic as syn
from test_gpu_lm_geometry import _clone, _guarded, _same
from test_gpu_parity import D, N, T, close, ops  # noqa: F401  (ops: the module-scoped build fixture)
from test_gpu_rgbd import CROPS, HO, PARAMS, WO, _rgbd_args, _scene, _seed, _sphere_plane_depth, _weight

pytestmark = pytest.mark.gpu

# (id, group sizes): singletons around a group of three; two pairs; one group wider than any unrolled width
LAYOUTS = [("1_3_1", [1, 3, 1]), ("2_2", [2, 2]), ("9", [9])]
EPS64, EPS32 = 2.0 ** -52, 2.0 ** -24


def _starts(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def _rig(sizes, seed):
    """camera-from-rig of every view: rotations of up to 80 degrees about random axes, translations of up to 1 m; the views of a
    group of one are the rig itself (E = I)"""
    rng = np.random.default_rng(seed)
    E = []
    for n in sizes:
        for _ in range(n):
            axis = rng.standard_normal(3)
            ang = np.deg2rad(rng.uniform(20.0, 80.0)) * rng.choice([-1.0, 1.0])
            t = rng.uniform(-1.0, 1.0, 3)
            e = vr.se3_exp(np.concatenate([np.zeros(3), axis / np.linalg.norm(axis) * ang]))
            e[:3, 3] = t
            E.append(np.eye(4) if n == 1 else e)
    return np.stack(E).astype(np.float32)


def _case(name, H, W, sizes):
    B = sum(sizes)
    s = _scene(name, B, H, W, False, _seed(name, B, False))
    E = _rig(sizes, _seed(name, B, True))
    return s, _weight("desc", s), E, _starts(sizes)


def _depth_kw(args):
    return dict(obs_depth=args[5], theta=args[6], K_obs=args[7], src_index=args[8], **PARAMS)


# ------------------------------------------------------------------------------------------------ 1-4. one grouped step against the restatement
@pytest.mark.parametrize("lname,sizes", LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize("name,H,W", CROPS, ids=[c[0] for c in CROPS])
def test_views_step_vs_restatement(ops, name, H, W, lname, sizes):
    s, wgt, E, starts = _case(name, H, W, sizes)
    B, ng = s["B"], len(sizes)
    args = _rgbd_args(s, "absolute", wgt)
    groups = ops.ViewGroups(starts, E, B, "cuda")
    assert groups.n_groups == ng and groups.host == tuple(starts)
    for term in ("plain", "depth"):
        what = f"{name} {lname} {term}"
        kw = dict(rgbd=_depth_kw(args)) if term == "depth" else {}
        out = _clone(ops.lm_step_views(*args[:5], groups, num_iters=1, **kw))
        G, Hm, bv, Hg, bg, xi, info = out[:7]
        # 1. every view's system is the ungrouped entry's, bit for bit
        if term == "depth":
            want = ops.lm_normal_eq_rgbd(*args, **PARAMS)
            assert torch.equal(Hm, want[0]) and torch.equal(bv, want[1]) and torch.equal(out[7], want[2]), f"per-view systems ({what})"
            assert float(out[7][:, 0].max()) > 0
        else:
            want = ops.lm_normal_eq(*args[:5])
            assert torch.equal(Hm, want[0]) and torch.equal(bv, want[1]), f"per-view systems ({what})"
            assert len(out) == 7
        # 2. the group system: fp64 rounding bound of a 36 V-term sum, with margin
        wH, wb = vr.group_system(N(Hm), N(bv), E, starts)
        aH, ab = vr.group_system(N(Hm), N(bv), E, starts, absolute=True)
        for g, V in enumerate(sizes):
            eH, eb = np.abs(N(Hg)[g] - wH[g]), np.abs(N(bg)[g] - wb[g])
            print(f"GROUP {what} group {g} (V = {V}): max |Hg - ref| / bound {float((eH / (64 * V * EPS64 * aH[g] + 1e-300)).max()):.3e}, "
                  f"b {float((eb / (64 * V * EPS64 * ab[g] + 1e-300)).max()):.3e}")
            assert (eH <= 64 * V * EPS64 * aH[g]).all(), f"Hg ({what}, group {g})"
            assert (eb <= 64 * V * EPS64 * ab[g]).all(), f"bg ({what}, group {g})"
        assert torch.equal(Hg, Hg.transpose(1, 2)), f"Hg is not symmetric ({what})"
        assert _same(out, ops.lm_step_views(*args[:5], groups, num_iters=1, **kw)), f"two launches differ ({what})"
        # 3. the solve of the damped group system
        wxi, winfo = vr.solve(N(Hg), N(bg))
        close(xi, wxi, 1e-6, what=f"xi ({what})")                       # (the bound of tests/test_gpu_lm_geometry.py's solve tests)
        assert np.array_equal(N(info), winfo) and int(info.abs().sum()) == 0 and float(xi.abs().max()) > 0, what
        # 4. the pose update from the kernel's own xi
        wG = vr.apply_increment(N(s["G"]), E, N(xi), starts)
        sc = max(1.0, float(np.abs(E).max()), float(s["G"].abs().max()))
        err = float(np.abs(N(G) - wG).max())
        print(f"UPDATE {what}: max |G - E exp(xi) E^-1 G| {err:.3e}, bound {32 * EPS32 * sc * sc:.3e}")
        assert err <= 32 * EPS32 * sc * sc, f"G ({what})"
        chained = (args[4],)
        for _ in range(3):
            chained = _clone(ops.lm_step_views(*args[:4], chained[0], groups, num_iters=1, **kw))
        assert _same(_clone(ops.lm_step_views(*args[:5], groups, num_iters=3, **kw)), chained), f"three iterations != three chained steps ({what})"


# ------------------------------------------------------------------------------------------------ 5. groups of one with E = I == the ungrouped steps
@pytest.mark.parametrize("name,H,W", CROPS, ids=[c[0] for c in CROPS])
def test_views_groups_of_one_are_the_ungrouped_steps_bit_for_bit(ops, name, H, W):
    B = 3
    s = _scene(name, B, H, W, False, _seed(name, B, False))
    wgt = _weight("desc", s)
    args = _rgbd_args(s, "absolute", wgt)
    for groups in (ops.ViewGroups(list(range(B + 1)), None, B, "cuda"), ops.ViewGroups([0, 1, 2], torch.eye(4).repeat(B, 1, 1), B, "cuda")):
        for iters in (1, 3):
            plain = _clone(ops.lm_step(*args[:5], num_iters=iters))
            got = _clone(ops.lm_step_views(*args[:5], groups, num_iters=iters))
            assert _same((got[0], got[1], got[2], got[5], got[6]), plain), f"{name} iters={iters}: plain"
            assert torch.equal(got[3], got[1]) and torch.equal(got[4], got[2]), f"{name} iters={iters}: Hg, bg"
            rgbd = _clone(ops.lm_step_rgbd(*args, num_iters=iters, **PARAMS))
            got = _clone(ops.lm_step_views(*args[:5], groups, rgbd=_depth_kw(args), num_iters=iters))
            assert _same((got[0], got[1], got[2], got[5], got[6], got[7]), rgbd), f"{name} iters={iters}: depth-aware"
            assert torch.equal(got[3], got[1]) and torch.equal(got[4], got[2]), f"{name} iters={iters}: Hg, bg (depth-aware)"


# ------------------------------------------------------------------------------------------------ 6. coupling
def _rot_y(deg):
    return vr.se3_exp(np.array([0, 0, 0, 0, np.deg2rad(deg), 0.0]))


def test_views_coupling_a_view_without_data_follows_the_group(ops):
    """One rigid body seen by three cameras (in every camera a sphere in front of a plane, rendered where the estimate stands: G = I),
    displaced by Delta* in the rig frame: the targets of view v are the re-projections under E_v Delta* E_v^-1.  View 0 has all-zero
    weights.  Grouped, it follows the other two to E_0 Delta* E_0^-1 (1e-5 after the 8 iterations of
    test_gpu_rgbd.test_rgbd_exact_recovery_of_a_displaced_pose); the plain step leaves it where it started."""
    H, W, B = 96, 128, 3
    K = np.array([[140.0, 0, 63.5], [0, 140.0, 47.5], [0, 0, 1]], np.float64)
    E = np.stack([_rot_y(10.0), _rot_y(40.0), _rot_y(-30.0)])
    E[:, :3, 3] = [[0.05, 0.02, 0.1], [-0.6, 0.0, 0.25], [0.5, -0.05, 0.15]]
    E = E.astype(np.float32)
    Ds = vr.se3_exp(np.array([0.004, -0.003, 0.04, 0.01, -0.015, 0.02]))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    tgt, wg, dp, Gs = [], [], [], []
    for v in range(B):
        centre, radius, plane_z = np.array([0.02 - 0.03 * v, -0.01 + 0.02 * v, 1.0 + 0.05 * v]), 0.2, 1.3
        dep, on_sphere = _sphere_plane_depth(K, H, W, centre, radius, plane_z)
        Ev = E[v].astype(np.float64)
        Gv = Ev @ Ds @ vr.rigid_inverse(Ev)
        Z0 = dep.astype(np.float32).astype(np.float64) + np.float64(np.float32(1e-5))
        P0 = np.stack([Z0 * (xs - K[0, 2]) / K[0, 0], Z0 * (ys - K[1, 2]) / K[1, 1], Z0], -1)
        P1 = P0 @ Gv[:3, :3].T + Gv[:3, 3]
        tgt.append(np.stack([K[0, 0] * P1[..., 0] / P1[..., 2] + K[0, 2], K[1, 1] * P1[..., 1] / P1[..., 2] + K[1, 2]], -1))
        wg.append(np.zeros((H, W)) if v == 0 else np.ones((H, W)))
        dp.append(dep[None])
        Gs.append(Gv)
    Gs = np.stack(Gs)
    args = (D(np.stack(tgt).astype(np.float32)), D(np.stack(wg).astype(np.float32)), D(np.stack(dp).astype(np.float32)),
            D(np.tile(K[None], (B, 1, 1)).astype(np.float32)))
    groups = ops.ViewGroups([0, B], E, B, "cuda")
    start = torch.eye(4, device="cuda").repeat(B, 1, 1)
    for ep in (100.0, 0.0):
        G = start.clone()
        for k in range(8):
            G, Hm, bv, Hg, bg, xi, info = ops.lm_step_views(*args, G, groups, num_iters=1, ep_lambda=ep)
            errs = np.abs(N(G) - Gs).reshape(B, -1).max(1)
            print(f"COUPLING ep_lambda={ep} step {k}: max |G_v - E_v D* E_v^-1| per view {errs}  |xi| {float(xi.abs().max()):.3e}")
            assert int(info.abs().sum()) == 0
        assert float(Hm[0].abs().max()) == 0.0 and float(bv[0].abs().max()) == 0.0          # view 0 contributes nothing
        assert errs[0] < 1e-5, f"view 0 did not follow (ep_lambda = {ep}): {errs}"
        assert (errs < 1e-5).all(), f"ep_lambda = {ep}: {errs}"
    plain = ops.lm_step(*args, start, num_iters=8)[0]
    assert torch.equal(plain[0], start[0]), "the ungrouped step moved a view without data"
    assert float(np.abs(N(plain)[1:] - Gs[1:]).max()) < 1e-5 and float(np.abs(N(plain)[0] - Gs[0]).max()) > 1e-2


# ------------------------------------------------------------------------------------------------ 7. output views, workspace slots, streams
CANARY = 1234.5


def _out_views(B, ng, depth):
    """the outputs of lm_step_views as views into ONE canary-filled fp64 buffer, four doubles apart"""
    sizes = [8 * B, 36 * B, 6 * B, 36 * ng, 6 * ng, 3 * ng, (ng + 1) // 2] + ([2 * B] if depth else [])
    buf = torch.full((sum(sizes) + 4 * (len(sizes) + 1),), CANARY, dtype=torch.float64, device="cuda")
    outside = torch.ones(buf.numel(), dtype=torch.bool)
    off, seg = 4, []
    for n in sizes:
        seg.append(buf[off:off + n])
        outside[off:off + n] = False
        off += n + 4
    views = (seg[0].view(torch.float32).view(B, 4, 4), seg[1].view(B, 6, 6), seg[2].view(B, 6), seg[3].view(ng, 6, 6), seg[4].view(ng, 6),
             seg[5].view(torch.float32).view(ng, 6), seg[6].view(torch.int32)[:ng]) + ((seg[7].view(B, 2),) if depth else ())
    return buf, views, outside


@pytest.mark.parametrize("name,H,W", CROPS, ids=[c[0] for c in CROPS])
def test_views_out_views_slots_and_streams(ops, name, H, W):
    sizes = [1, 3, 1]
    s, wgt, E, starts = _case(name, H, W, sizes)
    B, ng = s["B"], len(sizes)
    args = _rgbd_args(s, "planar", wgt)
    groups = ops.ViewGroups(starts, E, B, "cuda")
    for term in ("plain", "depth"):
        kw = dict(rgbd=_depth_kw(args)) if term == "depth" else {}
        for iters in (1, 3):
            want = _clone(ops.lm_step_views(*args[:5], groups, num_iters=iters, **kw))
            bufs = [_out_views(B, ng, term == "depth") for _ in range(2)]
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            torch.cuda.synchronize()
            for slot, (st, (buf, views, outside)) in enumerate(zip(streams, bufs)):
                with torch.cuda.stream(st):
                    got = ops.lm_step_views(*args[:5], groups, num_iters=iters, out=views, slot=slot, **kw)
                    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, views))
            torch.cuda.synchronize()
            for slot, (buf, views, outside) in enumerate(bufs):
                assert _same(views, want), f"{name} {term} iters={iters} slot={slot}: out= views differ"
                assert bool((buf.cpu()[outside] == CANARY).all()), f"{name} {term} iters={iters} slot={slot}: bytes outside the outputs were written"
            # a group-aligned batch part in its own slot: the refiner's chains
            buf, views, outside = _out_views(B, ng, term == "depth")
            for (b0, b1), (g0, g1) in (((0, 1), (0, 1)), ((1, 5), (1, 3))):
                part = groups.rows(b0, b1)
                pkw = dict(rgbd=dict(_depth_kw(args), obs_depth=args[5][b0:b1], theta=args[6][b0:b1], K_obs=args[7][b0:b1])) if term == "depth" else {}
                sub = tuple(v[b0:b1] for v in views[:3]) + tuple(v[g0:g1] for v in views[3:7]) + tuple(v[b0:b1] for v in views[7:])
                ops.lm_step_views(*(a[b0:b1] for a in args[:5]), part, num_iters=iters, out=sub, slot=b0, **pkw)
            assert _same(views, want) and bool((buf.cpu()[outside] == CANARY).all()), f"{name} {term} iters={iters}: group-aligned parts"
            # the fused step on the same workspace afterwards: the tail left its arrival counters at zero
            assert _same(_clone(ops.lm_step(*args[:5], num_iters=iters)), _clone(ops.lm_step(*args[:5], num_iters=iters, slot=7)))


# ------------------------------------------------------------------------------------------------ 8. bad arguments
def test_views_bad_arguments(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    B, H, W = 3, 8, 8
    s = _scene("8x8", B, H, W, False, 1)
    wgt = _weight("ones", s)
    t, w, d, K, G, obs, th, Ko = (D(x) for x in (s["absolute"], wgt, s["depth"], s["K"], s["G"], s["obs"], s["theta"], s["K_obs"]))
    E = D(_rig([3], 5))
    n = int(lib.rnnpose_lm_workspace_bytes(B, H, W))
    ws = torch.zeros(n // 8, dtype=torch.float64).cuda()
    ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    full = lambda shape, dt=torch.float64: torch.full(shape, 7, dtype=dt).cuda()

    def outputs(ng=B):
        return dict(Gn=full((B, 4, 4), torch.float32), Hm=full((B, 6, 6)), bv=full((B, 6)), Hg=full((ng, 6, 6)), bg=full((ng, 6)),
                    xi=full((ng, 6), torch.float32), info=full((ng,), torch.int32), ds=full((B, 2)))
    o = outputs()
    gs = i32([0, 2, 3])

    def step(tt=t, mode=0, Bc=B, iters=1, ob=None, S=B, dw=1.0, start=gs, ng=2, Ev=E, wsb=n, o=o, **nulls):
        p = {k: (None if k in nulls else v) for k, v in o.items()}
        return lib.rnnpose_lm_step_views_io_f32(ptr(tt), mode, ptr(w), ptr(d), 1e-5, ptr(K), ptr(G), ptr(p["Gn"]), Bc, H, W, iters, 100.0, 1e-4, 1.0,
                                                ptr(ob), None, ptr(th), ptr(Ko), S, HO, WO, dw, 0.05, 0.02, ptr(start), ng, ptr(Ev), ptr(ws), wsb,
                                                ptr(p["Hm"]), ptr(p["bv"]), ptr(p["Hg"]), ptr(p["bg"]), ptr(p["xi"]), ptr(p["info"]), ptr(p["ds"]),
                                                ops._stream())
    cases = [(dict(start=None), b"group_start"), (dict(Ev=None), b"group_start"), (dict(Hg=1), b"group_start"), (dict(bg=1), b"group_start"),
             (dict(xi=1), b"group_start"), (dict(info=1), b"group_start"), (dict(ng=0), b"n_groups"), (dict(ng=-1), b"n_groups"),
             (dict(ng=B + 1), b"n_groups"), (dict(tt=None), b"null"), (dict(Gn=1), b"null"), (dict(Hm=1), b"null"), (dict(bv=1), b"null"),
             (dict(mode=2), b"target_mode"), (dict(Bc=0), b"bad size"), (dict(Bc=65536), b"bad size"), (dict(iters=0), b"at least one iteration"),
             (dict(wsb=n - 1), b"workspace"),
             # with an observed depth: what the depth-aware entries refuse
             (dict(ob=obs, S=0), b"S >= 1"), (dict(ob=obs, S=1), b"src_index"), (dict(ob=obs, dw=-1.0), b"depth_weight"),
             (dict(ob=obs, dw=float("nan")), b"depth_weight")]
    for kw, msg in cases:
        assert step(**kw) == 1 and msg in lib.rnnpose_last_error(), (kw, lib.rnnpose_last_error())
    torch.cuda.synchronize()
    assert all(bool((x == 7).all()) for x in o.values()) and not bool(ws.any())               # refused before any launch
    # accepted: the plain sums ignore the other depth arguments; dstats may be null with the term on
    assert step(S=-3, dw=float("nan")) == 0 and step(ob=obs) == 0 and step(ob=obs, ds=1) == 0 and step(ng=B, start=i32([0, 1, 2, 3])) == 0
    torch.cuda.synchronize()
    assert not bool(ws[:B].any()), "the grouped step left an arrival counter non-zero"
    # an empty group, and contents outside [0, B], from hand-made device arrays: info = -1, nothing else of that group is written
    want = outputs(2)
    assert step(o=want) == 0
    # (start, {live group: the group of the regular layout it equals}); clamped to [0, 3]: [0, 2, 7, 3] is the regular layout and an
    # empty group behind it; [-5, 2, 99, 1] is [0, 2), [2, 3), empty; [0, 2, 2] leaves view 2 in no group
    for start, live in (([0, 2, 2, 3], {0: 0, 2: 1}), ([0, 2, 7, 3], {0: 0, 1: 1}), ([-5, 2, 99, 1], {0: 0, 1: 1}), ([0, 2, 2], {0: 0})):
        ng = len(start) - 1
        got = outputs(ng)
        assert step(start=i32(start), ng=ng, o=got) == 0
        torch.cuda.synchronize()
        assert N(got["info"]).tolist() == [0 if g in live else -1 for g in range(ng)], start
        for g in range(ng):
            for k in ("Hg", "bg", "xi"):
                assert torch.equal(got[k][g], want[k][live[g]]) if g in live else bool((got[k][g] == 7).all()), (start, g, k)
        if 1 in live.values():
            assert all(torch.equal(got[k], want[k]) for k in ("Gn", "Hm", "bv"))
        else:                                                           # view 2 is in no group: nothing of it is written
            assert all(torch.equal(got[k][:2], want[k][:2]) and bool((got[k][2] == 7).all()) for k in ("Gn", "Hm", "bv"))
    # ViewGroups refuses on the host
    good = N(E)
    for bad, msg in (([1, 3], "start at 0"), ([0, 2, 2, 3], "increase strictly"), ([0, 2, 4], "group_of_view"), ([0, 0, 2], "group_of_view"),
                     ([0, 1], "group_of_view"), ([], "at least one"), ([0, 1, 1, 3], "increase strictly")):
        with pytest.raises(ValueError, match=msg):
            ops.ViewGroups(bad, good, B, "cuda")
    with pytest.raises(ValueError, match="1-D integer"):
        ops.ViewGroups(torch.tensor([0.0, 3.0]), good, B, "cuda")
    for k, (idx, v) in enumerate((((0, 0, 0), float("nan")), ((1, 2, 3), float("inf")), ((2, 3, 0), 0.5), ((0, 3, 3), 2.0))):
        e = good.copy()
        e[idx] = v
        with pytest.raises(ValueError, match="last row"):
            ops.ViewGroups([0, 3], e, B, "cuda")
    with pytest.raises(ValueError, match="transforms"):
        ops.ViewGroups([0, 3], good[:2], B, "cuda")
    assert ops.ViewGroups([0, 0, 1], None, B, "cuda").host == (0, 2, 3) and ops.ViewGroups(torch.tensor([0, 3]), good, B, "cuda").host == (0, 3)
    g = ops.ViewGroups([0, 2, 3], good, B, "cuda")
    assert g.rows(0, 3) is g and g.rows(2, 3).host == (0, 1) and torch.equal(g.rows(2, 3).E, g.E[2:3]) and N(g.rows(0, 2).group_start).tolist() == [0, 2]
    with pytest.raises(ValueError, match="group boundaries"):
        g.rows(1, 3)
    a = (t, w, d, K, G)
    with pytest.raises(ValueError, match="cover"):
        ops.lm_step_views(*a, ops.ViewGroups([0, 2], None, 2, "cuda"))
    with pytest.raises(ValueError, match="num_iters"):
        ops.lm_step_views(*a, g, num_iters=0)
    with pytest.raises(TypeError, match="ViewGroups"):
        ops.lm_step_views(*a, [0, 2, 3])
    with pytest.raises(ValueError, match="rgbd"):
        ops.lm_step_views(*a, g, rgbd=dict(obs_depth=obs))
    with pytest.raises(ValueError, match="depth_gate"):
        ops.lm_step_views(*a, g, rgbd=dict(obs_depth=obs, theta=th, K_obs=Ko, depth_gate=-1.0))


# ------------------------------------------------------------------------------------------------ 9. dispatcher
def test_views_dispatcher_op_and_fake_kernel(ops):
    import rnnpose_amd.torch_ops  # noqa: F401
    name, H, W, sizes = "64x96", 64, 96, [2, 2]
    s, wgt, E, starts = _case(name, H, W, sizes)
    t, w, d, K, G = (D(x) for x in (s["flow"], wgt, s["depth"], s["K"], s["G"]))
    want = ops.lm_step_views(t, w, d, K, G, ops.ViewGroups(starts, E, s["B"], "cuda"), num_iters=2)
    gs, Ed = torch.tensor(starts, device="cuda"), D(E)
    Gn, xi, Hg, bg = torch.ops.rnnpose.lm_step_views(t, w, d, K, G, gs, Ed, 2)
    assert _same((Gn, xi, Hg, bg), (want[0], want[5], want[3], want[4]))
    with pytest.raises(ValueError, match="group_start"):
        torch.ops.rnnpose.lm_step_views(t, w, d, K, G, torch.tensor([0, 0, 1, 1], device="cuda"), Ed)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        fk = [mode.from_tensor(x) for x in (t, w, d, K, G, gs, Ed)]
        fake = torch.ops.rnnpose.lm_step_views(*fk)
    assert [f.shape for f in fake] == [x.shape for x in (Gn, xi, Hg, bg)] and [f.dtype for f in fake] == [x.dtype for x in (Gn, xi, Hg, bg)]
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.rnnpose.lm_step_views(*(x.detach().cpu() for x in (t, w, d, K, G, gs, Ed)))


# ------------------------------------------------------------------------------------------------ 10. end to end
def _about(centre, deg):
    """camera-from-rig of a camera turned by `deg` about the vertical axis through `centre`"""
    E = _rot_y(deg)
    E[:3, 3] = np.asarray(centre) - E[:3, :3] @ np.asarray(centre)
    return E


def test_views_end_to_end_refine_frame(ops, monkeypatch):
    """synthetic_scenes, 1 frame x 2 objects x 3 cameras (the rig turned by 0, +20, -20 degrees about the scene centre) at 240 x 320,
    crops of 128 x 128, schedule 2 x 2 x 1, random network weights as in the RGB-D end-to-end test; HipEpoch.refine_frame groups the
    items by object_id.  Graph replay == eager bit for bit and a graph was captured; every item its own group with cam_from_rig = None
    == today's refine_frame; the views of a group stay tied, |Ti_v - E_v T_rig| <= 32 n 2^-24 s^2 with n = 20 fp32 pose products per
    view: 2 to tie the initial poses, per outer iteration (2) the accumulate and the legacy product (2) and 3 per LM step (2), the
    final accumulate, and E_first^-1 Ti of T_rig.  A group that would straddle the cut of a two-chain schedule: the convolution kernel
    a launch takes depends on how many pixels it has (tests/test_gpu_refiner.test_two_chains_equal_one_chain), so one chain and two do
    not agree bit for bit at this shape; asserted instead: every chain's rows start and end at group starts, and the views stay tied.
    No accuracy claim with random weights: the tz errors of the grouped and ungrouped runs are printed for the record only."""
    import dataclasses
    from oracle import rnnpose_oracle as orc
    from rnnpose_amd import eval_epoch as ee
    from rnnpose_amd.pose_refiner import default_config
    torch.manual_seed(0)
    models = ee.synthetic_models(("ape", "cat", "glue"), sub=3)
    cfg = lambda: default_config(RENDER_ITER_COUNT=2, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=(240, 320), zoom_crop_size=(128, 128))

    def epoch(use_graph=True):
        hip = ee.HipEpoch(models, cfg=cfg())
        hip.refiner.use_graph = use_graph
        hip.refiner.cf_net.update_block.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
        hip.refiner.image_fea_enc.fnet.load_state_dict({k: T(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
        return hip

    centre = (0.0, 0.0, 0.83)
    cams = [_about(centre, a) for a in (0.0, 20.0, -20.0)]
    first = epoch()
    items = ee.synthetic_scenes(models, 1, 2, image_size=(240, 320), seed=3, renderer=first.renderer, cameras=cams)
    assert [it.object_id for it in items] == [(0, 0), (0, 1)] * 3 and [it.frame_id for it in items] == [(0, 0)] * 2 + [(0, 1)] * 2 + [(0, 2)] * 2
    assert all(float((it.depth > 0).float().mean()) > 0.005 for it in items)

    def tied(poses, T_rig, batch, what, n=20):
        obj = {}
        for it in batch:
            obj.setdefault(it.object_id, len(obj))
        Tr = N(T_rig).astype(np.float64)
        for j, it in enumerate(batch):
            want = np.asarray(it.cam_from_rig, np.float64) @ Tr[obj[it.object_id]]
            sc = max(1.0, float(np.abs(want).max()), float(np.abs(it.cam_from_rig).max()))
            err = float(np.abs(N(poses)[j] - want).max())
            print(f"TIED {what} item {j}: |Ti_v - E_v T_rig| {err:.3e}, bound {32 * n * EPS32 * sc * sc:.3e}")
            assert err <= 32 * n * EPS32 * sc * sc, (what, j, err)

    got = first.refine_frame(items).clone()
    rig = first.last_rig_poses.clone()
    assert rig.shape == (2, 4, 4) and bool(torch.isfinite(got).all())
    replay = first.refine_frame(items).clone()                         # a second call replays the captured graphs
    ref = first.refiner
    assert ref.use_graph and (ref._graph is not None or ref._graph_static is not None), "the grouped loop was not captured"
    eager = epoch(use_graph=False).refine_frame(items)
    assert torch.equal(got, eager) and torch.equal(replay, eager), "graph replay != eager launches with view groups"
    tied(got, rig, items, "grouped")
    # every item its own group, one camera == today's refine_frame
    bare = [dataclasses.replace(it, object_id=None, cam_from_rig=None) for it in items]
    solo = [dataclasses.replace(it, object_id=("solo", j), cam_from_rig=None) for j, it in enumerate(items)]
    today = epoch().refine_frame(bare).clone()
    solo_epoch = epoch()
    assert torch.equal(solo_epoch.refine_frame(solo), today), "groups of one != the ungrouped refine_frame"
    assert solo_epoch.last_rig_poses.shape == (6, 4, 4) and torch.equal(solo_epoch.last_rig_poses, today)
    # the caller's order is kept: the same items shuffled give the same poses per item
    perm = [3, 0, 5, 2, 1, 4]
    sh_epoch = epoch()
    shuffled = sh_epoch.refine_frame([items[j] for j in perm])
    tied(shuffled, sh_epoch.last_rig_poses, [items[j] for j in perm], "shuffled")          # (groups in order of first appearance)
    assert shuffled.shape == got.shape
    # a group that would straddle the cut of a two-chain schedule: B = 5, groups [3, 2], the half-batch cut at row 2 moves to row 3
    five = [it for j, it in enumerate(sorted(items, key=lambda it: it.object_id)) if j != 5]
    monkeypatch.setenv("RNNPOSE_PARTS", "2")
    two = epoch()
    p2 = two.refine_frame(five).clone()
    vg = dict(groups=next(iter(two._view_groups.values())))
    assert vg["groups"].host == (0, 3, 5) and two.refiner._chains(5, vg) == [(0, 3), (3, 5)], two.refiner._chains(5, vg)
    assert two.refiner.cf_net.engine().halves(5) == [(0, 2), (2, 5)]
    tied(p2, two.last_rig_poses, five, "two chains")
    monkeypatch.delenv("RNNPOSE_PARTS")
    one = epoch()
    p1 = one.refine_frame(five)
    assert one.refiner._chains(5, vg) == [(0, 5)]
    tied(p1, one.last_rig_poses, five, "one chain")
    print(f"CHAINS max |poses(two chains) - poses(one chain)| {float((p1 - p2).abs().max()):.3e} (for the record: kernel choice depends on the launch size)")
    gt_z = np.array([it.pose_gt[2, 3] for it in items])
    e_grouped, e_today = np.abs(N(got)[:, 2, 3] - gt_z), np.abs(N(today)[:, 2, 3] - gt_z)
    print(f"END_TO_END |tz| error per item: grouped {np.round(e_grouped, 5)} mean {e_grouped.mean():.6f}; ungrouped {np.round(e_today, 5)} mean {e_today.mean():.6f}")
