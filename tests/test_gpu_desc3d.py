"""KPSuperpoint3Dv2 on the HIP kernels (rnnpose_amd/descriptor3d.py, csrc/nhwc_ops.hip): against the reference's own outputs
(tests/golden/desc3d.npz), against the fp64 restatement of tests/desc3d_fp64.py at 20 000 points, each kernel against fp64,
the radius search and grid subsampling against their numpy restatements (exactly), determinism and the interface."""
import os
import sys

import numpy as np
import pytest
import torch


pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import desc3d_fp64 as R  # noqa: E402

L = R.BASE["num_layers"]
GATE = 2e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from rnnpose_amd import build, ops as _ops
    build.build()
    return _ops


def D(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    return t if dt is None else t.to(dt)


def make_net(name):
    from rnnpose_amd.descriptor3d import KPSuperpoint3Dv2
    cfg = R.DESC if name == "desc" else R.CTX
    net = KPSuperpoint3Dv2(dict(cfg))
    w = R.make_weights({k: tuple(v.shape) for k, v in net.state_dict().items()}, cfg, R.SEEDS[name])
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    return net.cuda().eval(), w, cfg


def fixture_batch(g, case, idx_dtype=torch.int64):
    return {"points": [D(g[f"{case}_points_{l}"]) for l in range(L)],
            "neighbors": [D(g[f"{case}_neighbors_{l}"], idx_dtype) for l in range(L)],
            "pools": [D(g[f"{case}_pools_{l}"], idx_dtype) for l in range(L - 1)] + [torch.zeros(0, 1, dtype=idx_dtype, device="cuda")],
            "upsamples": [D(g[f"{case}_upsamples_{l}"], idx_dtype) for l in range(L - 1)] + [torch.zeros(0, 1, dtype=idx_dtype, device="cuda")],
            "features": torch.ones(g[f"{case}_points_0"].shape[0], 1, device="cuda"),
            "stack_lengths": [torch.from_numpy(g[f"{case}_lengths_{l}"]) for l in range(L)]}


def gate(name, ref):
    return GATE if name == "desc" else GATE * max(1.0, float(np.abs(ref).max()))


# ---- the whole network ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("name", ["desc", "ctx"])
def test_desc3d_matches_the_reference_fixture(ops, golden, case, name):
    g = golden("desc3d")
    net, _, _ = make_net(name)
    n0 = g[f"{case}_points_0"].shape[0]
    y = net(fixture_batch(g, case, torch.int32 if case == "b" else torch.int64))
    assert tuple(y.shape) == (n0, R.DESC["final_feats_dim"] if name == "desc" else R.CTX["final_feats_dim"]) and y.dtype == torch.float32
    y = y[torch.from_numpy(R.output_rows(n0, name)).cuda()]
    want = g[f"{case}_{name}"]
    assert tuple(y.shape) == want.shape
    err = float(np.abs(y.cpu().numpy() - want).max())
    print(f"{case}/{name}: max|HIP - reference| = {err:.2e}")
    assert err <= gate(name, want)


def big_batch(ops, n=20000):
    from rnnpose_amd.descriptor3d import kpconv_inputs
    pts = R.ellipsoid_cloud("big", n, axes=(0.5, 0.4, 0.3))
    return kpconv_inputs(D(pts), R.DESC, [40, 40, 40, 40]), pts


@pytest.mark.parametrize("name", ["desc", "ctx"])
def test_desc3d_at_20000_points_vs_fp64(ops, name):
    batch, _ = big_batch(ops)
    net, w, cfg = make_net(name)
    y = net(batch).double()
    ref = R.Net64(w, cfg, device="cuda")
    want = ref(batch)
    keep = ~ref.uncertain
    excluded = int((~keep).sum())
    err = float((y - want)[keep].abs().max())
    print(f"20000 points {name}: levels {[p.shape[0] for p in batch['points']]}, widths {[n.shape[1] for n in batch['neighbors']]}, "
          f"max|HIP - fp64| = {err:.2e}, close count decisions {ref.n_close}, excluded points {excluded}")
    assert excluded <= 1e-3 * y.shape[0]
    assert err <= gate(name, want.abs().max().item())


def test_desc3d_is_deterministic(ops, golden):
    g = golden("desc3d")
    net, _, _ = make_net("ctx")
    b = fixture_batch(g, "a")
    y1, y2 = net(b).clone(), net(b).clone()
    assert torch.equal(y1, y2)
    batch, _ = big_batch(ops, 6000)
    batch2, _ = big_batch(ops, 6000)
    for k in ("neighbors", "pools", "upsamples", "points"):
        for a, c in zip(batch[k], batch2[k]):
            assert torch.equal(a, c), k
    assert torch.equal(net(batch), net(batch2))


# ---- kernels against fp64 ----------------------------------------------------------------------------------------------------------
def kpconv64(q, s, nb, kp, extent, x, W):
    q, s, kp, x, W = (torch.as_tensor(v).double() for v in (q, s, kp, x, W))
    nb = torch.as_tensor(nb).long()
    s_ = torch.cat([s, torch.full_like(s[:1], 1e6)])
    d2 = (((s_[nb] - q[:, None])[:, :, None, :] - kp) ** 2).sum(-1)
    infl = torch.clamp(1 - torch.sqrt(d2) / extent, min=0)
    x_ = torch.cat([x, torch.zeros_like(x[:1])])
    out = torch.einsum("nmk,nmc,kco->no", infl, x_[nb], W)
    cnt = (x_.sum(1)[nb] > 0).sum(1).clamp(min=1)
    return out / cnt[:, None]


@pytest.mark.parametrize("c_in,n", [(1, 500), (32, 700), (64, 300), (128, 220), (256, 100)])
def test_kpconv_vs_fp64(ops, c_in, n):
    rng = np.random.default_rng(c_in)
    s = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    q = s[: n // 2] + rng.normal(0, 0.01, (n // 2, 3)).astype(np.float32)
    x = rng.normal(0.3, 1.0, (n, c_in)).astype(np.float32)
    x[::7] = -np.abs(x[::7])                                     # rows with a non-positive sum: not counted
    x[::11] = 0.0
    nb = np.full((n // 2, 40), n, np.int64)                     # shadow padding
    for i in range(n // 2):
        d = np.linalg.norm(s - q[i], axis=1)
        idx = np.argsort(d, kind="stable")[: rng.integers(0, 41)]
        nb[i, : len(idx)] = idx
    nb[3] = n                                                   # all-shadow rows
    nb[5] = n
    kp = rng.uniform(-0.1, 0.1, (15, 3)).astype(np.float32)
    kp[0] = 0
    c_out = 64 if c_in == 1 else c_in
    W = rng.normal(0, (2.0 / (15 * c_in)) ** 0.5, (15, c_in, c_out)).astype(np.float32)
    extent = 0.12
    t = ops.neighbor_table(D(nb), n)
    wf = ops.kpconv_aggregate(D(q), D(s), t, D(kp), extent, D(x))
    y = ops.point_linear(wf, D(W).reshape(15 * c_in, c_out))
    want = kpconv64(q, s, nb, kp, extent, x, W)
    err = float((y.cpu().double() - want).abs().max())
    print(f"c_in {c_in}: max|HIP - fp64| = {err:.2e} (max {float(want.abs().max()):.2f})")
    assert err <= 1e-5 * max(1.0, float(want.abs().max()))
    assert float(y[3].abs().max()) == 0.0 and float(y[5].abs().max()) == 0.0
    # a strided view as the source (a channel slice of a wider buffer)
    buf = torch.zeros(n, c_in + 8, device="cuda")
    buf[:, 4:4 + c_in] = D(x)
    wf2 = ops.kpconv_aggregate(D(q), D(s), t, D(kp), extent, buf[:, 4:4 + c_in])
    assert torch.equal(wf, wf2)


def test_linear_norm_and_tail_vs_fp64(ops):
    rng = np.random.default_rng(1)
    for n in (97, 20000):
        a = rng.normal(0, 1, (n, 96)).astype(np.float32)
        w = rng.normal(0, 0.1, (96, 130)).astype(np.float32)
        b = rng.uniform(-0.05, 0.05, 130).astype(np.float32)
        y = ops.point_linear(D(a), D(w), D(b))
        y64 = torch.from_numpy(a).double() @ torch.from_numpy(w).double() + torch.from_numpy(b).double()
        assert float((y.cpu().double() - y64).abs().max()) <= 2e-6 * float(y64.abs().max())
        r = rng.normal(1, 2, (n, 130)).astype(np.float32)
        mr, mrr = ops.point_norm_stats(y), ops.point_norm_stats(D(r))
        out = ops.point_norm_apply(y, mr, leaky=True, res=D(r), res_mean_rstd=mrr)
        nrm = lambda v: (v - v.mean(0)) / torch.sqrt(v.var(0, unbiased=False) + 1e-5)
        z = nrm(y64) + nrm(torch.from_numpy(r).double())
        z = torch.where(z > 0, z, 0.1 * z)
        assert float((out.cpu().double() - z).abs().max()) <= 1e-5
        plain = ops.point_norm_apply(y, mr, leaky=False)
        assert float((plain.cpu().double() - nrm(y64)).abs().max()) <= 1e-5


def test_maxpool_and_gather_with_shadow(ops):
    rng = np.random.default_rng(2)
    x = rng.normal(-1, 1, (50, 12)).astype(np.float32)
    idx = rng.integers(0, 51, (30, 6))
    idx[0] = 50                                                 # all shadow -> zeros
    idx[1, :5] = 50
    t = ops.neighbor_table(D(idx), 50)
    x_ = np.concatenate([x, np.zeros((1, 12), np.float32)])
    mp = ops.point_maxpool(D(x), t)
    assert np.array_equal(mp.cpu().numpy(), x_[idx].max(1))
    buf = torch.full((30, 20), 7.0, device="cuda")
    ops.point_gather_rows(D(x), t, out=buf[:, 3:15])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, 3:15], x_[idx[:, 0]]) and np.all(got[:, :3] == 7) and np.all(got[:, 15:] == 7)
    assert np.all(got[0, 3:15] == 0)


def test_index_beyond_the_shadow_is_refused(ops, golden):
    g = golden("desc3d")
    with pytest.raises(ValueError, match="shadow"):
        ops.neighbor_table(D(np.array([[0, 51]])), 50)
    net, _, _ = make_net("desc")
    b = fixture_batch(g, "b")
    b["neighbors"][1] = b["neighbors"][1].clone()
    b["neighbors"][1][4, 0] = b["points"][1].shape[0] + 1
    with pytest.raises(ValueError, match="shadow"):
        net(b)


# ---- the pyramid ------------------------------------------------------------------------------------------------------------------
def test_radius_search_equals_brute_force(ops):
    rng = np.random.default_rng(3)
    lat = (rng.integers(0, 12, (900, 3)) / 32.0).astype(np.float32)       # a lattice: many exactly equal distances (ties)
    q_l, s_l = [300, 200, 100], [450, 250, 200]
    sup = lat
    qry = lat[rng.permutation(900)[:600]]
    for radius, limit in ((0.07, None), (0.07, 9), (0.1, 20), (0.2, 0)):
        got = ops.radius_neighbors(D(qry), D(sup), q_l, s_l, radius, limit).cpu().numpy()
        want = R.np_radius(qry, sup, q_l, s_l, radius, limit)
        assert got.shape == want.shape and np.array_equal(got, want), (radius, limit)
    pts = R.ellipsoid_cloud("rs", 3000)
    got = ops.radius_neighbors(D(pts), D(pts), [3000], [3000], 0.0625, None).cpu().numpy()
    assert np.array_equal(got, R.np_radius(pts, pts, [3000], [3000], 0.0625, None))


def test_grid_subsampling_barycentres_and_order(ops):
    from rnnpose_amd.descriptor3d import grid_subsample
    a = R.ellipsoid_cloud("gs1", 3000)
    b = R.ellipsoid_cloud("gs2", 1000, axes=(0.2, 0.3, 0.1), center=(0.05, 0.0, 0.0))
    pts = np.concatenate([a, b])
    for dl in (0.05, 0.1, 0.2):
        got, gl = grid_subsample(D(pts), [3000, 1000], dl)
        want, wl = R.np_grid_subsample(pts, [3000, 1000], dl)
        assert np.array_equal(gl.numpy(), wl) and np.array_equal(got.cpu().numpy(), want), dl


def test_kpconv_inputs_match_the_fixture_pyramid(ops, golden):
    from rnnpose_amd.descriptor3d import kpconv_inputs
    g = golden("desc3d")
    for case in ("a", "b"):
        lens = [int(v) for v in g[f"{case}_lengths_0"]]
        limits = [int(v) for v in g[f"{case}_limits"]]
        b = kpconv_inputs(D(g[f"{case}_points_0"]), R.DESC, limits if any(limits) else None, lengths=lens)
        for l in range(L):
            assert np.array_equal(b["points"][l].cpu().numpy(), g[f"{case}_points_{l}"])
            assert np.array_equal(b["neighbors"][l].cpu().numpy(), g[f"{case}_neighbors_{l}"])
            if l < L - 1:
                assert np.array_equal(b["pools"][l].cpu().numpy(), g[f"{case}_pools_{l}"])
                assert np.array_equal(b["upsamples"][l].cpu().numpy(), g[f"{case}_upsamples_{l}"])


# ---- interface ----------------------------------------------------------------------------------------------------------------------
def test_class_features(ops):
    from rnnpose_amd.descriptor3d import class_features
    from rnnpose_amd.eval_epoch import ClassModel
    desc, _, _ = make_net("desc")
    ctx, _, _ = make_net("ctx")
    pts = R.ellipsoid_cloud("cf", 3000)
    fea, geo = class_features(D(pts), desc, ctx, [40, 40, 40, 40])
    assert tuple(fea.shape) == (1, 3000, 256) and tuple(geo.shape) == (1, 3000, 32)
    assert float((geo.norm(dim=2) - 1).abs().max()) < 1e-5
    cm = ClassModel("x", pts, np.zeros((1, 3), np.int32), np.ones_like(pts), fea, geo, 1.0)
    assert cm.fea_3d.shape[1] == cm.geofea_3d.shape[1] == len(pts)
