"""The fp64 restatements of tests/point_ref.py (the references of tests/test_gpu_point_edges.py) against torch's own operators and
against the reference-generated pyramid of tests/golden/desc3d.npz.  CPU only."""
import numpy as np
import torch
import torch.nn.functional as F

import desc3d_fp64 as R
import point_ref as pr


def _rng(seed):
    return np.random.default_rng(seed)


def test_norm_is_torch_instance_norm_and_leaky_relu():
    x = _rng(0).normal(0.5, 2.0, (37, 9))
    st = pr.norm_stats(x.astype(np.float32))
    x32 = x.astype(np.float32).astype(np.float64)
    want = F.instance_norm(torch.from_numpy(x32).t()[None], eps=float(np.float32(1e-5)))[0].t().numpy()
    mr = np.stack([st["mean"], st["rstd"]], 1)
    got, _ = pr.norm_apply(x32, mr, leaky=False)
    assert np.abs(got - want).max() <= 1e-12
    got, _ = pr.norm_apply(x32, mr, leaky=True, slope=0.1)
    assert np.abs(got - F.leaky_relu(torch.from_numpy(want), 0.1).numpy()).max() <= 1e-12
    r = _rng(1).normal(-1, 3, (37, 9))
    sr = pr.norm_stats(r)
    mrr = np.stack([sr["mean"], sr["rstd"]], 1)
    both = F.leaky_relu(torch.from_numpy(want) + F.instance_norm(torch.from_numpy(r).t()[None], eps=float(np.float32(1e-5)))[0].t(), 0.1).numpy()
    got, b = pr.norm_apply(x32, mr, res=r, mr_res=mrr)
    assert np.abs(got - both).max() <= 1e-12 and (b >= 0).all()
    got, _ = pr.norm_apply(x32, mr, res=r, leaky=False)
    assert np.abs(got - (want + r)).max() <= 1e-12
    one = pr.norm_stats(np.full((1, 3), 4.0, np.float32))                       # n = 1: variance 0
    assert np.array_equal(one["var"], np.zeros(3)) and np.allclose(one["rstd"], 1 / np.sqrt(float(np.float32(1e-5))), rtol=1e-15)


def test_l2_linear_rowsum_and_pools_are_torch():
    x = _rng(2).normal(0, 1, (11, 70)).astype(np.float32)
    x[3] = 0
    x[4] = 0
    x[4, 7] = 1e-13
    got, b = pr.l2_normalize(x)
    want = F.normalize(torch.from_numpy(x).double(), p=2, dim=1, eps=float(np.float32(1e-12))).numpy()
    assert np.abs(got - want).max() <= 1e-15 and not got[3].any() and got[4, 7] == float(np.float32(1e-13)) / float(np.float32(1e-12))
    w, bias = _rng(3).normal(0, 1, (70, 5)), _rng(4).normal(0, 1, 5)
    y, yb = pr.linear(x, w, bias)
    assert np.abs(y - F.linear(torch.from_numpy(x).double(), torch.from_numpy(w).t(), torch.from_numpy(bias)).numpy()).max() <= 1e-12
    assert (yb > 0).all()
    s, sb = pr.row_sum(x)
    assert np.abs(s - torch.from_numpy(x).double().sum(1).numpy()).max() <= 1e-12 and np.abs(x.sum(1) - s).max() <= sb.max()
    idx = _rng(5).integers(0, 12, (6, 4))
    idx[0] = 11
    xn = x.copy()
    xn[2, 5] = np.nan
    x_ = torch.cat([torch.from_numpy(xn), torch.zeros(1, 70)])
    want = x_[torch.from_numpy(idx)].max(1).values.numpy()                      # (kpconv_blocks.py:103)
    assert np.array_equal(pr.maxpool(xn, idx), want, equal_nan=True) and np.isnan(want).any() == bool((idx == 2).any())
    assert np.array_equal(pr.gather_rows(xn, idx), x_[torch.from_numpy(idx[:, 0])].numpy(), equal_nan=True)
    assert np.array_equal(pr.maxpool(x, np.array([[-1, 3]])), np.zeros((1, 70), np.float32))        # a negative id is the shadow


def test_kpconv_aggregate_is_the_network_restatement_and_its_bound_holds_for_fp32():
    """the same quantity as tests/desc3d_fp64.py::Net64._kpconv (einsum with the weights) once multiplied by the weights; an fp32
    evaluation of the formula in torch lies inside the derived bound"""
    rng = _rng(6)
    n_s, n_q, w, K, c = 30, 7, 9, 15, 5
    s = rng.uniform(-0.2, 0.2, (n_s, 3)).astype(np.float32)
    q = s[:n_q] + rng.normal(0, 0.01, (n_q, 3)).astype(np.float32)
    kp = rng.uniform(-0.08, 0.08, (K, 3)).astype(np.float32)
    x = rng.normal(0.4, 1, (n_s, c)).astype(np.float32)
    nb = rng.integers(0, n_s + 1, (n_q, w))
    nb[2] = n_s
    W = rng.normal(0, 0.3, (K, c, 4))
    ref = pr.kpconv_aggregate(q, s, nb, kp, 0.12, x)
    net = R.Net64({"c.weights": W, "c.kernel_points": kp}, dict(KP_extent=0.12, conv_radius=1.0))
    want, _ = net._kpconv("c", torch.from_numpy(q).double(), torch.from_numpy(s).double(), torch.from_numpy(nb), torch.from_numpy(x).double(),
                          torch.zeros(n_s, dtype=torch.bool), 1.0)
    got = np.einsum("qkc,kco->qo", ref["wf"], W)
    assert np.abs(got - want.numpy()).max() <= 1e-12 and not ref["wf"][2].any()
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    s_ = torch.cat([t(s), torch.full((1, 3), 1e6)])
    x_ = torch.cat([t(x), torch.zeros(1, c)])
    d = (s_[nb] - t(q)[:, None])[:, :, None, :] - t(kp)
    infl = torch.clamp(1 - torch.sqrt((d * d).sum(-1)) / np.float32(0.12), min=0)
    wf32 = torch.zeros(n_q, K, c)
    for j in range(w):
        wf32 += infl[:, j, :, None] * x_[nb[:, j]][:, None, :]
    wf32 = wf32 / torch.from_numpy(ref["count"]).float()[:, None, None]
    err = np.abs(wf32.double().numpy() - ref["wf"])
    assert (err <= ref["bound"]).all() and err.max() > 0
    assert np.array_equal(pr.kpconv_aggregate(q, s, np.where(nb == n_s, -3, nb), kp, 0.12, x)["wf"], ref["wf"])


def test_pyramid_restatements_reproduce_the_reference_fixture(golden):
    """np_radius / np_grid_subsample (tests/desc3d_fp64.py) and point_ref.voxel_keys on the reference-generated arrays of desc3d.npz"""
    g = golden("desc3d")
    for case in ("a", "b"):
        lens = [[int(v) for v in g[f"{case}_lengths_{l}"]] for l in range(2)]
        limits = [int(v) for v in g[f"{case}_limits"]]
        p0, p1 = g[f"{case}_points_0"], g[f"{case}_points_1"]
        r0 = R.BASE["first_subsampling_dl"] * R.BASE["conv_radius"]
        sub, sl = R.np_grid_subsample(p0, lens[0], 2 * r0 / R.BASE["conv_radius"])
        assert np.array_equal(sub, p1) and [int(v) for v in sl] == lens[1]
        lim = limits[0] if any(limits) else None
        assert np.array_equal(R.np_radius(p0, p0, lens[0], lens[0], r0, lim), g[f"{case}_neighbors_0"])
        assert np.array_equal(R.np_radius(p1, p0, lens[1], lens[0], r0, lim), g[f"{case}_pools_0"])
        keys, _, _ = pr.voxel_keys(p0[:lens[0][0]], 2 * r0 / R.BASE["conv_radius"])
        assert len(np.unique(keys)) == lens[1][0]
    sub, sl = R.np_grid_subsample(np.array([[0.3, 0.1, 0.2], [0.0, 0.0, 0.0], [0.01, 0.0, 0.0]], np.float32), [1, 0, 2], 0.05)
    assert list(sl) == [1, 0, 1] and np.array_equal(sub[0], np.array([0.3, 0.1, 0.2], np.float32))
