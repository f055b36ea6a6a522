"""Test-side restatements for KPSuperpoint3Dv2 (model/descriptor3D.py, thirdparty/kpconv): the collate's pyramid in numpy and the
network in torch fp64.  Written for the tests from the reference's definitions (cited line by line); they share no code with
rnnpose_amd.descriptor3d.  Used by tests/golden/gen_golden_desc3d.py, tests/test_desc3d_host.py and tests/test_gpu_desc3d.py."""
from __future__ import annotations

import numpy as np
import torch

from rnnpose_amd import synthetic as syn

# config/linemod/template_fw0.5.yml:33-72
BASE = dict(num_layers=4, KP_extent=2.0, batch_norm_momentum=0.02, use_batch_norm=True, in_points_dim=3, fixed_kernel_points="center",
            KP_influence="linear", aggregation_mode="sum", modulated=False, first_subsampling_dl=0.025, conv_radius=2.5, deform_radius=5,
            in_features_dim=1, first_feats_dim=128, num_kernel_points=15, gnn_feats_dim=128)
DESC = dict(BASE, final_feats_dim=32, normalize_output=True)
CTX = dict(BASE, final_feats_dim=256, normalize_output=False)
SEEDS = {"desc": 5, "ctx": 6}
ROW_STEP = {"desc": 8, "ctx": 32}          # tests/golden/desc3d.npz keeps the outputs on these row lattices


def output_rows(n, name):
    """Rows of an (n, C) network output that tests/golden/desc3d.npz keeps: every ROW_STEP[name]-th and the last."""
    return np.unique(np.r_[np.arange(0, n, ROW_STEP[name]), n - 1])


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def ellipsoid_cloud(name, n, axes=(0.5, 0.35, 0.25), center=(0.0, 0.0, 0.0), seed=0):
    """n points on an ellipsoid surface (a normalised model's scale, data/preprocess.py:397-406), fp32."""
    d = syn.normal(f"kp3d_cloud_{name}", (n, 3), seed).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * np.asarray(axes) + np.asarray(center)).astype(np.float32)


def encoder_radii(cfg):
    """Convolution radius of each encoder block (model/descriptor3D.py:44-82: r doubles after each strided block)."""
    arch = ["simple", "resnetb"] + ["resnetb_strided", "resnetb", "resnetb"] * (cfg["num_layers"] - 1)
    r, out = cfg["first_subsampling_dl"] * cfg["conv_radius"], []
    for b in arch:
        out.append(r)
        if "strided" in b:
            r *= 2
    return out


def make_weights(shapes: dict, cfg, seed):
    """Seeded parameters for a {name: shape} state_dict: KPConv weights std sqrt(2 / (K Cin)), kernel points uniform in the cube
    of half-side 0.66 radius with the first at the origin ('center'), Linear / Conv1d weights std sqrt(2 / fan_in), biases
    uniform +-0.05, epsilon -5."""
    radii = encoder_radii(cfg)
    out = {}
    for name, shape in shapes.items():
        shape = tuple(int(s) for s in shape)
        if name == "epsilon":
            out[name] = np.array(-5.0, dtype=np.float32)
        elif name.endswith("KPConv.weights"):
            out[name] = syn.normal("w:" + name, shape, seed, std=float(np.sqrt(2.0 / (shape[0] * shape[1]))))
        elif name.endswith("kernel_points"):
            r = radii[int(name.split(".")[1])]
            kp = syn.uniform("w:" + name, shape, seed, -0.66 * r, 0.66 * r)
            kp[0] = 0.0
            out[name] = kp.astype(np.float32)
        else:
            out.update(syn.make_module_weights({name: shape}, seed=seed))
    return out


# ---- the pyramid (data/preprocess.py:564-690 on cpp_wrappers) ---------------------------------------------------------------------
def np_grid_subsample(points, lengths, dl):
    """grid_subsampling.cpp:4-211 in fp32, voxels in ascending key order."""
    dl = np.float32(dl)
    inv = np.float32(1) / dl
    outs, lens, s = [], [], 0
    for ln in lengths:
        p = points[s:s + ln]
        s += ln
        if ln == 0:                                         # an empty cloud keeps its place in the lengths
            lens.append(0)
            continue
        mn, mx = p.min(0), p.max(0)
        origin = np.floor(mn * inv).astype(np.float32) * dl
        ijk = np.floor((p - origin) / dl).astype(np.int64)
        nxy = np.floor((mx - origin) / dl).astype(np.int64) + 1
        key = ijk[:, 0] + nxy[0] * ijk[:, 1] + nxy[0] * nxy[1] * ijk[:, 2]
        keys = np.unique(key)
        bary = np.zeros((len(keys), 3), np.float32)
        for v, k in enumerate(keys):
            acc = np.zeros(3, np.float32)
            rows = np.nonzero(key == k)[0]
            for i in rows:                                  # input order
                acc = (acc + p[i]).astype(np.float32)
            bary[v] = acc * np.float32(1.0 / len(rows))
        outs.append(bary)
        lens.append(len(keys))
    return np.concatenate(outs, 0), np.asarray(lens, np.int64)


def np_radius(queries, supports, q_lengths, s_lengths, radius, limit):
    """neighbors.cpp:229-330 + batch_neighbors_kpconv (preprocess.py:544-561): per query, the supports of its own cloud with
    ((dx^2 + dy^2) + dz^2) < r^2 in fp32, sorted by (d2, index), width min(limit, max count), padded with len(supports)."""
    r = np.float32(radius)
    r2 = r * r
    rows, qs, ss = [], 0, 0
    for ql, sl in zip(q_lengths, s_lengths):
        Q, S = queries[qs:qs + ql], supports[ss:ss + sl]
        d = Q[:, None, :] - S[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        for i in range(ql):
            idx = np.nonzero(d2[i] < r2)[0]
            order = np.lexsort((idx, d2[i, idx]))
            rows.append(idx[order] + ss)
        qs += ql
        ss += sl
    width = max((len(x) for x in rows), default=0)
    if limit is not None and limit > 0:
        width = min(width, limit)
    out = np.full((len(rows), width), len(supports), np.int64)
    for i, x in enumerate(rows):
        x = x[:width]
        out[i, :len(x)] = x
    return out


def np_pyramid(points, lengths, cfg, limits):
    """collate_fn_descriptor's point / neighbors / pools / upsamples lists for one stacked batch."""
    L = cfg["num_layers"]
    r_normal = cfg["first_subsampling_dl"] * cfg["conv_radius"]
    pts, lens = points.astype(np.float32), list(lengths)
    P = {"points": [], "neighbors": [], "pools": [], "upsamples": [], "stack_lengths": []}
    for layer in range(L):
        lim = None if limits is None else limits[layer]
        P["neighbors"].append(np_radius(pts, pts, lens, lens, r_normal, lim))
        if layer < L - 1:
            pp, pb = np_grid_subsample(pts, lens, 2 * r_normal / cfg["conv_radius"])
            P["pools"].append(np_radius(pp, pts, pb, lens, r_normal, lim))
            P["upsamples"].append(np_radius(pts, pp, lens, pb, 2 * r_normal, lim))
        else:
            pp, pb = np.zeros((0, 3), np.float32), np.zeros(0, np.int64)
            P["pools"].append(np.zeros((0, 1), np.int64))
            P["upsamples"].append(np.zeros((0, 1), np.int64))
        P["points"].append(pts)
        P["stack_lengths"].append(np.asarray(lens, np.int64))
        pts, lens = pp, list(pb)
        r_normal *= 2
    return P


# ---- the network in fp64 ------------------------------------------------------------------------------------------------------
class Net64:
    """KPSuperpoint3Dv2's forward in torch fp64 from a state_dict (model/descriptor3D.py:132-196, kpconv_blocks.py).
    Also tracks, per row, whether a positive-sum neighbour-count decision upstream had a margin below rel * sum|x|
    (`uncertain`), and how many such decisions there were (`n_close`)."""

    def __init__(self, sd, cfg, device="cpu", rel=1e-6):
        self.sd = {k: torch.as_tensor(np.asarray(v)).to(device=device, dtype=torch.float64) for k, v in sd.items()}
        self.cfg, self.dev, self.rel = cfg, device, rel
        self.n_close = 0

    def _t(self, a, dt=torch.float64):
        return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(device=self.dev, dtype=dt)

    @staticmethod
    def _norm(x):                                            # InstanceNorm1d over all rows (kpconv_blocks.py:456-473)
        m = x.mean(0, keepdim=True)
        v = ((x - m) ** 2).mean(0, keepdim=True)
        return (x - m) / torch.sqrt(v + 1e-5)

    @staticmethod
    def _leaky(x):
        return torch.where(x > 0, x, 0.1 * x)

    def _kpconv(self, pre, q, s, nb, x, ux, radius):         # kpconv_blocks.py:300-372
        W, kp = self.sd[pre + ".weights"], self.sd[pre + ".kernel_points"]
        extent = radius * self.cfg["KP_extent"] / self.cfg["conv_radius"]
        s_ = torch.cat([s, torch.full_like(s[:1], 1e6)], 0)
        nbr = s_[nb] - q[:, None, :]
        d2 = ((nbr[:, :, None, :] - kp) ** 2).sum(-1)
        infl = torch.clamp(1 - torch.sqrt(d2) / extent, min=0.0)
        x_ = torch.cat([x, torch.zeros_like(x[:1])], 0)
        nx = x_[nb]
        out = torch.einsum("nmk,nmc,kco->no", infl, nx, W)
        rs = x_.sum(1)
        cnt = (rs[nb] > 0).sum(1).clamp(min=1)
        close = torch.cat([rs[:-1].abs() <= self.rel * x.abs().sum(1), torch.zeros(1, dtype=torch.bool, device=self.dev)])
        self.n_close += int(close[nb].any(1).sum())
        u_ = torch.cat([ux, torch.zeros(1, dtype=torch.bool, device=self.dev)])
        unc = (close[nb] | u_[nb]).any(1)
        return out / cnt[:, None], unc

    def _lin(self, name, x, bias=None):
        w = self.sd[name]
        w = w.reshape(w.shape[0], -1)
        y = x @ w.t()
        return y if bias is None else y + self.sd[bias]

    def __call__(self, batch):
        cfg, L = self.cfg, self.cfg["num_layers"]
        pts = [self._t(p) for p in batch["points"][:L]]
        nbs = [self._t(n, torch.int64) for n in batch["neighbors"][:L]]
        pools = [self._t(n, torch.int64) for n in batch["pools"][:L - 1]]
        ups = [self._t(n, torch.int64) for n in batch["upsamples"][:L - 1]]
        x = self._t(batch["features"])
        u = torch.zeros(x.shape[0], dtype=torch.bool, device=self.dev)
        radii = encoder_radii(cfg)
        arch = ["simple", "resnetb"] + ["resnetb_strided", "resnetb", "resnetb"] * (L - 1)
        layer, skips = 0, []
        for i, b in enumerate(arch):
            pre = f"encoder_blocks.{i}"
            if "strided" in b:
                skips.append((x, u))
                q, s, nb = pts[layer + 1], pts[layer], pools[layer]
            else:
                q, s, nb = pts[layer], pts[layer], nbs[layer]
            if b == "simple":
                y, u = self._kpconv(pre + ".KPConv", q, s, nb, x, u, radii[i])
                x = self._leaky(self._norm(y))
            else:
                h = self._leaky(self._norm(self._lin(pre + ".unary1.mlp.weight", x))) if pre + ".unary1.mlp.weight" in self.sd else x
                y, uy = self._kpconv(pre + ".KPConv", q, s, nb, h, u, radii[i])
                z = self._norm(self._lin(pre + ".unary2.mlp.weight", self._leaky(self._norm(y))))
                if "strided" in b:                           # max_pool with a zero shadow row (:88-104)
                    x_ = torch.cat([x, torch.zeros_like(x[:1])], 0)
                    sc = x_[nb].max(1).values
                    u_ = torch.cat([u, torch.zeros(1, dtype=torch.bool, device=self.dev)])
                    usc = u_[nb].any(1)
                else:
                    sc, usc = x, u
                if pre + ".unary_shortcut.mlp.weight" in self.sd:
                    sc = self._norm(self._lin(pre + ".unary_shortcut.mlp.weight", sc))
                x, u = self._leaky(z + sc), uy | usc
            if "strided" in b:
                layer += 1
        x = self._lin("bottle.weight", x, "bottle.bias")
        x = self._lin("proj_gnn.weight", x, "proj_gnn.bias")
        di = 0
        for lv in range(L - 2, -1, -1):                      # nearest_upsample (:703-714) + cat([x, skip]) + unary
            sx, su = skips.pop()
            x_ = torch.cat([x, torch.zeros_like(x[:1])], 0)
            u_ = torch.cat([u, torch.zeros(1, dtype=torch.bool, device=self.dev)])
            x = torch.cat([x_[ups[lv][:, 0]], sx], 1)
            u = u_[ups[lv][:, 0]] | su
            y = self._lin(f"decoder_blocks.{di + 1}.mlp.weight", x)
            x = y if lv == 0 else self._leaky(self._norm(y))
            di += 2
        x = x[:, :cfg["final_feats_dim"]]
        if cfg["normalize_output"]:
            x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
        self.uncertain = u
        return x
