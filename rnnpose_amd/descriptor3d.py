"""KPSuperpoint3Dv2 (model/descriptor3D.py), the 3-D branch of HybridDescNet (model/HybridNet.py:68,87-95) and of
ContextFeatureNet (model/HybridNet.py:29-56): the per-point descriptors (`geofea_3d`, 32 channels) and context features
(`fea_3d`, 256 channels) that PoseRefiner consumes, computed on the library's point kernels (the KPSuperpoint3Dv2 section of csrc/nhwc_ops.hip).

    KPConv (kpconv_blocks.py:300-372)   kpconv_aggregate: per query, the K linear influences of its neighbours and
                                        WF[k, c] = sum_j infl_kj x_jc / max(1, #positive-sum neighbours) -> (N, K Cin);
                                        point_linear: (N, K Cin) x (K Cin, Cout), fp32 FMA
    BatchNormBlock = InstanceNorm1d     point_norm_stats over ALL rows of the stacked batch + point_norm_apply (LeakyReLU 0.1)
    UnaryBlock / bottle / proj_gnn      point_linear (+ bias for the Conv1d layers)
    ResnetBottleneckBlock tail          point_norm_apply(unary2, res = shortcut normalised on load, leaky)
    max_pool (strided shortcut)         point_maxpool (shadow row = 0)
    nearest_upsample + torch.cat        point_gather_rows into channels [0, Cx) of a (N, Cx + Cskip) buffer whose other
                                        channels the encoder's last block of that level wrote directly: no concatenation copy
    F.normalize                         point_l2_normalize

kpconv_inputs() builds the collate's pyramid (data/preprocess.py:564-690) on the GPU: radius searches on
rnnpose_radius_*_f32, grid subsampling in torch.  Inference only.  DESIGN.md section 13.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from . import ops

F32 = torch.float32
LEAKY = 0.1                # nn.LeakyReLU(0.1) everywhere (kpconv_blocks.py:512, :583, :657)
IN_EPS = 1e-5              # nn.InstanceNorm1d's default eps


def _cfg(config, k, default=None):
    if isinstance(config, dict):
        return config.get(k, default)
    return getattr(config, k, default)


def architecture(num_layers: int):
    """The block list KPSuperpoint3Dv2.__init__ builds (model/descriptor3D.py:16-29)."""
    arch = ["simple", "resnetb"]
    for _ in range(num_layers - 1):
        arch += ["resnetb_strided", "resnetb", "resnetb"]
    for _ in range(num_layers - 2):
        arch += ["nearest_upsample", "unary"]
    return arch + ["nearest_upsample", "last_unary"]


def default_kernel_points(radius: float, K: int = 15):
    """A fixed 'center' disposition (the origin, 6 axis points, 8 cube diagonals at 0.66 radius) for modules built without a
    checkpoint.  The reference optimises its disposition at construction (kernels/kernel_points.py:391-460) and saves it as a
    parameter: load_state_dict replaces this."""
    if K != 15:
        raise NotImplementedError("default_kernel_points: K = 15 only (load a checkpoint for other kernels)")
    pts = [(0.0, 0.0, 0.0)]
    for ax in range(3):
        for s in (1.0, -1.0):
            p = [0.0, 0.0, 0.0]
            p[ax] = s
            pts.append(tuple(p))
    d = 1.0 / math.sqrt(3.0)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                pts.append((sx * d, sy * d, sz * d))
    return torch.tensor(pts, dtype=F32) * (0.66 * radius)


# ---- modules with the reference's parameter names (kpconv_blocks.py) -------------------------------------------------------
class KPConv(nn.Module):
    def __init__(self, K, in_channels, out_channels, KP_extent, radius):
        super().__init__()
        self.K, self.in_channels, self.out_channels = K, in_channels, out_channels
        self.KP_extent, self.radius = KP_extent, radius
        self.weights = nn.Parameter(torch.empty(K, in_channels, out_channels, dtype=F32))
        nn.init.kaiming_uniform_(self.weights, a=math.sqrt(5))
        self.kernel_points = nn.Parameter(default_kernel_points(radius, K), requires_grad=False)


class UnaryBlock(nn.Module):
    def __init__(self, in_dim, out_dim, no_relu=False):
        super().__init__()
        self.mlp = nn.Linear(in_dim, out_dim, bias=False)
        self.no_relu = no_relu


class LastUnaryBlock(nn.Module):
    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.mlp = nn.Linear(in_dim, out_dim, bias=False)


class SimpleBlock(nn.Module):
    def __init__(self, block_name, in_dim, out_dim, radius, layer_ind, config):
        super().__init__()
        self.block_name, self.layer_ind = block_name, layer_ind
        extent = radius * config["KP_extent"] / config["conv_radius"]
        self.KPConv = KPConv(config["num_kernel_points"], in_dim, out_dim // 2, extent, radius)


class ResnetBottleneckBlock(nn.Module):
    def __init__(self, block_name, in_dim, out_dim, radius, layer_ind, config):
        super().__init__()
        self.block_name, self.layer_ind = block_name, layer_ind
        extent = radius * config["KP_extent"] / config["conv_radius"]
        self.unary1 = UnaryBlock(in_dim, out_dim // 4) if in_dim != out_dim // 4 else None
        self.KPConv = KPConv(config["num_kernel_points"], out_dim // 4, out_dim // 4, extent, radius)
        self.unary2 = UnaryBlock(out_dim // 4, out_dim, no_relu=True)
        self.unary_shortcut = UnaryBlock(in_dim, out_dim, no_relu=True) if in_dim != out_dim else None


class NearestUpsampleBlock(nn.Module):
    def __init__(self, layer_ind):
        super().__init__()
        self.layer_ind = layer_ind


def _block(name, radius, in_dim, out_dim, layer, config):
    if name == "unary":
        return UnaryBlock(in_dim, out_dim)
    if name == "last_unary":
        return LastUnaryBlock(in_dim, config["final_feats_dim"] + 2)
    if name == "simple":
        return SimpleBlock(name, in_dim, out_dim, radius, layer, config)
    if name in ("resnetb", "resnetb_strided"):
        return ResnetBottleneckBlock(name, in_dim, out_dim, radius, layer, config)
    if name == "nearest_upsample":
        return NearestUpsampleBlock(layer)
    raise ValueError(f"unknown block {name!r}")


_KEYS = ("num_layers", "first_subsampling_dl", "conv_radius", "in_features_dim", "first_feats_dim", "num_kernel_points",
         "final_feats_dim", "gnn_feats_dim", "KP_extent")


class KPSuperpoint3Dv2(nn.Module):
    """Drop-in for model/descriptor3D.py:KPSuperpoint3Dv2 (same parameters, shapes and state_dict keys) on the HIP kernels.
    forward(batch) takes the reference's batch3d dict -- points, neighbors, pools, upsamples (int32 or int64), features,
    stack_lengths -- on the GPU and returns (N0, final_feats_dim) fp32."""

    def __init__(self, config):
        super().__init__()
        cfg = {k: _cfg(config, k) for k in _KEYS}
        missing = [k for k, v in cfg.items() if v is None]
        if missing:
            raise ValueError(f"KPSuperpoint3Dv2: config lacks {missing}")
        for k, want in (("KP_influence", "linear"), ("aggregation_mode", "sum")):
            got = _cfg(config, k, want)
            if got != want:
                raise NotImplementedError(f"KPSuperpoint3Dv2: {k} = {got!r} is not implemented (only {want!r})")
        if _cfg(config, "fixed_kernel_points", "center") != "center":
            raise NotImplementedError("KPSuperpoint3Dv2: only fixed_kernel_points = 'center' is implemented")
        if _cfg(config, "modulated", False):
            raise NotImplementedError("KPSuperpoint3Dv2: modulated (deformable) kernels are not implemented")
        if not _cfg(config, "use_batch_norm", True):
            raise NotImplementedError("KPSuperpoint3Dv2: use_batch_norm = False is not implemented")
        if _cfg(config, "in_points_dim", 3) != 3:
            raise NotImplementedError("KPSuperpoint3Dv2: in_points_dim must be 3")
        if cfg["num_layers"] < 2:
            raise ValueError("KPSuperpoint3Dv2: num_layers must be at least 2")
        arch = list(_cfg(config, "architecture", None) or architecture(cfg["num_layers"]))
        if arch != architecture(cfg["num_layers"]):
            raise NotImplementedError("KPSuperpoint3Dv2: only the block list of model/descriptor3D.py:16-29 is implemented "
                                      "(deformable blocks are refused)")
        self.config = dict(cfg, normalize_output=bool(_cfg(config, "normalize_output", True)))
        self.normalize_output = self.config["normalize_output"]
        self.architecture = arch
        self.K = cfg["num_kernel_points"]
        self.final_feats_dim = cfg["final_feats_dim"]
        self.epsilon = nn.Parameter(torch.tensor(-5.0))

        # model/descriptor3D.py:31-123, line for line
        layer = 0
        r = cfg["first_subsampling_dl"] * cfg["conv_radius"]
        in_dim, out_dim = cfg["in_features_dim"], cfg["first_feats_dim"]
        self.encoder_blocks = nn.ModuleList()
        self.encoder_skip_dims, self.encoder_skips = [], []
        for block_i, block in enumerate(arch):
            if any(t in block for t in ("pool", "strided", "upsample", "global")):
                self.encoder_skips.append(block_i)
                self.encoder_skip_dims.append(in_dim)
            if "upsample" in block:
                break
            self.encoder_blocks.append(_block(block, r, in_dim, out_dim, layer, cfg))
            in_dim = out_dim // 2 if "simple" in block else out_dim
            if "pool" in block or "strided" in block:
                layer += 1
                r *= 2
                out_dim *= 2
        bott = cfg["gnn_feats_dim"]
        self.bottle = nn.Conv1d(in_dim, bott, kernel_size=1, bias=True)
        self.proj_gnn = nn.Conv1d(bott, bott, kernel_size=1, bias=True)
        out_dim = bott
        self.decoder_blocks = nn.ModuleList()
        self.decoder_concats = []
        start_i = next(i for i, b in enumerate(arch) if "upsample" in b)
        for block_i, block in enumerate(arch[start_i:]):
            if block_i > 0 and "upsample" in arch[start_i + block_i - 1]:
                in_dim += self.encoder_skip_dims[layer]
                self.decoder_concats.append(block_i)
            self.decoder_blocks.append(_block(block, r, in_dim, out_dim, layer, cfg))
            in_dim = out_dim
            if "upsample" in block:
                layer -= 1
                r *= 0.5
                out_dim = out_dim // 2

    # ---- the forward pass -------------------------------------------------------------------------------------------------
    @staticmethod
    def _linear_w(mod):
        w = mod.weight.detach()
        return w.reshape(w.shape[0], -1).t().float().contiguous()

    @staticmethod
    def _unary(x, mod, leaky=True, out=None):
        """Linear (no bias) -> InstanceNorm -> [LeakyReLU], normalised in place (or into out)."""
        y = ops.point_linear(x, KPSuperpoint3Dv2._linear_w(mod.mlp))
        return ops.point_norm_apply(y, ops.point_norm_stats(y, IN_EPS), leaky=leaky, slope=LEAKY, out=y if out is None else out)

    def _kpconv(self, conv, q, s, nb, x):
        wf = ops.kpconv_aggregate(q, s, nb, conv.kernel_points, float(conv.KP_extent), x)
        w = conv.weights.detach().float().reshape(-1, conv.weights.shape[2]).contiguous()
        return ops.point_linear(wf, w)

    def _encoder_block(self, blk, x, P, out):
        l = blk.layer_ind
        strided = "strided" in blk.block_name
        q, s = (P["points"][l + 1], P["points"][l]) if strided else (P["points"][l], P["points"][l])
        nb = P["pools"][l] if strided else P["neighbors"][l]
        if isinstance(blk, SimpleBlock):
            y = self._kpconv(blk.KPConv, q, s, nb, x)
            return ops.point_norm_apply(y, ops.point_norm_stats(y, IN_EPS), leaky=True, slope=LEAKY, out=out)
        h = x if blk.unary1 is None else self._unary(x, blk.unary1)
        y = self._kpconv(blk.KPConv, q, s, nb, h)
        ops.point_norm_apply(y, ops.point_norm_stats(y, IN_EPS), leaky=True, slope=LEAKY, out=y)
        z = ops.point_linear(y, self._linear_w(blk.unary2.mlp))
        sc = ops.point_maxpool(x, nb) if strided else x
        sc_mr = None
        if blk.unary_shortcut is not None:
            sc = ops.point_linear(sc, self._linear_w(blk.unary_shortcut.mlp))
            sc_mr = ops.point_norm_stats(sc, IN_EPS)
        return ops.point_norm_apply(z, ops.point_norm_stats(z, IN_EPS), leaky=True, slope=LEAKY, res=sc, res_mean_rstd=sc_mr, out=out)

    def _prepare(self, batch):
        pts = batch["points"]
        if not isinstance(pts, (list, tuple)) or not all(isinstance(p, torch.Tensor) for p in pts):
            raise ValueError("batch['points'] must be a list of (N_l, 3) tensors")
        if any(p.device.type != "cuda" for p in pts):
            raise RuntimeError("KPSuperpoint3Dv2 runs on the GPU only (no CPU path in rnnpose_amd)")
        L = self.config["num_layers"]
        if len(pts) < L:
            raise ValueError(f"batch holds {len(pts)} point levels, the network needs {L}")
        dev = pts[0].device
        P = {"points": [p.to(device=dev, dtype=F32).contiguous() for p in pts[:L]]}
        n = [p.shape[0] for p in P["points"]]
        P["neighbors"] = [ops.neighbor_table(batch["neighbors"][l].to(dev), n[l], f"neighbors[{l}]") for l in range(L)]
        P["pools"] = [ops.neighbor_table(batch["pools"][l].to(dev), n[l], f"pools[{l}]") for l in range(L - 1)]
        P["upsamples"] = [ops.neighbor_table(batch["upsamples"][l].to(dev), n[l + 1], f"upsamples[{l}]") for l in range(L - 1)]
        for l in range(L):
            if P["neighbors"][l].shape[0] != n[l]:
                raise ValueError(f"neighbors[{l}] must have {n[l]} rows")
        for l in range(L - 1):
            if P["pools"][l].shape[0] != n[l + 1] or P["upsamples"][l].shape[0] != n[l]:
                raise ValueError(f"pools[{l}] must have {n[l + 1]} rows and upsamples[{l}] {n[l]}")
        x = batch["features"].to(device=dev, dtype=F32).contiguous()
        if tuple(x.shape) != (n[0], self.config["in_features_dim"]):
            raise ValueError(f"features must be ({n[0]}, {self.config['in_features_dim']}), got {tuple(x.shape)}")
        return P, x

    @torch.no_grad()
    def forward(self, batch):
        P, x = self._prepare(batch)
        dev = x.device
        n = [p.shape[0] for p in P["points"]]
        # the decoder's concat buffers: channels [0, Cx) take the up-sampled rows, [Cx, Cx + Cskip) the skip of that level,
        # written there by the encoder's last block of the level
        n_skips = len(self.encoder_skips) - 1                  # the last entry is the first up-sampling block itself
        cat, cat_off = {}, {}
        for j, bi in enumerate(self.decoder_concats):
            lv = n_skips - 1 - j
            c_in = self.decoder_blocks[bi].mlp.in_features
            cat[lv] = torch.empty(n[lv], c_in, device=dev, dtype=F32)
            cat_off[lv] = c_in - self.encoder_skip_dims[lv]
        skip_writer = {self.encoder_skips[lv] - 1: lv for lv in range(n_skips)}
        for i, blk in enumerate(self.encoder_blocks):
            lv = skip_writer.get(i)
            out = None if lv is None else cat[lv][:, cat_off[lv]:]
            x = self._encoder_block(blk, x, P, out)
        x = ops.point_linear(x, self._linear_w(self.bottle), self.bottle.bias.detach().float())
        x = ops.point_linear(x, self._linear_w(self.proj_gnn), self.proj_gnn.bias.detach().float())
        for blk in self.decoder_blocks:
            if isinstance(blk, NearestUpsampleBlock):
                lv = blk.layer_ind - 1
                buf = cat[lv]
                ops.point_gather_rows(x, P["upsamples"][lv], out=buf[:, :cat_off[lv]])
                x = buf
            elif isinstance(blk, LastUnaryBlock):
                w = self._linear_w(blk.mlp)[:, :self.final_feats_dim].contiguous()     # feats_f = x[:, :final_feats_dim]
                x = ops.point_linear(x, w)
            else:
                x = self._unary(x, blk)
        if self.normalize_output:
            ops.point_l2_normalize(x, out=x)
        return x


# ---- the collate's pyramid (data/preprocess.py:564-690) ------------------------------------------------------------------------
def grid_subsample(points, lengths, dl: float):
    """batch_grid_subsampling_kpconv (cpp_subsampling/grid_subsampling/grid_subsampling.cpp:4-211), per cloud, fp32:
    origin = floor(min * (1 / dl)) * dl; voxel (floor((p - origin) / dl) per axis), key ix + nx iy + nx ny iz; barycentre =
    fp32 sum in input order * fp32(1.0 / count).  Voxels come out in ASCENDING KEY order (the reference emits its hash map's
    order, which is unspecified).  -> (points (M, 3) fp32, lengths (B,) int64)."""
    dev = points.device
    d = np.float32(dl)
    inv = np.float32(1) / d
    outs, lens = [], []
    s = 0
    for ln in [int(v) for v in lengths]:
        p = points[s:s + ln]
        s += ln
        if ln == 0:
            lens.append(0)
            continue
        mn = p.min(0).values.cpu().numpy()                  # 3 values each: the grid's corner and extent in fp32 on the host
        mx = p.max(0).values.cpu().numpy()
        origin = np.floor(mn * inv).astype(np.float32) * d
        nxy = np.floor((mx - origin) / d).astype(np.int64) + 1
        key = ops.grid_voxel_keys(p, origin, d, int(nxy[0]), int(nxy[1]))
        skey, perm = torch.sort(key, stable=True)
        _, counts = torch.unique_consecutive(skey, return_counts=True)
        starts = torch.cumsum(counts, 0) - counts
        acc = torch.zeros(counts.shape[0], 3, device=dev, dtype=F32)
        ps = p[perm]
        for j in range(int(counts.max())):                  # fp32 sum of each voxel in input order
            sel = torch.nonzero(counts > j).squeeze(1)
            acc[sel] = acc[sel] + ps[starts[sel] + j]
        scale = torch.from_numpy((1.0 / counts.cpu().numpy().astype(np.float64)).astype(np.float32)).to(dev)
        outs.append(acc * scale[:, None])
        lens.append(counts.shape[0])
    pts = torch.cat(outs, 0) if outs else torch.zeros(0, 3, device=dev, dtype=F32)
    return pts.contiguous(), torch.tensor(lens, dtype=torch.int64)


def kpconv_inputs(points, config, neighborhood_limits, lengths=None, features=None):
    """The batch3d dict of collate_fn_descriptor (data/preprocess.py:583-690) built on the GPU: per level l (radius
    r_l = first_subsampling_dl * conv_radius * 2^l) neighbors (radius r_l), and below the last level pools (radius r_l from the
    grid-subsampled level l+1, dl = 2 r_l / conv_radius) and upsamples (radius 2 r_l from level l+1).
    points (N, 3) (stacked clouds of `lengths`, default one cloud); neighborhood_limits: one limit per level (the reference
    calibrates them on the dataset, preprocess.py:856-890), or None for no truncation; features default to ones (N, 1)
    (data/linemod_dataset.py:379).  Level l+1 is in ascending voxel-key order (see grid_subsample)."""
    L = int(_cfg(config, "num_layers"))
    r_normal = float(_cfg(config, "first_subsampling_dl")) * float(_cfg(config, "conv_radius"))
    conv_radius = float(_cfg(config, "conv_radius"))
    if neighborhood_limits is not None and len(neighborhood_limits) < L:
        raise ValueError(f"neighborhood_limits needs {L} entries")
    dev = torch.device("cuda", torch.cuda.current_device()) if not points.is_cuda else points.device
    pts = points.to(device=dev, dtype=F32).contiguous()
    lens = [pts.shape[0]] if lengths is None else [int(v) for v in lengths]
    if sum(lens) != pts.shape[0]:
        raise ValueError("lengths must sum to the number of points")
    out = {"points": [], "neighbors": [], "pools": [], "upsamples": [], "stack_lengths": []}
    for layer in range(L):
        lim = None if neighborhood_limits is None else neighborhood_limits[layer]
        r = r_normal
        conv = ops.radius_neighbors(pts, pts, lens, lens, r, lim)
        if layer < L - 1:
            pool_p, pool_b = grid_subsample(pts, lens, 2 * r_normal / conv_radius)
            pool_b = [int(v) for v in pool_b]
            pool = ops.radius_neighbors(pool_p, pts, pool_b, lens, r, lim)
            up = ops.radius_neighbors(pts, pool_p, lens, pool_b, 2 * r, lim)
        else:
            pool_p, pool_b = torch.zeros(0, 3, device=dev, dtype=F32), []
            pool = torch.zeros(0, 1, device=dev, dtype=torch.int64)
            up = torch.zeros(0, 1, device=dev, dtype=torch.int64)
        out["points"].append(pts)
        out["neighbors"].append(conv)
        out["pools"].append(pool)
        out["upsamples"].append(up)
        out["stack_lengths"].append(torch.tensor(lens, dtype=torch.int64))
        pts, lens = pool_p, pool_b
        r_normal *= 2
    n0 = out["points"][0].shape[0]
    out["features"] = torch.ones(n0, 1, device=dev, dtype=F32) if features is None else features.to(device=dev, dtype=F32)
    return out


def _same_pyramid(a, b):
    keys = ("num_layers", "first_subsampling_dl", "conv_radius")
    return all(a.config[k] == b.config[k] for k in keys)


@torch.no_grad()
def class_features(points, desc_net, ctx_net, neighborhood_limits):
    """(fea_3d (1, P, 256), geofea_3d (1, P, 32)) of one object's model points (P, 3), as model/RNNPose.py:162-206 slices
    ContextFeatureNet's and HybridDescNet's outputs: ready for eval_epoch.ClassModel.  The points are used as given (the
    caller normalises the model, data/preprocess.py:397-406)."""
    batch = kpconv_inputs(points, desc_net.config, neighborhood_limits)
    n0 = int(batch["stack_lengths"][0][0])
    geo = desc_net(batch)[:n0]
    if not _same_pyramid(desc_net, ctx_net):
        batch = kpconv_inputs(points, ctx_net.config, neighborhood_limits)
    ctx = ctx_net(batch)[:n0]
    return ctx[None].contiguous(), geo[None].contiguous()
