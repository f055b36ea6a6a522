"""SuperPoint2D (model/descriptor2D.py), the 2-D branch of HybridDescNet (model/HybridNet.py:97): the per-pixel descriptors of the
observed image that PoseRefiner consumes as `geofea_2d`, computed NHWC on the library's kernels.

    conv1a..conv4b   3x3 + ReLU           conv2d_nhwc(EPI_RELU), 160-row strips (conv1a: 3 channels padded to 4, 128-row kernel)
    pool             MaxPool2d(2, 2)      maxpool2x2_nhwc after conv1b, conv2b, conv3b
    decode1..3       Upsample(2) -> 3x3 -> InstanceNorm -> ReLU
                                          upsample2x_nhwc of [previous stage | skip] as two launches into ONE buffer (the previous
                                          stage's norm + ReLU applied tap by tap), conv2d_nhwc with tile statistics,
                                          instnorm_tiles_nhwc(stats_only) -- the norm itself is never materialised
    convDa, convDb   3x3 + ReLU, 1x1      conv2d_nhwc(in_norm = decode3's statistics, EPI_RELU), pixel_head_nhwc(L2) -> NCHW
    convPa, convPb   3x3 + IN + ReLU, 1x1 conv2d_nhwc(in_norm, tile statistics), pixel_head_nhwc(norm + ReLU on load, sigmoid) -> NCHW
                     (only with compute_scores: HybridDescNet discards the scores)

The batch runs in chunks of images (every operation is per image, so the result is bit-identical for any chunking: each layer's
kernel is fixed, not chosen by launch size).  Always three fp16 products per multiply-add (the reference runs this network in
fp32 whatever raft.mixed_precision says).  DESIGN.md section 12.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops

_CONVS = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b")
_TILE_STRIP160 = 5          # conv2d_nhwc tile code: 160-row strips (sources of whole 32-channel blocks)
_TILE_128x64 = 1            # the 128-row kernel, 128 x 64 tiles (conv1a's 4-channel source)


class DescriptorEngine:
    """SuperPoint2D's forward pass on one stream with eager launches (see the module docstring)."""

    MAX_TENSOR_BYTES = 5 << 28        # 1.25 GiB: the largest activation of a chunk (the 256-channel full-resolution map) stays below it

    def __init__(self, net):
        self.net = net
        self._key = None
        self._w = None

    def _mods(self):
        n = self.net
        m = {k: getattr(n, k) for k in _CONVS}
        m.update(d1=n.decode1[1], d2=n.decode2[1], d3=n.decode3[1], Da=n.convDa, Pa=n.convPa[0], Db=n.convDb, Pb=n.convPb)
        return m

    def _weights(self):
        mods = self._mods()
        key = ops.param_key(mods.values())
        if key == self._key:
            return self._w
        P = ops.PackedConv
        w = {}
        for k, m in mods.items():
            if k in ("Db", "Pb"):
                w[k] = (m.weight.detach().float().reshape(m.weight.shape[0], -1).contiguous(), m.bias.detach().float().contiguous())
            elif k == "conv1a":            # PackedConv segments are multiples of 4 channels: a zero fourth input channel
                wt = m.weight.detach().float()
                w4 = torch.zeros(wt.shape[0], 4, 3, 3, device=wt.device, dtype=torch.float32)
                w4[:, :wt.shape[1]] = wt
                pc = P(w4, m.bias, [4])
                pc.c_in_real = wt.shape[1]
                w[k] = pc
            else:
                w[k] = P(m.weight, m.bias, [m.weight.shape[1]])
        self._key, self._w = key, w
        return w

    def chunk_images(self, H, W):
        return max(1, self.MAX_TENSOR_BYTES // (H * W * 256 * 4))

    @staticmethod
    def _conv(pc, src, relu=True, stats=False, in_norm=None):
        tile = _TILE_128x64 if pc.seg_counts[0] % 32 else _TILE_STRIP160
        # src_bounded stays False: these layers see raw image values and un-normalised activations (the range check counts)
        return ops.conv2d_nhwc_new(pc, src, ops.EPI_RELU if relu else ops.EPI_LINEAR, 1, stats, in_norm, tile, src_bounded=False,
                                   single_product=False)

    def _chunk(self, W, img, desc_out, score_out, normalize_output):
        n, _, H, Wd = img.shape
        dev = img.device
        C, pool, up = self._conv, ops.maxpool2x2_nhwc, ops.upsample2x_nhwc
        x = torch.zeros(n, H, Wd, 4, device=dev, dtype=torch.float32)
        ops.nchw_to_nhwc(img, x)
        a, _ = C(W["conv1a"], x)
        a, _ = C(W["conv1b"], a)
        a, _ = C(W["conv2a"], pool(a))
        s2, _ = C(W["conv2b"], a)                               # skip of decode3
        a, _ = C(W["conv3a"], pool(s2))
        s3, _ = C(W["conv3b"], a)                               # skip of decode2
        a, _ = C(W["conv4a"], pool(s3))
        a, _ = C(W["conv4b"], a)
        r, ts = C(W["d1"], up(a), relu=False, stats=True)        # decode1
        mr = ops.instnorm_tiles_nhwc(r, ts, stats_only=True)
        for name, skip in (("d2", s3), ("d3", s2)):             # decode2 / decode3: up(cat(relu(IN(r)), skip)) = cat(up(.), up(skip))
            h, w = 2 * r.shape[1], 2 * r.shape[2]
            u = torch.empty(n, h, w, r.shape[3] + skip.shape[3], device=dev, dtype=torch.float32)
            up(r, u, mean_rstd=mr, relu=True)
            up(skip, u, dst_c_offset=r.shape[3])
            r, ts = C(W[name], u, relu=False, stats=True)
            mr = ops.instnorm_tiles_nhwc(r, ts, stats_only=True)
        del u, s2, s3, a
        da, _ = C(W["Da"], r, in_norm=mr)                       # relu(convDa(relu(IN(decode3))))
        wD, bD = W["Db"]
        ops.pixel_head_nhwc(da, wD, bD, ops.PH_L2 if normalize_output else ops.PH_LINEAR, out=desc_out)
        del da
        if score_out is not None:
            pa, tsp = C(W["Pa"], r, relu=False, stats=True, in_norm=mr)
            mrp = ops.instnorm_tiles_nhwc(pa, tsp, stats_only=True)
            wP, bP = W["Pb"]
            ops.pixel_head_nhwc(pa, wP, bP, ops.PH_SIGMOID, mean_rstd=mrp, relu=True, out=score_out)

    @torch.no_grad()
    def __call__(self, image, compute_scores=True, normalize_output=True, chunk=None):
        """image (B,3,H,W) fp32 CUDA, H and W multiples of 8 -> (descriptors (B,D,H,W), scores (B,1,H,W) or None)."""
        W = self._weights()
        img = ops._chk(image, "image")
        B, _, H, Wd = img.shape
        D = W["Db"][0].shape[0]
        desc = torch.empty(B, D, H, Wd, device=img.device, dtype=torch.float32)
        scores = torch.empty(B, 1, H, Wd, device=img.device, dtype=torch.float32) if compute_scores else None
        step = int(chunk) if chunk else self.chunk_images(H, Wd)
        for b0 in range(0, B, step):
            b1 = min(B, b0 + step)
            self._chunk(W, img[b0:b1], desc[b0:b1], None if scores is None else scores[b0:b1], normalize_output)
        return desc, scores


def _cfg_get(cfg, k, default=None):
    if isinstance(cfg, dict):
        return cfg.get(k, default)
    return getattr(cfg, k, default)


class SuperPoint2D(nn.Module):
    """Drop-in for model/descriptor2D.py:SuperPoint2D (parameter names and state_dict keys are the reference's) running on the
    HIP kernels.  The constructor loads no weight file (the reference reads weights/superpoint_v1.pth): pass `weights=` for the
    same shape-filtered load, or load_state_dict."""

    default_config = {
        "descriptor_dim": 256,
        "nms_radius": 4,
        "keypoint_threshold": 0.005,
        "max_keypoints": -1,
        "remove_borders": 4,
        "saliency_score_normalization_fuc": "sigmoid",
        "use_instance_norm": True,
    }

    def __init__(self, config, compute_scores: bool = True, weights=None, chunk=None):
        super().__init__()
        cfg = dict(self.default_config)
        keys = list(config.keys()) if hasattr(config, "keys") else [k for k in vars(config)]
        cfg.update({k: _cfg_get(config, k) for k in keys})
        self.config = cfg
        self.normalize_output = bool(cfg.get("normalize_output", True))
        if cfg.get("input_dim", 3) != 3:
            raise NotImplementedError("SuperPoint2D: only input_dim = 3 is implemented (the shipped configuration)")
        if not cfg["use_instance_norm"]:
            raise NotImplementedError("SuperPoint2D: use_instance_norm = False is not implemented")
        if cfg["saliency_score_normalization_fuc"] == "softmax":
            raise NotImplementedError("SuperPoint2D: the softmax saliency mode is not implemented")
        if cfg["saliency_score_normalization_fuc"] != "sigmoid":
            raise ValueError("saliency_score_normalization_fuc must be 'sigmoid' or 'softmax'")
        mk = cfg["max_keypoints"]
        if mk == 0 or mk < -1:
            raise ValueError('"max_keypoints" must be positive or "-1"')
        D = int(cfg["descriptor_dim"])
        if not 0 < D <= 32:
            raise NotImplementedError("SuperPoint2D: descriptor_dim must be at most 32 (the 1x1 head kernel's limit)")
        self.input_dim = 3
        self.compute_scores = bool(compute_scores)
        self.chunk = chunk
        c1, c2, c3, c4, c5 = 64, 64, 128, 128, 256
        cv = lambda i, o, k=3: nn.Conv2d(i, o, kernel_size=k, stride=1, padding=k // 2)
        self.conv1a, self.conv1b = cv(3, c1), cv(c1, c1)
        self.conv2a, self.conv2b = cv(c1, c2), cv(c2, c2)
        self.conv3a, self.conv3b = cv(c2, c3), cv(c3, c3)
        self.conv4a, self.conv4b = cv(c3, c4), cv(c4, c4)
        self.convPa = nn.Sequential(cv(c4, c5), nn.InstanceNorm2d(c5))
        self.convPb = cv(c5, 1, 1)
        self.convDa = cv(c4, c5)
        self.convDb = cv(c5, D, 1)
        stage = lambda i: nn.Sequential(nn.Upsample(scale_factor=2, mode="bilinear"), cv(i, c4), nn.InstanceNorm2d(c4), nn.ReLU())
        self.decode1, self.decode2, self.decode3 = stage(c4), stage(c4 + c3), stage(c4 + c2)
        self.engine = DescriptorEngine(self)
        self.last_range_events = None
        if weights is not None:
            self.load_state_dict(torch.load(str(weights), map_location="cpu"), strict=False)

    def load_state_dict(self, state_dict, strict=True):
        """The reference's semantics (descriptor2D.py:100-110): strict=False loads only the keys whose name AND shape match."""
        if not strict:
            own = self.state_dict()
            state_dict = {k: v for k, v in state_dict.items() if k in own and tuple(v.shape) == tuple(own[k].shape)}
        return super().load_state_dict(state_dict, strict)

    def _check(self, image):
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise RuntimeError("SuperPoint2D runs on the GPU only (no CPU path in rnnpose_amd)")
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError(f"image must be (B, 3, H, W), got {tuple(image.shape)}")
        H, W = image.shape[2:]
        if H % 8 or W % 8:
            raise ValueError(f"image height and width must be multiples of 8 (got {H} x {W}): three 2x2 poolings and up-samplings")

    @torch.no_grad()
    def forward(self, image):
        """image (B,3,H,W) fp32 CUDA -> {'keypoints': None, 'scores': (B,1,H,W) or None (compute_scores off),
        'descriptors': (B,D,H,W), 'f16x3_range_events': the sticky fp16x3 range-guard counter after the call (device tensor)}."""
        self._check(image)
        desc, scores = self.engine(image, compute_scores=self.compute_scores, normalize_output=self.normalize_output, chunk=self.chunk)
        self.last_range_events = ops.saturation_events()
        return {"keypoints": None, "scores": scores, "descriptors": desc, "f16x3_range_events": self.last_range_events}

    @torch.no_grad()
    def descriptors(self, image):
        """forward(image)['descriptors'] without the score branch."""
        self._check(image)
        desc, _ = self.engine(image, compute_scores=False, normalize_output=self.normalize_output, chunk=self.chunk)
        self.last_range_events = ops.saturation_events()
        return desc
