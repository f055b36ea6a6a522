"""Torch-tensor front end of the C ABI (include/rnnpose_hip.h): device memory and streams come from
PyTorch-ROCm, every computation is a hand-written HIP kernel in librnnpose_hip.so.

All ops take CUDA(=HIP) tensors, enqueue on torch's current stream, never synchronise and never fall back
to a CPU or ATen implementation: a non-GPU tensor or a missing library raises RuntimeError.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager

import torch

from . import _lib, env

F32 = torch.float32
F64 = torch.float64

# ---- optional per-op HIP-event timing (used by bench.py for the roofline object) -------------------------
_prof = None   # None or dict name -> list[(start_evt, end_evt)]


_event_pool = []        # timing events are reused across profile() contexts: creating ~1300 of them costs ~10 ms per step


@contextmanager
def profile(names=None):
    """Record HIP events around every op call (or only the ops in `names`) on the current stream.
    Yields a dict; after the context exits and the device is synchronised, call summarize()."""
    global _prof
    prev = _prof
    rec = {"_only": set(names) if names else None, "_next": 0}
    _prof = rec
    try:
        yield rec
    finally:
        _prof = prev


def profile_begin(names=None):
    """Non-context form of profile(): start recording, return the record dict; stop with profile_end()."""
    global _prof
    rec = {"_only": set(names) if names else None, "_next": 0, "_prev": _prof}
    _prof = rec
    return rec


def profile_end(rec):
    global _prof
    _prof = rec.get("_prev")


def profiling() -> bool:
    """True while a profile() context is recording (HIP events cannot be recorded into a captured graph)."""
    return _prof is not None


def summarize(rec) -> dict:
    """-> {name: (n_calls, mean_ms, total_ms, total_work, total_bytes)} (synchronises).  total_work / total_bytes = sums of
    the ALGORITHMIC flops / HBM bytes each launch declared for ITS OWN arguments (a half-batch launch declares half)."""
    torch.cuda.synchronize()
    out = {}
    for k, evs in rec.items():
        if k.startswith("_"):
            continue
        ms = [a.elapsed_time(b) for a, b, _, _ in evs]
        out[k] = (len(ms), sum(ms) / max(len(ms), 1), sum(ms), sum(w for _, _, w, _ in evs), sum(n for _, _, _, n in evs))
    return out


def _launch(name, *args, work=0, nbytes=0, products=3):
    """products: fp16 MFMA products per algorithmic multiply-add this launch executes (3 = fp16x3 split; 1 = a single-product
    strip launch) -- summed into rec["_exec"][name] as EXECUTED flops next to the algorithmic `work`."""
    rec = _prof
    if rec is not None and (rec["_only"] is None or name in rec["_only"]):
        ex = rec.setdefault("_exec", {})
        ex[name] = ex.get(name, 0.0) + products * work
        i = rec["_next"]
        rec["_next"] = i + 2
        while len(_event_pool) < i + 2:
            _event_pool.append(torch.cuda.Event(enable_timing=True))
        a, b = _event_pool[i], _event_pool[i + 1]
        a.record()
        _lib.call(name, *args)
        b.record()
        rec.setdefault(name, []).append((a, b, work, nbytes))
    else:
        _lib.call(name, *args)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: torch.Tensor, name: str, dtype=F32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); rnnpose_amd has no CPU path")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ---- a1+a2 ---------------------------------------------------------------------------------------------
def pyramid_layout(B, h, w, levels=4):
    offs = (C.c_int64 * (levels + 1))()
    hl = (C.c_int * levels)()
    wl = (C.c_int * levels)()
    _lib.call("rnnpose_corr_pyramid_layout", B, h, w, levels, offs, hl, wl)
    return list(offs), list(hl), list(wl)


def pyramid_level0_dense(buf, B, h, w):
    """Level 0 of a pyramid buffer in the reference's shape (B*h*w, 1, h, w): the buffer holds it j-patch-major
    ([b][8 x 16 patch][i][8][16], include/rnnpose_hip.h); a COPY made with torch indexing -- for the CorrBlock facade's
    `corr_pyramid` attribute and for tests, never on the refinement path (1 GB at the headline shape)."""
    N, npy, npx = h * w, -(-h // 8), -(-w // 16)
    v = buf[:B * npy * npx * N * 128].view(B, npy, npx, N, 8, 16)
    return v.permute(0, 3, 1, 4, 2, 5).reshape(B * N, 1, npy * 8, npx * 16)[:, :, :h, :w].contiguous()


def pyramid_from_levels(levels):
    """Inverse of PyramidLevels: the reference-shaped list [(B*h*w, 1, h_l, w_l)] -> the flat buffer the lookup kernels read
    (level 0 re-blocked j-patch-major with zero padding).  For the dispatcher-level operator set (torch_ops), which carries the
    pyramid as Tensor[]; the refinement path never leaves the buffer form."""
    l0 = levels[0]
    BN, _, h, w = l0.shape
    N = h * w
    B = BN // N
    npy, npx = -(-h // 8), -(-w // 16)
    p = torch.nn.functional.pad(l0[:, 0], (0, npx * 16 - w, 0, npy * 8 - h))
    blocked = p.view(B, N, npy, 8, npx, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1)
    return torch.cat([blocked] + [lv.reshape(-1) for lv in levels[1:]])


class PyramidLevels:
    """The levels of a pyramid buffer as the reference's list of (B*h*w, 1, h_l, w_l) tensors (thirdparty/raft/corr.py:23-34),
    materialised on access: levels 1.. are views of the buffer, level 0 is un-blocked into a copy (pyramid_level0_dense)."""

    def __init__(self, buf, offs, hl, wl, B, h, w):
        self.buf, self.offs, self.hl, self.wl, self.B, self.h, self.w = buf, offs, hl, wl, B, h, w

    def __len__(self):
        return len(self.hl)

    def __getitem__(self, l):
        if isinstance(l, slice):
            return [self[i] for i in range(*l.indices(len(self)))]
        l = range(len(self))[l]
        if l == 0:
            return pyramid_level0_dense(self.buf, self.B, self.h, self.w)
        return self.buf[self.offs[l]:self.offs[l + 1]].view(self.B * self.h * self.w, 1, self.hl[l], self.wl[l])

    def __iter__(self):
        return (self[i] for i in range(len(self)))


def _pyramid_bytes(B, Cc, h, w, levels, hl, wl):
    """algorithmic bytes of a volume build: both operands read once, every pyramid cell written once (fp32) --
    without the padding cells of level 0's border patches"""
    return 4.0 * (2 * B * h * w * Cc + B * h * w * sum(hl[l] * wl[l] for l in range(levels)))


def corr_pyramid(fmap1, fmap2, levels: int = 4, out=None, precision: str = "f32"):
    """fmap1,fmap2 (B,C,h,w) -> (flat buffer, [views (B*h*w,1,h_l,w_l)])   thirdparty/raft/corr.py:13-34.
    `out`: an existing flat buffer of the right size to overwrite (keeps the address stable for captured graphs).
    precision "f32": fp32 MFMA kernel on the NCHW maps; "f16x3": transpose to pixel-major + fp16x3-split kernel."""
    fmap1, fmap2 = _chk(fmap1, "fmap1"), _chk(fmap2, "fmap2")
    if fmap1.shape != fmap2.shape or fmap1.dim() != 4:
        raise ValueError("fmap1/fmap2 must both be (B,C,h,w)")
    B, Cc, h, w = fmap1.shape
    if precision == "f16x3":
        return _corr_pyramid_f16x3(fmap1, fmap2, 0, B, Cc, h, w, levels, out, A_SCALE)
    if precision != "f32":
        raise ValueError("precision must be 'f32' or 'f16x3'")
    offs, hl, wl = pyramid_layout(B, h, w, levels)
    buf = out if (out is not None and out.numel() == offs[-1] and out.device == fmap1.device) else \
        torch.empty(offs[-1], device=fmap1.device, dtype=F32)
    _launch("rnnpose_corr_pyramid_f32", _ptr(fmap1), _ptr(fmap2), B, Cc, h, w, levels, _ptr(buf), _stream(),
            work=2.0 * B * (h * w) ** 2 * Cc, nbytes=_pyramid_bytes(B, Cc, h, w, levels, hl, wl))
    return buf, PyramidLevels(buf, offs, hl, wl, B, h, w)


_pyr_ws = {}


CORR_VARIANT_DEFAULT = 0      # (the library's own default: csrc/corr_pyramid.hip g_corr_variant)


def corr_variant(variant: int):
    """Measurement switch (RNNPOSE_CORR_VARIANT): which fp16x3 volume kernel is launched -- 0 operands through registers + ds_write,
    1 operands by LDS-DMA (r06); bit-identical results."""
    _apply_conv_env()
    _lib.call("rnnpose_corr_variant", int(variant))


def _corr_pyramid_f16x3(f1, f2, layout, B, Cc, h, w, levels, out, a_scale):
    _apply_conv_env()
    n = int(_lib.load().rnnpose_corr_pyramid_f16x3_workspace_bytes(B, Cc, h, w))
    key = (f1.device, n)
    ws = _pyr_ws.get(key)
    if ws is None:
        range_guard_arm(f1.device)
        ws = _pyr_ws[key] = torch.empty(n // 2, device=f1.device, dtype=torch.float16)
    offs, hl, wl = pyramid_layout(B, h, w, levels)
    buf = out if (out is not None and out.numel() == offs[-1] and out.device == f1.device) else \
        torch.empty(offs[-1], device=f1.device, dtype=F32)
    _launch("rnnpose_corr_pyramid_f16x3", _ptr(f1), _ptr(f2), layout, B, Cc, h, w, levels, float(a_scale), _ptr(ws), n,
            _ptr(buf), _stream(), work=2.0 * B * (h * w) ** 2 * Cc, nbytes=_pyramid_bytes(B, Cc, h, w, levels, hl, wl))
    return buf, PyramidLevels(buf, offs, hl, wl, B, h, w)


def corr_pyramid_nhwc(f1, f2, levels: int = 4, out=None, a_scale: float = 8.0):
    """f1,f2 (B,h,w,C) pixel-major -> same (buffer, views) as corr_pyramid, fp16x3-split MFMA (fp32-class accuracy)."""
    f1, f2 = _nhwc(f1, "f1"), _nhwc(f2, "f2")
    if f1.shape != f2.shape:
        raise ValueError("f1/f2 must have the same (B,h,w,C) shape")
    B, h, w, Cc = f1.shape
    return _corr_pyramid_f16x3(f1, f2, 1, B, Cc, h, w, levels, out, a_scale)


class SplitTensor:
    """A (B,C,h,w) feature map held as a pixel-major split tensor (rnnpose_hip.h "SPLIT TENSORS": per 8-channel group fp16
    hi x 8 | fp16 lo x 8 of a_scale * x, in a float32-typed (B,h,w,C) buffer): what the encoder's output convolution writes
    for the volume build.  `shape` is the NCHW shape of the map it stands for; dense() converts back (tests, facade)."""

    def __init__(self, data, a_scale: float = 8.0):
        self.data = _nhwc(data, "split tensor")
        self.a_scale = float(a_scale)

    @property
    def shape(self):
        B, h, w, Cc = self.data.shape
        return torch.Size((B, Cc, h, w))

    @property
    def device(self):
        return self.data.device

    def float(self):
        return self

    def __getitem__(self, sl):
        if not isinstance(sl, slice):
            raise TypeError("SplitTensor supports batch slices only")
        return SplitTensor(self.data[sl], self.a_scale)

    def dense(self):
        return unsplit_hl(self.data, self.a_scale).permute(0, 3, 1, 2).contiguous()


def corr_pyramid_split(f1: SplitTensor, f2: SplitTensor, levels: int = 4, out=None):
    """Volume + pyramid from operands that are split tensors already (no pre-pass): (buffer, views) as corr_pyramid."""
    _apply_conv_env()
    if f1.shape != f2.shape or f1.a_scale != f2.a_scale:
        raise ValueError("f1/f2 must have the same shape and scale")
    B, Cc, h, w = f1.shape
    offs, hl, wl = pyramid_layout(B, h, w, levels)
    dev = f1.device
    buf = out if (out is not None and out.numel() == offs[-1] and out.device == dev) else torch.empty(offs[-1], device=dev, dtype=F32)
    _launch("rnnpose_corr_pyramid_split", _ptr(f1.data), _ptr(f2.data), B, Cc, h, w, levels, f1.a_scale, _ptr(buf), _stream(),
            work=2.0 * B * (h * w) ** 2 * Cc, nbytes=_pyramid_bytes(B, Cc, h, w, levels, hl, wl))
    return buf, PyramidLevels(buf, offs, hl, wl, B, h, w)


# ---- a3' (volume-free lookup: a measured alternative, thirdparty/raft/corr.py:70-98) ------------------------
def fmap_pyramid(f2, levels: int = 4):
    """f2 (B,h,w,C) pixel-major -> flat buffer holding levels 1..levels-1 of the 2x2-mean pyramid of the feature map."""
    f2 = _nhwc(f2, "f2")
    B, h, w, Cc = f2.shape
    n = int(_lib.load().rnnpose_fmap_pyramid_floats(B, h, w, Cc, levels))
    buf = torch.empty(max(n, 4), device=f2.device, dtype=F32)
    _launch("rnnpose_fmap_pyramid_f32", _ptr(f2), B, h, w, Cc, levels, _ptr(buf), _stream())
    return buf


def corr_alt_lookup(f1, f2, pooled, coords, levels: int = 4, radius: int = 4, out=None):
    """Window features computed on the fly (no volume): f1, f2 (B,h,w,C) pixel-major, pooled = fmap_pyramid(f2, levels),
    coords (B,2,h,w) -> (B,h,w,levels*81) pixel-major (the layout corr_lookup_nhwc writes)."""
    f1, f2 = _nhwc(f1, "f1"), _nhwc(f2, "f2")
    coords = _chk(coords, "coords")
    B, h, w, Cc = f1.shape
    if f2.shape != f1.shape or tuple(coords.shape) != (B, 2, h, w):
        raise ValueError("f1/f2 must share (B,h,w,C) and coords must be (B,2,h,w)")
    nch = levels * (2 * radius + 1) ** 2
    if out is None:
        out = torch.empty(B, h, w, nch, device=f1.device, dtype=F32)
    _launch("rnnpose_corr_alt_lookup_f32", _ptr(f1), _ptr(f2), _ptr(pooled), _ptr(coords), B, h, w, Cc, levels, radius, _ptr(out),
            out.shape[3], 0, _stream(), work=2.0 * B * h * w * levels * 100 * Cc)
    return out


# ---- a3 ------------------------------------------------------------------------------------------------
def _lookup_bytes(B, h, w, levels, radius):
    """per pixel and level a (2r+2)^2 texel footprint read + (2r+1)^2 outputs written, + 2 coords."""
    return 4.0 * B * h * w * (levels * (2 * radius + 2) ** 2 + levels * (2 * radius + 1) ** 2 + 2)


def corr_lookup(pyramid_buf, coords, levels: int = 4, radius: int = 4):
    """coords (B,2,h,w) -> (B, levels*81, h, w)                       thirdparty/raft/corr.py:36-57"""
    coords = _chk(coords, "coords")
    pyramid_buf = _chk(pyramid_buf, "pyramid")
    B, two, h, w = coords.shape
    if two != 2:
        raise ValueError("coords must be (B,2,h,w)")
    offs, _, _ = pyramid_layout(B, h, w, levels)
    if pyramid_buf.numel() != offs[-1]:
        raise ValueError("pyramid buffer does not match coords shape")
    out = torch.empty(B, levels * (2 * radius + 1) ** 2, h, w, device=coords.device, dtype=F32)
    _launch("rnnpose_corr_lookup_f32", _ptr(pyramid_buf), _ptr(coords), B, h, w, levels, radius, _ptr(out), _stream(),
            nbytes=_lookup_bytes(B, h, w, levels, radius))
    return out


# ---- a5 ------------------------------------------------------------------------------------------------
def context_prep(ctx, h, w, hdim: int = 128):
    ctx = _chk(ctx, "context_fea")
    B, Cc, H, W = ctx.shape
    net = torch.empty(B, hdim, h, w, device=ctx.device, dtype=F32)
    inp = torch.empty(B, Cc - hdim, h, w, device=ctx.device, dtype=F32)
    _launch("rnnpose_context_prep_f32", _ptr(ctx), B, Cc, H, W, h, w, hdim, _ptr(net), _ptr(inp), _stream(),
            nbytes=4.0 * B * Cc * h * w * 5)        # 4 taps read + 1 value written per low-res element
    return net, inp


def flow_to_coords(flow_init, h, w):
    flow_init = _chk(flow_init, "flow_init")
    B, two, H, W = flow_init.shape
    out = torch.empty(B, 2, h, w, device=flow_init.device, dtype=F32)
    _launch("rnnpose_flow_to_coords_f32", _ptr(flow_init), B, H, W, h, w, _ptr(out), _stream())
    return out


# ---- a6 ------------------------------------------------------------------------------------------------
def convex_upsample(flow, mask, scale: int = 8):
    flow, mask = _chk(flow, "flow"), _chk(mask, "mask")
    B, _, h, w = flow.shape
    if mask.shape != (B, 9 * scale * scale, h, w):
        raise ValueError(f"mask must be (B,{9*scale*scale},h,w)")
    out = torch.empty(B, 2, scale * h, scale * w, device=flow.device, dtype=F32)
    _launch("rnnpose_convex_upsample_f32", _ptr(flow), _ptr(mask), B, h, w, scale, _ptr(out), _stream(),
            nbytes=4.0 * B * h * w * (9 * scale * scale + 2 + 2 * scale * scale))
    return out


# ---- a7 ------------------------------------------------------------------------------------------------
def induced_flow(depth, K, G, eps: float = 1e-5, want_vmask: bool = True, absolute: bool = False):
    """depth (B,1,H,W) raw, K (B,3,3), G (B,[1,]4,4) -> flow (B,2,H,W), vmask (B,H,W) or None.
    absolute=True returns the raw re-projected coordinates (SE3.transform) instead of the masked flow."""
    depth, K, G = _chk(depth, "depth"), _chk(K, "intrinsics"), _chk(G, "G")
    B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    flow = torch.empty(B, 2, H, W, device=depth.device, dtype=F32)
    vmask = torch.empty(B, H, W, device=depth.device, dtype=F32) if want_vmask else None
    _launch("rnnpose_induced_flow_f32", _ptr(depth), _ptr(K), _ptr(G), B, H, W, eps, int(absolute), _ptr(flow), _ptr(vmask),
            _stream())
    return flow, vmask


def induced_coords_lowres(depth, K, G, h, w, eps: float = 1e-5, out=None):
    depth, K, G = _chk(depth, "depth"), _chk(K, "intrinsics"), _chk(G, "G")
    B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    if out is None:
        out = torch.empty(B, 2, h, w, device=depth.device, dtype=F32)
    _launch("rnnpose_induced_coords_lowres_f32", _ptr(depth), _ptr(K), _ptr(G), B, H, W, h, w, eps, _ptr(out), _stream())
    return out


# ---- a8 ------------------------------------------------------------------------------------------------
def _target_mode(target, H, W):
    if target.dim() >= 3 and target.shape[-1] == 2 and target.shape[-3:-1] == (H, W):
        return 0      # (B,[K,]H,W,2) absolute coordinates
    if target.dim() == 4 and target.shape[1] == 2 and target.shape[-2:] == (H, W):
        return 1      # (B,2,H,W) planar flow, grid added in-kernel
    raise ValueError(f"target has shape {tuple(target.shape)}; expected (B,H,W,2) or (B,2,H,W)")


def corr_weight(g1, g2, target, depth, sigma, out=None):
    g1, g2, target, depth = _chk(g1, "g1"), _chk(g2, "g2"), _chk(target, "target"), _chk(depth, "depth")
    sigma = _chk(sigma.reshape(-1)[:1], "sigma")
    B, D, H, W = g1.shape
    mode = _target_mode(target, H, W)
    if out is None:
        out = torch.empty(B, H, W, device=g1.device, dtype=F32)
    _launch("rnnpose_corr_weight_f32", _ptr(g1), _ptr(g2), _ptr(target), mode, _ptr(depth), _ptr(sigma), B, D, H, W,
            _ptr(out), _stream(), nbytes=4.0 * B * H * W * (2 * D + 2 + 1 + 1))   # g1, g2 (unique texels), target, depth, w
    return out


# ---- a9-a11 --------------------------------------------------------------------------------------------
_ws_cache = {}


def _workspace(B, H, W, device, slot=0):
    """slot: calls that may run concurrently on different streams (the two batch halves) need distinct workspaces."""
    n = int(_lib.load().rnnpose_lm_workspace_bytes(B, H, W))
    # keyed on the SHAPE, not on the byte count: the first B doubles are the arrival counters of the fused LM step (zero between
    # launches), the partial records follow -- two shapes of equal size would find each other's partial sums where their counters
    # should be zero and the fused tail would never fire
    key = (device, int(B), int(H), int(W), slot)
    ws = _ws_cache.get(key)
    if ws is None:
        ws = torch.zeros(n // 8, device=device, dtype=F64)      # (zero: the arrival counters live in the first B doubles)
        _ws_cache[key] = ws
    return ws, n


def _lm_front(target, weight, depth, K, slot=0):
    """What the four LM functions do first -> (target, weight, depth, K, B, H, W, target mode, workspace, its bytes)."""
    target, weight, depth = _chk(target, "target"), _chk(weight, "weight"), _chk(depth, "depth")
    K = _chk(K, "intrinsics")
    B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    mode = _target_mode(target, H, W)
    ws, n = _workspace(B, H, W, depth.device, slot)
    return target, weight, depth, K, B, H, W, mode, ws, n


_LM_OUT = dict(G=((4, 4), F32), Hm=((6, 6), F64), bv=((6,), F64), xi=((6,), F32), info=((), torch.int32), dstats=((2,), F64))


def _lm_out(out, B, device, names):
    """The caller's preallocated views, or fresh buffers of the named outputs."""
    if out is not None:
        return tuple(out)
    return tuple(torch.empty(B, *_LM_OUT[k][0], device=device, dtype=_LM_OUT[k][1]) for k in names.split())


def _pose_in(G):
    G = _chk(G, "G").reshape(-1, 4, 4)
    return G if G.is_contiguous() else G.contiguous()


def lm_normal_eq(target, weight, depth, K, G, eps: float = 1e-5):
    """-> Hm (B,6,6) fp64 (undamped), bv (B,6) fp64             geometry/transformation.py:286-297"""
    target, weight, depth, K, B, H, W, mode, ws, n = _lm_front(target, weight, depth, K)
    G = _chk(G, "G")
    Hm, bv = _lm_out(None, B, depth.device, "Hm bv")
    _launch("rnnpose_lm_normal_eq_f64", _ptr(target), mode, _ptr(weight), _ptr(depth), eps, _ptr(K), _ptr(G), B, H, W,
            _ptr(ws), n, _ptr(Hm), _ptr(bv), _stream(), nbytes=16.0 * B * H * W, work=200.0 * B * H * W)
    return Hm, bv


def lm_solve_update(Hm, bv, G, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0):
    """-> G_new (B,4,4), xi (B,6) fp32, info (B,) int32"""
    Hm, bv, G = _chk(Hm, "H", F64), _chk(bv, "b", F64), _chk(G, "G")
    B = Hm.shape[0]
    G_new = torch.empty(B, 4, 4, device=G.device, dtype=F32)
    xi = torch.empty(B, 6, device=G.device, dtype=F32)
    info = torch.empty(B, device=G.device, dtype=torch.int32)
    _launch("rnnpose_lm_solve_update_f32", _ptr(Hm), _ptr(bv), _ptr(G), B, float(ep_lambda), float(lm_lambda),
            float(max_update), _ptr(G_new), _ptr(xi), _ptr(info), _stream())
    return G_new, xi, info


def lm_step(target, weight, depth, K, G, num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0, eps=1e-5, out=None,
            slot=0):
    """num_iters fused GN steps; returns (G_new (B,4,4), Hm, bv, xi, info) of the last iteration.
    out: optional preallocated (G_new, Hm, bv, xi, info) views to write into; slot: workspace slot (see _workspace)."""
    _apply_lm_env()
    target, weight, depth, K, B, H, W, mode, ws, n = _lm_front(target, weight, depth, K, slot)
    Gd, Hm, bv, xi, info = _lm_out(out, B, depth.device, "G Hm bv xi info")
    cost = dict(nbytes=16.0 * B * H * W * int(num_iters), work=200.0 * B * H * W * int(num_iters))
    if out is not None and int(num_iters) >= 1:         # (every step writes all five outputs for every image)
        _launch("rnnpose_lm_step_io_f32", _ptr(target), mode, _ptr(weight), _ptr(depth), eps, _ptr(K), _ptr(_pose_in(G)), _ptr(Gd), B, H, W,
                int(num_iters), float(ep_lambda), float(lm_lambda), float(max_update), _ptr(ws), n, _ptr(Hm), _ptr(bv),
                _ptr(xi), _ptr(info), _stream(), **cost)
        return Gd, Hm, bv, xi, info
    # in place on a copy of G; without an iteration that copy, a zero xi and a zero info are the result
    Gd.copy_(_chk(G, "G").reshape(-1, 4, 4))
    xi.zero_()
    info.zero_()
    _launch("rnnpose_lm_step_f32", _ptr(target), mode, _ptr(weight), _ptr(depth), eps, _ptr(K), _ptr(Gd), B, H, W,
            int(num_iters), float(ep_lambda), float(lm_lambda), float(max_update), _ptr(ws), n, _ptr(Hm), _ptr(bv),
            _ptr(xi), _ptr(info), _stream(), **cost)
    return Gd, Hm, bv, xi, info


DEPTH_TERM_DEFAULTS = dict(depth_weight=1.0, depth_gate=0.05, edge_tol=0.02)      # DESIGN.md section 18 (gate and edge tolerance: unmeasured choices)


def depth_term_params(depth_term):
    """None / False -> None (term off); True -> the defaults; a dict of any of depth_weight, depth_gate, edge_tol -> the full dict.
    Values must be finite and >= 0 (ValueError)."""
    if depth_term is None or depth_term is False:
        return None
    p = dict(DEPTH_TERM_DEFAULTS)
    if depth_term is not True:
        extra = set(depth_term) - set(p)
        if extra:
            raise ValueError(f"depth_term: unknown keys {sorted(extra)}; known: {sorted(p)}")
        p.update({k: float(v) for k, v in depth_term.items()})
    for k, v in p.items():
        if not (v >= 0.0 and v != float("inf")):
            raise ValueError(f"depth_term: {k} must be finite and >= 0, got {v}")
    return p


def _rgbd_args(fn, B, obs_depth, theta, K_obs, src_index, index_rows, depth_weight, depth_gate, edge_tol):
    """Host-side checks of the depth arguments -> (obs_depth, theta, K_obs, index device tensor or None, S, Ho, Wo)."""
    obs_depth, theta, K_obs = _chk(obs_depth, "obs_depth"), _chk(theta, "theta"), _chk(K_obs, "K_obs")
    if obs_depth.dim() == 4 and obs_depth.shape[1] == 1:
        obs_depth = obs_depth[:, 0]
    if obs_depth.dim() != 3 or obs_depth.numel() == 0:
        raise ValueError(f"{fn}: obs_depth must be (S,Ho,Wo) or (S,1,Ho,Wo), got {tuple(obs_depth.shape)}")
    S, Ho, Wo = obs_depth.shape
    if tuple(theta.shape) != (B, 2, 3):
        raise ValueError(f"{fn}: theta must be ({B},2,3), got {tuple(theta.shape)}")
    if tuple(K_obs.shape) != (B, 3, 3):
        raise ValueError(f"{fn}: K_obs must be ({B},3,3), got {tuple(K_obs.shape)}")
    for name, v in (("depth_weight", depth_weight), ("depth_gate", depth_gate), ("edge_tol", edge_tol)):
        if not (float(v) >= 0.0 and float(v) != float("inf")):
            raise ValueError(f"{fn}: {name} must be finite and >= 0, got {v}")
    idx = None
    if src_index is None:
        if S != B:
            raise ValueError(f"{fn}: without src_index the observed depth holds one frame per object: {S} frames, {B} objects")
    else:
        if not isinstance(src_index, SourceIndex):
            src_index = SourceIndex(src_index, S, obs_depth.device)
        b0, b1 = index_rows if index_rows is not None else (0, len(src_index))
        if src_index.S != S or not 0 <= b0 < b1 <= len(src_index) or b1 - b0 != B:
            raise ValueError(f"{fn}: src_index rows [{b0}, {b1}) of {len(src_index)} objects in {src_index.S} frames; there are {B} objects, "
                             f"{S} frames")
        idx = src_index.dev[b0:b1]
    return obs_depth.contiguous(), theta, K_obs, idx, S, Ho, Wo


def lm_normal_eq_rgbd(target, weight, depth, K, G, obs_depth, theta, K_obs, src_index=None, depth_weight=1.0, depth_gate=0.05,
                      edge_tol=0.02, eps: float = 1e-5, index_rows=None):
    """lm_normal_eq with the depth term of the observed depth (include/rnnpose_hip.h).
    obs_depth (S,Ho,Wo) or (S,1,Ho,Wo); theta (B,2,3) the crop maps; K_obs (B,3,3) full-frame intrinsics; src_index: an
    ops.SourceIndex, B integers or None (S == B); index_rows (b0, b1): the objects are rows [b0, b1) of src_index.
    -> Hm (B,6,6), bv (B,6), dstats (B,2) fp64 [active pixels, sum v w omega |r3|^2]."""
    target, weight, depth, K, B, H, W, mode, ws, n = _lm_front(target, weight, depth, K)
    G = _chk(G, "G")
    obs_depth, theta, K_obs, idx, S, Ho, Wo = _rgbd_args("lm_normal_eq_rgbd", B, obs_depth, theta, K_obs, src_index, index_rows, depth_weight,
                                                         depth_gate, edge_tol)
    Hm, bv, dstats = _lm_out(None, B, depth.device, "Hm bv dstats")
    _launch("rnnpose_lm_normal_eq_rgbd_f64", _ptr(target), mode, _ptr(weight), _ptr(depth), eps, _ptr(K), _ptr(G), B, H, W, _ptr(obs_depth),
            _ptr(idx), _ptr(theta), _ptr(K_obs), S, Ho, Wo, float(depth_weight), float(depth_gate), float(edge_tol), _ptr(ws), n, _ptr(Hm),
            _ptr(bv), _ptr(dstats), _stream(), nbytes=32.0 * B * H * W, work=300.0 * B * H * W)
    return Hm, bv, dstats


def lm_step_rgbd(target, weight, depth, K, G, obs_depth, theta, K_obs, src_index=None, depth_weight=1.0, depth_gate=0.05, edge_tol=0.02,
                 num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0, eps=1e-5, out=None, slot=0, index_rows=None):
    """lm_step with the depth term (arguments: lm_normal_eq_rgbd); num_iters >= 1 fused GN steps.
    -> (G_new (B,4,4), Hm, bv, xi, info, dstats (B,2) fp64) of the last iteration.  out: optional preallocated
    (G_new, Hm, bv, xi, info, dstats) views to write into; slot: workspace slot, as for lm_step."""
    _apply_lm_env()
    if int(num_iters) < 1:
        raise ValueError("lm_step_rgbd: num_iters must be >= 1")
    target, weight, depth, K, B, H, W, mode, ws, n = _lm_front(target, weight, depth, K, slot)
    obs_depth, theta, K_obs, idx, S, Ho, Wo = _rgbd_args("lm_step_rgbd", B, obs_depth, theta, K_obs, src_index, index_rows, depth_weight,
                                                         depth_gate, edge_tol)
    Gin = _pose_in(G)
    Gd, Hm, bv, xi, info, dstats = _lm_out(out, B, depth.device, "G Hm bv xi info dstats")
    _launch("rnnpose_lm_step_rgbd_io_f32", _ptr(target), mode, _ptr(weight), _ptr(depth), eps, _ptr(K), _ptr(Gin), _ptr(Gd), B, H, W,
            int(num_iters), float(ep_lambda), float(lm_lambda), float(max_update), _ptr(obs_depth), _ptr(idx), _ptr(theta), _ptr(K_obs), S, Ho,
            Wo, float(depth_weight), float(depth_gate), float(edge_tol), _ptr(ws), n, _ptr(Hm), _ptr(bv), _ptr(xi), _ptr(info), _ptr(dstats),
            _stream(), nbytes=32.0 * B * H * W * int(num_iters), work=300.0 * B * H * W * int(num_iters))
    return Gd, Hm, bv, xi, info, dstats


# ---- views of one object from several calibrated cameras ---------------------------------------
class ViewGroups:
    """Which rows of a batch are views of one object, and every view's camera-from-rig transform (`lm_step_views`,
    `PoseRefiner.forward(view_groups=)`).  groups: either group_of_view, B group numbers 0, 0, .., 1, 1, .. (starting at 0, every next
    one equal or one larger: the views of a group are contiguous rows), or group_start, n_groups + 1 row numbers 0 < .. < B (the list
    whose last entry is B).  cam_from_rig: (B,4,4) rigid transforms E_v (finite, last row 0 0 0 1), or None = the identity for every
    view.  Checked ON THE HOST once (ValueError); holds the device copies the kernel reads.  Build it once per batch."""

    def __init__(self, groups, cam_from_rig, B, device):
        B = int(B)
        if isinstance(groups, torch.Tensor):
            if groups.dtype.is_floating_point or groups.dtype == torch.bool or groups.dim() != 1:
                raise ValueError("ViewGroups: groups must be a 1-D integer tensor")
            groups = groups.detach().cpu().tolist()
        host = [int(v) for v in groups]
        if B < 1 or not host:
            raise ValueError(f"ViewGroups: needs at least one view and one group (B = {B}, {len(host)} entries)")
        if host[-1] != B:                                               # group_of_view -> group_start
            if len(host) != B or host[0] != 0 or any(b - a not in (0, 1) for a, b in zip(host, host[1:])):
                raise ValueError(f"ViewGroups: group_of_view must name {B} views with group numbers that start at 0 and stay or grow by one "
                                 f"from row to row; got {host[:8]}{'...' if len(host) > 8 else ''}")
            host = [0] + [i for i in range(1, B) if host[i] != host[i - 1]] + [B]
        if host[0] != 0 or len(host) < 2 or any(b <= a for a, b in zip(host, host[1:])):
            raise ValueError(f"ViewGroups: group_start must start at 0, increase strictly and end at B = {B}; got {host[:8]}"
                             f"{'...' if len(host) > 8 else ''}")
        if cam_from_rig is None:
            E = torch.eye(4, dtype=F32).repeat(B, 1, 1)
        else:
            E = torch.as_tensor(cam_from_rig).detach().to(device="cpu", dtype=F32).reshape(-1, 4, 4).contiguous()
            if E.shape[0] != B:
                raise ValueError(f"ViewGroups: cam_from_rig holds {E.shape[0]} transforms, the batch {B} views")
            last = torch.tensor([0.0, 0.0, 0.0, 1.0])
            if not bool(torch.isfinite(E).all()) or not bool((E[:, 3] == last).all()):
                raise ValueError("ViewGroups: cam_from_rig must be finite with the last row 0 0 0 1")
        self.B = B
        self.host = tuple(host)
        self.E_host = E
        self.group_start = torch.tensor(host, dtype=torch.int32, device=device)
        self.E = E.to(device)

    @classmethod
    def from_device(cls, group_start, E, host, E_host):
        """Checked groups over other device copies of the same entries (the persistent input buffers of a captured graph)."""
        self = cls.__new__(cls)
        self.host, self.E_host, self.group_start, self.E = tuple(host), E_host, group_start, E
        self.B = self.host[-1]
        return self

    @property
    def n_groups(self):
        return len(self.host) - 1

    def __len__(self):
        return self.B

    def key(self):
        """The group layout (what a captured graph depends on besides the buffers)."""
        return self.host

    def first_rows(self):
        return self.host[:-1]

    def first_rows_dev(self):
        """(n_groups,) int64 device tensor: the row of every group's first view"""
        if getattr(self, "_first_rows", None) is None:
            self._first_rows = torch.tensor(self.host[:-1], dtype=torch.int64, device=self.E.device)
        return self._first_rows

    def first_of_view(self):
        """(B,) int64 device tensor: for every view, the row of its group's first view"""
        if getattr(self, "_first_of_view", None) is None:
            rows = [a for a, b in zip(self.host, self.host[1:]) for _ in range(b - a)]
            self._first_of_view = torch.tensor(rows, dtype=torch.int64, device=self.E.device)
        return self._first_of_view

    def rows(self, b0, b1):
        """The groups of rows [b0, b1) as ViewGroups of that batch part; b0 and b1 must be group boundaries (ValueError)."""
        b0, b1 = int(b0), int(b1)
        if b0 == 0 and b1 == self.B:
            return self
        parts = self.__dict__.setdefault("_parts", {})                  # (memoised: a captured graph reads the part's device array)
        if (b0, b1) in parts:
            return parts[(b0, b1)]
        if b0 not in self.host or b1 not in self.host or not b0 < b1:
            raise ValueError(f"ViewGroups.rows: [{b0}, {b1}) does not start and end at group boundaries {self.host}")
        g0, g1 = self.host.index(b0), self.host.index(b1)
        part = ViewGroups.__new__(ViewGroups)
        part.B = b1 - b0
        part.host = tuple(v - b0 for v in self.host[g0:g1 + 1])
        part.E_host, part.E = self.E_host[b0:b1], self.E[b0:b1]
        part.group_start = torch.tensor(part.host, dtype=torch.int32, device=self.group_start.device)
        parts[(b0, b1)] = part
        return part


def lm_step_views(target, weight, depth, K, G, groups, rgbd=None, num_iters=1, ep_lambda=100.0, lm_lambda=1e-4, max_update=1.0, eps=1e-5,
                  out=None, slot=0):
    """The grouped LM step (include/rnnpose_hip.h: rnnpose_lm_step_views_io_f32): ONE increment per group of views, solved from the summed
    systems of the group's views.  groups: an ops.ViewGroups over the B rows.  rgbd: None = the plain sums, or a dict of lm_step_rgbd's
    depth arguments (obs_depth, theta, K_obs and optionally src_index, index_rows, depth_weight, depth_gate, edge_tol): the depth term
    composes, it is per view.  num_iters >= 1.
    -> (G_new (B,4,4), Hm (B,6,6), bv (B,6), Hg (n_groups,6,6), bg (n_groups,6), xi (n_groups,6), info (n_groups,)[, dstats (B,2)]) of
    the last iteration; out: optional preallocated views of these to write into; slot: workspace slot, as for lm_step."""
    if not isinstance(groups, ViewGroups):
        raise TypeError("lm_step_views: groups must be an ops.ViewGroups")
    if int(num_iters) < 1:
        raise ValueError("lm_step_views: num_iters must be >= 1")
    target, weight, depth, K, B, H, W, mode, ws, n = _lm_front(target, weight, depth, K, slot)
    if len(groups) != B:
        raise ValueError(f"lm_step_views: the groups cover {len(groups)} views, the batch holds {B}")
    ng = groups.n_groups
    if rgbd is not None:
        r = dict(DEPTH_TERM_DEFAULTS, src_index=None, index_rows=None)
        extra = set(rgbd) - set(r) - {"obs_depth", "theta", "K_obs"}
        if extra or not {"obs_depth", "theta", "K_obs"} <= set(rgbd):
            raise ValueError(f"lm_step_views: rgbd needs obs_depth, theta, K_obs and takes {sorted(r)}; unknown keys {sorted(extra)}")
        r.update(rgbd)
        obs_depth, theta, K_obs, idx, S, Ho, Wo = _rgbd_args("lm_step_views", B, r["obs_depth"], r["theta"], r["K_obs"], r["src_index"],
                                                             r["index_rows"], r["depth_weight"], r["depth_gate"], r["edge_tol"])
        dargs = (_ptr(obs_depth), _ptr(idx), _ptr(theta), _ptr(K_obs), S, Ho, Wo, float(r["depth_weight"]), float(r["depth_gate"]),
                 float(r["edge_tol"]))
    else:
        dargs = (_ptr(None), _ptr(None), _ptr(None), _ptr(None), 0, 0, 0, 0.0, 0.0, 0.0)
    Gin = _pose_in(G)
    dev = depth.device
    if out is not None:
        outs = tuple(out)
    else:
        outs = _lm_out(None, B, dev, "G Hm bv") + _lm_out(None, ng, dev, "Hm bv xi info") + (_lm_out(None, B, dev, "dstats") if rgbd is not None else ())
    Gd, Hm, bv, Hg, bg, xi, info = outs[:7]
    dstats = outs[7] if rgbd is not None else None
    per_px = 32.0 if rgbd is not None else 16.0
    _launch("rnnpose_lm_step_views_io_f32", _ptr(target), mode, _ptr(weight), _ptr(depth), eps, _ptr(K), _ptr(Gin), _ptr(Gd), B, H, W,
            int(num_iters), float(ep_lambda), float(lm_lambda), float(max_update), *dargs, _ptr(groups.group_start), ng, _ptr(groups.E),
            _ptr(ws), n, _ptr(Hm), _ptr(bv), _ptr(Hg), _ptr(bg), _ptr(xi), _ptr(info), _ptr(dstats), _stream(),
            nbytes=per_px * B * H * W * int(num_iters), work=(300.0 if rgbd is not None else 200.0) * B * H * W * int(num_iters))
    return outs[:8] if rgbd is not None else outs[:7]


_lm_fused_env_applied = False


def _apply_lm_env():
    """RNNPOSE_LM_FUSED=0/1 selects the LM step form at first use (same-box A/B); default: the library's."""
    global _lm_fused_env_applied
    if not _lm_fused_env_applied:
        _lm_fused_env_applied = True
        v = env.flag("RNNPOSE_LM_FUSED", None)
        if v is not None:
            _lib.call("rnnpose_lm_fused_tail", int(v))


def lm_fused_tail(enable: bool = True):
    """One launch per LM step (default) or the r02 three-launch form (measurement switch; drop captured graphs when toggling)."""
    _lib.call("rnnpose_lm_fused_tail", int(bool(enable)))


def se3_exp(xi):
    xi = _chk(xi, "xi")
    sh = xi.shape[:-1]
    x = xi.reshape(-1, 6)
    out = torch.empty(x.shape[0], 4, 4, device=xi.device, dtype=F32)
    _launch("rnnpose_se3_exp_f32", _ptr(x), x.shape[0], _ptr(out), _stream())
    return out.reshape(*sh, 4, 4)


def se3_compose(A, Bm):
    A, Bm = _chk(A, "A"), _chk(Bm, "B")
    if A.shape != Bm.shape:
        raise ValueError("se3_compose needs equal shapes")
    out = torch.empty_like(A)
    _launch("rnnpose_se3_compose_f32", _ptr(A), _ptr(Bm), A.numel() // 16, _ptr(out), _stream())
    return out


def se3_outer_update(Tij, Ti, literal: bool = True):
    """-> (Ti_new, Tij_new) = (Tij Ti, literal ? Ti_new Ti_new^-1 : I): the pose bookkeeping between two outer iterations
    (model/PoseRefiner.py:241-244) as one launch; bit-identical to se3_compose / se3_inverse / se3_compose."""
    Tij, Ti = _chk(Tij, "Tij"), _chk(Ti, "Ti")
    if Tij.shape != Ti.shape:
        raise ValueError("se3_outer_update needs equal shapes")
    Ti_new, Tij_new = torch.empty_like(Ti), torch.empty_like(Tij)
    _launch("rnnpose_se3_outer_update_f32", _ptr(Tij), _ptr(Ti), Ti.numel() // 16, int(bool(literal)), _ptr(Ti_new), _ptr(Tij_new), _stream())
    return Ti_new, Tij_new


def se3_inverse(A):
    A = _chk(A, "A")
    out = torch.empty_like(A)
    _launch("rnnpose_se3_inverse_f32", _ptr(A), A.numel() // 16, _ptr(out), _stream())
    return out


# ---- a4 pointwise ---------------------------------------------------------------------------------------
def gru_gate(zr, hcat, z_out, rhx, C: int = 128):
    """zr (B,2C,h,w) pre-activations; hcat (B,Ctot,h,w) with h in [:C]; writes z_out (B,C,h,w), rhx[:, :C]."""
    B, Ctot = hcat.shape[0], hcat.shape[1]
    hw = hcat.shape[2] * hcat.shape[3]
    _launch("rnnpose_gru_gate_f32", _ptr(zr), _ptr(hcat), B, C, Ctot, hw, _ptr(z_out), _ptr(rhx), _stream())


def gru_update(z, q_pre, hcat, hout, C: int = 128):
    """hout[:, :C] = (1-z)*hcat[:, :C] + z*tanh(q_pre)  (hout may be hcat itself)."""
    B = hcat.shape[0]
    hw = hcat.shape[2] * hcat.shape[3]
    _launch("rnnpose_gru_update_f32", _ptr(z), _ptr(q_pre), _ptr(hcat), B, C, hcat.shape[1], hw, _ptr(hout), hout.shape[1],
            _stream())


# ---- a4 dense convolutions: NHWC implicit GEMM on the fp16 matrix cores with fp16x3 split (fp32-class accuracy) ----
EPI_LINEAR, EPI_RELU, EPI_GRU_ZR, EPI_GRU_Q = 0, 1, 2, 3
# Activation scale of the fp16x3 split (x * A_SCALE = hi + lo in fp16).  Range: |x| <= 65504 / A_SCALE = 8188; full 21-22
# bit precision while lo stays a normal fp16 (|x| >= 2^-3 / A_SCALE = 0.016), below that the ABSOLUTE error stays under
# 2^-25 / A_SCALE = 4e-9 -- fp32-class for O(1) activations either way.  (r01 used 64: range 1023, too tight for
# real correlation magnitudes; saturation is counted by the range guard, ops.saturation_check.)
A_SCALE = 8.0


class PackedConv:
    """Weights of one convolution, split into fp16 hi/lo and laid out for csrc/conv_igemm.hip.
    weight (Cout,Cin,kh,kw), bias (Cout,), seg_counts = channel counts of the virtual-concat sources (sum = Cin).
    post_scale is folded into weight and bias (the 0.25 of the mask head, update.py:187)."""

    def __init__(self, weight, bias, seg_counts=None, post_scale: float = 1.0, a_scale: float = A_SCALE):
        import math
        range_guard_arm(weight.device)
        w = _chk(weight.detach(), "weight") * post_scale
        b = _chk(bias.detach(), "bias") * post_scale
        self.c_out, self.c_in, self.kh, self.kw = w.shape
        self.c_in_real = self.c_in          # engines that zero-pad input channels overwrite this for flop accounting
        self.seg_counts = [int(c) for c in (seg_counts or [self.c_in])]
        if sum(self.seg_counts) != self.c_in:
            raise ValueError("seg_counts must sum to the input channels")
        wmax = float(w.abs().max())
        self.w_scale = float(2.0 ** math.floor(math.log2(1024.0 / wmax))) if wmax > 0 else 1.0
        self.a_scale = float(a_scale)
        segs = (C.c_int * len(self.seg_counts))(*self.seg_counts)
        n = int(_lib.load().rnnpose_conv_packed_halfs(self.c_out, self.kh, self.kw, segs, len(self.seg_counts)))
        if n <= 0:
            raise ValueError("unsupported convolution shape")
        self.w_packed = torch.empty(n, device=w.device, dtype=torch.float16)
        self.bias = b.contiguous()
        _lib.call("rnnpose_conv_pack_weights_f16x3", _ptr(w), self.c_out, self.c_in, self.kh, self.kw, segs,
                  len(self.seg_counts), self.w_scale, _ptr(self.w_packed), _stream())


def param_key(modules):
    """Identity of the live parameters of `modules` (each with .weight and .bias): changes on load_state_dict / in-place updates / .to().
    The packed copies the engines cache, and every captured graph, depend on it."""
    return tuple((m.weight._version, m.weight.data_ptr(), m.bias._version, m.bias.data_ptr()) for m in modules)


def _nhwc(t, name):
    if not (t.is_cuda and t.dtype == F32 and t.is_contiguous() and t.dim() == 4):
        raise ValueError(f"{name} must be a contiguous fp32 CUDA tensor shaped (B,H,W,C)")
    return t


def conv2d_nhwc(pc: PackedConv, srcs, dst, epilogue: int = EPI_LINEAR, aux0=None, aux1=None, dst2=None, gru_c: int = 0,
                stride: int = 1, tile_stats=None, add_map=None, in_norm=None, src_hl: bool = False, dst_hl: bool = False,
                dst2_hl: bool = False, dst_split=None, tile: int = 0, src_bounded: bool = False, ksplit_ws=None,
                single_product=None):
    """srcs: list of (tensor (B,H,W,C), c_offset) matched with pc.seg_counts; dst/aux0/aux1/dst2: (tensor, c_offset).
    ksplit_ws: a conv_ksplit_workspace() buffer -- lets a launch of few tiles (B = 1 crops) split its K loop over several
    workgroups per tile; launches that may run concurrently (two streams) need separate buffers.
    Writes in place into dst (and dst2); returns nothing.
    src_hl / dst_hl / dst2_hl: the sources / dst / dst2 are SPLIT tensors (fp16 hi|lo per 8-channel group in a buffer of the
    fp32 tensor's shape: include/rnnpose_hip.h; split_hl / unsplit_hl convert); dst_split = (tensor, c_offset): an additional
    split-form copy of the primary result; tile: 0 auto, 1..4 tile shapes of the 128-row kernels, 5 / 6 / 7 the strip kernels with 160- / 32- / 96-row strips
    (160-row strips, operands by LDS-DMA: include/rnnpose_hip.h)."""
    _apply_conv_env()
    d = _lib.ConvDesc()
    if len(srcs) != len(pc.seg_counts):
        raise ValueError("number of sources differs from the packed segment list")
    B, H, W, _ = srcs[0][0].shape
    for i, ((t, off), cnt) in enumerate(zip(srcs, pc.seg_counts)):
        _nhwc(t, f"src{i}")
        if t.shape[:3] != (B, H, W):
            raise ValueError("sources must share (B,H,W)")
        d.src[i] = _lib.ConvSrc(t.data_ptr(), t.shape[3], off, cnt)
    d.n_src = len(srcs)
    d.B, d.H, d.W, d.kh, d.kw, d.stride = B, H, W, pc.kh, pc.kw, stride
    d.w_packed, d.bias = pc.w_packed.data_ptr(), pc.bias.data_ptr()
    d.c_out, d.a_scale, d.w_scale, d.epilogue = pc.c_out, pc.a_scale, pc.w_scale, epilogue

    def put(prefix, spec):
        if spec is None:
            return
        t, off = spec
        _nhwc(t, prefix)
        setattr(d, prefix, t.data_ptr())
        setattr(d, prefix + "_c_stride", t.shape[3])
        setattr(d, prefix + "_c_offset", off)

    put("dst", dst)
    put("aux0", aux0)
    put("aux1", aux1)
    put("dst2", dst2)
    if add_map is not None:          # (tensor (B,H,W,Cs), c_offset): per-pixel bias added before the epilogue
        t, off = add_map
        _nhwc(t, "add_map")
        d.add_map, d.add_c_stride, d.add_c_offset = t.data_ptr(), t.shape[3], off
    d.gru_c = gru_c
    if in_norm is not None:          # (B, C_src, 2) mean / rstd of source 0: read relu((x - mean) * rstd) instead of x
        if not (in_norm.is_cuda and in_norm.dtype == F32 and in_norm.is_contiguous() and tuple(in_norm.shape) == (B, srcs[0][0].shape[3], 2)):
            raise ValueError("in_norm must be a contiguous fp32 CUDA tensor of (B, C_source, 2)")
        d.src0_mean_rstd = in_norm.data_ptr()
    d.src_hl, d.dst_hl, d.dst2_hl, d.tile = int(bool(src_hl)), int(bool(dst_hl)), int(bool(dst2_hl)), int(tile)
    if tile_stats is not None:
        # (B * tiles per image, c_out, 2) fp64 per-tile column sums / sums of squares for instnorm_tiles_nhwc.  The tile count is the one
        # of the kernel THIS launch takes: asked from the library with the descriptor itself (the launch checks it again)
        tpi = int(_lib.load().rnnpose_conv_tiles_per_image_desc(C.byref(d)))
        if not (tile_stats.is_cuda and tile_stats.dtype == F64 and tile_stats.is_contiguous()
                and tile_stats.numel() == B * tpi * pc.c_out * 2):      # exact: the consumer takes the tiling from this shape
            raise ValueError("tile_stats must be a contiguous FP64 CUDA tensor of (B * conv_tiles_per_image(H, W, kh, kw, stride, c_out, tile, B, "
                             f"src_counts, fused_norm) = {B * tpi}, c_out, 2): the tile count depends on the kernel the launch takes")
        d.tile_stats, d.tile_stats_records = tile_stats.data_ptr(), B * tpi
    d.src_bounded = int(bool(src_bounded))      # caller's guarantee that the sources cannot leave the fp16x3 range: no range check
    if dst_split is not None:
        t, off = dst_split
        _nhwc(t, "dst_split")
        d.dst_split, d.dst_split_c_stride, d.dst_split_c_offset = t.data_ptr(), t.shape[3], off
    if ksplit_ws is not None:
        d.ksplit_ws, d.ksplit_ws_bytes = ksplit_ws.data_ptr(), ksplit_ws.numel() * ksplit_ws.element_size()
    d.single_product = int(_single_product if single_product is None else bool(single_product))
    Ho, Wo = -(-H // stride), -(-W // stride)
    # algorithmic bytes of the launch: every input element and weight read once, every output written once, the
    # epilogue's operands (additive map; h of the gate, h and z of the state update) read once -- 4 bytes each
    nb = B * H * W * pc.c_in_real + pc.c_out * pc.c_in_real * pc.kh * pc.kw + B * Ho * Wo * pc.c_out
    nb += B * Ho * Wo * pc.c_out * (add_map is not None) + B * Ho * Wo * (gru_c if epilogue == EPI_GRU_ZR else 0)
    nb += 2 * B * Ho * Wo * pc.c_out * (epilogue == EPI_GRU_Q) + B * Ho * Wo * pc.c_out * (dst_split is not None)
    products = 3
    if d.single_product and _prof is not None:       # (flop accounting only: which launches the library runs single-product)
        products = int(_lib.load().rnnpose_conv_products_desc(C.byref(d)))
    _launch("rnnpose_conv2d_nhwc_f16x3", C.byref(d), _stream(),
            work=2.0 * B * Ho * Wo * pc.c_out * pc.c_in_real * pc.kh * pc.kw, nbytes=4.0 * nb, products=products)


_single_product = False


def single_product(enable=None) -> bool:
    """Process-wide default of conv2d_nhwc's `single_product` for callers that do not pass it (measurement scripts).  The package itself
    never sets it: since r05 the mode is carried by the engines a PoseRefiner configures (engine.UpdateEngine / EncoderEngine
    .single_product) and passed explicitly with every launch.  -> the current value."""
    global _single_product
    if enable is not None:
        _single_product = bool(enable)
    return _single_product


def conv_tiles_per_image(H, W, kh, kw, stride=1, c_out=None, tile: int = 0, batch: int = 1, src_counts=None, fused_norm: bool = False) -> int:
    """Records per image of a convolution's tile_stats = how the launch tiles (rnnpose_conv_tiles_per_image_desc: the rules are in
    include/rnnpose_hip.h).  Without c_out: the 128-row kernels' rule (3x3 stride 1 on 8 x 16 patches, else runs of 128 output pixels);
    with c_out: for the kernel a launch of `batch` images of that width and `tile` request takes.  src_counts (channel counts of the
    sources) and fused_norm (the launch passes in_norm) complete the description; without src_counts one source of 32 channels stands in
    (whole 32-channel blocks, as the strip kernels want them).  Stride 2 with c_out but without src_counts raises ValueError for every
    shape unless `tile` forces a 128-row form (1..4): there the sources decide the kernel family, and no shape-only answer is given."""
    _apply_conv_env()
    if c_out is None:
        c_out, tile = 64, 1                                  # (the forced 128-row form: its tiling does not depend on the width)
    elif src_counts is None and stride == 2 and tile not in (1, 2, 3, 4):
        raise ValueError("conv_tiles_per_image: whether a stride-2 launch takes the strip kernels depends on its sources: pass src_counts")
    d = _lib.ConvDesc()
    for i, c in enumerate(src_counts or [32]):
        d.src[i] = _lib.ConvSrc(None, int(c), 0, int(c))
    d.n_src = len(src_counts or [32])
    d.B, d.H, d.W, d.kh, d.kw, d.stride, d.c_out, d.tile = int(batch), int(H), int(W), int(kh), int(kw), int(stride), int(c_out), int(tile)
    d.src0_mean_rstd = 16 if fused_norm else None        # (only its null-ness is looked at)
    return int(_lib.load().rnnpose_conv_tiles_per_image_desc(C.byref(d)))


_conv_env_applied = False


def _apply_conv_env():
    """RNNPOSE_SPATIAL_TILES=0 restores the row-major tiling of 3x3 layers (same-box A/B)."""
    global _conv_env_applied
    if not _conv_env_applied:
        _conv_env_applied = True
        # same-box A/B switches (what each does: env.py); unset: nothing is called, the library's own default stays
        for name, entry, read in (("RNNPOSE_SPATIAL_TILES", "rnnpose_conv_spatial_tiles", env.flag),
                                  ("RNNPOSE_KSPLIT", "rnnpose_conv_ksplit", env.flag),
                                  ("RNNPOSE_LOOKUP_VARIANT", "rnnpose_corr_lookup_variant", env.flag),
                                  ("RNNPOSE_STRIP", "rnnpose_conv_strip", env.number),
                                  ("RNNPOSE_CORR_VARIANT", "rnnpose_corr_variant", env.number)):
            v = read(name, None)
            if v is not None:
                _lib.call(entry, int(v))
        v = env.text("RNNPOSE_KSPLIT_LIMITS")                 # "max_tiles,max_splits" (measurement)
        if v:
            a, b = (int(t) for t in v.split(","))
            _lib.call("rnnpose_conv_ksplit_limits", a, b)


def conv_spatial_tiles(enable: bool = True):
    _lib.call("rnnpose_conv_spatial_tiles", int(bool(enable)))


def conv_strip(mode=True):
    """Measurement switch (RNNPOSE_STRIP): False / 0 = the automatic tile choice never takes the strip kernels; 2 = not the two-wave
    workgroups of 64-channel layers; 3 = two 32-column tiles per wave; 4 = 160-row strips only (no 32-row strips); 5 = automatic
    without the stride-2 form (stride-2 3x3 layers then run the 128-row kernel's tap-per-staging mode, as until r04); 6 = automatic
    without r06's 32- / 96-row strips for launches of few waves; 7 = automatic WITH persistent launches of the fp32-source strip forms
    (r06, measured slower: off by default)."""
    _apply_conv_env()
    _lib.call("rnnpose_conv_strip", int(mode))


def conv_ksplit(enable: bool = True):
    """Measurement switch: False = launches never split K even when a workspace is passed (RNNPOSE_KSPLIT=0)."""
    _lib.call("rnnpose_conv_ksplit", int(bool(enable)))


def conv_ksplit_workspace(device):
    """Zeroed workspace for conv2d_nhwc(ksplit_ws=...): one per chain of launches that can run concurrently with another."""
    n = int(_lib.load().rnnpose_conv_ksplit_workspace_bytes())
    return torch.zeros((n + 3) // 4, device=device, dtype=torch.int32)


KSPLIT_MAX_PIXELS = 96 * 128      # the library splits launches of at most 96 tiles (rnnpose_conv_ksplit_limits) of 128 output pixels


def ksplit_workspace_in(reg, key, enabled, pixels, device, keep=None):
    """The engines' registry of K-split workspaces: -> reg[key], allocated on first use (i.e. in the eager warm-up runs before a hipGraph
    capture), or None: K-split off, or none of the chain's launches can split (more than KSPLIT_MAX_PIXELS output pixels in its smallest).
    keep(k): which other entries survive a new allocation."""
    if not enabled or pixels > KSPLIT_MAX_PIXELS:
        return None
    if key not in reg:
        for k in [k for k in reg if keep is not None and not keep(k)]:
            del reg[k]
        reg[key] = conv_ksplit_workspace(device)
    return reg[key]


def conv2d_nhwc_new(pc: PackedConv, x, epilogue: int = EPI_LINEAR, stride: int = 1, stats: bool = False, in_norm=None, tile: int = 0, **kw):
    """conv2d_nhwc of the one source x (B,H,W,C) into a fresh tensor -> (out, tile_stats or None).  stats: the epilogue also emits the per-tile
    column statistics the following instance norm needs (saves re-reading the tensor once; output rows are tiled per image for that), sized for
    the kernel this launch takes.  in_norm: mean / rstd of `x`, then a RAW convolution output normalised (+ ReLU) in this convolution's load."""
    B, H, W, _ = x.shape
    out = torch.empty(B, -(-H // stride), -(-W // stride), pc.c_out, device=x.device, dtype=F32)
    ts = None
    if stats:
        tpi = conv_tiles_per_image(H, W, pc.kh, pc.kw, stride, pc.c_out, tile, B, src_counts=pc.seg_counts, fused_norm=in_norm is not None)
        ts = torch.empty(B * tpi, pc.c_out, 2, device=x.device, dtype=F64)
    conv2d_nhwc(pc, [(x, 0)], (out, 0), epilogue, stride=stride, tile_stats=ts, in_norm=in_norm, tile=tile, **kw)
    return out, ts


_nchw_pc = {}


def conv2d_nchw(weight, bias, x, relu: bool = False):
    """NCHW facade of the implicit-GEMM kernel: F.conv2d(x, weight, bias, stride=1, padding=k//2) [+ ReLU] for the odd
    "same" convolutions of the update block (thirdparty/raft/update.py).  Layout transposes on both sides, channel counts
    padded to multiples of 4; packed weights are cached per parameter identity.  The fused NHWC engine does not use this."""
    x = _chk(x, "x")
    B, Cin, H, W = x.shape
    Cout, Cin_w, kh, kw = weight.shape
    if Cin_w != Cin:
        raise ValueError(f"weight expects {Cin_w} input channels, got {Cin}")
    cin_p, cout_p = -(-Cin // 4) * 4, -(-Cout // 4) * 4
    # the entry keeps the parameter tensors alive: a freed module's storage could otherwise be handed to a new parameter of the
    # same shape at the same address and version, and the facade would compute with the previous module's packed weights
    key = (weight.data_ptr(), weight._version, bias.data_ptr(), bias._version, tuple(weight.shape))
    ent = _nchw_pc.get(key)
    pc = ent[0] if (ent is not None and ent[1] is weight and ent[2] is bias) else None
    if pc is None:
        w = _chk(weight.detach(), "weight")
        if cin_p != Cin:
            w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, cin_p - Cin))
        pc = PackedConv(w, bias, [cin_p])
        pc.c_in_real = Cin
        if len(_nchw_pc) >= 64:
            _nchw_pc.pop(next(iter(_nchw_pc)))
        _nchw_pc[key] = (pc, weight, bias)
    xn = (torch.zeros if cin_p != Cin else torch.empty)(B, H, W, cin_p, device=x.device, dtype=F32)
    nchw_to_nhwc(x, xn)
    out = torch.empty(B, H, W, cout_p, device=x.device, dtype=F32)
    conv2d_nhwc(pc, [(xn, 0)], (out, 0), EPI_RELU if relu else EPI_LINEAR)
    return nhwc_to_nchw(out, 0, Cout)


# ---- NHWC companions ------------------------------------------------------------------------------------------
def corr_lookup_nhwc(pyramid_buf, coords, out=None, levels: int = 4, radius: int = 4):
    """coords (B,2,h,w) -> (B,h,w,levels*81)"""
    coords = _chk(coords, "coords")
    B, _, h, w = coords.shape
    if out is None:
        out = torch.empty(B, h, w, levels * (2 * radius + 1) ** 2, device=coords.device, dtype=F32)
    _launch("rnnpose_corr_lookup_nhwc_f32", _ptr(pyramid_buf), _ptr(coords), B, h, w, levels, radius, _ptr(out), _stream(),
            nbytes=_lookup_bytes(B, h, w, levels, radius))
    return out


def corr_lookup_nhwc_part(pyramid_buf, coords, out, B, b0, b1, levels: int = 4, radius: int = 4):
    """NHWC lookup of images [b0, b1) of a batch-B pyramid: coords (b1-b0,2,h,w) and out (b1-b0,h,w,levels*81) are the
    SUB-BATCH tensors."""
    coords = _chk(coords, "coords")
    n, _, h, w = coords.shape
    if n != b1 - b0:
        raise ValueError("coords must hold the b1 - b0 images of the part")
    _launch("rnnpose_corr_lookup_nhwc_part_f32", _ptr(pyramid_buf), _ptr(coords), B, b0, b1, h, w, levels, radius, _ptr(out),
            _stream(), nbytes=_lookup_bytes(b1 - b0, h, w, levels, radius))
    return out


class InducedCoords:
    """Where an iteration's coords1 comes from when its first consumers form it themselves (r06): depth (n,1,H,W), K (n,3,3), G (n,4,4) of
    the chain's images, the low-resolution size, and `out` (n,2,h,w) = the tensor the lookup launch writes the coordinates to (the flow
    head reads them there).  Same values as induced_coords_lowres(depth, K, G, h, w, eps), bit for bit (csrc/induced.cuh)."""

    def __init__(self, depth, K, G, h, w, eps, out):
        self.depth, self.K, self.G = _chk(depth, "depth"), _chk(K, "K"), _chk(G, "G")
        self.h, self.w, self.eps, self.out = int(h), int(w), float(eps), out
        self.H, self.W = int(depth.shape[-2]), int(depth.shape[-1])
        n = depth.shape[0]
        if tuple(K.shape[-2:]) != (3, 3) or tuple(G.shape[-2:]) != (4, 4) or K.reshape(-1, 3, 3).shape[0] != n or G.reshape(-1, 4, 4).shape[0] != n:
            raise ValueError("K (n,3,3) and G (n,4,4) must match depth (n,1,H,W)")
        if tuple(out.shape) != (n, 2, self.h, self.w) or not out.is_contiguous():
            raise ValueError("out must be a contiguous (n,2,h,w) tensor")


def corr_lookup_induced_nhwc_part(pyramid_buf, ic: InducedCoords, out, B, b0, b1, levels: int = 4, radius: int = 4):
    """corr_lookup_nhwc_part with the coordinates formed inside the launch (and written to ic.out)."""
    if ic.depth.shape[0] != b1 - b0:
        raise ValueError("the coordinate source must hold the b1 - b0 images of the part")
    _launch("rnnpose_corr_lookup_induced_nhwc_part_f32", _ptr(pyramid_buf), _ptr(ic.depth), _ptr(ic.K), _ptr(ic.G), ic.H, ic.W, ic.eps, B, b0, b1,
            ic.h, ic.w, levels, radius, _ptr(ic.out), _ptr(out), _stream(), nbytes=_lookup_bytes(b1 - b0, ic.h, ic.w, levels, radius))
    return out


def flow_features_induced(ic: InducedCoords, w_t, bias, out, motion, motion_c_offset, out_c_offset=0, out_split: bool = False,
                          motion_split: bool = False, a_scale: float = 8.0):
    """flow_features with coords1 formed inside the launch (grid subtracted)."""
    B, c_out = ic.depth.shape[0], w_t.shape[1]
    _launch("rnnpose_flow_features_induced_f32", _ptr(ic.depth), _ptr(ic.K), _ptr(ic.G), ic.H, ic.W, ic.eps, _ptr(w_t), _ptr(bias), B, ic.h, ic.w,
            c_out, _ptr(out), out.shape[-1], out_c_offset, _ptr(motion), motion.shape[3], motion_c_offset, int(bool(out_split)),
            int(bool(motion_split)), float(a_scale), _stream(), work=2.0 * 98 * c_out * B * ic.h * ic.w)
    return out


def nchw_to_nhwc(src, dst=None, c_offset: int = 0):
    """src (B,C,H,W) -> channels [c_offset, c_offset+C) of dst (B,H,W,Cs) (allocated (B,H,W,C) if None)."""
    src = _chk(src, "src")
    B, Cc, H, W = src.shape
    if dst is None:
        dst = torch.empty(B, H, W, Cc, device=src.device, dtype=F32)
    _launch("rnnpose_nchw_to_nhwc_f32", _ptr(src), B, Cc, H * W, _ptr(dst), dst.shape[3], c_offset, _stream())
    return dst


def nhwc_to_nchw(src, c_offset: int = 0, c_count: int | None = None, out=None):
    """channels [c_offset, c_offset+c_count) of src (B,H,W,Cs) -> (B,c_count,H,W)"""
    B, H, W, Cs = src.shape
    c_count = Cs - c_offset if c_count is None else c_count
    dst = out if out is not None else torch.empty(B, c_count, H, W, device=src.device, dtype=F32)
    _launch("rnnpose_nhwc_to_nchw_f32", _ptr(src), B, c_count, H * W, Cs, c_offset, _ptr(dst), _stream())
    return dst


def flow_prep(coords1, flow4, motion, motion_c_offset, subtract_grid: bool = True):
    """coords1 (B,2,h,w): absolute coordinates (subtract_grid) or the flow itself -> flow4 (B,h,w,4), motion[..., co:co+2]."""
    B, _, h, w = coords1.shape
    _launch("rnnpose_flow_prep_f32", _ptr(coords1), int(subtract_grid), B, h, w, _ptr(flow4), _ptr(motion), motion.shape[3],
            motion_c_offset, _stream())


def flow_conv7x7_relu(flow4, w_t, bias, out, out_c_offset=0):
    """relu(convf1(flow)) (update.py:84,91): flow4 (B,h,w,4), w_t (98,c_out) -> channels of NHWC `out`."""
    B, h, w, _ = flow4.shape
    c_out = w_t.shape[1]
    _launch("rnnpose_flow_conv7x7_relu_f32", _ptr(flow4), _ptr(w_t), _ptr(bias), B, h, w, c_out, _ptr(out), out.shape[-1],
            out_c_offset, _stream(), work=2.0 * 98 * c_out * B * h * w)
    return out


def flow_features(coords1, w_t, bias, out, motion, motion_c_offset, out_c_offset=0, subtract_grid: bool = True,
                  out_split: bool = False, motion_split: bool = False, a_scale: float = 8.0):
    """flow_prep + flow_conv7x7_relu in one launch: coords1 (B,2,h,w) -> relu(convf1(flow)) into `out` (NHWC), flow into
    motion[..., co:co+2] (update.py:84,91,97).  out_split / motion_split: the destinations are split tensors."""
    B, _, h, w = coords1.shape
    c_out = w_t.shape[1]
    _launch("rnnpose_flow_features_f32", _ptr(coords1), int(subtract_grid), _ptr(w_t), _ptr(bias), B, h, w, c_out, _ptr(out),
            out.shape[-1], out_c_offset, _ptr(motion), motion.shape[3], motion_c_offset, int(bool(out_split)), int(bool(motion_split)),
            float(a_scale), _stream(), work=2.0 * 98 * c_out * B * h * w)
    return out


# ---- split tensors (fp16 hi|lo per 8-channel group; include/rnnpose_hip.h "SPLIT TENSORS") ------------------------------
def split_hl(src, dst=None, src_c_offset: int = 0, c_count: int | None = None, dst_c_offset: int = 0, a_scale: float = 8.0):
    """channels [src_c_offset, +c_count) of the fp32 NHWC tensor `src` -> split form in channels [dst_c_offset, +c_count) of
    `dst` (allocated with c_count channels if None).  The split tensor is an opaque float32-typed buffer of the same shape."""
    _nhwc(src, "src")
    B, H, W, Cs = src.shape
    c_count = Cs - src_c_offset if c_count is None else c_count
    if dst is None:
        dst = torch.empty(B, H, W, c_count, device=src.device, dtype=F32)
    _lib.call("rnnpose_split_hl_f32", _ptr(src), Cs, int(src_c_offset), B * H * W, int(c_count), float(a_scale), _ptr(dst),
              dst.shape[3], int(dst_c_offset), _stream())
    return dst


def unsplit_hl(t, a_scale: float = 8.0):
    """Split tensor (..., C) -> the fp32 values (hi + lo) / a_scale it stands for (torch arithmetic: tests and the NCHW facade)."""
    sh = t.shape
    v = t.contiguous().view(torch.float16).view(*sh[:-1], sh[-1] // 8, 2, 8).float()
    return ((v[..., 0, :] + v[..., 1, :]) / a_scale).reshape(sh)


def flow_head_out(x, x_c_offset, c_in, weight, bias, coords1, delta, coords1_out, flow_lr):
    B, h, w, cs = x.shape
    _launch("rnnpose_flow_head_out_f32", _ptr(x), cs, x_c_offset, c_in, _ptr(weight), _ptr(bias), _ptr(coords1), B, h, w,
            _ptr(delta), _ptr(coords1_out), _ptr(flow_lr), _stream())


def convex_upsample_nhwc(flow_lr, mask, out=None):
    B, h, w, _ = mask.shape
    if out is None:
        out = torch.empty(B, 2, 8 * h, 8 * w, device=mask.device, dtype=F32)
    _launch("rnnpose_convex_upsample_nhwc_f32", _ptr(flow_lr), _ptr(mask), B, h, w, _ptr(out), _stream(),
            nbytes=4.0 * B * h * w * (576 + 2 + 128))
    return out


class PackedConv1x1:
    """Weights of a 1x1 convolution with 256 outputs and <= 352 inputs for the LDS-resident kernel (csrc/conv1x1_resident.hip)."""

    @staticmethod
    def fits(weight) -> bool:
        """Can the LDS-resident kernel run this layer: a (256, c_in <= 352, 1, 1) weight with c_in % 4 == 0."""
        s = tuple(weight.shape)
        return len(s) == 4 and s[0] == 256 and s[2:] == (1, 1) and s[1] % 4 == 0 and s[1] <= 352

    def __init__(self, weight, bias, a_scale: float = A_SCALE):
        import math
        range_guard_arm(weight.device)
        w = _chk(weight.detach(), "weight")
        if not self.fits(w):
            raise ValueError("needs a (256, c_in <= 352, 1, 1) weight with c_in % 4 == 0")
        self.c_in = int(w.shape[1])
        wmax = float(w.abs().max())
        self.w_scale = float(2.0 ** math.floor(math.log2(1024.0 / wmax))) if wmax > 0 else 1.0
        self.a_scale = float(a_scale)
        self.bias = _chk(bias.detach(), "bias").contiguous()
        n = int(_lib.load().rnnpose_conv1x1_resident_packed_bytes(self.c_in))
        self.w_packed = torch.empty(n // 2, device=w.device, dtype=torch.float16)
        _lib.call("rnnpose_conv1x1_resident_pack_f16x3", _ptr(w), 256, self.c_in, self.w_scale, _ptr(self.w_packed), _stream())


def conv1x1_resident(pc: PackedConv1x1, src, dst, relu: bool = True, dst_split: bool = False):
    """src, dst: (tensor (B,h,w,C), c_offset).  dst[..., off:off+256] = act(conv1x1(src[..., off:off+c_in])).
    dst_split: dst is written as a split tensor (for a consuming convolution with src_hl)."""
    x, xo = src
    y, yo = dst
    _nhwc(x, "src"); _nhwc(y, "dst")
    n = x.shape[0] * x.shape[1] * x.shape[2]
    if y.shape[:3] != x.shape[:3]:
        raise ValueError("src and dst must share (B,h,w)")
    _launch("rnnpose_conv1x1_resident_f16x3", _ptr(x), x.shape[3], int(xo), pc.c_in, _ptr(pc.w_packed), _ptr(pc.bias), pc.a_scale,
            pc.w_scale, int(bool(relu)), n, _ptr(y), y.shape[3], int(yo), int(bool(dst_split)), _stream(), work=2.0 * n * 256 * pc.c_in)


def corr_lookup_convc1(pc: PackedConv1x1, pyramid_buf, coords, dst, B_total, b0, b1, levels=4, radius=4, relu: bool = True,
                       dst_split: bool = False):
    """r06: window lookup + convc1 in one launch (model/CFNet.py:147-152): dst[..., off:off+256] = act(convc1(corr_fn(coords))) for the
    images [b0, b1) of a pyramid built for B_total images; coords (b1-b0,2,h,w); dst = (tensor (b1-b0,h,w,C), c_offset).  The
    (B,h,w,324) window-feature tensor is never materialised (csrc/corr_convc1.hip).  Not faster than the two kernels (engine.py): an option."""
    y, yo = dst
    _nhwc(y, "dst")
    coords = _chk(coords, "coords")
    nb, two, h, w = coords.shape
    if pc.c_in != 324 or two != 2 or nb != b1 - b0 or tuple(y.shape[:3]) != (nb, h, w):
        raise ValueError("corr_lookup_convc1: weights packed for c_in = 324, coords (b1-b0,2,h,w), dst (b1-b0,h,w,C)")
    n = nb * h * w
    _launch("rnnpose_corr_lookup_convc1_f16x3", _ptr(pyramid_buf), _ptr(coords), int(B_total), int(b0), int(b1), h, w, int(levels), int(radius),
            _ptr(pc.w_packed), _ptr(pc.bias), pc.a_scale, pc.w_scale, int(bool(relu)), _ptr(y), y.shape[3], int(yo), int(bool(dst_split)),
            _stream(), work=2.0 * n * 256 * 324, nbytes=4.0 * n * (levels * 100 + 2 + 256))


class PackedMaskHead:
    """mask.2 weights (576,256,1,1) + bias, post-scaled (the 0.25 of update.py:187) and split into fp16 hi/lo MFMA fragments
    for the fused mask + up-sampling kernel (csrc/mask_upsample.hip)."""

    def __init__(self, weight, bias, post_scale: float = 0.25, a_scale: float = A_SCALE):
        import math
        range_guard_arm(weight.device)
        w = _chk(weight.detach(), "weight")
        if tuple(w.shape) != (576, 256, 1, 1):
            raise ValueError("mask.2 weight must be (576,256,1,1)")
        wmax = float(w.abs().max()) * post_scale
        self.w_scale = float(2.0 ** math.floor(math.log2(1024.0 / wmax))) if wmax > 0 else 1.0
        self.a_scale = float(a_scale)
        self.bias = (_chk(bias.detach(), "bias") * post_scale).contiguous()
        n = int(_lib.load().rnnpose_mask_upsample_packed_bytes())
        self.w_packed = torch.empty(n // 2, device=w.device, dtype=torch.float16)
        _lib.call("rnnpose_mask_upsample_pack_f16x3", _ptr(w), float(post_scale), self.w_scale, _ptr(self.w_packed), _stream())


def mask_upsample(pm: PackedMaskHead, x, x_c_offset, flow_lr, out=None):
    """mask.2 + convex 8x up-sampling in one kernel (update.py:183-187, CFNet.py:95-106).  x (B,h,w,C) with relu(mask.0(h))
    in channels [x_c_offset, +256); flow_lr (B,h,w,2) -> (B,2,8h,8w).  Agrees with the 1x1 convolution + convex_upsample_nhwc
    to fp32 round-off (online softmax); the mask tensor is never materialised."""
    _nhwc(x, "x")
    B, h, w, cs = x.shape
    if out is None:
        out = torch.empty(B, 2, 8 * h, 8 * w, device=x.device, dtype=F32)
    _launch("rnnpose_mask_upsample_f16x3", _ptr(x), cs, int(x_c_offset), _ptr(pm.w_packed), 576, _ptr(pm.bias), pm.a_scale,
            pm.w_scale, _ptr(_chk(flow_lr, "flow_lr")), B, h, w, _ptr(out), _stream(), work=2.0 * B * h * w * 576 * 256,
            nbytes=4.0 * B * h * w * (256 + 2 + 128))
    return out


# ---- fp16x3 range guard ------------------------------------------------------------------------------------------------
# ON BY DEFAULT (round 3): every kernel that splits fp32 values into fp16 hi|lo counts the quads it had to clamp in a sticky
# device counter; PoseRefiner.forward returns the counter as a device tensor ("f16x3_range_events"), so a silent clamp --
# something the fp32 reference cannot do -- is visible in the public output without a host synchronisation.
# RNNPOSE_RANGE_GUARD=0 switches it off (measurement only).
_guard_env = env.flag("RNNPOSE_RANGE_GUARD", True)
_guard_on = False
_guard_devices = set()


def range_guard_arm(device=None):
    """Allocate the current device's counter and switch counting on (idempotent; never called under stream capture: the
    Packed* constructors and PoseRefiner.forward call it before any launch)."""
    global _guard_on
    if not _guard_env:
        return
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    if dev in _guard_devices and _guard_on:
        return
    with torch.cuda.device(dev):
        _lib.call("rnnpose_f16x3_saturation_check", 1)
    _guard_devices.add(dev)
    _guard_on = True


def range_guard_state() -> bool:
    """Part of every captured graph's key: the counter pointer is baked into the captured launches."""
    return _guard_on


def saturation_check(enable: bool = True):
    """Switch the fp16x3 range guard on/off (process-global): with it on, every fp16x3 kernel counts the activation quads
    whose scaled magnitude left the fp16 range (|x * a_scale| > 65504) -- values the fp32 reference would handle."""
    global _guard_on
    _lib.call("rnnpose_f16x3_saturation_check", int(bool(enable)))
    _guard_on = bool(enable)
    if enable:
        _guard_devices.add(torch.cuda.current_device())


def saturation_events(out=None):
    """-> device tensor (1,) int64 holding the sticky counter NOW in stream order; no host synchronisation."""
    if out is None:
        out = torch.zeros(1, device="cuda", dtype=torch.int64)
    _lib.call("rnnpose_f16x3_saturation_peek", _ptr(out), _stream())
    return out


def saturation_count(reset: bool = True) -> int:
    """Clamped / non-finite quads seen since the last reset (synchronises the current stream)."""
    n = C.c_ulonglong(0)
    _lib.call("rnnpose_f16x3_saturation_count", C.byref(n), int(bool(reset)), _stream())
    return int(n.value)


# ---- f1: encoder stem ---------------------------------------------------------------------------------------------------
class PackedStem:
    """conv1 of the RAFT encoder (64,3,7,7) split into fp16 hi/lo MFMA fragments for csrc/stem.hip."""

    def __init__(self, weight, bias, a_scale: float = 8.0):
        import math
        range_guard_arm(weight.device)
        w = _chk(weight.detach(), "weight")
        if tuple(w.shape) != (64, 3, 7, 7):
            raise ValueError("the stem kernel is the RAFT encoder's conv1: weight must be (64,3,7,7)")
        wmax = float(w.abs().max())
        self.w_scale = float(2.0 ** math.floor(math.log2(1024.0 / wmax))) if wmax > 0 else 1.0
        self.a_scale = float(a_scale)
        n = int(_lib.load().rnnpose_stem_packed_halfs())
        self.w_hi = torch.empty(n, device=w.device, dtype=torch.float16)
        self.w_lo = torch.empty(n, device=w.device, dtype=torch.float16)
        self.bias = _chk(bias.detach(), "bias")
        _lib.call("rnnpose_stem_pack_weights_f16x3", _ptr(w), self.w_scale, _ptr(self.w_hi), _ptr(self.w_lo), _stream())


def stem_conv(ps: PackedStem, img, normalize: bool = True):
    """img (N,3,H,W) NCHW -> (out (N,ceil(H/2),ceil(W/2),64) NHWC, tile_stats or None)
    = conv7x7 stride 2 pad 3 of (2*(img/255)-1 if normalize else img) + bias   (model/CFNet.py:42-43, extractor.py:131,197)."""
    img = _chk(img, "image")
    N, Cc, H, W = img.shape
    if Cc != 3:
        raise ValueError("image must have 3 channels")
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    tiles, exact = C.c_int(0), C.c_int(0)
    _lib.call("rnnpose_stem_tiles", H, W, C.byref(tiles), C.byref(exact))
    out = torch.empty(N, Ho, Wo, 64, device=img.device, dtype=F32)
    ts = torch.empty(N * tiles.value, 64, 2, device=img.device, dtype=F64) if exact.value else None      # fp64 sums (cancellation in E[x^2] - mean^2)
    _launch("rnnpose_stem_conv7x7_s2_f16x3", _ptr(img), N, H, W, int(bool(normalize)), _ptr(ps.w_hi), _ptr(ps.w_lo),
            _ptr(ps.bias), ps.a_scale, ps.w_scale, _ptr(out), _ptr(ts), _stream(), work=2.0 * N * Ho * Wo * 64 * 147)
    return out, ts


# ---- f1: instance norm on NHWC --------------------------------------------------------------------------------
_in_ws = {}


def instnorm_nhwc(x, relu=True, residual=None, out=None, eps: float = 1e-5):
    """x (B,H,W,C) -> act((x-mean)*rstd) [then relu(residual + .)], nn.InstanceNorm2d semantics (no affine)."""
    _nhwc(x, "x")
    B, H, W, Cc = x.shape
    n = int(_lib.load().rnnpose_instnorm_workspace_bytes(B, H * W, Cc))
    key = (x.device, n, torch.cuda.current_stream().cuda_stream)     # (calls on different streams may run concurrently)
    ws = _in_ws.get(key)
    if ws is None:
        ws = _in_ws[key] = torch.empty(n // 8, device=x.device, dtype=F64)
    if out is None:
        out = torch.empty_like(x)
    stats = torch.empty(B, Cc, 2, device=x.device, dtype=F32)
    _launch("rnnpose_instnorm_nhwc_f32", _ptr(x), B, H * W, Cc, eps, int(bool(relu)), _ptr(residual), _ptr(ws), n,
            _ptr(stats), _ptr(out), _stream(), nbytes=4.0 * x.numel() * (3 + (residual is not None)))
    return out


def instnorm_tiles_nhwc(x, tile_stats, relu=True, residual=None, out=None, eps: float = 1e-5, stats_only: bool = False,
                        residual_norm=None, residual_relu: bool = False):
    """instnorm_nhwc with the statistics pass replaced by the producing convolution's tile_stats (B * ceil(HW/128) records).
    stats_only: -> mean_rstd (B,C,2) only (for a consumer that normalises in its load: conv2d_nhwc(in_norm=...)).
    residual_norm (B,C,2): the residual is a RAW convolution output, normalised [+ ReLU] on the fly with these statistics."""
    _nhwc(x, "x")
    B, H, W, Cc = x.shape
    tpi = tile_stats.shape[0] // B              # records per image, as the producing convolution tiled it
    stats = torch.empty(B, Cc, 2, device=x.device, dtype=F32)
    if stats_only:
        _launch("rnnpose_instnorm_tiles_nhwc_f32", _ptr(None), B, H * W, Cc, eps, int(bool(relu)), _ptr(None), _ptr(None), 0,
                _ptr(tile_stats), tpi, _ptr(stats), _ptr(None), _stream())
        return stats
    if out is None:
        out = torch.empty_like(x)
    _launch("rnnpose_instnorm_tiles_nhwc_f32", _ptr(x), B, H * W, Cc, eps, int(bool(relu)), _ptr(residual), _ptr(residual_norm),
            int(bool(residual_relu)), _ptr(tile_stats), tpi, _ptr(stats), _ptr(out), _stream(),
            nbytes=4.0 * x.numel() * (2 + (residual is not None)))
    return out


# ---- SuperPoint2D glue (model/descriptor2D.py; rnnpose_amd/descriptor2d.py) --------------------------------------------
def _window(t, c_offset, c_count, name):
    _nhwc(t, name)
    Cs = t.shape[3]
    c_count = Cs - c_offset if c_count is None else int(c_count)
    if not (c_count > 0 and c_offset >= 0 and c_offset + c_count <= Cs):
        raise ValueError(f"{name}: channel window [{c_offset}, {c_offset}+{c_count}) outside its {Cs} channels")
    return c_count


def _mean_rstd(mr, B, Cc):
    if mr is None:
        return None
    if not (mr.is_cuda and mr.dtype == F32 and mr.is_contiguous() and tuple(mr.shape) == (B, Cc, 2)):
        raise ValueError(f"mean_rstd must be a contiguous fp32 CUDA tensor of (B, C, 2) = ({B}, {Cc}, 2)")
    return mr


def maxpool2x2_nhwc(src, dst=None, src_c_offset: int = 0, c_count: int | None = None, dst_c_offset: int = 0):
    """nn.MaxPool2d(2, 2) (floor) of channels [src_c_offset, +c_count) of src (B,H,W,Cs) -> channels [dst_c_offset, +c_count) of
    dst (B,H//2,W//2,Cd) (allocated (B,H//2,W//2,c_count) if None)."""
    c_count = _window(src, src_c_offset, c_count, "src")
    B, H, W, _ = src.shape
    if dst is None:
        dst = torch.empty(B, H // 2, W // 2, c_count, device=src.device, dtype=F32)
    _window(dst, dst_c_offset, c_count, "dst")
    if tuple(dst.shape[:3]) != (B, H // 2, W // 2):
        raise ValueError("dst must be (B, H//2, W//2, C)")
    n_out = B * (H // 2) * (W // 2) * c_count
    _launch("rnnpose_maxpool2x2_nhwc_f32", _ptr(src), B, H, W, src.shape[3], src_c_offset, c_count, _ptr(dst), dst.shape[3],
            dst_c_offset, _stream(), work=3.0 * n_out, nbytes=4.0 * 5 * n_out)
    return dst


def upsample2x_nhwc(src, dst=None, src_c_offset: int = 0, c_count: int | None = None, dst_c_offset: int = 0, mean_rstd=None,
                    relu: bool = False):
    """nn.Upsample(scale_factor=2, mode='bilinear') (align_corners=False) of channels [src_c_offset, +c_count) of src (B,h,w,Cs)
    -> channels [dst_c_offset, +c_count) of dst (B,2h,2w,Cd) (allocated (B,2h,2w,c_count) if None).
    mean_rstd (B, c_count, 2) (instnorm_tiles_nhwc(..., stats_only=True) of the window): taps are read as (x - mean) * rstd
    [then ReLU]: up(relu(IN(x))) without materialising the norm.  Per channel, so up(cat(a, b)) = cat(up(a), up(b))."""
    c_count = _window(src, src_c_offset, c_count, "src")
    B, h, w, _ = src.shape
    if dst is None:
        dst = torch.empty(B, 2 * h, 2 * w, c_count, device=src.device, dtype=F32)
    _window(dst, dst_c_offset, c_count, "dst")
    if tuple(dst.shape[:3]) != (B, 2 * h, 2 * w):
        raise ValueError("dst must be (B, 2h, 2w, C)")
    mr = _mean_rstd(mean_rstd, B, c_count)
    n_out = B * 4 * h * w * c_count
    _launch("rnnpose_upsample2x_bilinear_nhwc_f32", _ptr(src), B, h, w, src.shape[3], src_c_offset, c_count, _ptr(mr), int(bool(relu)),
            _ptr(dst), dst.shape[3], dst_c_offset, _stream(), work=(6.0 + 12.0 * (mr is not None)) * n_out,
            nbytes=4.0 * (n_out + B * h * w * c_count))
    return dst


PH_LINEAR, PH_L2, PH_SIGMOID = 0, 1, 2


def pixel_head_nhwc(src, weight, bias, mode: int = PH_LINEAR, src_c_offset: int = 0, c_in: int | None = None, mean_rstd=None,
                    relu: bool = False, out=None):
    """1x1 convolution of channels [src_c_offset, +c_in) of src (B,H,W,Cs) (c_in <= 256) with weight (c_out, c_in[,1,1]) (c_out
    <= 32) + bias -> out (B,c_out,H,W) NCHW.  The source is read as relu?((x - mean) * rstd) with mean_rstd (B,c_in,2), relu(x)
    with relu alone.  mode: PH_LINEAR, PH_L2 (F.normalize over the outputs, eps 1e-12), PH_SIGMOID."""
    c_in = _window(src, src_c_offset, c_in, "src")
    B, H, W, _ = src.shape
    w = _chk(weight.detach(), "weight")
    w = w.reshape(w.shape[0], -1)
    b = _chk(bias.detach(), "bias")
    c_out = w.shape[0]
    if w.shape[1] != c_in or tuple(b.shape) != (c_out,):
        raise ValueError(f"weight must be (c_out, {c_in}) and bias (c_out,)")
    if int(mode) not in (PH_LINEAR, PH_L2, PH_SIGMOID):
        raise ValueError("mode must be PH_LINEAR, PH_L2 or PH_SIGMOID")
    mr = _mean_rstd(mean_rstd, B, c_in)
    if out is None:
        out = torch.empty(B, c_out, H, W, device=src.device, dtype=F32)
    if not (out.is_cuda and out.dtype == F32 and out.is_contiguous() and tuple(out.shape) == (B, c_out, H, W)):
        raise ValueError(f"out must be a contiguous fp32 CUDA tensor of ({B}, {c_out}, {H}, {W})")
    npx = B * H * W
    _launch("rnnpose_pixel_head_nhwc_f32", _ptr(src), B, H * W, src.shape[3], src_c_offset, c_in, _ptr(mr), int(bool(relu)), _ptr(w),
            _ptr(b), c_out, int(mode), _ptr(out), _stream(), work=2.0 * npx * c_in * c_out,
            nbytes=4.0 * (npx * (c_in + c_out) + c_out * (c_in + 1)))
    return out


# ---- KPSuperpoint3Dv2 (model/descriptor3D.py, thirdparty/kpconv; rnnpose_amd/descriptor3d.py) ---------------------------------
def _rows(t, name, cols=None):
    """A (N, C) fp32 CUDA matrix whose rows may be strided (a channel slice of a wider buffer): returns its row stride."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == F32 and t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1)):
        raise ValueError(f"{name} must be a 2-D fp32 CUDA tensor with unit column stride")
    if cols is not None and t.shape[1] != cols:
        raise ValueError(f"{name} must have {cols} columns, got {t.shape[1]}")
    if t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError(f"{name} is empty")
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


def _points(p, name):
    if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == F32 and p.is_contiguous() and p.dim() == 2 and p.shape[1] == 3):
        raise ValueError(f"{name} must be a contiguous (N, 3) fp32 CUDA tensor")
    return p


def neighbor_table(idx, n_s, name="neighbors"):
    """int32 contiguous copy of an (n_q, width) neighbour table (int32 or int64) after checking every value is in 0..n_s
    (n_s = the shadow neighbour)."""
    if not (isinstance(idx, torch.Tensor) and idx.dim() == 2 and idx.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"{name} must be a 2-D int32 or int64 tensor")
    if idx.shape[0] == 0 or idx.shape[1] == 0:
        raise ValueError(f"{name} is empty")
    if not idx.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {idx.device}); rnnpose_amd has no CPU path")
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi > n_s:
        raise ValueError(f"{name}: indices must lie in 0..{n_s} ({n_s} = the shadow neighbour), got {lo}..{hi}")
    return idx.to(torch.int32).contiguous()


def point_row_sum(x, out=None):
    """out[i] = sum_c x[i, c] (fp32): the positive-sum test of KPConv's neighbour count (kpconv_blocks.py:366-369)."""
    ld = _rows(x, "x")
    n, c = x.shape
    if out is None:
        out = torch.empty(n, device=x.device, dtype=F32)
    _launch("rnnpose_point_row_sum_f32", _ptr(x), n, c, ld, _ptr(out), _stream(), work=n * c, nbytes=4.0 * n * (c + 1))
    return out


def kpconv_aggregate(q_pts, s_pts, neighbors, kernel_points, extent: float, x, row_sum=None, out=None):
    """KPConv.forward (kpconv_blocks.py:300-372: linear influence, sum aggregation) up to the weight product:
    (n_q, K * c_in) with column k * c_in + c = sum_j infl_kj x[j, c] / max(1, #{j : sum_c x[j, c] > 0}).
    neighbors: an int32 table from neighbor_table (values 0..n_s); x (n_s, c_in) rows may be strided."""
    _points(q_pts, "q_pts")
    _points(s_pts, "s_pts")
    ld = _rows(x, "x")
    n_s, c_in = x.shape
    if s_pts.shape[0] != n_s:
        raise ValueError(f"x has {n_s} rows for {s_pts.shape[0]} support points")
    if not (neighbors.dtype == torch.int32 and neighbors.is_contiguous() and neighbors.dim() == 2 and neighbors.shape[0] == q_pts.shape[0]):
        raise ValueError("neighbors must be a contiguous int32 (n_q, width) table (ops.neighbor_table)")
    kp = _chk(kernel_points.detach(), "kernel_points")
    K = kp.shape[0]
    if tuple(kp.shape) != (K, 3):
        raise ValueError("kernel_points must be (K, 3)")
    n_q, width = neighbors.shape
    if row_sum is None:
        row_sum = point_row_sum(x)
    if out is None:
        out = torch.empty(n_q, K * c_in, device=x.device, dtype=F32)
    if not (out.is_contiguous() and tuple(out.shape) == (n_q, K * c_in) and out.dtype == F32):
        raise ValueError(f"out must be a contiguous fp32 ({n_q}, {K * c_in}) tensor")
    _launch("rnnpose_kpconv_aggregate_f32", _ptr(q_pts), n_q, _ptr(s_pts), n_s, _ptr(neighbors), width, _ptr(kp), K, float(extent),
            _ptr(x), c_in, ld, _ptr(row_sum), _ptr(out), _stream(), work=2.0 * n_q * width * K * (c_in + 6),
            nbytes=4.0 * n_q * (width * (c_in + 5) + K * c_in))
    return out


def point_linear(a, w, bias=None, out=None):
    """out (n, m) = a (n, k) @ w (k, m) (+ bias (m,)): fp32 FMA in k order.  a's and out's rows may be strided (channel slices)."""
    lda = _rows(a, "a")
    n, k = a.shape
    wt = _chk(w.detach(), "w")
    if wt.dim() != 2 or wt.shape[0] != k:
        raise ValueError(f"w must be ({k}, m), got {tuple(wt.shape)}")
    m = wt.shape[1]
    b = None
    if bias is not None:
        b = _chk(bias.detach(), "bias")
        if tuple(b.shape) != (m,):
            raise ValueError(f"bias must be ({m},)")
    if out is None:
        out = torch.empty(n, m, device=a.device, dtype=F32)
    ldo = _rows(out, "out", m)
    if out.shape[0] != n:
        raise ValueError(f"out must have {n} rows")
    _launch("rnnpose_point_linear_f32", _ptr(a), n, k, lda, _ptr(wt), m, _ptr(b), _ptr(out), ldo, _stream(), work=2.0 * n * k * m,
            nbytes=4.0 * (n * (k + m) + k * m))
    return out


def point_norm_stats(x, eps: float = 1e-5):
    """InstanceNorm1d statistics over ALL rows of x (n, c) (BatchNormBlock, kpconv_blocks.py:456-473): (c, 2) fp32 (mean, rstd)."""
    ld = _rows(x, "x")
    n, c = x.shape
    nb = int(_lib.load().rnnpose_point_norm_workspace_bytes(n, c))
    ws = torch.empty(max(1, nb // 8), device=x.device, dtype=F64)
    mr = torch.empty(c, 2, device=x.device, dtype=F32)
    _launch("rnnpose_point_norm_stats_f32", _ptr(x), n, c, ld, float(eps), _ptr(ws), nb, _ptr(mr), _stream(), work=3.0 * n * c,
            nbytes=4.0 * n * c)
    return mr


def point_norm_apply(x, mean_rstd, leaky: bool = True, res=None, res_mean_rstd=None, slope: float = 0.1, out=None):
    """out = (x - mean) * rstd [+ res (normalised by res_mean_rstd if given)] [LeakyReLU(slope)]; out may be x or a channel slice."""
    ld = _rows(x, "x")
    n, c = x.shape
    mr = _chk(mean_rstd, "mean_rstd")
    if tuple(mr.shape) != (c, 2):
        raise ValueError(f"mean_rstd must be ({c}, 2)")
    ldr, rmr = 0, None
    if res is not None:
        ldr = _rows(res, "res", c)
        if res.shape[0] != n:
            raise ValueError(f"res must have {n} rows")
        if res_mean_rstd is not None:
            rmr = _chk(res_mean_rstd, "res_mean_rstd")
            if tuple(rmr.shape) != (c, 2):
                raise ValueError(f"res_mean_rstd must be ({c}, 2)")
    elif res_mean_rstd is not None:
        raise ValueError("res_mean_rstd without res")
    if out is None:
        out = torch.empty(n, c, device=x.device, dtype=F32)
    ldo = _rows(out, "out", c)
    if out.shape[0] != n:
        raise ValueError(f"out must have {n} rows")
    _launch("rnnpose_point_norm_apply_f32", _ptr(x), n, c, ld, _ptr(mr), _ptr(res), ldr, _ptr(rmr), int(bool(leaky)), float(slope),
            _ptr(out), ldo, _stream(), work=4.0 * n * c, nbytes=4.0 * n * c * (2 + (res is not None)))
    return out


def point_maxpool(x, idx, out=None):
    """max_pool (kpconv_blocks.py:88-104): out[q] = max over idx[q, :] of the rows of x, the shadow index (n_s) a zero row."""
    ld = _rows(x, "x")
    n_s, c = x.shape
    if not (idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 2):
        raise ValueError("idx must be a contiguous int32 table (ops.neighbor_table)")
    n_q, width = idx.shape
    if out is None:
        out = torch.empty(n_q, c, device=x.device, dtype=F32)
    ldo = _rows(out, "out", c)
    if out.shape[0] != n_q:
        raise ValueError(f"out must have {n_q} rows")
    _launch("rnnpose_point_maxpool_f32", _ptr(x), n_s, c, ld, _ptr(idx), n_q, width, _ptr(out), ldo, _stream(), work=n_q * width * c,
            nbytes=4.0 * n_q * c * (width + 1))
    return out


def point_gather_rows(x, idx, out=None):
    """closest_pool (kpconv_blocks.py:73-85): out[q] = x[idx[q, 0]], zeros for the shadow index (n_s)."""
    ld = _rows(x, "x")
    n_s, c = x.shape
    if not (idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 2):
        raise ValueError("idx must be a contiguous int32 table (ops.neighbor_table)")
    n_q = idx.shape[0]
    if out is None:
        out = torch.empty(n_q, c, device=x.device, dtype=F32)
    ldo = _rows(out, "out", c)
    if out.shape[0] != n_q:
        raise ValueError(f"out must have {n_q} rows")
    _launch("rnnpose_point_gather_rows_f32", _ptr(x), n_s, c, ld, _ptr(idx), n_q, idx.shape[1], _ptr(out), ldo, _stream(),
            work=n_q * c, nbytes=8.0 * n_q * c)
    return out


def point_l2_normalize(x, out=None):
    """F.normalize(x, p=2, dim=1, eps=1e-12) row by row (model/descriptor3D.py:134-136); out may be x."""
    ld = _rows(x, "x")
    n, c = x.shape
    if out is None:
        out = torch.empty(n, c, device=x.device, dtype=F32)
    ldo = _rows(out, "out", c)
    if out.shape[0] != n:
        raise ValueError(f"out must have {n} rows")
    _launch("rnnpose_point_l2_normalize_f32", _ptr(x), n, c, ld, _ptr(out), ldo, _stream(), work=3.0 * n * c, nbytes=8.0 * n * c)
    return out


def grid_voxel_keys(points, origin, dl, nx: int, ny: int):
    """Voxel keys of grid_subsampling.cpp:50-56: ix + nx iy + nx ny iz, ix = floor((p.x - origin.x) / dl) in fp32 (correctly
    rounded division), for (N, 3) points of one cloud -> int64 (N,).  origin: 3 floats (fp32 values), dl: fp32 value."""
    _points(points, "points")
    n = points.shape[0]
    keys = torch.empty(n, device=points.device, dtype=torch.int64)
    if n == 0:
        return keys
    ox, oy, oz = (float(v) for v in origin)
    _launch("rnnpose_grid_voxel_keys_f32", _ptr(points), n, ox, oy, oz, float(dl), int(nx), int(ny), _ptr(keys), _stream(), work=9.0 * n,
            nbytes=20.0 * n)
    return keys


def _starts(lengths, n, dev, name):
    ln = [int(v) for v in lengths]
    if any(v < 0 for v in ln) or sum(ln) != n:
        raise ValueError(f"{name} must be non-negative and sum to {n}, got {ln}")
    st = [0]
    for v in ln:
        st.append(st[-1] + v)
    return torch.tensor(st, device=dev, dtype=torch.int32)


def radius_neighbors(queries, supports, q_lengths, s_lengths, radius: float, limit=None):
    """batch_neighbors_kpconv (data/preprocess.py:544-561 on cpp_neighbors/neighbors/neighbors.cpp:229-330): for each query, the
    supports of ITS cloud (stacked lengths) with ((dx^2 + dy^2) + dz^2) < radius^2 in fp32, sorted by (d2, index); the table is
    min(limit, largest count) wide (limit None or <= 0: no truncation) and padded with len(supports).  -> int64 (n_q, width)."""
    _points(queries, "queries")
    _points(supports, "supports")
    n_q, n_s = queries.shape[0], supports.shape[0]
    if len(q_lengths) != len(s_lengths):
        raise ValueError("q_lengths and s_lengths must have one entry per cloud")
    dev = queries.device
    qs, ss = _starts(q_lengths, n_q, dev, "q_lengths"), _starts(s_lengths, n_s, dev, "s_lengths")
    B = len(q_lengths)
    if n_q == 0:
        return torch.zeros(0, 1, device=dev, dtype=torch.int64)
    counts = torch.empty(n_q, device=dev, dtype=torch.int32)
    if n_s == 0:
        counts.zero_()
    else:
        _launch("rnnpose_radius_count_f32", _ptr(queries), n_q, _ptr(supports), _ptr(qs), _ptr(ss), B, float(radius), _ptr(counts),
                _stream(), work=9.0 * n_q * n_s / B, nbytes=12.0 * (n_q + n_s))
    max_count = int(counts.max())
    width = max_count if (limit is None or limit <= 0) else min(int(limit), max_count)
    out = torch.full((n_q, max(width, 1)), n_s, device=dev, dtype=torch.int32)
    if width == 0:
        return out[:, :0].long()
    offsets = torch.zeros(n_q, device=dev, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts.long(), 0)[:-1]
    total = int(offsets[-1]) + int(counts[-1])
    cand_idx = torch.empty(total, device=dev, dtype=torch.int32)
    cand_d2 = torch.empty(total, device=dev, dtype=F32)
    _launch("rnnpose_radius_neighbors_f32", _ptr(queries), n_q, _ptr(supports), _ptr(qs), _ptr(ss), B, float(radius), _ptr(offsets),
            _ptr(cand_idx), _ptr(cand_d2), width, _ptr(out), _stream(), work=9.0 * n_q * n_s / B, nbytes=12.0 * (n_q + n_s) + 8.0 * total)
    return out.long()


# ---- f2/f3: evaluator metrics ------------------------------------------------------------------------------------
def nn_search(ref_pts, que_pts, exclude_self: bool = False):
    """ref (B,N1,D), que (B,N2,D) fp32 on the GPU, D in {2,3} -> idx (B,N2) int32: first nearest reference point.
    Shapes are checked here (ValueError); nothing is launched then."""
    ref_pts, que_pts = _chk(ref_pts, "ref_pts"), _chk(que_pts, "que_pts")
    if ref_pts.dim() != 3 or ref_pts.shape[2] not in (2, 3) or ref_pts.shape[0] < 1 or ref_pts.shape[1] < 1:
        raise ValueError(f"nn_search: ref_pts must be (B,N1,D) with B, N1 >= 1 and D in (2, 3), got {tuple(ref_pts.shape)}")
    B, n1, dim = ref_pts.shape
    if que_pts.dim() != 3 or que_pts.shape[0] != B or que_pts.shape[2] != dim or que_pts.shape[1] < 1:
        raise ValueError(f"nn_search: que_pts must be ({B},N2,{dim}) with N2 >= 1, as ref_pts {tuple(ref_pts.shape)}, got {tuple(que_pts.shape)}")
    n2 = que_pts.shape[1]
    idx = torch.empty(B, n2, device=ref_pts.device, dtype=torch.int32)
    _launch("rnnpose_nn_search_f32", _ptr(ref_pts), _ptr(que_pts), _ptr(idx), B, n1, n2, dim, int(exclude_self), _stream())
    return idx


def pose_metrics(model, pose_pred, pose_gt, K, symmetric: bool = False):
    """model (P,3), pose_pred/pose_gt (B,3,4), K (3,3) -> (B,5) fp64 [ADD, ADD-S (-1 if not symmetric), proj2d px,
    translation cm, rotation deg]   (utils/eval_metric.py:102-192).  Shapes are checked here (ValueError); nothing is launched then."""
    model, pose_pred, pose_gt, K = _chk(model, "model"), _chk(pose_pred, "pose_pred"), _chk(pose_gt, "pose_gt"), _chk(K, "K")
    if model.dim() != 2 or model.shape[1] != 3 or model.shape[0] < 1:
        raise ValueError(f"pose_metrics: model must be (P,3) with P >= 1, got {tuple(model.shape)}")
    if pose_pred.dim() != 3 or pose_pred.shape[1:] != (3, 4) or pose_pred.shape[0] < 1:
        raise ValueError(f"pose_metrics: pose_pred must be (B,3,4) with B >= 1, got {tuple(pose_pred.shape)}")
    if pose_gt.shape != pose_pred.shape:
        raise ValueError(f"pose_metrics: pose_gt must be {tuple(pose_pred.shape)}, as pose_pred, got {tuple(pose_gt.shape)}")
    if K.shape != (3, 3):
        raise ValueError(f"pose_metrics: K must be (3,3), got {tuple(K.shape)}")
    P, B = model.shape[0], pose_pred.shape[0]
    n = int(_lib.load().rnnpose_pose_metrics_workspace_bytes(B, P)) if symmetric else 0
    ws = torch.empty(max(n, 4) // 4, device=model.device, dtype=F32)
    out = torch.empty(B, 5, device=model.device, dtype=F64)
    _launch("rnnpose_pose_metrics_f64", _ptr(model), P, _ptr(pose_pred), _ptr(pose_gt), _ptr(K), B, int(symmetric),
            _ptr(ws), n, _ptr(out), _stream())
    return out


# ---- BOP pose-error functions (MSSD / MSPD / VSD; definitions in include/rnnpose_hip.h) ----------------------------------
BOP_MAX_TAUS = 16


def bop_sym_dist(model, sym, pose_est, pose_gt, K):
    """model (P,3), sym (S,3,4) symmetry transformations (S >= 1; the identity for an object without symmetries), pose_est /
    pose_gt (B,3,4), K (3,3) or (B,3,3) -> (B,2) fp64 [MSSD, MSPD px]: min over the symmetries of the max over the model points
    of the 3-D distance / of the distance of the projections (rnnpose_bop_sym_dist_f64).  Shapes are checked here (ValueError)."""
    model, sym, pose_est, pose_gt, K = _chk(model, "model"), _chk(sym, "sym"), _chk(pose_est, "pose_est"), _chk(pose_gt, "pose_gt"), \
        _chk(K, "K")
    if model.dim() != 2 or model.shape[1] != 3 or model.shape[0] < 1:
        raise ValueError(f"bop_sym_dist: model must be (P,3) with P >= 1, got {tuple(model.shape)}")
    if sym.dim() != 3 or sym.shape[1:] != (3, 4) or sym.shape[0] < 1:
        raise ValueError(f"bop_sym_dist: sym must be (S,3,4) with S >= 1, got {tuple(sym.shape)}")
    if pose_est.dim() != 3 or pose_est.shape[1:] != (3, 4) or pose_gt.shape != pose_est.shape or pose_est.shape[0] < 1:
        raise ValueError(f"bop_sym_dist: pose_est and pose_gt must both be (B,3,4), got {tuple(pose_est.shape)} and {tuple(pose_gt.shape)}")
    P, S, B = model.shape[0], sym.shape[0], pose_est.shape[0]
    if K.shape == (3, 3):
        K = K.expand(B, 3, 3).contiguous()
    if K.shape != (B, 3, 3):
        raise ValueError(f"bop_sym_dist: K must be (3,3) or ({B},3,3), got {tuple(K.shape)}")
    n = int(_lib.load().rnnpose_bop_sym_dist_workspace_bytes(B, S))
    ws = torch.empty(n // 8, device=model.device, dtype=F64)
    out = torch.empty(B, 2, device=model.device, dtype=F64)
    _launch("rnnpose_bop_sym_dist_f64", _ptr(model), P, _ptr(sym), S, _ptr(pose_est), _ptr(pose_gt), _ptr(K), B, _ptr(ws), n, _ptr(out),
            _stream())
    return out


def bop_vsd(depth_est, depth_gt, depth_obs, src_index, K, diameter, delta, taus):
    """Visible surface discrepancy.  depth_est / depth_gt (B,H,W) fp32: z-buffer depths of the model under the two poses (empty
    where not > 0); depth_obs (S,H,W) fp32 observed depth (missing where not > 0 or not finite); src_index: an ops.SourceIndex, B
    integers (tensor / sequence) or None (= sample b reads depth_obs[b]); K (3,3) or (B,3,3); diameter: a number or B values (> 0
    normalises the distances, <= 0 leaves them); delta a number; taus 1..16 numbers (host values).
    -> err (B,NT) fp64, counts (B, 2+NT) int64 [#union, #inter, n_tau...]   (rnnpose_bop_vsd_f64).
    Shapes, NT and the index range are checked here, on the host (ValueError); nothing is launched then."""
    depth_est, depth_gt, depth_obs, K = _chk(depth_est, "depth_est"), _chk(depth_gt, "depth_gt"), _chk(depth_obs, "depth_obs"), _chk(K, "K")
    taus = [float(t) for t in (taus.detach().cpu().tolist() if isinstance(taus, torch.Tensor) else taus)]
    NT = len(taus)
    if not 1 <= NT <= BOP_MAX_TAUS:
        raise ValueError(f"bop_vsd: between 1 and {BOP_MAX_TAUS} taus, got {NT}")
    if depth_est.dim() != 3 or depth_gt.shape != depth_est.shape or depth_est.numel() == 0:
        raise ValueError(f"bop_vsd: depth_est and depth_gt must both be (B,H,W), got {tuple(depth_est.shape)} and {tuple(depth_gt.shape)}")
    B, H, W = depth_est.shape
    if depth_obs.dim() != 3 or depth_obs.shape[1:] != (H, W) or depth_obs.shape[0] < 1:
        raise ValueError(f"bop_vsd: depth_obs must be (S,{H},{W}), got {tuple(depth_obs.shape)}")
    S = depth_obs.shape[0]
    if src_index is None:
        src_index = range(B)
    if not isinstance(src_index, SourceIndex):
        src_index = SourceIndex(src_index, S, depth_est.device)
    if src_index.S != S or len(src_index) != B:
        raise ValueError(f"bop_vsd: src_index covers {len(src_index)} samples of {src_index.S} sources; there are {B} samples, {S} sources")
    if K.shape == (3, 3):
        K = K.expand(B, 3, 3).contiguous()
    if K.shape != (B, 3, 3):
        raise ValueError(f"bop_vsd: K must be (3,3) or ({B},3,3), got {tuple(K.shape)}")
    if isinstance(diameter, torch.Tensor):
        diameter = _chk(diameter.reshape(-1), "diameter")
    else:
        diameter = torch.as_tensor(diameter, dtype=F32).reshape(-1).to(depth_est.device)
    if diameter.numel() == 1:
        diameter = diameter.expand(B).contiguous()
    if diameter.numel() != B:
        raise ValueError(f"bop_vsd: diameter must be a number or {B} values")
    n = int(_lib.load().rnnpose_bop_vsd_workspace_bytes(B, H, W, NT))
    if n == 0:
        raise ValueError(f"bop_vsd: {H} x {W} pixels are more than one call takes")
    ws = torch.empty(n // 4, device=depth_est.device, dtype=torch.int32)
    counts = torch.empty(B, 2 + NT, device=depth_est.device, dtype=torch.int64)
    err = torch.empty(B, NT, device=depth_est.device, dtype=F64)
    tv = (C.c_double * NT)(*taus)
    _launch("rnnpose_bop_vsd_f64", _ptr(depth_est), _ptr(depth_gt), _ptr(depth_obs), S, _ptr(src_index.dev), _ptr(K), _ptr(diameter), B, H, W,
            float(delta), C.cast(tv, C.c_void_p), NT, _ptr(ws), n, _ptr(counts), _ptr(err), _stream())
    return err, counts


# ---- f4: zoom-crop on device ---------------------------------------------------------------------------------------
def pointcloud_depth(verts, vert_offsets, T, K, size):
    """verts (P,3) fp32 (all models concatenated), vert_offsets (B+1,) int32 device tensor, T (B,4,4), K (B,3,3), size (H,W)
    -> (B,1,H,W) depth splat of every image's vertices (geometry/diff_render_optim.py:369-401)."""
    verts, T, K = _chk(verts, "verts"), _chk(T, "T"), _chk(K, "K")
    if not (vert_offsets.is_cuda and vert_offsets.dtype == torch.int32 and vert_offsets.is_contiguous()):
        raise RuntimeError("vert_offsets must be a contiguous int32 GPU tensor of B+1 entries")
    B = T.shape[0]
    H, W = int(size[0]), int(size[1])
    n = int(_lib.load().rnnpose_pointcloud_depth_workspace_bytes(B, H, W))
    ws = torch.empty(n // 4, device=T.device, dtype=torch.int32)
    out = torch.empty(B, 1, H, W, device=T.device, dtype=F32)
    _launch("rnnpose_pointcloud_depth_f32", _ptr(verts), _ptr(vert_offsets), int(verts.shape[0]), _ptr(T), _ptr(K), B, H, W, _ptr(ws), n,
            _ptr(out), _stream())
    return out


def mask_bbox(depth):
    """depth (B,1,H,W) -> (B,4) int32 [xmin, ymin, xmax, ymax] of depth > 0 (model/PoseRefiner.py:154-158,259)."""
    depth = _chk(depth, "depth")
    B, _, H, W = depth.shape
    bbox = torch.empty(B, 4, device=depth.device, dtype=torch.int32)
    _launch("rnnpose_mask_bbox_f32", _ptr(depth), B, H, W, _ptr(bbox), _stream())
    return bbox


def zoom_crop_params(bbox, K, T, image_size, crop_size, margin_ratio=0.4):
    """-> theta (B,2,3) for F.affine_grid and K_crop (B,3,3)   (model/PoseRefiner.py:145-218, no host round trip)."""
    K, T = _chk(K, "K"), _chk(T, "T")
    if not (bbox.is_cuda and bbox.dtype == torch.int32 and bbox.is_contiguous()):
        raise RuntimeError("bbox must be a contiguous int32 GPU tensor (from mask_bbox)")
    B = K.shape[0]
    theta = torch.empty(B, 2, 3, device=K.device, dtype=F32)
    K_crop = torch.empty(B, 3, 3, device=K.device, dtype=F32)
    _launch("rnnpose_zoom_crop_params_f32", _ptr(bbox), _ptr(K), _ptr(T), B, int(image_size[0]), int(image_size[1]),
            int(crop_size[0]), int(crop_size[1]), float(margin_ratio), _ptr(theta), _ptr(K_crop), _stream())
    return theta, K_crop


class SourceIndex:
    """Which source image every crop of a batch reads (`zoom_crop(..., src_index=)`), checked ON THE HOST once: index (B,) with
    0 <= index[b] < S.  Holds the device copy the kernel reads.
    Build it once per batch (rnnpose_amd.PoseRefiner does, per forward) and every crop of that batch launches without a
    device->host copy; a plain tensor / list passed as src_index is checked -- and copied -- on every call."""

    def __init__(self, index, S, device):
        if isinstance(index, torch.Tensor):
            if index.dtype.is_floating_point or index.dtype == torch.bool or index.dim() != 1:
                raise ValueError("src_index must be a 1-D integer tensor")
            host = [int(v) for v in index.detach().cpu().tolist()]
        else:
            host = [int(v) for v in index]
        self.S = int(S)
        bad = [v for v in host if not 0 <= v < self.S]
        if not host or bad:
            raise ValueError(f"src_index entries must lie in [0, {self.S}) and there must be at least one: got {bad[:4] or host}")
        self.host = tuple(host)
        self.dev = torch.tensor(host, dtype=torch.int32, device=device)

    @classmethod
    def from_device(cls, dev, host, S):
        """A checked index over another device copy `dev` of the same entries (the persistent input buffers of a captured graph)."""
        obj = cls.__new__(cls)
        obj.S, obj.host, obj.dev = int(S), tuple(host), dev
        return obj

    def __len__(self):
        return len(self.host)

    def gather(self, x):
        """x (S, ...) -> (B, ...) = x[index] (torch indexing; for the few callers that need the copy)."""
        return x[self.dev.long()]


def zoom_crop(x, theta, crop_size, want_grid=False, src_index=None):
    """F.grid_sample(x, F.affine_grid(theta, (B,C,*crop_size))) fused (bilinear, zeros, align_corners=False).
    x (B,C,H,W) or None (grid only) -> out (B,C,hc,wc) [, grid (B,hc,wc,2)].
    src_index (None = crop b reads x[b]): a SourceIndex, or B integers (tensor / sequence) with 0 <= src_index[b] < S for
    x (S,C,H,W): crop b reads x[src_index[b]] -- one image shared by several crops (rnnpose_zoom_crop_indexed_f32).  Entries
    outside [0, S) raise ValueError here, on the host; nothing is launched."""
    theta = _chk(theta, "theta")
    B = theta.shape[0]
    hc, wc = int(crop_size[0]), int(crop_size[1])
    out = None
    C_, H, W = 0, 1, 1
    if src_index is not None:
        if x is None:
            raise ValueError("src_index needs a source tensor x")
        x = _chk(x, "x")
        S, C_, H, W = x.shape
        if not isinstance(src_index, SourceIndex):
            src_index = SourceIndex(src_index, S, theta.device)
        if src_index.S != S or len(src_index) != B:
            raise ValueError(f"src_index covers {len(src_index)} crops of {src_index.S} sources; theta has {B} crops, x {S} sources")
        out = torch.empty(B, C_, hc, wc, device=theta.device, dtype=F32)
        grid = torch.empty(B, hc, wc, 2, device=theta.device, dtype=F32) if want_grid else None
        _launch("rnnpose_zoom_crop_indexed_f32", _ptr(x), _ptr(src_index.dev), _ptr(theta), S, B, C_, H, W, hc, wc, _ptr(out), _ptr(grid), _stream())
        return (out, grid) if want_grid else out
    if x is not None:
        x = _chk(x, "x")
        _, C_, H, W = x.shape
        out = torch.empty(B, C_, hc, wc, device=theta.device, dtype=F32)
    grid = torch.empty(B, hc, wc, 2, device=theta.device, dtype=F32) if want_grid else None
    _launch("rnnpose_zoom_crop_f32", _ptr(x), _ptr(theta), B, C_, H, W, hc, wc, _ptr(out), _ptr(grid), _stream())
    return (out, grid) if want_grid else out


# ---- occlusion between the objects of one frame ------------------------------------------------------------------------
class OcclusionPairs:
    """Which objects of a batch may hide which (`raster_occlusion`, `MeshRenderer.occlusion`): all ORDERED pairs (b, j), b != j, of
    objects that crop the same source image -- target b, occluder j.  Objects are paired by batch index, not by class: two instances
    of one class occlude each other.  image_index: an ops.SourceIndex, B integers, or None = every object has its own image = no
    pairs.  Checked ON THE HOST once (ValueError); holds the device copies the kernel reads.  Build it once per batch."""

    MAX_PAIRS = 65535

    def __init__(self, image_index, B, device):
        B = int(B)
        if image_index is None:
            pairs = []
        else:
            host = image_index.host if isinstance(image_index, SourceIndex) else tuple(int(v) for v in (
                image_index.detach().cpu().tolist() if isinstance(image_index, torch.Tensor) else image_index))
            if len(host) != B:
                raise ValueError(f"image_index names {len(host)} objects, the batch holds {B}")
            pairs = [(b, j) for b in range(B) for j in range(B) if b != j and host[b] == host[j]]
        self._set(pairs, B, device)

    @classmethod
    def from_pairs(cls, pairs, B, device):
        """An explicit list of (target, occluder) batch indices; every index in [0, B) and target != occluder, else ValueError."""
        self = cls.__new__(cls)
        self._set([(int(b), int(j)) for b, j in pairs], int(B), device)
        return self

    def _set(self, pairs, B, device):
        if B < 1:
            raise ValueError(f"OcclusionPairs: B must be positive, got {B}")
        bad = [(b, j) for b, j in pairs if not (0 <= b < B and 0 <= j < B) or b == j]
        if bad:
            raise ValueError(f"occlusion pairs must name two different objects in [0, {B}): got {bad[:4]}")
        if len(pairs) > self.MAX_PAIRS:
            raise ValueError(f"{len(pairs)} occlusion pairs: one call takes at most {self.MAX_PAIRS}")
        self.B = B
        self.host = tuple(pairs)
        self.target = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=device)
        self.occluder = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=device)

    def __len__(self):
        return len(self.host)


def _i32_dev(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise RuntimeError(f"{name} must be a contiguous int32 GPU tensor")
    return t


def raster_keys(verts, faces, vert_off, face_off, face_cnt, max_faces, T, K, size, near=0.1, pixel_center=0.5, perspective=True):
    """Pass 1 of the mesh rasteriser (rnnpose_raster_mesh_f32) -> the (B*H*W,) int64 key buffer the resolve passes and
    `raster_occlusion` read.  Geometry as in include/rnnpose_hip.h: all meshes back to back, per-image offsets."""
    B, H, W = int(T.shape[0]), int(size[0]), int(size[1])
    n = int(_lib.load().rnnpose_raster_workspace_bytes(B, H, W))
    ws = torch.empty(n // 8, dtype=torch.int64, device=T.device)
    _launch("rnnpose_raster_mesh_f32", _ptr(verts), _ptr(faces), _ptr(vert_off), _ptr(face_off), _ptr(face_cnt), int(max_faces),
            _ptr(T), _ptr(K), B, H, W, float(near), float(pixel_center), int(perspective), _ptr(ws), n, _stream())
    return ws


def raster_occlusion(verts, faces, vert_off, face_off, face_cnt, max_faces, T, K, size, pairs: OcclusionPairs, margin: float = 0.0,
                     near: float = 0.1, pixel_center: float = 0.5, own_keys=None, depth=None, want_occluder: bool = True):
    """Which pixels of every object's own view another object of the batch hides (rnnpose_raster_occlusion_f32).
    verts (V,3) fp32, faces (F,3) int32, vert_off / face_off / face_cnt (B,) int32: the rasteriser's geometry; T (B,4,4), K (B,3,3)
    the poses and (crop) intrinsics of the own views; size (H, W); pairs: an OcclusionPairs built for this batch.
    Pixel of object b is occluded iff an occluder j of b reaches depth D there with D + margin < z_own (strict, fp32); margin is in
    the meshes' length unit, 0 = the pure depth test.
    own_keys: the key buffer of `raster_keys` for the same T, K, size with perspective=True (None: rasterised here).
    depth (B,1,H,W) fp32 contiguous: occluded pixels are set to 0 IN PLACE, the others are not touched.
    -> visible (B,1,H,W) fp32 in {0, 1} (own coverage and not occluded), occluder (B,1,H,W) int32 (-1 = not occluded) or None."""
    if not isinstance(pairs, OcclusionPairs):
        raise TypeError("pairs must be an ops.OcclusionPairs")
    verts, T, K = _chk(verts, "verts"), _chk(T, "T"), _chk(K, "K")
    faces = _i32_dev(faces, "faces")
    vert_off, face_off, face_cnt = _i32_dev(vert_off, "vert_off"), _i32_dev(face_off, "face_off"), _i32_dev(face_cnt, "face_cnt")
    B, H, W = int(T.shape[0]), int(size[0]), int(size[1])
    if pairs.B != B:
        raise ValueError(f"the occlusion pairs were built for {pairs.B} objects, the poses hold {B}")
    if T.shape[1:] != (4, 4) or K.shape != (B, 3, 3) or min(vert_off.numel(), face_off.numel(), face_cnt.numel()) < B:
        raise ValueError("raster_occlusion: T (B,4,4), K (B,3,3) and B entries of vert_off / face_off / face_cnt")
    margin = float(margin)
    if margin != margin:
        raise ValueError("raster_occlusion: margin is NaN")
    if depth is not None:
        if not (depth.is_cuda and depth.dtype == F32 and depth.is_contiguous() and depth.numel() == B * H * W):
            raise ValueError(f"depth must be a contiguous fp32 GPU tensor of {B} x {H} x {W} pixels")
    n = int(_lib.load().rnnpose_raster_workspace_bytes(B, H, W))
    if own_keys is None:
        own_keys = raster_keys(verts, faces, vert_off, face_off, face_cnt, max_faces, T, K, (H, W), near, pixel_center, True)
    elif not (own_keys.is_cuda and own_keys.is_contiguous() and own_keys.numel() * own_keys.element_size() >= n):
        raise ValueError("own_keys must be the key buffer of raster_keys for this batch and size")
    ws = torch.empty(n // 8, dtype=torch.int64, device=T.device)
    visible = torch.empty(B, 1, H, W, device=T.device, dtype=F32)
    occluder = torch.empty(B, 1, H, W, device=T.device, dtype=torch.int32) if want_occluder else None
    P = len(pairs)
    _launch("rnnpose_raster_occlusion_f32", _ptr(verts), _ptr(faces), _ptr(vert_off), _ptr(face_off), _ptr(face_cnt), int(max_faces),
            _ptr(T), _ptr(K), B, H, W, float(near), float(pixel_center), _ptr(pairs.target if P else None),
            _ptr(pairs.occluder if P else None), P, margin, _ptr(own_keys), _ptr(ws), n, _ptr(visible), _ptr(occluder), _ptr(depth),
            _stream())
    return visible, occluder


# ---- initial poses from 2D-3D descriptor matches (definitions in include/rnnpose_hip.h) -------------------------
DESC_DIM = 32


def _source_index(fn, src_index, S, B, dev, what="objects", sources="sources"):
    """src_index (an ops.SourceIndex, B integers, or None: row b reads source b) -> an ops.SourceIndex over S sources with B entries."""
    if not isinstance(src_index, SourceIndex):
        src_index = SourceIndex(range(B) if src_index is None else src_index, S, dev)
    if src_index.S != S or len(src_index) != B:
        raise ValueError(f"{fn}: src_index covers {len(src_index)} {what} of {src_index.S} {sources}; there are {B} {what}, {S} {sources}")
    return src_index


def _cached_workspace(cache, key, n_bytes, dtype):
    """The workspace of `key` (its first entry is the device) in `cache`, n_bytes of 8-byte `dtype` elements; at most 8 keys are kept,
    the oldest leaves first."""
    ws = cache.get(key)
    if ws is None:
        if len(cache) >= 8:
            cache.pop(next(iter(cache)))
        ws = cache[key] = torch.empty(n_bytes // 8, device=key[0], dtype=dtype)
    return ws


def _point_offsets(pt_off, total, max_points, device):
    """-> (device int32 (B+1,), B, largest count).  A host sequence is checked here (ascending, inside [0, total]); a device tensor is
    taken as it is, with max_points from the caller (the kernel gives count = 0 to an object whose range does not fit)."""
    if isinstance(pt_off, torch.Tensor) and pt_off.is_cuda:
        _i32_dev(pt_off, "pt_off")
        if pt_off.dim() != 1 or pt_off.numel() < 2:
            raise ValueError("desc_match: pt_off must hold B + 1 offsets")
        if max_points is None:
            raise ValueError("desc_match: a device pt_off needs max_points (the largest point count), as the rasteriser's max_faces")
        return pt_off, pt_off.numel() - 1, int(max_points)
    host = [int(v) for v in (pt_off.tolist() if hasattr(pt_off, "tolist") else pt_off)]
    if len(host) < 2 or host[0] < 0 or host[-1] > total or any(b < a for a, b in zip(host, host[1:])):
        raise ValueError(f"desc_match: pt_off must be B + 1 ascending offsets inside [0, {total}], got {host[:6]}")
    largest = max(b - a for a, b in zip(host, host[1:]))
    if largest < 1:
        raise ValueError("desc_match: no object has a point")
    return torch.tensor(host, dtype=torch.int32, device=device), len(host) - 1, largest if max_points is None else int(max_points)


def desc_match(desc3d, points, pt_off, desc2d, src_index, bbox, step=2, min_sim=0.5, mutual=True, pixel_center=0.5, M=None,
               max_points=None, out=None):
    """2D-3D descriptor matcher (rnnpose_desc_match_f32).  desc3d (total,32) / points (total,3): the objects' point descriptors and
    points back to back, object b = rows [pt_off[b], pt_off[b+1]) (pt_off: B+1 host integers, or a device int32 tensor with
    max_points=); desc2d (S,32,H,W); src_index: an ops.SourceIndex, B integers or None (object b reads desc2d[b]); bbox (B,4) int32
    [xmin, ymin, xmax, ymax] inclusive (ops.mask_bbox; a host sequence is copied), clamped to the image in the kernel; the box pixels
    `step` apart from its (clamped) corner take part.  A point is a correspondence when its best pixel's similarity is >= min_sim
    and, with mutual, that pixel's best point is the point itself.  M: output capacity per object (None: the largest point count,
    so nothing is dropped).  out: (X, x, sim, point_idx, count) to write into.
    -> X (B,M,3), x (B,M,2) pixel + pixel_center, sim (B,M), point_idx (B,M) int32, count (B) int32; rows >= count are NOT written
    (fresh outputs are zero-filled).  Shapes, dtypes, devices and the index range are checked here, on the host (ValueError)."""
    desc3d, points, desc2d = _chk(desc3d, "desc3d"), _chk(points, "points"), _chk(desc2d, "desc2d")
    if desc3d.dim() != 2 or desc3d.shape[1] != DESC_DIM or desc3d.shape[0] < 1:
        raise ValueError(f"desc_match: desc3d must be (points, {DESC_DIM}), got {tuple(desc3d.shape)}")
    total = desc3d.shape[0]
    if points.shape != (total, 3):
        raise ValueError(f"desc_match: points must be ({total}, 3), got {tuple(points.shape)}")
    if desc2d.dim() != 4 or desc2d.shape[1] != DESC_DIM or desc2d.numel() == 0:
        raise ValueError(f"desc_match: desc2d must be (S, {DESC_DIM}, H, W), got {tuple(desc2d.shape)}")
    if not (desc3d.device == points.device == desc2d.device):
        raise ValueError("desc_match: desc3d, points and desc2d must live on one device")
    S, _, H, W = desc2d.shape
    dev = desc3d.device
    pt_off, B, largest = _point_offsets(pt_off, total, max_points, dev)
    if not 1 <= largest <= total:
        raise ValueError(f"desc_match: max_points must lie in [1, {total}], got {largest}")
    src_index = _source_index("desc_match", src_index, S, B, dev, "objects", "sources")
    if not isinstance(bbox, torch.Tensor) or not bbox.is_cuda:
        bbox = torch.as_tensor(bbox, dtype=torch.int32).to(dev)
    _i32_dev(bbox, "bbox")
    if bbox.shape != (B, 4):
        raise ValueError(f"desc_match: bbox must be ({B}, 4), got {tuple(bbox.shape)}")
    step, M = int(step), int(largest if M is None else M)
    min_sim = float(min_sim)
    if step < 1 or M < 1 or min_sim != min_sim:
        raise ValueError(f"desc_match: step >= 1, M >= 1 and a min_sim that is a number, got {step}, {M}, {min_sim}")
    if out is None:
        out = (torch.zeros(B, M, 3, device=dev, dtype=F32), torch.zeros(B, M, 2, device=dev, dtype=F32), torch.zeros(B, M, device=dev, dtype=F32),
               torch.zeros(B, M, device=dev, dtype=torch.int32), torch.zeros(B, device=dev, dtype=torch.int32))
    X, x, sim, pidx, count = out
    for t, shape, dt, nm in ((X, (B, M, 3), F32, "X"), (x, (B, M, 2), F32, "x"), (sim, (B, M), F32, "sim"), (pidx, (B, M), torch.int32, "point_idx"),
                             (count, (B,), torch.int32, "count")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"desc_match: out {nm} must be a contiguous {dt} GPU tensor of shape {shape}")
    n = int(_lib.load().rnnpose_desc_match_workspace_bytes(total, B, H, W, step))
    ws = torch.empty(n // 8, device=dev, dtype=torch.int64)
    _launch("rnnpose_desc_match_f32", _ptr(desc3d), _ptr(points), _ptr(pt_off), total, largest, _ptr(desc2d), S, DESC_DIM, H, W,
            _ptr(src_index.dev), _ptr(bbox), B, step, min_sim, int(bool(mutual)), float(pixel_center), M, _ptr(ws), n, _ptr(X), _ptr(x),
            _ptr(sim), _ptr(pidx), _ptr(count), _stream())
    return X, x, sim, pidx, count


def random_words(rnd):
    """Random 32-bit words as the int32 bit patterns the kernel reads as uint32: an integer tensor with values in [0, 2^32) (int64) or any
    32-bit integer tensor."""
    if not isinstance(rnd, torch.Tensor) or rnd.dtype.is_floating_point or rnd.dtype == torch.bool:
        raise ValueError("rnd must be an integer tensor")
    if rnd.dtype == torch.int64:
        rnd = torch.where(rnd >= 2 ** 31, rnd - 2 ** 32, rnd).to(torch.int32)
    elif rnd.dtype != torch.int32:
        rnd = rnd.view(torch.int32) if rnd.element_size() == 4 else rnd.to(torch.int32)
    return rnd.contiguous()


def _pnp_inputs(fn, X, x, count, K, rnd, tau, n_polish, min_count):
    """The inputs of `pnp_ransac` and `pnp_ransac_topk`, checked (ValueError) and as the library takes them: K per object, rnd as int32
    words.  -> (X, x, count, K, rnd, B, M, Hyp, tau, n_polish, min_count, dev)."""
    for t, nm in ((X, "X"), (x, "x"), (K, "K")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype.is_floating_point):
            raise ValueError(f"{fn}: {nm} must be a floating-point GPU tensor")
    if not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype == torch.int32 and count.is_contiguous()):
        raise ValueError(f"{fn}: count must be a contiguous int32 GPU tensor")
    X, x, K = _chk(X, "X"), _chk(x, "x"), _chk(K, "K")
    if X.dim() != 3 or X.shape[2] != 3 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"{fn}: X must be (B,M,3), got {tuple(X.shape)}")
    B, M = X.shape[0], X.shape[1]
    if x.shape != (B, M, 2):
        raise ValueError(f"{fn}: x must be ({B},{M},2), got {tuple(x.shape)}")
    if count.shape != (B,):
        raise ValueError(f"{fn}: count must be ({B},), got {tuple(count.shape)}")
    if K.shape == (3, 3):
        K = K.expand(B, 3, 3).contiguous()
    if K.shape != (B, 3, 3):
        raise ValueError(f"{fn}: K must be (3,3) or ({B},3,3), got {tuple(K.shape)}")
    rnd = random_words(rnd)
    if not rnd.is_cuda or rnd.dim() != 3 or rnd.shape[0] != B or rnd.shape[2] != 3 or rnd.shape[1] < 1:
        raise ValueError(f"{fn}: rnd must be a GPU tensor of shape ({B},Hyp,3), got {tuple(rnd.shape)} on {rnd.device}")
    if not (X.device == x.device == count.device == K.device == rnd.device):
        raise ValueError(f"{fn}: all tensors must live on one device")
    Hyp = rnd.shape[1]
    tau, n_polish, min_count = float(tau), int(n_polish), int(min_count)
    if not (tau > 0.0 and tau < float("inf")) or not 0 <= n_polish <= 64 or min_count < 4:
        raise ValueError(f"{fn}: tau > 0 and finite, n_polish in [0,64], min_count >= 4; got {tau}, {n_polish}, {min_count}")
    return X, x, count, K, rnd, B, M, Hyp, tau, n_polish, min_count, X.device


def pnp_ransac(X, x, count, K, rnd, tau=4.0, n_polish=4, min_count=4, T=None):
    """P3P RANSAC with MSAC scoring and a Gauss-Newton polish, fp64 on the device (rnnpose_pnp_ransac_f64).  X (B,M,3), x (B,M,2),
    count (B) int32: the matcher's outputs; K (3,3) or (B,3,3); rnd (B,Hyp,3) random 32-bit words (ops.random_words): hypothesis h of
    object b samples the correspondences rnd[b,h,:] % count[b].  tau: inlier threshold in pixels.  T (B,4,4) fp32: written where
    info == 0 and left as it is elsewhere (None: identities).
    -> T (B,4,4), cost (B,Hyp) fp64, inliers (B,Hyp) int32, best (B) int32, inlier_mask (B,M) uint8, n_inliers (B) int32,
       final_cost (B) fp64, info (B) int32 (0, or -1: too few correspondences / no candidate / singular polish).
    Shapes, dtypes and devices are checked here, on the host (ValueError)."""
    fn = "pnp_ransac"
    X, x, count, K, rnd, B, M, Hyp, tau, n_polish, min_count, dev = _pnp_inputs(fn, X, x, count, K, rnd, tau, n_polish, min_count)
    if T is None:
        T = torch.eye(4, device=dev, dtype=F32).repeat(B, 1, 1)
    elif not (isinstance(T, torch.Tensor) and T.is_cuda and T.dtype == F32 and T.is_contiguous() and tuple(T.shape) == (B, 4, 4)):
        raise ValueError(f"{fn}: T must be a contiguous fp32 GPU tensor of shape ({B},4,4)")
    n = int(_lib.load().rnnpose_pnp_ransac_workspace_bytes(B, Hyp))
    ws = torch.empty(n // 8, device=dev, dtype=torch.int64)
    cost = torch.empty(B, Hyp, device=dev, dtype=F64)
    inliers = torch.empty(B, Hyp, device=dev, dtype=torch.int32)
    best = torch.empty(B, device=dev, dtype=torch.int32)
    mask = torch.zeros(B, M, device=dev, dtype=torch.uint8)
    n_inl = torch.empty(B, device=dev, dtype=torch.int32)
    fcost = torch.empty(B, device=dev, dtype=F64)
    info = torch.empty(B, device=dev, dtype=torch.int32)
    _launch("rnnpose_pnp_ransac_f64", _ptr(X), _ptr(x), _ptr(count), M, _ptr(K), _ptr(rnd), B, Hyp, tau, n_polish, min_count, _ptr(ws), n,
            _ptr(T), _ptr(cost), _ptr(inliers), _ptr(best), _ptr(mask), _ptr(n_inl), _ptr(fcost), _ptr(info), _stream())
    return T, cost, inliers, best, mask, n_inl, fcost, info


PNP_TOPK_MAX = 16
_topk_ws = {}


def pnp_ransac_topk(X, x, count, K, rnd, tau=4.0, n_polish=4, min_count=4, top_k=4, sep_frac=0.1, min_inliers=0, T=None):
    """The top_k best DISTINCT hypotheses of the P3P RANSAC, each polished (rnnpose_pnp_ransac_topk_f64).  The
    inputs of `pnp_ransac`; two poses are distinct when some corner of the correspondences' bounding box moves by more than
    sep_frac x the box diagonal between them; slot 0 is `pnp_ransac`'s hypothesis, slot k the cheapest one distinct from every slot
    before it with at least min_inliers inliers.  T (B,top_k,4,4) fp32: written where info == 0 and left as it is elsewhere (None:
    identities, so an unwritten slot is a harmless pose).
    -> T (B,top_k,4,4), cost (B,Hyp) fp64, inliers (B,Hyp) int32, hyp (B,top_k) int32 (-1: no such slot), inlier_mask (B,top_k,M)
       uint8, n_inliers (B,top_k) int32, final_cost (B,top_k) fp64, info (B,top_k) int32, dup_of (B,top_k) int32 (the earlier slot
       the polish led this one into, or -1), n_found (B) int32.
    Shapes, dtypes, devices, contiguity and ranges are checked here, on the host (ValueError).  The workspace is cached per
    (device, B, Hyp, top_k): calls of one shape must not overlap on different streams."""
    fn = "pnp_ransac_topk"
    X, x, count, K, rnd, B, M, Hyp, tau, n_polish, min_count, dev = _pnp_inputs(fn, X, x, count, K, rnd, tau, n_polish, min_count)
    sep_frac = float(sep_frac)
    if int(top_k) != top_k or not 1 <= int(top_k) <= PNP_TOPK_MAX or not 0.0 <= sep_frac < float("inf") or int(min_inliers) != min_inliers or min_inliers < 0:
        raise ValueError(f"{fn}: top_k in [1,{PNP_TOPK_MAX}], sep_frac >= 0 and finite, min_inliers >= 0; got {top_k}, {sep_frac}, {min_inliers}")
    Kt, min_inliers = int(top_k), int(min_inliers)
    if T is None:
        T = torch.eye(4, device=dev, dtype=F32).repeat(B, Kt, 1, 1)
    elif not (isinstance(T, torch.Tensor) and T.is_cuda and T.dtype == F32 and T.is_contiguous() and tuple(T.shape) == (B, Kt, 4, 4) and T.device == dev):
        raise ValueError(f"{fn}: T must be a contiguous fp32 GPU tensor of shape ({B},{Kt},4,4)")
    n = int(_lib.load().rnnpose_pnp_ransac_topk_workspace_bytes(B, Hyp, Kt))
    if n == 0 or B * M * Kt >= 2 ** 31:
        raise ValueError(f"{fn}: {B} objects x {Hyp} hypotheses x {Kt} slots x {M} correspondences are more than one call takes")
    ws = _cached_workspace(_topk_ws, (dev, B, Hyp, Kt), n, torch.int64)
    cost = torch.empty(B, Hyp, device=dev, dtype=F64)
    inliers = torch.empty(B, Hyp, device=dev, dtype=torch.int32)
    hyp = torch.empty(B, Kt, device=dev, dtype=torch.int32)
    mask = torch.zeros(B, Kt, M, device=dev, dtype=torch.uint8)
    n_inl = torch.empty(B, Kt, device=dev, dtype=torch.int32)
    fcost = torch.empty(B, Kt, device=dev, dtype=F64)
    info = torch.empty(B, Kt, device=dev, dtype=torch.int32)
    dup_of = torch.empty(B, Kt, device=dev, dtype=torch.int32)
    n_found = torch.empty(B, device=dev, dtype=torch.int32)
    _launch("rnnpose_pnp_ransac_topk_f64", _ptr(X), _ptr(x), _ptr(count), M, _ptr(K), _ptr(rnd), B, Hyp, tau, n_polish, min_count, Kt, sep_frac,
            min_inliers, _ptr(ws), n, _ptr(T), _ptr(cost), _ptr(inliers), _ptr(hyp), _ptr(mask), _ptr(n_inl), _ptr(fcost), _ptr(info),
            _ptr(dup_of), _ptr(n_found), _stream())
    return T, cost, inliers, hyp, mask, n_inl, fcost, info, dup_of, n_found


# ---- pose confidence: render-and-compare score of a pose against its frame (definitions in include/rnnpose_hip.h) ----
POSE_SCORE_COLUMNS = ("n_rend", "n_out", "n_occ", "n_cons", "n_viol", "n_hole", "n_desc", "sum_cos", "sum_abs_dd", "n_bad")
_score_ws = {}


def _strict(t, name, dtype, fn):
    """The tensor as it is, or ValueError: nothing is converted or copied for the caller here."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        what = f"{t.dtype} on {t.device}, contiguous: {t.is_contiguous()}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{fn}: {name} must be a contiguous {dtype} GPU tensor, got {what}")
    return t


def pose_score(rend_depth, rend_desc, window, desc2d, src_index=None, depth_obs=None, depth_tol=0.015):
    """Render-and-compare score of B poses (rnnpose_pose_score_f64).  rend_depth (B,h,w) or (B,1,h,w) and rend_desc (B,32,h,w) fp32:
    every object's z-buffer and descriptors rendered into its window of the frame with the principal point shifted by the window's
    corner; window (B,2) int32 (x0, y0) of any sign (a device tensor, or host values that are copied); desc2d (S,32,H,W) fp32;
    src_index: an ops.SourceIndex, B integers or None (pose b reads frame b); depth_obs (S,H,W) fp32 or None; depth_tol >= 0, in
    the depth maps' unit.
    -> stats (B,10) fp64 in the order of POSE_SCORE_COLUMNS, score (B) fp64.
    Shapes, dtypes, devices, contiguity and the index range are checked here, on the host (ValueError); nothing is converted.  The
    workspace is cached per (device, B, h, w): calls of one shape must not overlap on different streams."""
    fn = "pose_score"
    rend_depth, rend_desc, desc2d = _strict(rend_depth, "rend_depth", F32, fn), _strict(rend_desc, "rend_desc", F32, fn), _strict(desc2d, "desc2d", F32, fn)
    if rend_desc.dim() != 4 or rend_desc.shape[1] != DESC_DIM or rend_desc.numel() == 0:
        raise ValueError(f"{fn}: rend_desc must be (B, {DESC_DIM}, h, w), got {tuple(rend_desc.shape)}")
    B, _, h, w = rend_desc.shape
    if tuple(rend_depth.shape) not in ((B, h, w), (B, 1, h, w)):
        raise ValueError(f"{fn}: rend_depth must be ({B},{h},{w}) or ({B},1,{h},{w}), got {tuple(rend_depth.shape)}")
    if desc2d.dim() != 4 or desc2d.shape[1] != DESC_DIM or desc2d.numel() == 0:
        raise ValueError(f"{fn}: desc2d must be (S, {DESC_DIM}, H, W), got {tuple(desc2d.shape)}")
    S, _, H, W = desc2d.shape
    dev = rend_desc.device
    if depth_obs is not None:
        _strict(depth_obs, "depth_obs", F32, fn)
        if tuple(depth_obs.shape) != (S, H, W):
            raise ValueError(f"{fn}: depth_obs must be ({S},{H},{W}), got {tuple(depth_obs.shape)}")
    if not isinstance(window, torch.Tensor) or not window.is_cuda:
        window = torch.as_tensor(window, dtype=torch.int32).to(dev)
    _strict(window, "window", torch.int32, fn)
    if tuple(window.shape) != (B, 2):
        raise ValueError(f"{fn}: window must be ({B}, 2), got {tuple(window.shape)}")
    src_index = _source_index(fn, src_index, S, B, dev, "poses", "frames")
    if any(t.device != dev for t in (rend_depth, desc2d, window, src_index.dev) + (() if depth_obs is None else (depth_obs,))):
        raise ValueError(f"{fn}: all tensors must live on one device")
    depth_tol = float(depth_tol)
    if not 0.0 <= depth_tol < float("inf"):
        raise ValueError(f"{fn}: depth_tol must be non-negative and finite, got {depth_tol}")
    n = int(_lib.load().rnnpose_pose_score_workspace_bytes(B, h, w))
    if n == 0:
        raise ValueError(f"{fn}: {B} windows of {h} x {w} pixels are more than one call takes")
    ws = _cached_workspace(_score_ws, (dev, B, h, w), n, F64)
    stats = torch.empty(B, len(POSE_SCORE_COLUMNS), device=dev, dtype=F64)
    score = torch.empty(B, device=dev, dtype=F64)
    _launch("rnnpose_pose_score_f64", _ptr(rend_depth), _ptr(rend_desc), _ptr(window), _ptr(desc2d), _ptr(depth_obs), _ptr(src_index.dev), B, S,
            DESC_DIM, h, w, H, W, depth_tol, _ptr(ws), n, _ptr(stats), _ptr(score), _stream())
    return stats, score


# ---- object onboarding: exact diameter and farthest-point sampling ----------------------------------------------------
DIAMETER_MAX_POINTS = 1 << 20


def _object_offsets(fn, points, pt_off):
    """points (total,3) and pt_off (None: one object; B+1 host integers, checked here; or a device int32 tensor, taken as it is: the
    kernels give an object whose range does not fit nothing) -> points (at least one row behind the pointer), total, pt_off on the
    device, B."""
    _strict(points, "points", F32, fn)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{fn}: points must be (total, 3), got {tuple(points.shape)}")
    total, dev = points.shape[0], points.device
    if isinstance(pt_off, torch.Tensor) and pt_off.is_cuda:
        _strict(pt_off, "pt_off", torch.int32, fn)
        if pt_off.dim() != 1 or pt_off.numel() < 2 or pt_off.device != dev:
            raise ValueError(f"{fn}: pt_off must hold B + 1 offsets on the device of points")
    else:
        host = [0, total] if pt_off is None else [int(v) for v in (pt_off.tolist() if hasattr(pt_off, "tolist") else pt_off)]
        if len(host) < 2 or host[0] < 0 or host[-1] > total or any(b < a for a, b in zip(host, host[1:])):
            raise ValueError(f"{fn}: pt_off must be B + 1 ascending offsets inside [0, {total}], got {host[:6]}")
        pt_off = torch.tensor(host, dtype=torch.int32, device=dev)
    if total == 0:
        points = torch.zeros(1, 3, device=dev, dtype=F32)              # (a pointer to hand over; total_points stays 0)
    return points, total, pt_off, pt_off.numel() - 1


def point_diameter(points, pt_off=None):
    """Exact diameter of B point sets (rnnpose_point_diameter_f64).  points (total,3) fp32 on the GPU, object b = rows
    [pt_off[b], pt_off[b+1]) (None: one object of all rows; B+1 host integers; or a device int32 tensor).
    -> d2 (B) fp64 the largest pairwise squared distance, diameter (B) fp64, pair (B,2) int32 (i < j, the lowest on ties, (-1,-1) with
    fewer than two finite points), bounds (B,2,3) fp32 (min, max).  O(P^2) pair evaluations in fp64.
    Device, dtype, contiguity and the offsets are checked here, on the host (ValueError); nothing is converted."""
    fn = "point_diameter"
    points, total, pt_off, B = _object_offsets(fn, points, pt_off)
    n = int(_lib.load().rnnpose_point_diameter_workspace_bytes(total, B))
    if n == 0:
        raise ValueError(f"{fn}: {total} points in {B} objects are more than one call takes ({DIAMETER_MAX_POINTS} points, 65535 objects)")
    dev = points.device
    ws = torch.empty(n // 8, device=dev, dtype=F64)
    d2, diam = torch.empty(B, device=dev, dtype=F64), torch.empty(B, device=dev, dtype=F64)
    pair, bounds = torch.empty(B, 2, device=dev, dtype=torch.int32), torch.empty(B, 2, 3, device=dev, dtype=F32)
    _launch("rnnpose_point_diameter_f64", _ptr(points), _ptr(pt_off), total, B, _ptr(ws), n, _ptr(d2), _ptr(diam), _ptr(pair), _ptr(bounds), _stream())
    return d2, diam, pair, bounds


def farthest_points(points, n, pt_off=None, start=-1):
    """Farthest-point sampling, n picks per object (rnnpose_fps_f64).  points / pt_off as point_diameter; start: one integer for every
    object, B integers, or a device int32 tensor (B): >= 0 the first pick, -1 the point farthest from the origin (the rule of the
    reference's fragmentation_fps).
    -> idx (B,n) int32 in pick order and dist2 (B,n) fp64, the running squared distance of each pick when it was picked (+inf for a given
    first pick): sqrt(dist2[b][k]) is the coverage radius after k picks.  Rows past the last pickable point hold -1.
    Device, dtype, contiguity, the offsets and host start values are checked here (ValueError); nothing is converted."""
    fn = "farthest_points"
    points, total, pt_off, B = _object_offsets(fn, points, pt_off)
    n = int(n)
    if n < 1 or B * n >= 2 ** 31:
        raise ValueError(f"{fn}: n must be >= 1 and B * n < 2^31, got n = {n}, B = {B}")
    dev = points.device
    if isinstance(start, torch.Tensor) and start.is_cuda:
        _strict(start, "start", torch.int32, fn)
        if tuple(start.shape) != (B,) or start.device != dev:
            raise ValueError(f"{fn}: start must be ({B},) on the device of points, got {tuple(start.shape)}")
    else:
        host = [int(start)] * B if isinstance(start, int) else [int(v) for v in (start.tolist() if hasattr(start, "tolist") else start)]
        if len(host) != B or any(v < -1 for v in host):
            raise ValueError(f"{fn}: start must be {B} integers >= -1, got {host[:6]}")
        start = torch.tensor(host, dtype=torch.int32, device=dev)
    nb = int(_lib.load().rnnpose_fps_workspace_bytes(total, B))
    ws = torch.empty(nb // 8, device=dev, dtype=F64)
    idx, dist2 = torch.empty(B, n, device=dev, dtype=torch.int32), torch.empty(B, n, device=dev, dtype=F64)
    _launch("rnnpose_fps_f64", _ptr(points), _ptr(pt_off), total, B, n, _ptr(start), _ptr(ws), nb, _ptr(idx), _ptr(dist2), _stream())
    return idx, dist2
