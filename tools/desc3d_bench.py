#!/usr/bin/env python3
"""KPSuperpoint3Dv2 wall time: the HIP network (rnnpose_amd.descriptor3d) against the same network as torch fp32 operations on
the GPU (the reference's forward of model/descriptor3D.py on kpconv_blocks.py, restated with the same parameters), in one
process, device events.  Both networks of RNNPose (descriptors, 32 channels; context, 256 channels) and the pyramid build.

    python tools/desc3d_bench.py [--runs 10] [--warmup 2] [--points 3000,20000] [--out profiles/desc3d_bench.json]

The clouds are ellipsoid surfaces at a normalised model's scale; neighbourhood limits 40 per level."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import desc3d_fp64 as R  # noqa: E402
from rnnpose_amd.descriptor3d import KPSuperpoint3Dv2, kpconv_inputs  # noqa: E402

LIMITS = [40, 40, 40, 40]


def torch_forward(net, b):
    """model/descriptor3D.py:132-196 with torch fp32 operations (the reference's own formulation, kpconv_blocks.py)."""
    sd = {k: v.float() for k, v in net.state_dict().items()}
    pts, nbs, pools, ups = b["points"], [n.long() for n in b["neighbors"]], [n.long() for n in b["pools"]], [n.long() for n in b["upsamples"]]
    norm = lambda x: torch.nn.functional.instance_norm(x.t()[None])[0].t()
    leaky = lambda x: torch.nn.functional.leaky_relu(x, 0.1)
    pad = lambda x: torch.cat([x, torch.zeros_like(x[:1])], 0)
    radii = R.encoder_radii(net.config)

    def kpconv(pre, q, s, nb, x, radius):
        W, kp = sd[pre + ".weights"], sd[pre + ".kernel_points"]
        extent = radius * net.config["KP_extent"] / net.config["conv_radius"]
        s_ = torch.cat([s, torch.zeros_like(s[:1]) + 1e6], 0)
        d2 = torch.sum(((s_[nb] - q[:, None])[:, :, None, :] - kp) ** 2, dim=3)
        w = torch.clamp(1 - torch.sqrt(d2) / extent, min=0.0).transpose(1, 2)
        nx = pad(x)[nb]
        out = torch.matmul(torch.matmul(w, nx).permute(1, 0, 2), W).sum(0)
        cnt = torch.clamp((nx.sum(-1) > 0).sum(-1), min=1)
        return out / cnt[:, None]

    lin = lambda k, x: x @ sd[k].reshape(sd[k].shape[0], -1).t()
    x, layer, skips = b["features"], 0, []
    for i, blk in enumerate(net.encoder_blocks):
        pre, strided = f"encoder_blocks.{i}", "strided" in blk.block_name
        q, s, nb = (pts[layer + 1], pts[layer], pools[layer]) if strided else (pts[layer], pts[layer], nbs[layer])
        if strided:
            skips.append(x)
        if i == 0:
            x = leaky(norm(kpconv(pre + ".KPConv", q, s, nb, x, radii[i])))
        else:
            h = leaky(norm(lin(pre + ".unary1.mlp.weight", x))) if blk.unary1 is not None else x
            y = lin(pre + ".unary2.mlp.weight", leaky(norm(kpconv(pre + ".KPConv", q, s, nb, h, radii[i]))))
            sc = pad(x)[nb].max(1).values if strided else x
            if blk.unary_shortcut is not None:
                sc = norm(lin(pre + ".unary_shortcut.mlp.weight", sc))
            x = leaky(norm(y) + sc)
        if strided:
            layer += 1
    x = lin("bottle.weight", x) + sd["bottle.bias"]
    x = lin("proj_gnn.weight", x) + sd["proj_gnn.bias"]
    for lv, di in zip(range(len(skips) - 1, -1, -1), (1, 3, 5)):
        x = torch.cat([pad(x)[ups[lv][:, 0]], skips.pop()], 1)
        y = lin(f"decoder_blocks.{di}.mlp.weight", x)
        x = y if lv == 0 else leaky(norm(y))
    x = x[:, :net.final_feats_dim]
    return torch.nn.functional.normalize(x, p=2, dim=1) if net.normalize_output else x


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(e))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", default="3000,20000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev), "limits": LIMITS, "runs": a.runs, "shapes": []}
    nets = {}
    for name, cfg in (("desc", R.DESC), ("ctx", R.CTX)):
        net = KPSuperpoint3Dv2(dict(cfg))
        w = R.make_weights({k: tuple(v.shape) for k, v in net.state_dict().items()}, cfg, R.SEEDS[name])
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()})
        nets[name] = net.to(dev).eval()
    for n in [int(v) for v in a.points.split(",")]:
        pts = torch.from_numpy(R.ellipsoid_cloud(f"bench{n}", n, axes=(0.5, 0.4, 0.3))).to(dev)
        row = {"points": n, "pyramid": timed(lambda: kpconv_inputs(pts, R.DESC, LIMITS), a.runs, a.warmup)}
        b = kpconv_inputs(pts, R.DESC, LIMITS)
        row["levels"] = [int(p.shape[0]) for p in b["points"]]
        row["widths"] = [int(x.shape[1]) for x in b["neighbors"]]
        with torch.no_grad():
            for name, net in nets.items():
                hip = timed(lambda: net(b), a.runs, a.warmup)
                ref = timed(lambda: torch_forward(net, b), a.runs, a.warmup)
                d = float((net(b) - torch_forward(net, b)).abs().max())
                row[name] = {"hip": hip, "torch_fp32": ref, "speedup": ref["median_ms"] / hip["median_ms"], "max_abs_diff": d}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
