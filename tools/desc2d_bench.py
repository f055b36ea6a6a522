#!/usr/bin/env python3
"""SuperPoint2D wall time: the HIP network (rnnpose_amd.descriptor2d) against the same network as torch fp32 modules (MIOpen
convolutions, the reference's forward of model/descriptor2D.py restated with the same parameters), in one process, device events.

    python tools/desc2d_bench.py [--runs 20] [--warmup 3] [--shapes 16x480x640,8x480x640,1x480x640] [--out profiles/x.json]

Per shape: descriptors only (what HybridDescNet keeps) and full (scores too), median / min / max over --runs after --warmup, and
the achieved ALGORITHMIC TFLOP/s of the full-resolution 3x3 layers (decode3, convDa, convPa) from a per-launch profile of one HIP
run (ops.profile)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rnnpose_amd import synthetic as syn  # noqa: E402

CONFIG = dict(input_dim=3, descriptor_dim=32, normalize_output=True, use_instance_norm=True, saliency_score_normalization_fuc="sigmoid")


def torch_forward(net, x, scores=True):
    """model/descriptor2D.py:113-173 with torch fp32 modules (cuDNN/MIOpen convolutions)."""
    conv = lambda x, m: F.conv2d(x, m.weight, m.bias, padding=m.weight.shape[-1] // 2)
    up = lambda x: F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    skips = []
    for i, (a, b) in enumerate(((net.conv1a, net.conv1b), (net.conv2a, net.conv2b), (net.conv3a, net.conv3b), (net.conv4a, net.conv4b))):
        x = F.relu(conv(F.relu(conv(x, a)), b))
        if i < 3:
            skips.append(x)
            x = F.max_pool2d(x, 2, 2)
    x = F.relu(F.instance_norm(conv(up(x), net.decode1[1])))
    x = F.relu(F.instance_norm(conv(up(torch.cat([x, skips[2]], 1)), net.decode2[1])))
    x = F.relu(F.instance_norm(conv(up(torch.cat([x, skips[1]], 1)), net.decode3[1])))
    d = F.normalize(conv(F.relu(conv(x, net.convDa)), net.convDb), p=2, dim=1)
    s = torch.sigmoid(conv(F.relu(F.instance_norm(conv(x, net.convPa[0]))), net.convPb)) if scores else None
    return d, s


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="16x480x640,8x480x640,1x480x640")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from rnnpose_amd import build, ops
    from rnnpose_amd.descriptor2d import SuperPoint2D
    build.build()
    dev = torch.device("cuda")
    net = SuperPoint2D(CONFIG)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_module_weights(shapes, seed=4).items()}, strict=True)
    net = net.to(dev).eval()
    results = []
    with torch.no_grad():
        for sh in a.shapes.split(","):
            B, H, W = (int(t) for t in sh.split("x"))
            img = syn.uniform_t("desc2d_bench", (B, 3, H, W), 1, 0.0, 255.0, device=dev)
            row = {"B": B, "H": H, "W": W}
            for mode, sc in (("descriptors_only", False), ("full", True)):
                net.compute_scores = sc
                hip = timed(lambda: net(img), a.runs, a.warmup)
                tch = timed(lambda: torch_forward(net, img, sc), a.runs, a.warmup)
                row[mode] = {"hip": hip, "torch_fp32": tch, "speedup": round(tch["median_ms"] / hip["median_ms"], 3)}
            net.compute_scores = True
            # per-launch profile of one HIP run: the full-resolution 3x3 layers' achieved algorithmic rate, and every launch family
            torch.cuda.synchronize()
            with ops.profile() as rec:
                net(img)
            summ = ops.summarize(rec)
            flop = 2.0 * B * H * W * 9 * (192 * 128 + 2 * 128 * 256)
            # the full-resolution 3x3 layers are the three conv launches of most work per chunk (decode3, convDa, convPa)
            convs = sorted(((w, x.elapsed_time(y)) for x, y, w, _ in rec.get("rnnpose_conv2d_nhwc_f16x3", [])), reverse=True)
            top = convs[:3 * -(-B // net.engine.chunk_images(H, W))]
            ms_full = sum(t for _, t in top)
            row["fullres_3x3"] = {"algorithmic_gflop": round(flop / 1e9, 1), "ms": round(ms_full, 3),
                                  "tflops": round(flop / (ms_full * 1e-3) / 1e12, 1) if ms_full else None}
            row["per_family_ms"] = {k: round(v[2], 3) for k, v in summ.items()}
            row["range_events"] = int(ops.saturation_events().item())
            print(json.dumps(row), flush=True)
            results.append(row)
            del img
            torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "runs": a.runs, "warmup": a.warmup, "results": results}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"summary": [(r["B"], r["descriptors_only"]["hip"]["median_ms"], r["full"]["hip"]["median_ms"],
                                   r["full"]["torch_fp32"]["median_ms"], r["full"]["speedup"]) for r in results]}))


if __name__ == "__main__":
    main()
