#!/usr/bin/env python3
"""MeshRenderer cost of one render_tex call: rasterise (rnnpose_raster_mesh_f32) plus resolve, device events, in two colour
configurations on the same geometry:
  * "vertex_flat":   per-vertex colours, flat two-sided shading   (rnnpose_raster_resolve_f32, the existing entry point)
  * "texture_phong": a 1024^2 UV texture, per-pixel Phong shading (rnnpose_raster_resolve_tex_f32)
each with no attribute channel (the colour alone) and with the refiner's 288 (256 context + 32 descriptor channels).

    python tools/raster_bench.py [--runs 50] [--warmup 5] [--batch 8] [--size 480,640] [--out profiles/raster_tex_bench.json]

The mesh is a latitude-longitude ellipsoid of ~10k faces with its UVs (u = longitude, v = latitude) at LINEMOD object size
and distance (0.7 m, LINEMOD intrinsics)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rnnpose_amd import synthetic as syn  # noqa: E402
from rnnpose_amd.rasterizer import MeshRenderer  # noqa: E402


def uv_ellipsoid(n_lat=70, n_lon=72, scale=(0.09, 0.07, 0.05)):
    """-> verts (P,3), faces (F,3), uvs (P,2): a seam column is duplicated so that u runs 0..1 without wrapping"""
    lat = np.linspace(0, np.pi, n_lat + 1)
    lon = np.linspace(0, 2 * np.pi, n_lon + 1)
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    verts = np.stack([np.sin(la) * np.cos(lo), np.sin(la) * np.sin(lo), np.cos(la)], -1).reshape(-1, 3) * np.array(scale)
    uvs = np.stack([lo / (2 * np.pi), 1 - la / np.pi], -1).reshape(-1, 2)
    idx = np.arange((n_lat + 1) * (n_lon + 1)).reshape(n_lat + 1, n_lon + 1)
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    faces = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return verts.astype(np.float32), faces.astype(np.int32), uvs.astype(np.float32)


def time_call(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return dict(median_us=statistics.median(ts), min_us=min(ts), max_us=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", default="480,640")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split(","))
    B = a.batch
    verts, faces, uvs = uv_ellipsoid()
    P = verts.shape[0]
    rng = np.random.default_rng(0)
    tex = rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8).astype(np.float32) / np.float32(255.0)
    cols = syn.uniform("col", (P, 3), 1)
    renderers = {
        "vertex_flat": MeshRenderer({"obj": dict(verts=verts, faces=faces, colors=cols)}),
        "texture_phong": MeshRenderer({"obj": dict(verts=verts, faces=faces, verts_uvs=uvs, faces_uvs=faces, texture=tex)},
                                      shading="phong"),
    }
    K = torch.tensor([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]]).expand(B, 3, 3).contiguous().cuda()
    G = syn.se3_exp_np(syn.normal("g", (B, 6), 3, std=0.5))
    G[:, :3, 3] = syn.uniform("t", (B, 3), 3, -0.05, 0.05) + np.array([0, 0, 0.7])
    Tm = torch.from_numpy(G.astype(np.float32)).cuda()
    names = ["obj"] * B
    res = dict(device=torch.cuda.get_device_name(0) if a.out else None, batch=B, size=[H, W], faces=int(faces.shape[0]), verts=int(P),
               texture=[1024, 1024], runs=a.runs, configs={})
    for cname, ren in renderers.items():
        for C in (0, 288):
            attr = torch.from_numpy(syn.normal("a", (1, P, C), 2)).cuda() if C else torch.zeros(1, P, 0, device="cuda")
            bt = ren._batch(names)
            T_, K_ = ren._tk(Tm, K)
            ws = ren._raster(bt, T_, K_, (H, W), 0.1, True)
            attr_off = torch.zeros(B, dtype=torch.int64, device="cuda")
            if cname == "texture_phong":
                resolve = lambda: ren._resolve_tex(bt, T_, K_, (H, W), 0.1, ws, attr, attr_off, C)
            else:
                resolve = lambda: ren._resolve(bt, T_, K_, (H, W), 0.1, True, ws, attr=attr, attr_off=attr_off, Cc=C,
                                               with_color=True, want_zbuf=True)
            out = ren(names, attr, T=Tm, K=K, render_image_size=(H, W), render_tex=True)
            cover = float((out[1] > 0).float().mean())
            r = dict(channels=C, coverage=cover,
                     raster=time_call(lambda: ren._raster(bt, T_, K_, (H, W), 0.1, True), a.runs, a.warmup),
                     resolve=time_call(resolve, a.runs, a.warmup),
                     call=time_call(lambda: ren(names, attr, T=Tm, K=K, render_image_size=(H, W), render_tex=True), a.runs, a.warmup))
            res["configs"][f"{cname}_C{C}"] = r
            print(f"{cname:14s} C={C:3d}  coverage {cover:.3f}  raster {r['raster']['median_us']:8.1f} us  "
                  f"resolve {r['resolve']['median_us']:8.1f} us  whole call {r['call']['median_us']:8.1f} us")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
