"""Onboarding an object from its mesh: from a model file to the `eval_epoch.ClassModel` every stage is keyed on.

    info = read_models_info("models/models_info.json", scale=0.001)          # BOP: diameter, bounds, symmetries per object id
    cm = build_class_model("obj_05", "models/obj_000005.ply", desc_net, ctx_net, limits, scale=0.001,
                           n_eval_points=3000, symmetries=info[5]["symmetries"])
    centers, center_inds, vert_frag_ids = fragments(cm.verts, 64)            # the reference's fragmentation_fps, on the device

The diameter is the exact largest vertex distance (`ops.point_diameter`), subsets are farthest-point subsets (`ops.farthest_points`,
first pick = the vertex farthest from the origin, the rule of the reference's utils/furthest_point_sample.py).
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from . import mesh_io, ops


def _axis_rotation(axis, angle, offset):
    """(4,4) fp64: the rotation by `angle` about the line through `offset` along `axis` (Rodrigues)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    R = np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)
    o = np.asarray(offset, np.float64)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = o - R @ o
    return T


def read_models_info(path, scale=1.0, max_sym_disc_step=0.01):
    """A BOP models_info.json -> {obj_id (int): dict(diameter, bounds (2,3) = (min, max), symmetries (S,4,4) fp64)}.
    The symmetry set is defined HERE (bop_toolkit is not a dependency and its parity is not pinned): the
    identity, every `symmetries_discrete` matrix D, and for every `symmetries_continuous` entry the rotations C_k by 2 pi k / N about
    `axis` through `offset`, k = 1..N-1, N = ceil(pi / max_sym_disc_step), alone and composed with every discrete one (C_k D).  The
    identity comes first; exact duplicates are dropped, the first kept.  Translations, bounds and the diameter are multiplied by `scale`
    (BOP models are in millimetres: scale=0.001 for metres)."""
    with open(path, "r") as fh:
        raw = json.load(fh)
    if not max_sym_disc_step > 0.0:
        raise ValueError("max_sym_disc_step must be positive")
    N = int(math.ceil(math.pi / max_sym_disc_step))
    out = {}
    for key, m in raw.items():
        disc = [np.eye(4)] + [np.asarray(d, np.float64).reshape(4, 4) for d in m.get("symmetries_discrete", [])]
        syms = list(disc)
        for c in m.get("symmetries_continuous", []):
            off = c.get("offset", [0.0, 0.0, 0.0])
            for k in range(1, N):
                Ck = _axis_rotation(c["axis"], 2.0 * math.pi * k / N, off)
                syms += [Ck @ D for D in disc]
        seen, uniq = set(), []
        for S in syms:
            S = S.copy()
            S[:3, 3] *= scale
            b = S.tobytes()
            if b not in seen:
                seen.add(b)
                uniq.append(S)
        lo = np.array([m.get("min_x", 0.0), m.get("min_y", 0.0), m.get("min_z", 0.0)], np.float64)
        size = np.array([m.get("size_x", 0.0), m.get("size_y", 0.0), m.get("size_z", 0.0)], np.float64)
        out[int(key)] = dict(diameter=float(m["diameter"]) * scale if "diameter" in m else None, bounds=np.stack([lo, lo + size]) * scale,
                             symmetries=np.stack(uniq))
    return out


def _subset(verts_dev, n):
    """indices (n') int64 on the device of the farthest-point subset of one object, first pick the vertex farthest from the origin"""
    idx = ops.farthest_points(verts_dev, n, None, -1)[0][0]
    return idx[idx >= 0].long()


def build_class_model(name, mesh, desc_net=None, ctx_net=None, neighborhood_limits=None, scale=1.0, n_eval_points=None, symmetries=None,
                      device="cuda"):
    """-> eval_epoch.ClassModel.  mesh: a path (mesh_io.load_mesh: .obj or .ply) or a dict of arrays with the keys load_mesh gives
    (`verts`, `faces`; optional `colors`, `verts_uvs`, `faces_uvs`, `texture`).  verts are multiplied by `scale` (fp32); colours are
    0.5 grey when the mesh has none; diameter = the exact largest vertex distance (ops.point_diameter); eval_points = the
    n_eval_points farthest-point vertices (None: None, the metric then uses all vertices); fea_3d / geofea_3d =
    descriptor3d.class_features(verts, desc_net, ctx_net, neighborhood_limits) when BOTH networks are given, else None; symmetries
    (S,4,4) is passed through (read_models_info)."""
    from .eval_epoch import ClassModel
    m = mesh_io.load_mesh(mesh) if isinstance(mesh, (str, os.PathLike)) else dict(mesh)
    verts = np.ascontiguousarray(np.asarray(m["verts"], np.float32).reshape(-1, 3) * np.float32(scale))
    if verts.shape[0] < 1:
        raise ValueError(f"{name}: the mesh has no vertices")
    faces = np.ascontiguousarray(np.asarray(m["faces"], np.int32).reshape(-1, 3))
    colors = m.get("colors")
    colors = np.full_like(verts, 0.5) if colors is None else np.ascontiguousarray(np.asarray(colors, np.float32))
    dev = torch.device(device)
    vd = torch.from_numpy(verts).to(dev)
    diameter = float(ops.point_diameter(vd)[1][0])
    eval_points = None
    if n_eval_points is not None:
        eval_points = verts[_subset(vd, int(n_eval_points)).cpu().numpy()]
    fea = geo = None
    if desc_net is not None and ctx_net is not None:
        from .descriptor3d import class_features
        fea, geo = class_features(vd, desc_net, ctx_net, neighborhood_limits)
    sym = None if symmetries is None else np.asarray(symmetries, np.float64).reshape(-1, 4, 4)
    return ClassModel(name=name, verts=verts, faces=faces, colors=colors, fea_3d=fea, geofea_3d=geo, diameter=diameter, eval_points=eval_points,
                      verts_uvs=m.get("verts_uvs"), faces_uvs=m.get("faces_uvs"), texture=m.get("texture"), symmetries=sym)


def fragments(verts, n, device="cuda"):
    """The reference's fragmentation_fps (utils/furthest_point_sample.py) on the device: n fragment centres by farthest-point sampling
    from the origin (ops.farthest_points, start=-1, fp64 squared distances), every vertex assigned to its nearest centre
    (rnnpose_nn_search_f32: fp32, the first minimum wins).  verts (P,3): an array or a tensor.
    -> centers (n',3) fp32, center_inds (n') int64, vert_frag_ids (P) int64 on the device; n' = min(n, pickable vertices)."""
    v = verts if isinstance(verts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(verts, np.float32)))
    v = v.to(torch.device(device), torch.float32).reshape(-1, 3).contiguous()
    inds = _subset(v, int(n))
    if inds.numel() < 1:
        raise ValueError("fragments: no vertex to pick")
    centers = v[inds].contiguous()
    ids = ops.nn_search(centers[None], v[None])[0].long()
    return centers, inds, ids
