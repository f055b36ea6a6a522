"""OBJ loading for MeshRenderer.from_obj: what PyTorch3D's `load_obj` / `load_objs_as_meshes` hand the reference's DiffRender
(geometry/diff_render_optim.py:104-120) for a class's `textured.obj` and its `texture_map.png`:

    m = load_obj("models/cat/textured.obj")
    m["verts"] (V,3) f32, m["faces"] (F,3) i32, m["verts_uvs"] (U,2) f32 | None, m["faces_uvs"] (F,3) i32 | None,
    m["texture"] (Ht,Wt,3) f32 | None   (texel = u8 / 255 in fp32, rows as stored in the image file: row 0 = top)

* `v` keeps its first three values, `vt` its first two; `vn` is ignored (PyTorch3D shades with normals computed from the faces).
* `f` corners are `a`, `a/b`, `a//c` or `a/b/c`, 1-based or negative (relative to the file's vertex / uv count, as PyTorch3D
  resolves them); a polygon of n > 3 corners becomes the fan (c0, ci, ci+1).  Faces must all carry `vt` or none.
* `mtllib` / `usemtl` / `map_Kd` are resolved relative to the OBJ file; as `load_objs_as_meshes`, only the map of the first
  material (in `usemtl` order) that has one is used.
Lines are parsed with regular expressions over the whole text and numpy conversions, not a Python loop per vertex.
"""
from __future__ import annotations

import os
import re

import numpy as np

_V = re.compile(r"^v[ \t]+(\S+)[ \t]+(\S+)[ \t]+(\S+)", re.M)
_VT = re.compile(r"^vt[ \t]+(\S+)(?:[ \t]+(\S+))?", re.M)
_F = re.compile(r"^f[ \t]+([^\n#]*)", re.M)
_CORNER = re.compile(r"(-?\d+)(?:/(-?\d*))?(?:/(-?\d*))?")
_MTLLIB = re.compile(r"^mtllib[ \t]+([^\n]+?)[ \t]*$", re.M)
_USEMTL = re.compile(r"^usemtl[ \t]+([^\n]+?)[ \t]*$", re.M)


def _indices(s, n, what, path):
    """OBJ index strings -> 0-based int64: i > 0 -> i - 1, i < 0 -> i + n (PyTorch3D's _format_faces_indices)."""
    i = np.asarray(s).astype(np.int64)
    if i.size and (i == 0).any():
        raise ValueError(f"{path}: {what} index 0 (OBJ indices are 1-based)")
    i = np.where(i > 0, i - 1, i + n)
    if i.size and (i.min() < 0 or i.max() >= n):
        raise ValueError(f"{path}: {what} index out of range (the file has {n})")
    return i


def _materials(path, text):
    """-> path of the first used material's map_Kd, or None."""
    d = os.path.dirname(os.path.abspath(path))
    maps = {}
    for lib in _MTLLIB.findall(text):
        mp = os.path.join(d, lib)
        if not os.path.isfile(mp):
            continue
        name = None
        with open(mp, "r", errors="replace") as fh:
            for line in fh:
                tok = line.strip().split(None, 1)
                if not tok:
                    continue
                if tok[0] == "newmtl":
                    name = tok[1].strip() if len(tok) > 1 else ""
                elif tok[0] == "map_Kd" and name is not None and len(tok) > 1:
                    maps.setdefault(name, tok[1].strip())        # (file names may hold spaces: the rest of the line)
    for name in _USEMTL.findall(text):
        f = maps.get(name)
        if f is not None and os.path.isfile(os.path.join(d, f)):
            return os.path.join(d, f)
    return None


def load_texture(path):
    """(Ht,Wt,3) fp32: PIL .convert("RGB"), u8 / 255 in fp32 (PyTorch3D's texture read)."""
    import torch
    from PIL import Image
    with Image.open(path) as im:
        u8 = np.array(im.convert("RGB"), dtype=np.uint8)
    return (torch.from_numpy(u8).float() / 255.0).numpy()


def load_obj(path):
    """-> dict(verts, faces, verts_uvs, faces_uvs, texture); see the module docstring."""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".ply":
        raise ValueError(f"{path}: .ply meshes are not supported (load_obj reads Wavefront .obj only)")
    if ext != ".obj":
        raise ValueError(f"{path}: not an .obj file")
    with open(path, "r", errors="replace") as fh:
        text = fh.read()
    v = _V.findall(text)
    verts = np.array(v, dtype=np.float64).astype(np.float32).reshape(-1, 3)
    vt = _VT.findall(text)
    uvs = None
    if vt:
        t = np.array(vt).reshape(-1, 2)
        t[t == ""] = "0"
        uvs = t.astype(np.float64).astype(np.float32)
    lines = [ln.split("#", 1)[0] for ln in _F.findall(text)]
    counts = np.fromiter(map(len, map(str.split, lines)), dtype=np.int64, count=len(lines))
    if (counts < 3).any():
        raise ValueError(f"{path}: a face with fewer than 3 corners")
    corners = _CORNER.findall(" ".join(lines))
    if len(corners) != int(counts.sum()):
        raise ValueError(f"{path}: malformed face corners")
    cv = np.array(corners).reshape(-1, 3) if corners else np.zeros((0, 3), "<U1")
    vi = _indices(cv[:, 0], verts.shape[0], "vertex", path)
    has_t = cv[:, 1] != ""
    # fan triangulation (c0, ci, ci+1) of every polygon, in file order
    start = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    ntri = counts - 2
    line = np.repeat(np.arange(len(lines)), ntri)
    k = np.arange(int(ntri.sum())) - np.repeat(np.cumsum(ntri) - ntri, ntri) + 1
    tri = np.stack([start[line], start[line] + k, start[line] + k + 1], 1) if line.size else np.zeros((0, 3), np.int64)
    faces = vi[tri].astype(np.int32)
    verts_uvs = faces_uvs = texture = None
    if has_t.any():
        if not has_t.all():
            raise ValueError(f"{path}: only some face corners carry a texture (vt) index")
        if uvs is None:
            raise ValueError(f"{path}: faces index vt but the file has no vt lines")
        ti = _indices(cv[:, 1], uvs.shape[0], "vt", path)
        verts_uvs, faces_uvs = uvs, ti[tri].astype(np.int32)
    tex_path = _materials(path, text)
    if tex_path is not None:
        if faces_uvs is None:
            raise ValueError(f"{path}: material map {os.path.basename(tex_path)} but the faces carry no vt indices")
        texture = load_texture(tex_path)
    return dict(verts=verts, faces=faces, verts_uvs=verts_uvs, faces_uvs=faces_uvs, texture=texture)
