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

`load_ply` reads the PLY models BOP and LINEMOD ship (the same dict plus `colors` and `normals`), `load_mesh` picks the reader by the
file's extension.
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


# ---- PLY (the format BOP and LINEMOD ship their models in), written from the format description ---------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_PLY_UV = (("texture_u", "texture_v"), ("u", "v"), ("s", "t"))


def _ply_header(path, data):
    """-> (format, [(element, count, [(property, item type, count type or None)])], comments, offset of the body)"""
    if not data.startswith(b"ply"):
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic)")
    end = data.find(b"end_header")
    nl = data.find(b"\n", end)
    if end < 0 or nl < 0:
        raise ValueError(f"{path}: truncated PLY header (no end_header line)")
    fmt, elements, comments = None, [], []
    for line in data[:end].decode("ascii", errors="replace").splitlines()[1:]:
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1] if len(tok) > 1 else ""
        elif tok[0] in ("comment", "obj_info"):
            comments.append(line.strip()[len(tok[0]):].strip())
        elif tok[0] == "element" and len(tok) == 3 and tok[2].lstrip("-").isdigit() and int(tok[2]) >= 0:
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property" and elements and len(tok) == 5 and tok[1] == "list" and tok[2] in _PLY_TYPES and tok[3] in _PLY_TYPES:
            elements[-1][2].append((tok[4], _PLY_TYPES[tok[3]], _PLY_TYPES[tok[2]]))
        elif tok[0] == "property" and elements and len(tok) == 3 and tok[1] in _PLY_TYPES:
            elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
        else:
            raise ValueError(f"{path}: PLY header line not understood: {line.strip()!r}")
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{path}: unknown PLY format {fmt!r} (ascii, binary_little_endian or binary_big_endian)")
    return fmt, elements, comments, nl + 1


def _ply_binary_element(path, data, pos, name, count, props, order):
    """One element of a binary body -> ({property: (count,) array, or for a list property (count, n) array / list of arrays}, new offset)"""
    short = ValueError(f"{path}: truncated PLY body (element {name!r})")
    lists = [p for p in props if p[2] is not None]
    if count == 0:
        return {p[0]: np.zeros((0,), order + p[1]) for p in props}, pos
    if lists:                                         # the list lengths of the first record: all records alike is the fixed-record path
        q, first = pos, {}
        for pname, item, cnt in props:
            if cnt is None:
                q += np.dtype(item).itemsize
            else:
                if q + np.dtype(cnt).itemsize > len(data):
                    raise short
                first[pname] = int(np.frombuffer(data, order + cnt, 1, q)[0])
                q += np.dtype(cnt).itemsize + first[pname] * np.dtype(item).itemsize
    fields = []
    for pname, item, cnt in props:
        if cnt is None:
            fields.append((pname, order + item))
        else:
            fields += [("#" + pname, order + cnt), (pname, order + item, (first[pname],))]
    dt = np.dtype(fields)
    if pos + dt.itemsize * count <= len(data):
        rec = np.frombuffer(data, dt, count, pos)
        if all(bool((rec["#" + p[0]] == first[p[0]]).all()) for p in lists):
            return {p[0]: rec[p[0]] for p in props}, pos + dt.itemsize * count
    elif not lists:
        raise short
    out = {p[0]: [] for p in props}                   # records of different lengths: one by one
    for _ in range(count):
        for pname, item, cnt in props:
            n = 1
            if cnt is not None:
                if pos + np.dtype(cnt).itemsize > len(data):
                    raise short
                n = int(np.frombuffer(data, order + cnt, 1, pos)[0])
                pos += np.dtype(cnt).itemsize
            if pos + n * np.dtype(item).itemsize > len(data):
                raise short
            v = np.frombuffer(data, order + item, n, pos)
            pos += n * np.dtype(item).itemsize
            out[pname].append(v if cnt is not None else v[0])
    return {p[0]: (out[p[0]] if p[2] is not None else np.asarray(out[p[0]])) for p in props}, pos


def _ply_ascii_element(path, tok, pos, name, count, props):
    short = ValueError(f"{path}: truncated PLY body (element {name!r})")
    try:
        if all(p[2] is None for p in props):
            if pos + count * len(props) > len(tok):
                raise short
            a = np.array(tok[pos:pos + count * len(props)], dtype=np.float64).reshape(count, len(props))
            return {p[0]: a[:, k] for k, p in enumerate(props)}, pos + count * len(props)
        out = {p[0]: [] for p in props}
        for _ in range(count):
            for pname, item, cnt in props:
                n = 1
                if cnt is not None:
                    if pos >= len(tok):
                        raise short
                    n = int(tok[pos])
                    pos += 1
                if n < 0 or pos + n > len(tok):
                    raise short
                v = np.array(tok[pos:pos + n], dtype=np.float64)
                pos += n
                out[pname].append(v if cnt is not None else v[0])
        return {p[0]: (out[p[0]] if p[2] is not None else np.asarray(out[p[0]])) for p in props}, pos
    except (TypeError, ValueError) as e:
        if e is short:
            raise
        raise ValueError(f"{path}: malformed number in the PLY body (element {name!r})") from None


def load_ply(path):
    """-> the dict of load_obj (verts, faces, verts_uvs, faces_uvs, texture) plus colors (V,3) fp32 in [0,1] or None and normals (V,3)
    fp32 or None.  ascii, binary_little_endian and binary_big_endian; scalar types in both spellings (float / float32, uchar / uint8 ...).
    Vertex properties: x y z; optional nx ny nz; optional red green blue (uchar -> / 255, other integers / their maximum, floats as they
    are); optional texture_u texture_v (also u v / s t) -> verts_uvs with faces_uvs = faces, the uv convention of OBJ `vt`.  A
    `comment TextureFile NAME` is read next to the file through load_texture (ignored when the file is missing or the vertices carry
    no uv).  Faces: the `vertex_indices` / `vertex_index` list of the face element, polygons as the fans (c0, ci, ci+1) in file order.
    Other elements and properties, list properties included, are skipped.  Binary elements whose lists all have one length (all
    triangles) are read as fixed records by numpy.  A truncated file, an index out of range or an unknown format: ValueError."""
    path = os.fspath(path)
    with open(path, "rb") as fh:
        data = fh.read()
    fmt, elements, comments, pos = _ply_header(path, data)
    got = {}
    if fmt == "ascii":
        tok, at = data[pos:].split(), 0
        for name, count, props in elements:
            got[name], at = _ply_ascii_element(path, tok, at, name, count, props)
    else:
        order = "<" if fmt == "binary_little_endian" else ">"
        for name, count, props in elements:
            got[name], pos = _ply_binary_element(path, data, pos, name, count, props, order)
    kinds = {name: {p[0]: p[1] for p in props} for name, _, props in elements}
    v = got.get("vertex")
    if v is None or not all(k in v for k in "xyz"):
        raise ValueError(f"{path}: the PLY file has no vertex element with x, y, z")
    col = lambda names, dt: np.stack([np.asarray(v[k]) for k in names], 1).astype(dt) if len(v["x"]) else np.zeros((0, len(names)), dt)
    verts = col("xyz", np.float32)
    V = verts.shape[0]
    normals = col(("nx", "ny", "nz"), np.float32) if all(k in v for k in ("nx", "ny", "nz")) else None
    colors = None
    if all(k in v for k in ("red", "green", "blue")):
        kind = kinds["vertex"]["red"]
        colors = col(("red", "green", "blue"), np.float32)
        if kind[0] in "iu":
            colors = colors / np.float32(np.iinfo(np.dtype(kind)).max)
    verts_uvs = next((col(pair, np.float32) for pair in _PLY_UV if all(k in v for k in pair)), None)
    f = got.get("face", {})
    key = next((k for k in ("vertex_indices", "vertex_index") if k in f), None)
    if key is None or len(f[key]) == 0:
        faces = np.zeros((0, 3), np.int32)
    else:
        rows = f[key]
        if isinstance(rows, np.ndarray):              # (F, n): every face has n corners
            n = rows.shape[1]
            if n < 3:
                raise ValueError(f"{path}: a face with fewer than 3 corners")
            r = rows.astype(np.int64)
            faces = np.stack([np.broadcast_to(r[:, :1], (len(r), n - 2)), r[:, 1:-1], r[:, 2:]], 2).reshape(-1, 3)
        else:
            if any(len(r) < 3 for r in rows):
                raise ValueError(f"{path}: a face with fewer than 3 corners")
            faces = np.concatenate([np.stack([np.full(len(r) - 2, r[0]), r[1:-1], r[2:]], 1).astype(np.int64) for r in rows])
        if faces.size and (faces.min() < 0 or faces.max() >= V):
            raise ValueError(f"{path}: face index out of range (the file has {V} vertices)")
        faces = faces.astype(np.int32)
    texture = None
    name = next((c.split(None, 1)[1].strip() for c in comments if c.split(None, 1)[0:1] == ["TextureFile"] and len(c.split(None, 1)) > 1), None)
    if name is not None and verts_uvs is not None and os.path.isfile(os.path.join(os.path.dirname(os.path.abspath(path)), name)):
        texture = load_texture(os.path.join(os.path.dirname(os.path.abspath(path)), name))
    return dict(verts=verts, faces=faces, verts_uvs=verts_uvs, faces_uvs=faces.copy() if verts_uvs is not None else None, texture=texture,
                colors=colors, normals=normals)


def load_mesh(path):
    """load_obj or load_ply by the file's extension; a mesh from an .obj file carries colors = normals = None."""
    ext = os.path.splitext(os.fspath(path))[1].lower()
    if ext == ".ply":
        return load_ply(path)
    if ext == ".obj":
        return dict(load_obj(path), colors=None, normals=None)
    raise ValueError(f"{os.fspath(path)}: neither an .obj nor a .ply file")
