"""mesh_io.load_ply / load_mesh and model_prep.read_models_info on files the tests write themselves (CPU only)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rnnpose_amd import mesh_io  # noqa: E402

NUMPY = {"float": "f4", "float32": "f4", "double": "f8", "float64": "f8", "uchar": "u1", "uint8": "u1", "int": "i4", "int32": "i4", "uint": "u4",
         "ushort": "u2", "short": "i2", "char": "i1"}


def write_ply(path, fmt, vertex_props, vertex_rows, faces, face_decl=("uchar", "int", "vertex_indices"), comments=(), extra_elements=(),
              face_extra=None, cut=None):
    """vertex_props: [(type, name)], vertex_rows (V, len(props)); faces: lists of indices; extra_elements: [(header lines, rows as
    lists of (type, value) or (count type, item type, values))] written between the vertices and the faces; face_extra: an extra
    list property (count type, item type, name, rows) in front of the indices; cut: drop that many bytes from the end."""
    order = {"ascii": None, "binary_little_endian": "<", "binary_big_endian": ">"}[fmt]
    head = ["ply", f"format {fmt} 1.0"] + [f"comment {c}" for c in comments] + [f"element vertex {len(vertex_rows)}"]
    head += [f"property {t} {n}" for t, n in vertex_props]
    for lines, _ in extra_elements:
        head += lines
    head.append(f"element face {len(faces)}")
    if face_extra is not None:
        head.append(f"property list {face_extra[0]} {face_extra[1]} {face_extra[2]}")
    head += [f"property list {face_decl[0]} {face_decl[1]} {face_decl[2]}", "end_header"]
    body = bytearray()

    def put(t, v):
        nonlocal body
        if order is None:
            body += (repr(float(v)) if NUMPY[t][0] == "f" else str(int(v))).encode() + b" "
        else:
            body += np.asarray(v).astype(order + NUMPY[t]).tobytes()

    def end_row():
        nonlocal body
        if order is None:
            body += b"\n"
    for row in vertex_rows:
        for (t, _), v in zip(vertex_props, row):
            put(t, v)
        end_row()
    for _, rows in extra_elements:
        for row in rows:
            for field in row:
                if len(field) == 2:
                    put(*field)
                else:
                    put(field[0], len(field[2]))
                    for v in field[2]:
                        put(field[1], v)
            end_row()
    for k, f in enumerate(faces):
        if face_extra is not None:
            put(face_extra[0], len(face_extra[3][k]))
            for v in face_extra[3][k]:
                put(face_extra[1], v)
        put(face_decl[0], len(f))
        for v in f:
            put(face_decl[1], v)
        end_row()
    data = ("\n".join(head) + "\n").encode("ascii") + bytes(body)
    with open(path, "wb") as fh:
        fh.write(data if cut is None else data[:-cut])


RNG = np.random.default_rng(0)
XYZ = RNG.standard_normal((6, 3)).astype(np.float32)
NRM = RNG.standard_normal((6, 3)).astype(np.float32)
RGB = RNG.integers(0, 256, (6, 3))
UV = RNG.random((6, 2)).astype(np.float32)
TRIS = [[0, 1, 2], [2, 3, 4], [5, 4, 0]]
MIXED = [[0, 1, 2], [2, 3, 4, 5], [5, 4, 0], [0, 1, 2, 3, 4]]
FAN = [[0, 1, 2], [2, 3, 4], [2, 4, 5], [5, 4, 0], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
FORMATS = ["ascii", "binary_little_endian", "binary_big_endian"]


@pytest.mark.parametrize("spelling", ["short", "sized"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_all_properties_in_every_format_and_spelling(tmp_path, fmt, spelling):
    f32, u8, i32 = ("float", "uchar", "int") if spelling == "short" else ("float32", "uint8", "int32")
    props = [(f32, n) for n in ("x", "y", "z", "nx", "ny", "nz")] + [(u8, n) for n in ("red", "green", "blue")] + [(u8, "alpha")] + \
        [(f32, "texture_u"), (f32, "texture_v")]
    rows = np.concatenate([XYZ, NRM, RGB, np.full((6, 1), 255), UV], 1)
    p = str(tmp_path / "m.ply")
    write_ply(p, fmt, props, rows, MIXED, face_decl=(u8, i32, "vertex_indices"))
    m = mesh_io.load_ply(p)
    assert m["verts"].dtype == np.float32 and np.array_equal(m["verts"], XYZ) and np.array_equal(m["normals"], NRM)
    assert m["colors"].dtype == np.float32 and np.array_equal(m["colors"], RGB.astype(np.float32) / np.float32(255))
    assert np.array_equal(m["verts_uvs"], UV) and np.array_equal(m["faces_uvs"], m["faces"]) and m["texture"] is None
    assert m["faces"].dtype == np.int32 and m["faces"].tolist() == FAN
    assert set(m) == {"verts", "faces", "verts_uvs", "faces_uvs", "texture", "colors", "normals"}


@pytest.mark.parametrize("fmt", FORMATS)
def test_bare_file_float_colours_and_alternative_names(tmp_path, fmt):
    p = str(tmp_path / "bare.ply")
    write_ply(p, fmt, [("float", n) for n in "xyz"], XYZ, TRIS, face_decl=("uchar", "uint", "vertex_index"))
    m = mesh_io.load_ply(p)
    assert np.array_equal(m["verts"], XYZ) and m["faces"].tolist() == TRIS
    assert m["colors"] is None and m["normals"] is None and m["verts_uvs"] is None and m["faces_uvs"] is None and m["texture"] is None
    col = RNG.random((6, 3)).astype(np.float32)
    for names in (("u", "v"), ("s", "t")):
        write_ply(p, fmt, [("double", n) for n in "xyz"] + [("float", n) for n in ("red", "green", "blue")] + [("float", n) for n in names],
                  np.concatenate([XYZ, col, UV], 1), TRIS, face_decl=("int", "short", "vertex_indices"))
        m = mesh_io.load_ply(p)
        assert np.array_equal(m["verts"], XYZ) and np.array_equal(m["colors"], col) and np.array_equal(m["verts_uvs"], UV)      # floats as they are
    write_ply(p, fmt, [("float", n) for n in "xyz"], XYZ, [])                                                             # a point cloud
    assert mesh_io.load_ply(p)["faces"].shape == (0, 3)


@pytest.mark.parametrize("fmt", FORMATS)
def test_triangle_fast_path_equals_the_general_path(tmp_path, fmt):
    """The same triangles once as an all-triangle file (fixed records in the binary formats) and once behind a leading quad that forces
    the record-by-record path."""
    big = RNG.standard_normal((500, 3)).astype(np.float32)
    tris = RNG.integers(0, 500, (300, 3)).tolist()
    a, b = str(tmp_path / "tri.ply"), str(tmp_path / "mixed.ply")
    write_ply(a, fmt, [("float", n) for n in "xyz"], big, tris)
    write_ply(b, fmt, [("float", n) for n in "xyz"], big, [[0, 1, 2, 3]] + tris)
    fa, fb = mesh_io.load_ply(a)["faces"], mesh_io.load_ply(b)["faces"]
    assert fa.tolist() == tris and fb[:2].tolist() == [[0, 1, 2], [0, 2, 3]] and np.array_equal(fb[2:], fa)
    quads = RNG.integers(0, 500, (50, 4))
    write_ply(a, fmt, [("float", n) for n in "xyz"], big, quads.tolist())                                                  # all quads: fixed records too
    want = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3)
    assert np.array_equal(mesh_io.load_ply(a)["faces"], want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_other_elements_and_list_properties_are_skipped(tmp_path, fmt):
    edge = (["element edge 2", "property int vertex1", "property int vertex2", "property uchar flag"],
            [[("int", 0), ("int", 1), ("uchar", 7)], [("int", 1), ("int", 2), ("uchar", 9)]])
    strips = (["element tristrips 2", "property list int int strip", "property float weight"],
              [[("int", "int", [0, 1, 2, -1, 3]), ("float", 0.5)], [("int", "int", []), ("float", 1.5)]])
    p = str(tmp_path / "extra.ply")
    write_ply(p, fmt, [("float", n) for n in "xyz"] + [("float", "quality")], np.concatenate([XYZ, np.ones((6, 1))], 1), MIXED,
              extra_elements=[edge, strips], face_extra=("uchar", "float", "texcoord", [[0.1] * 6, [0.2] * 8, [], [0.3] * 10]),
              comments=["made by hand", "TextureFile missing.png"])
    m = mesh_io.load_ply(p)
    assert np.array_equal(m["verts"], XYZ) and m["faces"].tolist() == FAN and m["texture"] is None


def test_texture_file_comment(tmp_path):
    from PIL import Image
    px = np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [51, 102, 204]]], np.uint8)
    Image.fromarray(px).save(str(tmp_path / "tex map.png"))
    p = str(tmp_path / "t.ply")
    props = [("float", n) for n in "xyz"] + [("float", "texture_u"), ("float", "texture_v")]
    write_ply(p, "binary_little_endian", props, np.concatenate([XYZ, UV], 1), TRIS, comments=["TextureFile tex map.png"])
    m = mesh_io.load_ply(p)
    assert m["texture"].dtype == np.float32 and np.array_equal(m["texture"], px.astype(np.float32) / np.float32(255))
    assert np.array_equal(m["texture"], mesh_io.load_texture(str(tmp_path / "tex map.png")))
    write_ply(p, "ascii", [("float", n) for n in "xyz"], XYZ, TRIS, comments=["TextureFile tex map.png"])                  # no uv: no texture
    assert mesh_io.load_ply(p)["texture"] is None


def test_value_errors_name_the_file(tmp_path):
    p = str(tmp_path / "broken.ply")
    xyz = [("float", n) for n in "xyz"]

    def refused(what):
        with pytest.raises(ValueError) as e:
            mesh_io.load_ply(p)
        assert "broken.ply" in str(e.value), what
    for fmt in FORMATS:
        write_ply(p, fmt, xyz, XYZ, MIXED, cut=3)                                   # truncated in the faces (mixed: record by record)
        refused("cut faces")
        write_ply(p, fmt, xyz, XYZ, TRIS, cut=5)                                    # ... in the fixed-record path
        refused("cut triangles")
        write_ply(p, fmt, xyz, XYZ, [], cut=30)                                     # ... in the vertices
        refused("cut vertices")
        write_ply(p, fmt, xyz, XYZ, [[0, 1, 6]])                                    # an index out of range
        refused("index 6")
        write_ply(p, fmt, xyz, XYZ, [[0, -1, 2]])
        refused("index -1")
        write_ply(p, fmt, xyz, XYZ, [[0, 1]])                                       # a face of two corners
        refused("two corners")
    write_ply(p, "binary_big_endian", xyz, XYZ, TRIS)
    assert mesh_io.load_ply(p)["faces"].tolist() == TRIS                            # (a good file, then one flaw at a time)
    good = open(p, "rb").read()
    for old, new in ((b"format binary_big_endian 1.0", b"format binary_middle_endian 1.0"), (b"ply\n", b"plx\n"), (b"end_header\n", b""),
                     (b"property float x", b"property quad x"), (b"property float x\n", b"")):
        assert old in good
        open(p, "wb").write(good.replace(old, new, 1))
        refused(new)
    open(p, "wb").write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 two 3\n")
    refused("a word for a number")


def test_load_mesh_dispatches_on_the_extension(tmp_path):
    p = str(tmp_path / "a.PLY")
    write_ply(p, "ascii", [("float", n) for n in "xyz"], XYZ, TRIS)
    assert np.array_equal(mesh_io.load_mesh(p)["verts"], XYZ)
    o = str(tmp_path / "a.obj")
    with open(o, "w") as fh:
        fh.write("".join(f"v {x!r} {y!r} {z!r}\n" for x, y, z in XYZ.astype(np.float64).tolist()) + "f 1 2 3\n")
    m = mesh_io.load_mesh(o)
    assert np.array_equal(m["verts"], XYZ) and m["faces"].tolist() == [[0, 1, 2]] and m["colors"] is None and m["normals"] is None
    with pytest.raises(ValueError):
        mesh_io.load_mesh(str(tmp_path / "a.stl"))
    with pytest.raises(ValueError):                                                # load_obj keeps refusing .ply
        mesh_io.load_obj(p)


def test_read_models_info(tmp_path):
    from rnnpose_amd.model_prep import read_models_info
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])
    flip[:3, 3] = [10.0, 0.0, 0.0]
    info = {"1": dict(diameter=100.0, min_x=-10.0, min_y=-20.0, min_z=-30.0, size_x=20.0, size_y=40.0, size_z=60.0),
            "2": dict(diameter=50.0, min_x=0.0, min_y=0.0, min_z=0.0, size_x=1.0, size_y=1.0, size_z=1.0, symmetries_discrete=[flip.reshape(-1).tolist()]),
            "3": dict(diameter=80.0, min_x=0.0, min_y=0.0, min_z=0.0, size_x=1.0, size_y=1.0, size_z=1.0,
                      symmetries_continuous=[dict(axis=[0, 0, 1], offset=[5.0, 0.0, 0.0])],
                      symmetries_discrete=[np.diag([1.0, -1.0, -1.0, 1.0]).reshape(-1).tolist()])}
    p = str(tmp_path / "models_info.json")
    with open(p, "w") as fh:
        json.dump(info, fh)
    r = read_models_info(p, scale=0.001, max_sym_disc_step=0.1)
    assert sorted(r) == [1, 2, 3]
    assert r[1]["diameter"] == 100.0 * 0.001 and np.array_equal(r[1]["symmetries"], np.eye(4)[None]) and r[1]["symmetries"].dtype == np.float64
    assert np.allclose(r[1]["bounds"], [[-0.01, -0.02, -0.03], [0.01, 0.02, 0.03]], rtol=0, atol=1e-15)
    assert r[2]["symmetries"].shape == (2, 4, 4) and np.array_equal(r[2]["symmetries"][0], np.eye(4))
    want = flip.copy()
    want[:3, 3] *= 0.001                                                            # scale: the translation, not the rotation
    assert np.array_equal(r[2]["symmetries"][1], want)
    N = int(np.ceil(np.pi / 0.1))
    S = r[3]["symmetries"]
    assert N == 32 and S.shape == (N * 2, 4, 4) and np.array_equal(S[0], np.eye(4)) and r[3]["diameter"] == 80.0 * 0.001
    assert len({s.tobytes() for s in S}) == len(S)
    axis, on_axis = np.array([0.0, 0.0, 1.0]), np.array([5.0, 0.0, 0.0]) * 0.001
    for s in S:
        R, t = s[:3, :3], s[:3, 3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1.0) < 1e-12 and np.array_equal(s[3], [0, 0, 0, 1])
        # the axis line maps onto itself: its direction up to sign, and a point of it stays on it
        assert np.allclose(np.abs(R @ axis), axis, atol=1e-12)
        moved = R @ on_axis + t - on_axis
        assert np.allclose(np.cross(moved, axis), 0.0, atol=1e-12)
    angles = sorted(round(float(np.degrees(np.arctan2(s[1, 0], s[0, 0]))) % 360.0, 6) for s in S[2::2])      # the pure rotations C_k
    assert np.allclose(angles, np.arange(1, N) * 360.0 / N, atol=1e-6)
    same = read_models_info(p, scale=1.0, max_sym_disc_step=0.1)[3]["symmetries"]
    assert np.array_equal(same[:, :3, :3], S[:, :3, :3]) and np.allclose(same[:, :3, 3] * 0.001, S[:, :3, 3], rtol=0, atol=1e-18)
    full = read_models_info(p)[3]["symmetries"]
    assert full.shape[0] == 2 * int(np.ceil(np.pi / 0.01))
