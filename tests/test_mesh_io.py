"""rnnpose_amd.mesh_io.load_obj on tiny OBJ / MTL / PNG files: what PyTorch3D's load_obj / load_objs_as_meshes hand the
reference's DiffRender (fan triangulation, 1-based and negative indices, corner forms, material map, texel conversion)."""
import numpy as np
import pytest
import torch

from rnnpose_amd.mesh_io import load_obj

QUAD = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 0.5 1 7\n"


def write(p, text):
    p.write_text(text)
    return str(p)


def png(p, u8):
    from PIL import Image
    Image.fromarray(u8).save(p)


def test_quads_become_fans_and_vertices_keep_three_values(tmp_path):
    m = load_obj(write(tmp_path / "a.obj", QUAD + "f 1 2 3 4\nf 1 2 5\n# comment\nf 2 3 4 5 1\n"))
    assert m["verts"].dtype == np.float32 and m["verts"].shape == (5, 3)
    assert np.array_equal(m["verts"][4], np.float32([0.5, 0.5, 1.0]))
    assert m["faces"].dtype == np.int32
    assert m["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 3], [1, 3, 4], [1, 4, 0]]
    assert m["verts_uvs"] is None and m["faces_uvs"] is None and m["texture"] is None


def test_negative_indices_and_corner_forms(tmp_path):
    text = QUAD + "vt 0 0\nvt 1 0 0.5\nvt 1 1\nvn 0 0 1\nf -5/-3/1 -4/-2/1 -3/-1/1\nf 1/1 3/3 4/2\n"
    m = load_obj(write(tmp_path / "b.obj", text))
    assert m["faces"].tolist() == [[0, 1, 2], [0, 2, 3]]
    assert m["faces_uvs"].tolist() == [[0, 1, 2], [0, 2, 1]]
    assert np.array_equal(m["verts_uvs"], np.float32([[0, 0], [1, 0], [1, 1]]))        # vt keeps its first two values
    m = load_obj(write(tmp_path / "c.obj", QUAD + "f 1//1 2//1 3//1\n"))                  # a//c: no texture index
    assert m["faces"].tolist() == [[0, 1, 2]] and m["faces_uvs"] is None


def test_mixed_vt_and_bad_indices_raise(tmp_path):
    with pytest.raises(ValueError, match="only some"):
        load_obj(write(tmp_path / "d.obj", QUAD + "vt 0 0\nvt 1 0\nvt 1 1\nf 1/1 2/2 3/3\nf 1 3 4\n"))
    with pytest.raises(ValueError, match="out of range"):
        load_obj(write(tmp_path / "e.obj", QUAD + "f 1 2 9\n"))
    with pytest.raises(ValueError, match="1-based"):
        load_obj(write(tmp_path / "f.obj", QUAD + "f 0 1 2\n"))


def test_ply_and_other_files_are_rejected(tmp_path):
    with pytest.raises(ValueError, match=r"\.ply"):
        load_obj(write(tmp_path / "m.ply", "ply\n"))
    with pytest.raises(ValueError):
        load_obj(write(tmp_path / "m.stl", "solid\n"))


def test_material_map_is_resolved_relative_to_the_obj_and_texels_are_u8_over_255(tmp_path, monkeypatch):
    sub = tmp_path / "models" / "cat"
    (sub / "maps").mkdir(parents=True)
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    png(sub / "maps" / "tex one.png", u8)
    other = rng.integers(0, 256, (3, 3, 3), dtype=np.uint8)
    png(sub / "maps" / "other.png", other)
    write(sub / "mat.mtl", "newmtl unused\nmap_Kd maps/other.png\nnewmtl skin\nKd 1 1 1\nmap_Kd maps/tex one.png\n"
                           "newmtl second\nmap_Kd maps/other.png\n")
    obj = write(sub / "textured.obj", "mtllib mat.mtl\n" + QUAD + "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
                                      "usemtl skin\nf 1/1 2/2 3/3 4/4\nusemtl second\nf 1/1 2/2 5/3\n")
    monkeypatch.chdir(tmp_path)                                      # paths must not depend on the working directory
    m = load_obj(obj)
    want = u8.astype(np.float32) / np.float32(255.0)
    assert m["texture"].dtype == np.float32 and m["texture"].shape == (5, 7, 3)
    assert np.array_equal(m["texture"], want)                        # bit-equal to u8 / 255 in fp32, rows as in the file
    assert np.array_equal(m["texture"], (torch.from_numpy(u8) / 255.0).numpy())
    assert m["faces_uvs"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2]]


def test_texture_without_vt_raises(tmp_path):
    png(tmp_path / "t.png", np.zeros((2, 2, 3), np.uint8))
    write(tmp_path / "t.mtl", "newmtl a\nmap_Kd t.png\n")
    with pytest.raises(ValueError, match="no vt"):
        load_obj(write(tmp_path / "t.obj", "mtllib t.mtl\nusemtl a\n" + QUAD + "f 1 2 3\n"))


def test_rgba_and_grey_maps_convert_to_rgb(tmp_path):
    from PIL import Image
    g = np.arange(12, dtype=np.uint8).reshape(3, 4) * 20
    Image.fromarray(g, mode="L").save(tmp_path / "g.png")
    write(tmp_path / "g.mtl", "newmtl a\nmap_Kd g.png\n")
    m = load_obj(write(tmp_path / "g.obj", "mtllib g.mtl\nusemtl a\n" + QUAD + "vt 0 0\nf 1/1 2/1 3/1\n"))
    assert m["texture"].shape == (3, 4, 3)
    assert np.array_equal(m["texture"][..., 1], g.astype(np.float32) / np.float32(255.0))
