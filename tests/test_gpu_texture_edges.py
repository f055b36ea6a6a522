"""The COLOUR of a hit pixel (csrc/raster.hip: tex_color, sample_bilinear_border, plain_color, and the per-class tables
MeshRenderer._texture_data lays out for them) against tests/texture_ref.py (fp64) on the faces and weights of the fp64 ray caster
tests/raster_ref.py, at its edges: maps of 1 x 1, 1 x N, N x 1 and 2 x 2 texels, UVs on, next to and far beyond the border, seam
meshes (U > P, faces_uvs != faces), textured classes at non-zero table offsets in mixed batches, image sizes down to 1 x 1 with both
pixel centres, every shading with every albedo source, Phong's clamps, and the plain entry's colour.

Acceptance (texture_ref.color_bound derives it; nothing is fitted to the kernel): a CERTAIN pixel (raster_ref's mask) must match the
colour of the ray caster's face within the per-pixel bound = input term (the fp64 colour's own change under the weight error fp32
projection allows) + arithmetic term (the kernel's counted roundings, 4x margin); an UNCERTAIN pixel must match one of its candidate
faces within that face's bound, or be empty where no face surely covers it; uncertain pixels are capped at 2 % of the hit pixels of
every image.  A smooth map and a noise map go under the same bound.  Exact-arithmetic scenes (identity rotation, power-of-two focal
length and depth, dyadic vertices) need no mask: the sampler is compared bit for bit with an op-by-op fp32 statement of PyTorch's grid
sampler.  Every comparison prints err and err / bound (the largest over the image).

All cases are small (at most 64 x 80, icosphere sub 3): the whole module also runs on the host-executed kernels
(tests/test_texture_on_host.py).  Mutation record and measured figures: profiles/texture_edges_mutation.txt."""
import numpy as np
import pytest
import torch

import raster_ref as rr
import texture_ref as tr
from rnnpose_amd import synthetic as syn
from test_gpu_raster_edges import CAP, FX, Z0, camera, dev, exact_camera, npy, poses, to_object
from test_raster import icosphere

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from rnnpose_amd import build, ops as _ops
    build.build()
    return _ops


# ---- meshes, maps ----------------------------------------------------------------------------------------------------------------------
def contrast_map(Ht, Wt):
    """checker + per-channel ramps (the map of test_gpu_texture's texel-centre test): neighbouring texels differ by up to 0.8"""
    r, c = np.mgrid[0:Ht, 0:Wt]
    ch = ((r + c) % 2).astype(f32)
    return np.stack([0.1 + 0.8 * ch, 0.05 * c / Wt + 0.5 * ch, 0.9 - 0.04 * r - 0.3 * ch], -1).astype(f32)


def smooth_map(Ht=16, Wt=24):
    r, c = np.mgrid[0:Ht, 0:Wt]
    return np.stack([0.5 + 0.4 * np.sin(c / 4.0), 0.5 + 0.4 * np.cos(r / 3.0), 0.2 + 0.6 * r * c / (Ht * Wt)], -1).astype(f32)


def noise_map(Ht=13, Wt=19):
    return syn.uniform("texedges.noise", (Ht, Wt, 3), 3).astype(f32)


def seam_uvs(verts, faces, seed, extra=5):
    """A seam mesh: every odd face takes its UVs from a SECOND chart (rows P .. 2P-1, another projection of the vertices), `extra`
    rows are referenced by no face, and the rows are shuffled: U = 2P + extra > P, faces_uvs != faces on every face, and UVs vary
    across every face.  -> verts_uvs (U,2) in [0.04, 0.96], faces_uvs (F,3)"""
    P = verts.shape[0]
    rng = np.random.default_rng(seed)
    span = lambda a: (a - a.min(0)) / np.ptp(a, 0)
    uv = np.concatenate([0.05 + 0.9 * span(verts[:, :2]), 0.04 + 0.92 * span(verts[:, [2, 0]] @ np.array([[0.8, -0.6], [0.6, 0.8]])),
                         rng.uniform(0, 1, (extra, 2))])
    fuv = np.asarray(faces, np.int64).copy()
    fuv[1::2] += P
    perm = rng.permutation(uv.shape[0])
    out = np.empty_like(uv)
    out[perm] = uv
    fuv = perm[fuv]
    assert not np.any((fuv == faces).all(1))
    return out.astype(f32), fuv.astype(np.int32)


def variant(verts, faces, albedo, seed=1):
    """mesh dict with albedo from "smooth" | "noise" (textured seam mesh), "colors" or "white" """
    m = dict(verts=verts, faces=faces, colors=None)
    if albedo in ("smooth", "noise"):
        m["verts_uvs"], m["faces_uvs"] = seam_uvs(verts, faces, seed)
        m["texture"] = smooth_map() if albedo == "smooth" else noise_map()
    elif albedo == "colors":
        m["colors"] = syn.uniform("texedges.col", (verts.shape[0], 3), seed).astype(f32)
    return m


def tiny_textured():
    """a textured class that only routes a batch through the textured entry (MeshRenderer.__call__ takes it when any image is textured)"""
    v, f = icosphere(sub=0, scale=(0.05, 0.05, 0.05))
    uv, fuv = seam_uvs(v, f, 9, extra=1)
    return dict(verts=v, faces=f, colors=None, verts_uvs=uv, faces_uvs=fuv, texture=contrast_map(2, 3))


SHADE = {"none": dict(shade=False), "flat": dict(shading="flat"), "phong": dict(shading="phong")}
REF_SHADING = {"none": None, "flat": "flat", "phong": "phong"}


def draw(ren, names, G, K, size, C=0, attr=None):
    P = max(ren._vo[n][1] for n in names)
    a = torch.zeros(1, P, C, device="cuda") if attr is None else attr
    out, depth = ren(names, a, T=dev(G), K=dev(K), render_image_size=size, render_tex=True)
    assert out.shape == (len(names), 3 + (C if attr is None else a.shape[-1])) + tuple(size) and depth.shape == (len(names), 1) + tuple(size)
    return npy(out), npy(depth)[:, 0]


_REF = {}


def reference(key, mesh, G, K, H, W, pc=0.5):
    if key not in _REF:
        _REF[key] = rr.raycast(mesh["verts"], mesh["faces"], G, K, H, W, pixel_center=pc)
    return _REF[key]


# ---- acceptance ----------------------------------------------------------------------------------------------------------------------------
def compare_colour(ref, mesh, shading, got, depth, tag, arithmetic_only=False):
    """colour planes (3,H,W) and depth (H,W) of one image against one raycast() result under texture_ref.color_bound
    -> (uncertain share, err, err / bound).  arithmetic_only: an exact-arithmetic scene -- the weights are exact, no input term, no mask."""
    H, W = depth.shape
    faces = np.asarray(mesh["faces"])
    hit_k = depth > 0
    assert np.all(depth[~hit_k] == -1.0) and np.all(got[:, ~hit_k] == 0.0), tag        # colour planes exactly 0 at empty pixels
    assert np.isfinite(got).all(), tag
    c = np.ones((H, W), bool) if arithmetic_only else ref["certain"]
    h = ref["hit"]
    share = float((~c).sum()) / max(1, int(h.sum()))
    assert np.array_equal(hit_k[c], h[c]), (tag, int((hit_k != h)[c].sum()))
    g = got.reshape(3, -1)

    def within(pix, f, w):
        dw = np.zeros(f.shape) if arithmetic_only else tr.weight_slack(ref, faces, f)
        bound, col, _ = tr.color_bound(mesh, f, w, dw, shading)
        e = np.abs(g[:, pix].T - col)
        return e, e / bound
    idx = np.nonzero((c & h).ravel())[0]
    err = ratio = 0.0
    if idx.size:
        e, r = within(idx, ref["face"].ravel()[idx], ref["w"].reshape(-1, 3)[idx])
        err, ratio = float(e.max()), float(r.max())
    print(f"{tag}: hit {int(h.sum())} uncertain {share:.4f} err {err:.3e} err/bound {ratio:.3f}")
    assert ratio <= 1.0, (tag, err, ratio)
    assert share <= CAP, (tag, share)
    unc = ~c.ravel()
    if unc.any():
        cd = ref["candidates"]
        m = unc[cd["pix"]]
        pix = cd["pix"][m]
        okpix = np.zeros(H * W, bool)
        if pix.size:
            _, r = within(pix, cd["face"][m], cd["w"][m])
            np.logical_or.at(okpix, pix, (r <= 1.0).all(1) & hit_k.ravel()[pix])
        okpix |= ref["miss_ok"].ravel() & ~hit_k.ravel()
        assert np.all(okpix[unc]), (tag, "uncertain pixels that equal none of their candidates", int((~okpix)[unc].sum()))
    return share, err, ratio


# ---- a: the sampler on exact-arithmetic scenes, bit for bit ----------------------------------------------------------------------------------
def grid_sample_f32(tex, u, v):
    """PyTorch's grid sampler (bilinear, align_corners=True, padding_mode="border") on TexturesUV's flip(map, H) at (u, v) * 2 - 1, one
    fp32 operation per numpy operation: unnormalise ((g + 1) / 2) * (size - 1), clip to [0, size - 1], the four corner weights from the
    floor corner, taps outside the map contribute 0, out = nw * w_nw + ne * w_ne + sw * w_sw + se * w_se accumulated in that order."""
    m = np.asarray(tex, f32)[::-1]
    Ht, Wt = m.shape[:2]
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    gx, gy = u * f32(2) - f32(1), v * f32(2) - f32(1)
    ix = ((gx + f32(1)) / f32(2)) * f32(Wt - 1)
    iy = ((gy + f32(1)) / f32(2)) * f32(Ht - 1)
    ix = np.minimum(f32(Wt - 1), np.maximum(ix, f32(0)))
    iy = np.minimum(f32(Ht - 1), np.maximum(iy, f32(0)))
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1f, y1f = fx + f32(1), fy + f32(1)
    wnw, wne = (x1f - ix) * (y1f - iy), (ix - fx) * (y1f - iy)
    wsw, wse = (x1f - ix) * (iy - fy), (ix - fx) * (iy - fy)
    assert all(a.dtype == f32 for a in (ix, iy, wnw, wne, wsw, wse))

    def tap(y, x):
        ok = (x >= 0) & (x < Wt) & (y >= 0) & (y < Ht)
        return np.where(ok[:, None], m[np.clip(y, 0, Ht - 1), np.clip(x, 0, Wt - 1)], f32(0))
    out = tap(y0, x0) * wnw[:, None]
    out = out + tap(y0, x0 + 1) * wne[:, None]
    out = out + tap(y0 + 1, x0) * wsw[:, None]
    out = out + tap(y0 + 1, x0 + 1) * wse[:, None]
    assert out.dtype == f32
    return out


def cell_grid(H, W, x0, y0, nx, ny, step=4, pc=0.5):
    """(nx+1) x (ny+1) vertices on every `step`-th pixel centre from pixel (x0, y0), every cell split along its (0,0)-(1,1) diagonal: the
    doubled screen area of a face is step^2, a power of two, so fp32 and fp64 weights at pixel centres are the same dyadic numbers"""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    verts = to_object((x0 + step * gx + pc).ravel(), (y0 + step * gy + pc).ravel(), H, W)
    vid = lambda i, j: j * (nx + 1) + i
    faces = np.array([t for j in range(ny) for i in range(nx)
                      for t in ((vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)), (vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)))], np.int32)
    return verts, faces, gx.ravel(), gy.ravel()


def exact_weights(ref):
    """the ray caster's winners of an exact scene as fp32: face (N,), w (N,3), flat pixel index (N,)"""
    idx = np.nonzero(ref["hit"].ravel())[0]
    w = ref["w"].reshape(-1, 3)[idx]
    assert np.array_equal(w.astype(f32).astype(np.float64), w) and np.all(ref["z"].ravel()[idx] == Z0)
    return ref["face"].ravel()[idx], w.astype(f32), idx


def uv_catalogue(Ht, Wt):
    """(n,2) fp32 sample points: every texel centre; midpoints between texels in both axes (bilinear weights 1/2 and 1/4); quarter points;
    u or v exactly 0 and 1, 0 +- 2^-20, 1 +- 2^-20, and the outside values -3, -0.4, 1.3, 2.5, +-1e6 -- paired with each other, with
    every texel row and with every texel column"""
    def axis(n):
        d = max(n - 1, 1)
        cen = [i / d for i in range(n)] if n > 1 else [0.5]
        mid = [(i + 0.5) / d for i in range(max(n - 1, 1))]
        qua = [(i + 0.25) / d for i in range(max(n - 1, 1))]
        return cen, mid, qua
    e = 2.0 ** -20
    S = [0.0, 1.0, 1.0 + e, 1.0 - e, e, -e, -3.0, -0.4, 1.3, 2.5, 1e6, -1e6]
    (cu, mu, qu), (cv, mv, qv) = axis(Wt), axis(Ht)
    pts = [(a, b) for b in cv for a in cu] + [(a, b) for b in mv for a in mu] + [(a, b) for b in S for a in S]
    pts += [(a, b) for b in cv for a in S] + [(a, b) for b in S for a in cu] + [(a, b) for a, b in zip(qu * len(mv), mv * len(qu))]
    pts += [(a, b) for a, b in zip(mu * len(qv), qv * len(mu))]
    return np.array(pts, f32)


MAPS = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 9), (9, 17)]


@pytest.mark.parametrize("Ht,Wt", MAPS, ids=[f"map{a}x{b}" for a, b in MAPS])
def test_sampler_is_the_grid_sampler_bit_for_bit_on_exact_scenes(ops, Ht, Wt):
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W = 64, 80
    verts, faces, gi, gj = cell_grid(H, W, 2, 2, 19, 15)
    F = faces.shape[0]
    tex = contrast_map(Ht, Wt)
    K, G = exact_camera(H, W)
    ref = rr.raycast(verts, faces, G[0], K[0], H, W)
    face, w, idx = exact_weights(ref)
    assert idx.size == 77 * 61
    meshes = {}
    # "vary": one UV per vertex, one texel per cell, from two texels below 0: every pixel centre is a quarter-texel point -- texel centres,
    # midpoints, u and v exactly 0 and 1 and the outside on all four sides, with UVs that vary across every face (all dyadic: exact)
    uv = np.stack([(gi - 2.0) / max(Wt - 1, 1), (gj - 2.0) / max(Ht - 1, 1)], 1).astype(f32)
    meshes["vary"] = dict(verts=verts, faces=faces, colors=None, verts_uvs=uv, faces_uvs=faces, texture=tex)
    # "const k": one UV per FACE at all three corners, from the catalogue (values that are not dyadic: the interpolation rounds)
    cat = uv_catalogue(Ht, Wt)
    for k in range(-(-cat.shape[0] // F)):
        rows = cat[(k * F + np.arange(F)) % cat.shape[0]]
        meshes[f"const{k}"] = dict(verts=verts, faces=faces, colors=None, verts_uvs=rows, texture=tex,
                                   faces_uvs=np.repeat(np.arange(F, dtype=np.int32)[:, None], 3, 1))
    names = list(meshes)
    ren = MeshRenderer(meshes, shade=False)
    B = len(names)
    out, depth = draw(ren, names, np.tile(G, (B, 1, 1)), np.tile(K, (B, 1, 1)), (H, W))
    for b, n in enumerate(names):
        m = meshes[n]
        t = m["verts_uvs"][m["faces_uvs"][face]]                                # (N,3,2) fp32
        u = (w[:, 0] * t[:, 0, 0] + w[:, 1] * t[:, 1, 0]) + w[:, 2] * t[:, 2, 0]
        v = (w[:, 0] * t[:, 0, 1] + w[:, 1] * t[:, 1, 1]) + w[:, 2] * t[:, 2, 1]
        assert u.dtype == f32
        want = np.zeros((3, H * W), f32)
        want[:, idx] = grid_sample_f32(tex, u, v).T
        assert np.array_equal(depth[b] > 0, ref["hit"]) and np.all(depth[b][ref["hit"]] == Z0)
        bad = int((out[b].reshape(3, -1) != want).sum())
        print(f"sampler {Ht}x{Wt} {n}: {idx.size} pixels, {np.unique(np.stack([u, v]), axis=1).shape[1]} distinct uv, {bad} differ")
        assert np.array_equal(out[b].reshape(3, -1), want), (n, bad)
        # and the fp32 statement is torch's grid_sample: against the fp64 one to the arithmetic term
        ref64 = tr.sample_texture(tex, np.stack([u, v]).astype(np.float64)[:, None, :])[:, 0]
        assert np.abs(want[:, idx] - ref64).max() <= tr.arithmetic_bound(m, face, w, None).max()
    if Ht > 1 and Wt > 1:                                                       # the catalogue reached what it is for
        u, v = meshes["vary"]["verts_uvs"].T
        assert u.min() < 0 and u.max() > 1 and v.min() < 0 and v.max() > 1 and 0.0 in u and 1.0 in u and 0.0 in v and 1.0 in v


# ---- b: per-class tables in mixed batches -------------------------------------------------------------------------------------------------------
def four_classes():
    """constructor order: a vertex-coloured, b textured seam mesh (9 x 17), c colourless, d textured (another U, 5 x 3): no textured class
    sits at offset 0 of uv_off, tex_off or face_off"""
    va, fa = icosphere(sub=1, scale=(0.07, 0.08, 0.06))
    vb, fb = icosphere(sub=2)
    vc, fc = icosphere(sub=1, scale=(0.08, 0.05, 0.07))
    vd, fd = icosphere(sub=2, scale=(0.05, 0.09, 0.07))
    b = dict(verts=vb, faces=fb, colors=None, texture=contrast_map(9, 17))
    b["verts_uvs"], b["faces_uvs"] = seam_uvs(vb, fb, 4, extra=5)
    d = dict(verts=vd, faces=fd, colors=None, texture=contrast_map(5, 3))
    d["verts_uvs"], d["faces_uvs"] = seam_uvs(vd, fd, 5, extra=12)
    assert b["verts_uvs"].shape[0] > vb.shape[0] and d["verts_uvs"].shape[0] != b["verts_uvs"].shape[0]
    return dict(a=variant(va, fa, "colors", 6), b=b, c=dict(verts=vc, faces=fc, colors=None), d=d)


BATCHES = {"cbaadc": list("cbaadc"), "dacbca": list("dacbca")}


@pytest.mark.parametrize("shade", ["none", "flat", "phong"])
@pytest.mark.parametrize("order", list(BATCHES))
def test_mixed_batches_read_every_class_at_its_own_table_offsets(ops, order, shade):
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W, C = 37, 53, 5
    meshes = four_classes()
    names = BATCHES[order]
    B = len(names)
    ren = MeshRenderer(meshes, **SHADE[shade])
    tx = ren._tex
    assert tx["uv_off"]["b"] == 0 and tx["uv_off"]["d"] > 0 and tx["tex_off"]["d"] == 9 * 17 and ren._fo["b"][0] > 0
    K, G = camera(B, H, W), poses(B, seed=71)
    Pm = max(m["verts"].shape[0] for m in meshes.values())
    tab = syn.normal("texedges.attr", (Pm, C), 2).astype(f32)
    out, depth = draw(ren, names, G, K, (H, W), attr=dev(tab)[None])
    # depth and attribute channels equal the plain resolve's bit for bit (the two entries share everything but the colour)
    bt = ren._batch(names)
    Td, Kd = ren._tk(dev(G), dev(K))
    attr, off, Cc = ren._explicit_attr(bt, dev(tab)[None], B)
    ws = ren._raster(bt, Td, Kd, (H, W), 0.1, True)
    out_p, zb_p, _ = ren._resolve(bt, Td, Kd, (H, W), 0.1, True, ws, attr=attr, attr_off=off, Cc=Cc, want_zbuf=True)
    assert np.array_equal(out[:, 3:], npy(out_p)) and np.array_equal(depth, npy(zb_p)[:, 0])
    for b, n in enumerate(names):
        # each image == its own render outside the batch.  (An untextured class alone under flat / no shading would take the PLAIN entry,
        # whose colour is documented to differ in the last bit -- section e; a textured image behind it keeps the entry the same.)
        solo = [n] if shade == "phong" or ren.textured[n] else [n, "d"]
        one, d1 = draw(ren, solo, G[[b] * len(solo)], K[[b] * len(solo)], (H, W), attr=dev(tab)[None])
        assert np.array_equal(one[0], out[b]) and np.array_equal(d1[0], depth[b]), (b, n)
        ref = reference(("mixed", n, order, b), meshes[n], G[b], K[b], H, W)
        assert ref["hit"].mean() > 0.1
        compare_colour(ref, meshes[n], REF_SHADING[shade], out[b, :3], depth[b], f"mixed {order} {shade} image {b} ({n})")


@pytest.mark.parametrize("shade", ["none", "flat"])
def test_plain_entry_renders_a_coloured_class_in_its_colours_next_to_a_colourless_one(ops, shade):
    """Classes with and without vertex colours in one renderer, a batch without a textured image under flat shading: the plain entry
    (rnnpose_raster_resolve_f32).  The coloured class must come out in its colours and the colourless one white -- as the textured entry
    renders the same classes (its albedo table is filled per class)."""
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W = 37, 53
    meshes = four_classes()
    K, G = camera(3, H, W), poses(3, seed=72)
    names = ["a", "c", "a"]
    for ms in (meshes, {k: meshes[k] for k in "ac"}):                           # next to textured classes, and without any
        ren = MeshRenderer(ms, **SHADE[shade])
        out, depth = draw(ren, names, G, K, (H, W))
        for b, n in enumerate(names):
            ref = reference(("plainmix", n, b), meshes[n], G[b], K[b], H, W)
            compare_colour(ref, meshes[n], REF_SHADING[shade], out[b, :3], depth[b], f"plain entry {shade} image {b} ({n})")
    ren = MeshRenderer(meshes, **SHADE[shade])                                  # the two entries agree on the same images
    o_plain, d_plain = draw(ren, names, G, K, (H, W))
    o_tex, d_tex = draw(ren, names + ["b"], np.concatenate([G, G[:1]]), np.concatenate([K, K[:1]]), (H, W))
    assert np.array_equal(d_plain, d_tex[:3])
    for b, n in enumerate(names):
        ref = reference(("plainmix", n, b), meshes[n], G[b], K[b], H, W)
        idx = np.nonzero(d_plain[b].ravel() > 0)[0]
        a = tr.arithmetic_bound(meshes[n], ref["face"].ravel()[idx], ref["w"].reshape(-1, 3)[idx], REF_SHADING[shade])
        ok = ref["hit"].ravel()[idx]
        diff = np.abs(o_plain[b, :3].reshape(3, -1)[:, idx] - o_tex[b, :3].reshape(3, -1)[:, idx]).T
        assert np.all(diff[ok] <= a[ok]), (b, n, float(diff.max()))
    # a renderer whose classes all have colours keeps its table as given
    full = MeshRenderer({"a": meshes["a"]}, **SHADE[shade])
    assert torch.equal(full.colors.cpu(), torch.from_numpy(meshes["a"]["colors"])) and MeshRenderer({"c": meshes["c"]}).colors is None


# ---- c: image sizes, pixel centres, shadings, albedo sources against the ray caster ------------------------------------------------------------------
SIZES = [(1, 1, 1, 2), (7, 5, 2, 2), (37, 53, 5, 2), (64, 80, 2, 3)]


def size_scene(H, W, B, pc):
    """the scenes of test_gpu_raster_edges section 1; at 37 x 53 images 1-4 straddle a border each and a corner (the clamped box walk)"""
    K, G = camera(B, H, W, pc), poses(B, seed=H + B)
    if (H, W) == (37, 53):
        for k, (dx, dy) in enumerate(((-1, 0), (0, 1), (1, -1), (1, 0)), start=1):
            G[k, 0, 3] = dx * (W / 2.0) / K[k, 0, 0] * G[k, 2, 3]
            G[k, 1, 3] = dy * (H / 2.0) / K[k, 1, 1] * G[k, 2, 3]
    return K, G


def run_matrix(H, W, B, sub, pc, shade, albedo, entry, tag):
    """one case of the matrix through the textured entry ("tex": a textured image is appended where the batch has none) or the plain one"""
    from rnnpose_amd.rasterizer import MeshRenderer
    verts, faces = icosphere(sub=sub)
    mesh = variant(verts, faces, albedo)
    K, G = size_scene(H, W, B, pc)
    meshes, names = {"o": mesh}, ["o"] * B
    textured = "texture" in mesh
    if entry == "tex" and not textured and shade != "phong":
        meshes["t"] = tiny_textured()
        names = names + ["t"]
    ren = MeshRenderer(meshes, pixel_center=pc, **SHADE[shade])
    assert (ren._tex is None) == (entry == "plain")
    k = np.arange(len(names)) % B
    out, depth = draw(ren, names, G[k], K[k], (H, W))
    res = []
    for b in range(B):
        ref = reference(("size", H, W, B, sub, pc, b), mesh, G[b], K[b], H, W, pc)
        res.append(compare_colour(ref, mesh, REF_SHADING[shade], out[b, :3], depth[b], f"{tag} {H}x{W} pc{pc} {shade} {albedo} image {b}"))
    return out[:B], depth[:B], res


@pytest.mark.parametrize("albedo", ["smooth", "noise", "colors", "white"])
@pytest.mark.parametrize("shade", ["none", "flat", "phong"])
@pytest.mark.parametrize("pc", [0.5, 0.0], ids=["pc0.5", "pc0"])
@pytest.mark.parametrize("H,W,B,sub", SIZES, ids=[f"{s[0]}x{s[1]}-B{s[2]}" for s in SIZES])
def test_textured_entry_matches_the_ray_caster(ops, H, W, B, sub, pc, shade, albedo):
    _, depth, res = run_matrix(H, W, B, sub, pc, shade, albedo, "tex", "tex entry")
    if (H, W) == (37, 53):
        cover = (depth > 0).mean((1, 2))
        assert np.all(cover[1:] > 0.03) and np.all(cover[1:] < 0.8 * cover[0])          # partly visible: the object straddles the border
    if H >= 37 and albedo in ("smooth", "noise"):
        assert max(r[1] for r in res) > 0                                          # (something was compared)


# ---- e: the plain entry's colour ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("albedo", ["colors", "white"])
@pytest.mark.parametrize("shade", ["none", "flat"])
@pytest.mark.parametrize("pc", [0.5, 0.0], ids=["pc0.5", "pc0"])
@pytest.mark.parametrize("H,W,B,sub", SIZES, ids=[f"{s[0]}x{s[1]}-B{s[2]}" for s in SIZES])
def test_plain_entry_matches_the_ray_caster_and_tex_colors_flat_form(ops, H, W, B, sub, pc, shade, albedo):
    """plain_color (default contraction, rsqrtf) under the same reference and bound; against tex_color's flat form (op by op) on the same
    images it may differ in the last bits -- by the arithmetic term at most (each is within the COUNTED roundings of the exact value at
    the weights both share; the term is 4x the count, their difference at most 2x) -- and is not required to be equal."""
    o_p, d_p, _ = run_matrix(H, W, B, sub, pc, shade, albedo, "plain", "plain entry")
    o_t, d_t, _ = run_matrix(H, W, B, sub, pc, shade, albedo, "tex", "tex entry")
    assert np.array_equal(d_p, d_t)
    verts, faces = icosphere(sub=sub)
    mesh = variant(verts, faces, albedo)
    K, G = size_scene(H, W, B, pc)
    worst = 0.0
    for b in range(B):
        ref = reference(("size", H, W, B, sub, pc, b), mesh, G[b], K[b], H, W, pc)
        idx = np.nonzero((d_p[b] > 0).ravel() & ref["hit"].ravel())[0]
        if idx.size:
            a = tr.arithmetic_bound(mesh, ref["face"].ravel()[idx], ref["w"].reshape(-1, 3)[idx], REF_SHADING[shade])
            diff = np.abs(o_p[b, :3].reshape(3, -1)[:, idx] - o_t[b, :3].reshape(3, -1)[:, idx]).T
            worst = max(worst, float((diff / a).max()))
    print(f"plain vs tex flat form {H}x{W} pc{pc} {shade} {albedo}: largest difference / arithmetic term {worst:.3f}")
    assert worst <= 1.0


# ---- d: Phong and flat corner cases ------------------------------------------------------------------------------------------------------------------
def half_lit(alb32):
    """lit = 0.5 exactly (cos = 0): the kernel's colour is fl(fl(albedo * 0.5) + 0.2) of ITS OWN albedo, bit for bit"""
    return (alb32.astype(f32) * f32(0.5)) + f32(0.2)


def pose_facing(direction, tilt_deg, z=0.75):
    """a pose whose camera looks at the side of the object that faces -direction (object space), then tilted about the camera's x axis"""
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    a = np.cross(d, [0.0, 0.0, 1.0])
    a /= np.linalg.norm(a)
    R = np.stack([a, np.cross(d, a), d])                                        # R d = +z: the object's -d side faces the camera
    t = np.deg2rad(tilt_deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])
    G = np.eye(4)
    G[:3, :3] = Rx @ R
    assert abs(np.linalg.det(G[:3, :3]) - 1) < 1e-12
    G[:3, 3] = [0.003, -0.002, z]
    return G.astype(f32)[None]


@pytest.mark.parametrize("albedo", ["white", "noise"])
def test_phong_is_one_sided_on_the_side_facing_away_from_the_light(ops, albedo):
    """The hemisphere facing away from the object-space light (1, 1, -1), tilted by 50 degrees so that a lit crescent shows as well.
    Certain pixels whose fp64 n.l is negative by more than its own bound (the change of n.l under the weight error + the counted
    roundings of n, l and the dot product) must have lit = 0.5 EXACTLY: relu gives 0, so the colour is fl(fl(albedo * 0.5) + 0.2) of the
    kernel's own albedo (the unshaded render of the same scene), bit for bit.  Flat shading of the same scene is two-sided: brighter there."""
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W = 64, 80
    verts, faces = icosphere(sub=3)
    mesh = variant(verts, faces, albedo)
    G, K = pose_facing(tr.LIGHT, 50.0), camera(1, H, W)
    ref = reference(("dark",), mesh, G[0], K[0], H, W)
    outs = {s: draw(MeshRenderer({"o": mesh, "t": tiny_textured()}, **SHADE[s]), ["o", "t"], np.tile(G, (2, 1, 1)), np.tile(K, (2, 1, 1)), (H, W))
            for s in ("none", "flat", "phong")}
    for s in outs:
        compare_colour(ref, mesh, REF_SHADING[s], outs[s][0][0, :3], outs[s][1][0], f"dark side {albedo} {s}")
    idx = np.nonzero((ref["certain"] & ref["hit"]).ravel())[0]
    f, w = ref["face"].ravel()[idx], ref["w"].reshape(-1, 3)[idx]
    dw = tr.weight_slack(ref, faces, f)
    _, d = tr.color_at(mesh, f, w, "phong", detail=True)
    slack = np.zeros(idx.size)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for sg in (1.0, -1.0):
            wp = w.copy()
            wp[:, i] += sg * dw
            wp[:, j] -= sg * dw
            slack = np.maximum(slack, np.abs(tr.color_at(mesh, f, wp, "phong", detail=True)[1]["ndl"] - d["ndl"]))
    slack += tr.MARGIN4 * tr.EPS * (tr.K_NRM / np.minimum(1.0, d["nlen"]) + tr.K_LGT / np.minimum(1.0, d["llen"]) + tr.K_DOT)
    dark, lit = idx[d["ndl"] < -slack], idx[d["ndl"] > 0.05]
    print(f"dark side {albedo}: {idx.size} certain pixels, {dark.size} surely dark (largest slack {slack.max():.2e}), {lit.size} lit")
    assert dark.size > 0.4 * idx.size and lit.size > 0.03 * idx.size
    px = lambda s: outs[s][0][0, :3].reshape(3, -1)
    assert np.array_equal(px("phong")[:, dark], half_lit(px("none")[:, dark]))
    assert np.all(px("phong")[:, lit] > half_lit(px("none")[:, lit]))
    _, dfl = tr.color_at(mesh, f, w, "flat", detail=True)
    two_sided = idx[(d["ndl"] < -slack) & (np.abs(dfl["ndl"]) > 0.1)]
    assert two_sided.size > 0.3 * idx.size and np.all(px("flat")[:, two_sided] > px("phong")[:, two_sided] + 0.02 * px("none")[:, two_sided])


def test_vertex_normals_that_cancel_take_the_eps_clamp_and_stay_finite(ops):
    """A quad whose two faces are each present twice with opposite winding, on dyadic vertices: every vertex normal cancels to exactly 0 (in
    fp32 as in fp64), the interpolated normal is 0, the 1e-6 clamp applies: n = 0 / 1e-6, lit = 0.5 at every pixel, nothing is NaN or Inf."""
    from rnnpose_amd import rasterizer
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W = 37, 53
    verts = to_object([8.5, 40.5, 40.5, 8.5], [4.5, 4.5, 36.5, 36.5], H, W)
    faces = np.array([[0, 1, 2], [0, 2, 1], [0, 2, 3], [0, 3, 2]], np.int32)
    assert np.all(rasterizer.vertex_normals(verts, faces).numpy() == 0) and np.all(tr.vertex_normals(verts, faces) == 0)
    cols = (np.random.default_rng(1).integers(0, 65, (4, 3)) / 64.0).astype(f32)
    mesh = dict(verts=verts, faces=faces, colors=cols)
    K, G = exact_camera(H, W)
    ref = rr.raycast(verts, faces, G[0], K[0], H, W)
    assert ref["hit"].sum() == 33 * 33 and set(np.unique(ref["face"][ref["hit"]])) == {0, 2}       # ties go to the lower index
    out = {s: draw(MeshRenderer({"q": mesh}, **SHADE[s]), ["q"], G, K, (H, W)) for s in ("none", "phong")}
    hit = ref["hit"]
    assert np.array_equal(out["phong"][1][0] > 0, hit) and np.isfinite(out["phong"][0]).all()
    assert np.array_equal(out["phong"][0][0, :3][:, hit], half_lit(out["none"][0][0, :3][:, hit]))
    compare_colour(ref, mesh, "phong", out["phong"][0][0, :3], out["phong"][1][0], "zero normals", arithmetic_only=True)


def test_a_short_interpolated_normal_is_divided_by_the_eps_clamp_not_by_its_length(ops):
    """Between an exactly cancelling normal (above: 0 / 1e-6, and 0 / 0 would be swallowed by the relu's fmaxf just the same) and a
    normal of ordinary length lies 0 < |n| < 1e-6, where F.normalize(eps=1e-6) SHORTENS: n / 1e-6, not n / |n|.  Vertex normals are unit
    vectors or 0, so that needs near-cancellation across a face: the renderer's normal table is replaced by (0, 0, -1) on the quad's left
    vertices and (0, 0, 1 - 2^-19) on its right ones (the reference gets the same table).  On the pixel column midway the interpolated
    normal is (0, 0, -2^-20) = -9.54e-7 exactly (weights are multiples of 1/32, every partial sum a multiple of 2^-24 below 1), facing
    the light: cos = 0.954 |l_z| with the clamp, |l_z| without -- 0.008 of the albedo apart.  The column is held to the roundings of one
    division, l, the dot product and the final colour."""
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W = 37, 53
    verts = to_object([8.5, 40.5, 40.5, 8.5], [4.5, 4.5, 36.5, 36.5], H, W)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    s = 1.0 - 2.0 ** -19
    vn = np.array([[0, 0, -1], [0, 0, s], [0, 0, s], [0, 0, -1]], np.float64)
    mesh = dict(verts=verts, faces=faces, colors=None, _vn64=vn)
    K, G = exact_camera(H, W)
    ren = MeshRenderer({"q": mesh}, shading="phong")
    assert ren._tex["vnormals"].shape == (4, 3)
    ren._tex["vnormals"] = dev(vn.astype(f32))
    out, depth = draw(ren, ["q"], G, K, (H, W))
    ref = rr.raycast(verts, faces, G[0], K[0], H, W)
    f, w, idx = exact_weights(ref)
    col, d = tr.color_at(mesh, f, w, "phong", detail=True)
    mid = idx % W == 24                                                         # screen x = 24.5, halfway between 8.5 and 40.5
    assert mid.sum() == 33 and np.all(d["nlen"][mid] == 2.0 ** -20) and np.all(d["ndl"][mid] > 0.4) and np.all(d["ndl"][mid] < 0.7)
    tol = tr.MARGIN4 * tr.EPS * (0.3 * (2 + tr.K_LGT + tr.K_DOT) + tr.K_FIN)    # (1e-6f against 1e-6: 2.5e-9 relative, inside the division's share)
    err = np.abs(out[0, :3].reshape(3, -1)[:, idx[mid]].T - col[mid]).max()
    print(f"short normal: err {err:.3e} err/bound {err / tol:.3f}")
    assert err <= tol
    away = np.abs(idx % W - 24) >= 4                                            # |n| >= 0.24 elsewhere: the ordinary bound
    b = tr.arithmetic_bound(mesh, f[away], w[away], "phong")
    assert np.all(np.abs(out[0, :3].reshape(3, -1)[:, idx[away]].T - col[away]) <= b)


def test_unreferenced_vertex_and_zero_area_face_change_nothing_else(ops):
    """An unreferenced vertex (its normal stays 0) and zero-area faces (in front of, among and behind the others in the face list: they add
    exact zeros to the normals of their vertices and draw nothing): every image is bit-identical to the clean mesh's, under every shading."""
    from rnnpose_amd import rasterizer
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W = 37, 53
    v0, f0 = icosphere(sub=2)
    P0 = v0.shape[0]
    verts = np.concatenate([v0, [[0.01, 0.02, -0.2]]]).astype(f32)
    # (faces (i, i, j), (i, j, j), (i, i, i): one edge vector of (v2 - v1) x (v0 - v1) is exactly 0.  A face (i, j, i) crosses a vector with
    # itself, which a fused multiply-add leaves at a last-bit residue instead of 0: within the bound, not bit-identical, and not a case here.)
    faces = np.concatenate([[[3, 3, 7]], f0[:100], [[5, 9, 9]], f0[100:], [[11, 11, 11]]]).astype(np.int32)
    n_bad, n_ok = rasterizer.vertex_normals(verts, faces).numpy(), rasterizer.vertex_normals(v0, f0).numpy()
    assert np.array_equal(n_bad[:P0], n_ok) and np.all(n_bad[P0] == 0)
    want = tr.vertex_normals(verts, faces)
    assert np.abs(n_bad - want).max() <= 16 * tr.EPS and np.all(want[P0] == 0)
    cols = syn.uniform("texedges.degenerate", (P0 + 1, 3), 2).astype(f32)
    K, G = camera(2, H, W), poses(2, seed=73)
    for s in ("none", "flat", "phong"):
        clean = MeshRenderer({"o": dict(verts=v0, faces=f0, colors=cols[:P0]), "t": tiny_textured()}, **SHADE[s])
        bad = MeshRenderer({"o": dict(verts=verts, faces=faces, colors=cols), "t": tiny_textured()}, **SHADE[s])
        for names in (["o", "o"], ["o", "t"]):                                  # the plain entry (flat, none) and the textured one
            a, b = draw(clean, names, G, K, (H, W)), draw(bad, names, G, K, (H, W))
            assert (a[1][0] > 0).mean() > 0.1 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (s, names)
    ref = reference(("degenerate",), dict(verts=v0, faces=f0), G[0], K[0], H, W)
    compare_colour(ref, dict(verts=v0, faces=f0, colors=cols[:P0]), "phong", b[0][0, :3], b[1][0], "degenerate mesh phong")


def test_a_surface_point_at_the_light_is_finite_and_half_lit(ops):
    """The plane z = -1 (object space) through the light (1, 1, -1), seen fronto-parallel in an exact-arithmetic scene: the light's own
    position is the interpolated point of one pixel, strictly inside a face (weights 1/4, 1/2, 1/4), where light - p = 0 exactly.
    F.normalize(0, eps) = 0: cos = 0, lit = 0.5 under phong; the flat form multiplies 0 by rsqrt(1e-30): finite, lit = 0.5 as well."""
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W = 37, 53
    v, faces, _, _ = cell_grid(H, W, 6, 4, 8, 6)
    px, py = 6 + 4 * 3 + 2, 4 + 4 * 2 + 1                                       # pixel (20, 13): inside cell (3, 2)'s lower triangle
    off = to_object([px + 0.5], [py + 0.5], H, W)[0]                            # that pixel's object point before the shift
    verts = (v.astype(np.float64) - off + np.array([1.0, 1.0, -1.0]))
    assert np.array_equal(verts.astype(f32).astype(np.float64), verts)
    verts = verts.astype(f32)
    G = np.eye(4, dtype=f32)[None].copy()
    G[0, :3, 3] = [off[0] - 1.0, off[1] - 1.0, Z0 + 1.0]
    K, _ = exact_camera(H, W)
    cols = (np.random.default_rng(2).integers(0, 65, (verts.shape[0], 3)) / 64.0).astype(f32)
    mesh = dict(verts=verts, faces=faces, colors=cols)
    ref = rr.raycast(verts, faces, G[0], K[0], H, W)
    f, w, idx = exact_weights(ref)
    at = int(np.nonzero(idx == py * W + px)[0][0])
    assert sorted(w[at]) == [0.25, 0.25, 0.5]
    col, d = tr.color_at(mesh, f, w, "phong", detail=True)
    assert d["llen"][at] == 0.0 and np.sum(d["llen"] == 0) == 1 and d["ndl"][at] == 0.0
    out = {s: draw(MeshRenderer({"q": mesh, "t": tiny_textured()}, **SHADE[s]), ["q", "t"], np.tile(G, (2, 1, 1)), np.tile(K, (2, 1, 1)), (H, W))
           for s in ("none", "flat", "phong")}
    plain = draw(MeshRenderer({"q": mesh}, shading="flat"), ["q"], G, K, (H, W))
    for s in ("flat", "phong"):
        assert np.isfinite(out[s][0]).all()
        compare_colour(ref, mesh, s, out[s][0][0, :3], out[s][1][0], f"point at the light {s}", arithmetic_only=True)
        assert np.array_equal(out[s][0][0, :3, py, px], half_lit(out["none"][0][0, :3, py, px])), s
    compare_colour(ref, mesh, "flat", plain[0][0, :3], plain[1][0], "point at the light, plain entry", arithmetic_only=True)
    assert np.abs(plain[0][0, :3, py, px] - half_lit(out["none"][0][0, :3, py, px])).max() <= 2 * tr.EPS      # (contracted: one rounding fewer)


def test_reversed_winding_flips_phong_and_leaves_flat(ops):
    """Every face (a, b, c) -> (a, c, b), UV rows with it: coverage, depth and weights are those of the original (either winding is
    drawn).  Flat shading is two-sided: the colours agree with the original's within the two bounds.  Phong follows the vertex normals,
    which now point inwards: it matches the reference of the reversed mesh, where the lit side is the other one."""
    from rnnpose_amd.rasterizer import MeshRenderer
    H, W = 64, 80
    verts, faces = icosphere(sub=3)
    mesh = variant(verts, faces, "smooth")
    rev = dict(mesh, faces=np.ascontiguousarray(faces[:, [0, 2, 1]]), faces_uvs=np.ascontiguousarray(mesh["faces_uvs"][:, [0, 2, 1]]))
    assert np.abs(tr.vertex_normals(verts, rev["faces"]) + tr.vertex_normals(verts, faces)).max() < 1e-12
    K, G = camera(1, H, W), pose_facing(tr.LIGHT, 100.0)
    r0, r1 = reference(("wind", 0), mesh, G[0], K[0], H, W), reference(("wind", 1), rev, G[0], K[0], H, W)
    got = {}
    for s in ("flat", "phong"):
        for k, (m, r) in enumerate(((mesh, r0), (rev, r1))):
            o, dpt = draw(MeshRenderer({"o": m}, **SHADE[s]), ["o"], G, K, (H, W))
            compare_colour(r, m, s, o[0, :3], dpt[0], f"winding {s} {'reversed' if k else 'original'}")
            got[s, k] = o[0, :3].reshape(3, -1)
    idx = np.nonzero((r0["certain"] & r1["certain"] & r0["hit"]).ravel())[0]
    b0 = tr.color_bound(mesh, r0["face"].ravel()[idx], r0["w"].reshape(-1, 3)[idx], tr.weight_slack(r0, faces, r0["face"].ravel()[idx]), "flat")[0]
    b1 = tr.color_bound(rev, r1["face"].ravel()[idx], r1["w"].reshape(-1, 3)[idx], tr.weight_slack(r1, rev["faces"], r1["face"].ravel()[idx]), "flat")[0]
    assert np.all(np.abs(got["flat", 0][:, idx] - got["flat", 1][:, idx]).T <= b0 + b1)
    assert np.abs(got["phong", 0][:, idx] - got["phong", 1][:, idx]).mean() > 0.01
