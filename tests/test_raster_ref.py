"""tests/raster_ref.py (the fp64 ray caster the GPU tests of the rasteriser compare against) tied to oracle/raster_oracle.py, the
restatement of the kernel's algorithm the project already trusts, on the scene of tests/test_raster.py -- and the share of pixels its
certainty mask sets aside, which the GPU tests cap."""
import numpy as np
import pytest

import raster_ref as rr
from oracle import raster_oracle as ro
from test_raster import icosphere, scene


@pytest.mark.parametrize("perspective", [True, False])
def test_ray_caster_agrees_with_the_scan_converting_oracle(perspective):
    B, H, W = 2, 128, 160
    verts, faces, K, G = scene(B)
    for b in range(B):
        f, z, w, vz = ro.rasterize(verts, faces, G[b], K[b], H, W, perspective=perspective)
        r = rr.raycast(verts, faces, G[b], K[b], H, W, perspective=perspective)
        c, h = r["certain"], r["hit"]
        assert h.mean() > 0.15
        assert np.array_equal(r["face"][c], f[c])                               # the same face wherever no edge is within delta
        assert np.all((r["face"] == f) | ~c) and (r["face"] != f).sum() <= 2    # (both fp64: they may part only ON an edge)
        same = r["face"] == f
        assert np.abs(r["z"] - z)[same].max() < 1e-12 and np.abs(r["w"] - w)[same].max() < 1e-9
        assert np.array_equal(r["vz"][same & r["vd_certain"]], vz[same & r["vd_certain"]])
        assert (~c).sum() <= 0.02 * h.sum() and (~r["vd_certain"]).sum() <= 0.05 * h.sum()


def test_uncertain_share_stays_small_on_the_finer_meshes():
    """delta grows with the image and the edge density with the mesh: the reference alone stays inside the caps of the GPU tests"""
    for sub, (H, W) in ((4, (240, 320)),):
        verts, faces = icosphere(sub=sub)
        _, _, K, G = scene(1)
        K = K.copy()
        K[:, :2] *= W / 160.0
        r = rr.raycast(verts, faces, G[0], K[0], H, W)
        assert (~r["certain"]).sum() <= 0.02 * r["hit"].sum() and (~r["vd_certain"]).sum() <= 0.05 * r["hit"].sum()
