#!/usr/bin/env python3
"""Golden answers of the convolution dispatch: what rnnpose_conv_tiles_per_image_desc / rnnpose_conv_products_desc say for a sweep of
descriptors under every rnnpose_conv_strip mode -- recorded from the library of the commit BEFORE the dispatch moved into one
plan_conv() (csrc/conv_igemm.hip), replayed by tests/test_cabi.py::test_conv_plan_answers_match_the_recorded_dispatch on the
library of every commit after it.  Host functions only: nothing is launched, no GPU needed.  Run from the repo root, on a tree whose
dispatch is the one to record:
    python tests/golden/gen_golden_conv_plan.py [path/to/librnnpose_hip.so]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "conv_plan.npz")

# the axes of the sweep, slowest first (sources: channel counts, 0 = absent)
GRID = {
    "B": np.int32([1, 2, 4, 8, 16]),
    "HW": np.int32([(8, 16), (30, 30), (31, 45), (60, 80), (120, 160), (240, 320)]),
    "K": np.int32([(1, 1), (3, 3), (1, 5), (5, 1), (1, 7), (7, 7)]),
    "stride": np.int32([1, 2]),
    "c_out": np.int32([32, 64, 126, 128, 192, 256]),                   # (96 and 512 left out: the replay stays under 10 s)
    "tile": np.arange(8, dtype=np.int32),
    "sources": np.int32([(32, 0, 0), (36, 0, 0), (64, 0, 0), (128, 0, 0), (192, 64, 0), (128, 128, 128)]),
    "norm": np.int32([0, 1]),
    "src_hl": np.int32([0, 1]),
    "single_product": np.int32([0, 1]),
}
AXES = tuple(GRID)
# (rnnpose_conv_strip mode, rnnpose_conv_spatial_tiles): every strip mode with the patch tiling on, the default mode with it off
PASSES = np.int32([(m, 1) for m in range(8)] + [(1, 0)])


def descriptors(grid):
    """-> numpy array of rnnpose_conv_desc_t, the cross product of the grid's axes in AXES order (pointers: null, or 16 where only
    null-ness is looked at)."""
    sys.path.insert(0, ROOT)
    from rnnpose_amd import _lib
    idx = np.indices([len(grid[a]) for a in AXES]).reshape(len(AXES), -1)
    ax = {a: np.asarray(grid[a])[idx[i]] for i, a in enumerate(AXES)}
    d = np.zeros(idx.shape[1], dtype=np.dtype(_lib.ConvDesc))
    d["B"], d["H"], d["W"] = ax["B"], ax["HW"][:, 0], ax["HW"][:, 1]
    d["kh"], d["kw"], d["stride"], d["c_out"], d["tile"] = ax["K"][:, 0], ax["K"][:, 1], ax["stride"], ax["c_out"], ax["tile"]
    d["n_src"] = (ax["sources"] > 0).sum(axis=1)
    for s in range(ax["sources"].shape[1]):
        d["src"]["c_count"][:, s] = ax["sources"][:, s]
        d["src"]["c_stride"][:, s] = ax["sources"][:, s]
    d["src0_mean_rstd"] = 16 * ax["norm"]
    d["src_hl"], d["single_product"] = ax["src_hl"], ax["single_product"]
    return d


def sweep(lib_path, grid, passes):
    """-> (tiles_per_image_desc, products_desc): int16 arrays (pass, descriptor).  The library's defaults are restored afterwards."""
    lib = C.CDLL(lib_path)          # (a handle of its own: raw addresses as arguments, the package's prototypes stay untouched)
    queries = [getattr(lib, n) for n in ("rnnpose_conv_tiles_per_image_desc", "rnnpose_conv_products_desc")]
    for f in queries:
        f.restype, f.argtypes = C.c_int, [C.c_void_p]
    d = descriptors(grid)
    addr = range(d.ctypes.data, d.ctypes.data + d.nbytes, d.itemsize)
    out = np.empty((2, len(passes), len(d)), np.int16)
    try:
        for k, (mode, spatial) in enumerate(passes):
            assert lib.rnnpose_conv_strip(int(mode)) == 0 and lib.rnnpose_conv_spatial_tiles(int(spatial)) == 0
            for q, f in enumerate(queries):
                out[q, k] = np.fromiter(map(f, addr), np.int16, len(d))
    finally:
        lib.rnnpose_conv_strip(1)
        lib.rnnpose_conv_spatial_tiles(1)
    return out[0], out[1]


if __name__ == "__main__":
    import time
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        sys.path.insert(0, ROOT)
        from rnnpose_amd import build
        path = build.build()
    t0 = time.time()
    tiles, products = sweep(path, GRID, PASSES)
    assert int(tiles.max()) < 2 ** 15
    np.savez_compressed(OUT, tiles_per_image_desc=tiles, products_desc=products, passes=PASSES, **{"grid_" + a: GRID[a] for a in AXES})
    print(f"wrote {OUT}: {tiles.shape[1]} descriptors x {len(PASSES)} passes in {time.time() - t0:.1f} s, {os.path.getsize(OUT)} bytes; "
          f"{int((tiles < 0).sum())} answers of -1, {int((products == 1).sum())} single-product launches")
