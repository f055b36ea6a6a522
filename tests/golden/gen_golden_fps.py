#!/usr/bin/env python3
"""Golden vectors for the fragment centres from the REFERENCE's own `utils/furthest_point_sample.fragmentation_fps` (build container
only; the module needs numpy and scipy and nothing else).

    python tests/golden/gen_golden_fps.py        # writes tests/golden/fps_fragments.npz

Input: numpy.random.default_rng(0).standard_normal((300, 3)) as fp32, handed to the reference as fp64 (the test regenerates it; it is
not stored).  Stored: center_inds (64), vertex_frag_ids (300) and two margins, both asserted >= 1e-5 here:
  pick_margin    the smallest relative gap between the best and the runner-up running SQUARED distance over the 64 picks (the
                 reference compares distances; squares order alike) -- the picks do not hang on a rounding;
  assign_margin  the smallest relative gap between a vertex's nearest and second-nearest centre (squared distances) -- the fp32
                 nearest-neighbour kernel (relative rounding about 1e-7) cannot flip an assignment.
The reference's picks are also checked against tests/model_prep_ref.py, the fp64 squared-distance restatement of the kernel.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.path[:0] = [os.path.join(ROOT, "tests"), REF]

from utils.furthest_point_sample import fragmentation_fps  # noqa: E402  (the reference module)

import model_prep_ref as mr  # noqa: E402


def main():
    verts = np.random.default_rng(0).standard_normal((300, 3)).astype(np.float32)
    centers, center_inds, frag_ids = fragmentation_fps(verts.astype(np.float64), 64)
    idx, _, pick_margin = mr.fps(verts, 64, -1, want_margin=True)
    assert np.array_equal(idx, center_inds), "the reference's picks differ from the squared-distance restatement"
    assert np.array_equal(centers, verts[center_inds].astype(np.float64))
    v, c = verts.astype(np.float64), verts[center_inds].astype(np.float64)
    d = np.sort(((v[:, None] - c[None]) ** 2).sum(-1), 1)
    far = d[:, 1] > 0                                      # (a centre's own nearest distance is 0: its gap is relative to the second)
    assign_margin = float(((d[:, 1] - d[:, 0]) / d[:, 1])[far].min())
    assert np.array_equal(np.argmin(((v[:, None] - c[None]) ** 2).sum(-1), 1), frag_ids)
    assert np.array_equal(mr.fragments(verts, 64)[2], frag_ids)
    print(f"pick margin {pick_margin:.3e}, assignment margin {assign_margin:.3e}")
    assert pick_margin >= 1e-5 and assign_margin >= 1e-5
    path = os.path.join(HERE, "fps_fragments.npz")
    np.savez_compressed(path, center_inds=np.asarray(center_inds, np.int64), vertex_frag_ids=np.asarray(frag_ids, np.int64),
                        pick_margin=np.float64(pick_margin), assign_margin=np.float64(assign_margin))
    print(f"  fps_fragments.npz  {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
