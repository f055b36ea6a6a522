#!/usr/bin/env python3
"""Golden vectors of the 2-D descriptor network, from the REFERENCE's own model/descriptor2D.py:SuperPoint2D on the CPU
(build container only).

    python tests/golden/gen_golden_desc2d.py      # writes tests/golden/desc2d.npz

Shims (the module imports packages this image lacks): an attribute-dict for `easydict`; a stub `torchplus.nn.modules.common`
exposing `Empty` (importing the real torchplus pulls in numba and collections.Iterable); torch.load returning {} while the
module is constructed (it reads weights/superpoint_v1.pth, which ships with neither project).  Weights come from
synthetic.make_module_weights (kaiming gain 1, seed 4), images from synthetic.uniform: the fixture holds the reference's
OUTPUTS (scores at every pixel, descriptors on the pixel lattice of descriptor_sample) and the state_dict key list only.

    case a: B = 2, 3 x 64 x 96   the main comparison
    case b: B = 1, 3 x 40 x 56   the 1/8-resolution map is 5 x 7: the up-sampling's edge clamp on odd sizes
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.path[:0] = [ROOT, REF]
warnings.filterwarnings("ignore")

from rnnpose_amd import synthetic as syn  # noqa: E402

CONFIG = dict(input_dim=3, descriptor_dim=32, normalize_output=True, use_instance_norm=True,
              saliency_score_normalization_fuc="sigmoid")        # config/linemod/template_fw0.5.yml:27-31
SEED = 4
CASES = {"a": (2, 64, 96), "b": (1, 40, 56)}


class AttrDict(dict):
    __getattr__ = dict.__getitem__

    def __setattr__(self, k, v):
        self[k] = v


def reference_module():
    ed = types.ModuleType("easydict")
    ed.EasyDict = AttrDict
    sys.modules["easydict"] = ed
    names = ["torchplus", "torchplus.nn", "torchplus.nn.modules", "torchplus.nn.modules.common"]
    for n in names:
        sys.modules[n] = types.ModuleType(n)

    class Empty(torch.nn.Module):
        def forward(self, *args, **kwargs):
            return args[0] if len(args) == 1 else args

    sys.modules["torchplus.nn.modules.common"].Empty = Empty
    from model.descriptor2D import SuperPoint2D
    load = torch.load
    torch.load = lambda *a, **k: {}
    try:
        net = SuperPoint2D(AttrDict(CONFIG))
    finally:
        torch.load = load
    return net.eval()


def weights(shapes):
    return syn.make_module_weights(shapes, seed=SEED)


def image(case):
    return syn.uniform(f"desc2d_img_{case}", (CASES[case][0], 3) + CASES[case][1:], SEED)


# The fixture keeps the scores at every pixel and the descriptors (32 channels) on a pixel lattice that includes the last row and
# column (where the up-sampling's edge clamp acts): every 4th pixel in case a, every 2nd in case b -- it stays small.
STEP = {"a": 4, "b": 2}


def lattice(n, step):
    idx = list(range(0, n, step))
    return idx + [n - 1] if idx[-1] != n - 1 else idx


def descriptor_sample(case, d):
    """(B, D, H, W) -> the descriptors the fixture stores for `case`: (B, D, len(rows), len(cols))."""
    _, h, w = CASES[case]
    return d[:, :, lattice(h, STEP[case])][:, :, :, lattice(w, STEP[case])]


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    net = reference_module()
    sd = net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights(shapes).items()}, strict=True)
    out = {"keys": np.array(sorted(shapes))}
    with torch.no_grad():
        for case in CASES:
            r = net(torch.from_numpy(image(case)))
            out[f"{case}_descriptors"] = descriptor_sample(case, r["descriptors"].float().numpy())
            out[f"{case}_scores"] = r["scores"].float().numpy()
    path = os.path.join(HERE, "desc2d.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
