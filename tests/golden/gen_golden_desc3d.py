#!/usr/bin/env python3
"""Golden vectors of the 3-D descriptor / context network, from the REFERENCE's own model/descriptor3D.py:KPSuperpoint3Dv2 on
the CPU (build container only).

    python tests/golden/gen_golden_desc3d.py      # writes tests/golden/desc3d.npz

Shims: an attribute-dict for `easydict`; the reference's thirdparty/ directory on sys.path so that `kpconv.*` resolves;
kpconv_blocks.load_kernels replaced by zeros while the modules are built (it optimises a disposition and writes it under the
working directory; the kernel points are parameters and are loaded below).  The pyramids come from tests/desc3d_fp64.np_pyramid
(a numpy restatement of the collate: the reference's C++ extensions are not built here); weights and kernel points from
tests/desc3d_fp64.make_weights (the project's seeded generators).  The fixture holds the pyramid, both networks' outputs and the
state_dict key list.

    case a: one cloud of 2000 points, no truncation
    case b: two stacked, overlapping clouds of 700 and 450 points (shared norm statistics, per-cloud searches), limits that truncate

To keep the file small the outputs are stored on a lattice of rows (`desc3d_fp64.output_rows`: every 8th row for the descriptors, every 32nd
for the 256-channel context features, the last row included; both clouds of case b are covered), and the index tables as int16.
The GPU tests compare every row at 20 000 points against the fp64 restatement.
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), REF, os.path.join(REF, "thirdparty")]
warnings.filterwarnings("ignore")

import desc3d_fp64 as R  # noqa: E402

LIMITS_B = [9, 11, 12, 12]

def table(a):
    assert a.max() < 2 ** 15
    return a.astype(np.int16)


class AttrDict(dict):
    __getattr__ = dict.__getitem__

    def __setattr__(self, k, v):
        self[k] = v


def reference_net(cfg, seed):
    ed = types.ModuleType("easydict")
    ed.EasyDict = AttrDict
    sys.modules["easydict"] = ed
    import kpconv.kpconv_blocks as kb
    from model.descriptor3D import KPSuperpoint3Dv2
    load = kb.load_kernels
    kb.load_kernels = lambda radius, K, dimension, fixed, lloyd=False: np.zeros((K, dimension), np.float32)
    try:
        net = KPSuperpoint3Dv2(AttrDict(cfg))
    finally:
        kb.load_kernels = load
    sd = net.state_dict()
    w = R.make_weights({k: tuple(v.shape) for k, v in sd.items()}, cfg, seed)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(sd[k].shape) for k, v in w.items()}, strict=True)
    return net.eval(), list(sd.keys())


def clouds(case):
    if case == "a":
        return R.ellipsoid_cloud("a", 2000), [2000], None
    c1 = R.ellipsoid_cloud("b1", 700)
    c2 = R.ellipsoid_cloud("b2", 450, axes=(0.3, 0.3, 0.45), center=(0.1, 0.0, 0.05))
    return np.concatenate([c1, c2], 0), [700, 450], LIMITS_B


def main():
    out = {}
    nets = {name: reference_net(cfg, R.SEEDS[name]) for name, cfg in (("desc", R.DESC), ("ctx", R.CTX))}
    out["state_dict_keys"] = np.array(nets["desc"][1])
    for case in ("a", "b"):
        pts, lens, limits = clouds(case)
        P = R.np_pyramid(pts, lens, R.DESC, limits)
        L = R.DESC["num_layers"]
        out[f"{case}_limits"] = np.array(limits if limits else [0] * L, np.int64)
        for l in range(L):
            out[f"{case}_points_{l}"] = P["points"][l]
            out[f"{case}_neighbors_{l}"] = table(P["neighbors"][l])
            out[f"{case}_lengths_{l}"] = P["stack_lengths"][l]
            if l < L - 1:
                out[f"{case}_pools_{l}"] = table(P["pools"][l])
                out[f"{case}_upsamples_{l}"] = table(P["upsamples"][l])
        batch = {"points": [torch.from_numpy(p) for p in P["points"]],
                 "neighbors": [torch.from_numpy(n) for n in P["neighbors"]],
                 "pools": [torch.from_numpy(n) for n in P["pools"]],
                 "upsamples": [torch.from_numpy(n) for n in P["upsamples"]],
                 "features": torch.ones(len(pts), 1), "stack_lengths": [torch.from_numpy(s) for s in P["stack_lengths"]]}
        for name, (net, _) in nets.items():
            with torch.no_grad():
                out[f"{case}_{name}"] = net(batch).numpy().astype(np.float32)[R.output_rows(len(pts), name)]
        print(case, [p.shape[0] for p in P["points"]], [n.shape[1] for n in P["neighbors"]],
              {k: float(np.abs(out[f"{case}_{k}"]).max()) for k in nets})
    path = os.path.join(HERE, "desc3d.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
