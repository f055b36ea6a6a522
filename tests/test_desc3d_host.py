"""KPSuperpoint3Dv2 without a GPU: the test-side fp64 restatement (tests/desc3d_fp64.py) against the reference's own outputs
(tests/golden/desc3d.npz, tests/golden/gen_golden_desc3d.py), the numpy pyramid restatement against the fixture's pyramid, and
rnnpose_amd.descriptor3d's module structure (parameter names, shapes, state_dict keys) and config checks."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import desc3d_fp64 as R  # noqa: E402

L = R.BASE["num_layers"]


def fixture_batch(g, case):
    return {"points": [g[f"{case}_points_{l}"] for l in range(L)],
            "neighbors": [g[f"{case}_neighbors_{l}"] for l in range(L)],
            "pools": [g[f"{case}_pools_{l}"] for l in range(L - 1)] + [np.zeros((0, 1), np.int32)],
            "upsamples": [g[f"{case}_upsamples_{l}"] for l in range(L - 1)] + [np.zeros((0, 1), np.int32)],
            "features": np.ones((g[f"{case}_points_0"].shape[0], 1), np.float32),
            "stack_lengths": [g[f"{case}_lengths_{l}"] for l in range(L)]}


def weights(name, g=None):
    from rnnpose_amd.descriptor3d import KPSuperpoint3Dv2
    cfg = R.DESC if name == "desc" else R.CTX
    net = KPSuperpoint3Dv2(dict(cfg))
    return R.make_weights({k: tuple(v.shape) for k, v in net.state_dict().items()}, cfg, R.SEEDS[name]), cfg


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("name", ["desc", "ctx"])
def test_fp64_restatement_matches_the_reference_fixture(golden, case, name):
    g = golden("desc3d")
    w, cfg = weights(name)
    net = R.Net64(w, cfg)
    y = net(fixture_batch(g, case)).numpy()[R.output_rows(g[f"{case}_points_0"].shape[0], name)]
    want = g[f"{case}_{name}"]
    err = float(np.abs(y - want).max())
    scale = max(1.0, float(np.abs(want).max()))
    print(f"{case}/{name}: max|fp64 - reference fp32| = {err:.2e} (scale {scale:.2f}), close count decisions {net.n_close}")
    assert y.shape == want.shape
    assert err <= 3e-6 * scale


@pytest.mark.parametrize("case", ["a", "b"])
def test_numpy_pyramid_matches_the_fixture(golden, case):
    g = golden("desc3d")
    lens = [int(v) for v in g[f"{case}_lengths_0"]]
    limits = [int(v) for v in g[f"{case}_limits"]]
    P = R.np_pyramid(g[f"{case}_points_0"], lens, R.DESC, limits if any(limits) else None)
    for l in range(L):
        assert np.array_equal(P["points"][l], g[f"{case}_points_{l}"]), l
        assert np.array_equal(P["neighbors"][l], g[f"{case}_neighbors_{l}"]), l
        assert np.array_equal(P["stack_lengths"][l], g[f"{case}_lengths_{l}"]), l
        if l < L - 1:
            assert np.array_equal(P["pools"][l], g[f"{case}_pools_{l}"]), l
            assert np.array_equal(P["upsamples"][l], g[f"{case}_upsamples_{l}"]), l
    if case == "b":                       # the limits truncate, and each cloud only sees itself
        assert all(g[f"b_neighbors_{l}"].shape[1] == limits[l] for l in range(L))
        nb = g["b_neighbors_0"]
        n0 = lens[0]
        real = nb < nb.shape[0]
        assert np.all(nb[:n0][real[:n0]] < n0) and np.all(nb[n0:][real[n0:]] >= n0)


def test_module_parameters_match_the_reference_keys(golden):
    from rnnpose_amd.descriptor3d import KPSuperpoint3Dv2
    keys = [str(k) for k in golden("desc3d")["state_dict_keys"]]
    for cfg, final in ((R.DESC, 32), (R.CTX, 256)):
        net = KPSuperpoint3Dv2(dict(cfg))
        sd = net.state_dict()
        assert list(sd.keys()) == keys
        assert len(keys) == 54
        kp = [k for k in keys if k.endswith("KPConv.weights")]
        assert [tuple(sd[k].shape) for k in kp] == [(15, 1, 64)] + [(15, c, c) for c in (32, 32, 64, 64, 64, 128, 128, 128, 256, 256)]
        assert tuple(sd["bottle.weight"].shape) == (128, 1024, 1) and tuple(sd["proj_gnn.weight"].shape) == (128, 128, 1)
        assert tuple(sd["decoder_blocks.5.mlp.weight"].shape) == (final + 2, 160)
        assert not net.encoder_blocks[0].KPConv.kernel_points.requires_grad
        w = R.make_weights({k: tuple(v.shape) for k, v in sd.items()}, cfg, 1)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
        pre = "hybrid_desc_net.corr_fea_extractor_3d."      # a checkpoint's prefix, stripped
        ck = {pre + k: v for k, v in net.state_dict().items()}
        KPSuperpoint3Dv2(dict(cfg)).load_state_dict({k[len(pre):]: v for k, v in ck.items()}, strict=True)


@pytest.mark.parametrize("key,value", [("KP_influence", "gaussian"), ("aggregation_mode", "closest"), ("modulated", True),
                                       ("architecture", ["simple", "resnetb_deformable"])])
def test_unsupported_configurations_are_refused(key, value):
    from rnnpose_amd.descriptor3d import KPSuperpoint3Dv2
    with pytest.raises(NotImplementedError):
        KPSuperpoint3Dv2(dict(R.DESC, **{key: value}))


def test_forward_refuses_cpu_tensors(golden):
    from rnnpose_amd.descriptor3d import KPSuperpoint3Dv2
    g = golden("desc3d")
    b = {k: ([torch.from_numpy(np.asarray(x)) for x in v] if isinstance(v, list) else torch.from_numpy(v))
         for k, v in fixture_batch(g, "b").items()}
    with pytest.raises(RuntimeError, match="GPU"):
        KPSuperpoint3Dv2(dict(R.DESC))(b)
