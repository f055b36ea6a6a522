"""The library's HIP kernels EXECUTED ON THE HOST (tests/host_exec/), against the CPU oracle and the reference-generated golden vectors
-- in the `-m "not gpu"` tier.

tests/host_exec/build_host.py compiles the kernel sources of rnnpose_amd/csrc as plain C++ over tests/host_exec/harness.hpp: a launch
runs every workgroup as a set of fibers (one per GPU thread), `__shared__` is a thread-local static, `__syncthreads()` and the wave
collectives -- shuffles and the MFMA instructions, D = A B + C in the gfx950 register layout -- are yield points.  The C-ABI entry
points run as shipped (argument checks, launch geometry, kernel code) on host memory.  Two kinds of test use it:
  * direct calls through the product's own ctypes prototypes (the per-pixel kernels, below);
  * a curated small-shape subset of the `-m gpu` PARITY TESTS THEMSELVES, run in a subprocess under the plugin
    tests/host_exec/pytest_hostexec.py, which points the unmodified Python front end at the host library (hostmode.py): volume and
    pyramid (fp32 MFMA, fp16x3 MFMA, split operands), window lookup, the 128-row and the strip MFMA convolutions with every
    epilogue, the update block and one engine step, the LM normal equations / solve / SE(3), instance norm, stem -- and one complete PoseRefiner loop
    against a reference-generated fixture.
This is test infrastructure: nothing here is reachable from the product path (ops.py refuses CPU tensors outside the test context;
the library has no host build).  The strip convolution kernels (operands by LDS-DMA, inline assembly) run too: their scratch
copy gets host versions of the three request / wait helpers (tests/host_exec/build_host.py lists every rewrite).  What it adds to the
GPU tests: the product SOURCE is pinned to the reference's vectors before a GPU box is involved -- the fourth-fragment bug of the
32-row stride-2 strips (found on the GPU in round 5) fails here in a second."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import rnnpose_oracle as orc
from rnnpose_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests", "host_exec"))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    import build_host
    try:
        build_host.clang()
    except RuntimeError as e:              # (the same image as the hipcc build: present wherever the library itself can be built)
        pytest.skip(str(e))
    return build_host.build(str(tmp_path_factory.mktemp("host_exec")))


@pytest.fixture(scope="module")
def host(host_lib):
    from rnnpose_amd import _lib
    lib = C.CDLL(host_lib)
    for name, (res, args) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args          # the product's own prototypes

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        assert rc == 0, (name, lib.rnnpose_last_error())
    lib.call = call
    return lib


def A(x):
    return np.ascontiguousarray(np.asarray(x), dtype=np.float32)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def test_induced_flow_is_the_reference_geometry_bit_for_bit(host):
    """a7 (geometry/transformation.py:184-198, projective_ops.py:68-114, PoseRefiner.py:324-328): flow and validity mask of the shipped
    kernel == the oracle's fp32 statements, exactly, and within the oracle test's own tolerance of the reference's output (golden)."""
    d = syn.make_inputs(2, 64, 80, seed=5)
    depth, K, G = A(d["depth"]), A(d["K"]), A(d["G0"])
    B, _, H, W = depth.shape
    flow, vm = np.full((B, 2, H, W), 7.0, np.float32), np.full((B, H, W), 7.0, np.float32)
    host.call("rnnpose_induced_flow_f32", P(depth), P(K), P(G), B, H, W, 1e-5, 0, P(flow), P(vm), None)
    want, wvm = orc.induced_flow(depth, K, G)
    assert np.array_equal(flow, want.numpy()) and np.array_equal(vm, wvm.numpy())
    g = np.load(os.path.join(GOLD, "geometry.npz"))                 # the reference's own output (inputs: tests/golden/gen_golden.py)
    depth, K, G = A(g["depth"]), A(syn.make_inputs(2, 64, 96, seed=7, pose_sigma=0.03)["K"]), A(g["G"])
    B, _, H, W = depth.shape
    flow, vm = np.zeros((B, 2, H, W), np.float32), np.zeros((B, H, W), np.float32)
    host.call("rnnpose_induced_flow_f32", P(depth), P(K), P(G), B, H, W, 1e-5, 0, P(flow), P(vm), None)
    ref = g["flow_init"][:, 0].astype(np.float64)
    assert float(np.max(np.abs(flow - ref) - 1e-4 - 1e-6 * np.abs(ref))) <= 0        # (the oracle test's own mixed tolerance)
    assert np.array_equal(vm, g["vmask"].reshape(vm.shape).astype(np.float32))
    # argument validation is the shipped one
    assert host.rnnpose_induced_flow_f32(P(depth), P(K), P(G), B, H, W, 1e-5, 2, P(flow), P(vm), None) == 1
    assert b"mode must be 0 or 1" in host.rnnpose_last_error()


def test_induced_coords_lowres_is_flow_init_resized(host):
    """a7 + a5 fused (CFNet.py:136-144): coords1 = grid + resize_ac(flow_init / 8) evaluated at the four taps only == the two-step
    path of the same library (induced_flow -> flow_to_coords) bit for bit, and the oracle."""
    d = syn.make_inputs(2, 64, 80, seed=6)
    depth, K, G = A(d["depth"]), A(d["K"]), A(d["G0"])
    B, _, H, W = depth.shape
    h, w = H // 8, W // 8
    c1 = np.zeros((B, 2, h, w), np.float32)
    host.call("rnnpose_induced_coords_lowres_f32", P(depth), P(K), P(G), B, H, W, h, w, 1e-5, P(c1), None)
    flow = np.zeros((B, 2, H, W), np.float32)
    host.call("rnnpose_induced_flow_f32", P(depth), P(K), P(G), B, H, W, 1e-5, 0, P(flow), None, None)
    c2 = np.zeros_like(c1)
    host.call("rnnpose_flow_to_coords_f32", P(flow), B, H, W, h, w, P(c2), None)
    assert np.array_equal(c1, c2)
    want = orc.flow_init_to_coords1(orc.induced_flow(depth, K, G)[0]).numpy()
    assert np.abs(c1 - want).max() <= 1e-5


def test_corr_weight_vs_oracle_and_reference_vector(host):
    """a8 (PoseRefiner.py:342-345): exp(-|1 - <g1, bilinear(g2, target)>| / sigma) * [depth > 0], the align_corners mismatch of the
    reference included; both target forms of the entry point (absolute coordinates; planar flow + pixel grid)."""
    d = syn.make_inputs(2, 40, 56, seed=7)
    g1, g2, depth = A(d["g1"]), A(d["g2"]), A(d["depth"])
    B, D, H, W = g1.shape
    flow = A(syn.uniform("hostexec.flow", (B, 2, H, W), 7, -6.0, 6.0))
    flow[0, :, :3] = 200.0                          # taps far outside the map: zero padding
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    target = A(np.stack([flow[:, 0] + xs, flow[:, 1] + ys], -1))
    sigma = A([0.7])
    want = orc.corr_weight(g1, g2, target, depth, sigma).numpy()
    for mode, t in ((0, target), (1, flow)):
        wt = np.full((B, H, W), 7.0, np.float32)
        host.call("rnnpose_corr_weight_f32", P(g1), P(g2), P(t), mode, P(depth), P(sigma), B, D, H, W, P(wt), None)
        assert np.abs(wt - want).max() <= 2e-6, mode
        assert np.array_equal(wt == 0, want == 0)
    g = np.load(os.path.join(GOLD, "geometry.npz"))                 # the reference's own weight map for its own correspondence field
    d = syn.make_inputs(2, 64, 96, seed=7, pose_sigma=0.03)
    g1, g2, depth, t = A(d["g1"]), A(d["g2"]), A(g["depth"]), A(g["target"][:, 0])
    B, D, H, W = g1.shape
    wt = np.zeros((B, H, W), np.float32)
    host.call("rnnpose_corr_weight_f32", P(g1), P(g2), P(t), 0, P(depth), P(A(g["sigma"])), B, D, H, W, P(wt), None)
    assert np.abs(wt - g["weight"].reshape(wt.shape)).max() < 1e-4


def test_context_prep_and_convex_upsample_vs_reference_vectors(host):
    """a5 (CFNet.py:124-133: tanh / relu halves of the resized context) and a6 (CFNet.py:95-106: softmax over 9 taps of 8 x flow, the
    kernel with shared-memory staging and a workgroup barrier) on the reference-generated `upsample_ctx` vectors."""
    g = np.load(os.path.join(GOLD, "upsample_ctx.npz"))             # reference outputs; inputs regenerated as tests/test_oracle_golden.py does
    ctx = A(syn.normal("ctx", (1, 256, 64, 96), 5, std=0.1))
    B, Cc, H, W = ctx.shape
    h, w = g["net"].shape[-2:]
    net, inp = np.zeros(g["net"].shape, np.float32), np.zeros(g["inp"].shape, np.float32)
    host.call("rnnpose_context_prep_f32", P(ctx), B, Cc, H, W, h, w, g["net"].shape[1], P(net), P(inp), None)
    assert np.abs(net - g["net"]).max() < 1e-6 and np.abs(inp - g["inp"]).max() < 1e-6
    finit = A(syn.normal("finit", (2, 2, 64, 96), 5, std=4.0))
    c1 = np.zeros(g["coords1"].shape, np.float32)
    host.call("rnnpose_flow_to_coords_f32", P(finit), 2, 64, 96, 8, 12, P(c1), None)
    assert np.abs(c1 - g["coords1"]).max() < 1e-5
    flow, mask = A(syn.normal("up_flow", (2, 2, 16, 12), 5, std=3.0)), A(syn.normal("up_mask", (2, 576, 16, 12), 5, std=2.0))
    B, _, h, w = flow.shape
    up = np.zeros((B, 2, 8 * h, 8 * w), np.float32)
    host.call("rnnpose_convex_upsample_f32", P(flow), P(mask), B, h, w, 8, P(up), None)
    assert np.abs(up - g["flow_up"]).max() < 1e-4
    want = orc.convex_upsample(flow, mask).numpy()
    assert np.abs(up - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


def test_gru_pointwise_stages(host):
    """a4 (thirdparty/raft/update.py:45-60): z = sigmoid(.), r * h written into the concatenated buffer, h' = (1 - z) h + z tanh(q)."""
    B, Cn, hw, Ctot = 2, 16, 35, 40
    zr = A(syn.normal("hostexec.zr", (B, 2 * Cn, hw), 3, std=2.0))
    hcat = A(syn.normal("hostexec.h", (B, Ctot, hw), 3))
    q = A(syn.normal("hostexec.q", (B, Cn, hw), 3, std=2.0))
    z, rhx = np.zeros((B, Cn, hw), np.float32), hcat.copy()
    host.call("rnnpose_gru_gate_f32", P(zr), P(hcat), B, Cn, Ctot, hw, P(z), P(rhx), None)
    tz, tr, th = torch.sigmoid(torch.from_numpy(zr[:, :Cn])), torch.sigmoid(torch.from_numpy(zr[:, Cn:])), torch.from_numpy(hcat[:, :Cn])
    assert np.abs(z - tz.numpy()).max() <= 1e-6 and np.abs(rhx[:, :Cn] - (tr * th).numpy()).max() <= 1e-6
    assert np.array_equal(rhx[:, Cn:], hcat[:, Cn:])
    hout = np.zeros((B, Ctot, hw), np.float32)
    host.call("rnnpose_gru_update_f32", P(z), P(q), P(hcat), B, Cn, Ctot, hw, P(hout), Ctot, None)
    want = (1 - torch.from_numpy(z)) * th + torch.from_numpy(z) * torch.tanh(torch.from_numpy(q))
    assert np.abs(hout[:, :Cn] - want.numpy()).max() <= 1e-6


def test_instnorm_nhwc_size_check_holds_for_every_channel_count(host):
    """rnnpose_instnorm_nhwc_f32 refuses a bad B or HW whatever the channel count.  (With the channel alternatives `|| C == 96 || C == 192`
    unparenthesised after the `&&` chain, 96 and 192 skipped the tests on B and HW: the call was refused by the launch only, with another
    message.)  Each call returns 1 with the "bad size" text and launches nothing: every buffer keeps its sentinel.  Host library only."""
    for B, HW, Cc in ((0, 4, 96), (1, 0, 96), (65536, 1, 192)):
        x, out = np.full((4, Cc), 3.0, np.float32), np.full((4, Cc), 7.0, np.float32)
        mr, ws = np.full((1, Cc, 2), 7.0, np.float32), np.full(Cc * 2, 7.0, np.float64)
        n_ws = ws.nbytes if B < 65536 else 0        # (were the size check skipped again, the workspace check refuses B = 65536: no launch over these buffers)
        rc = host.rnnpose_instnorm_nhwc_f32(P(x), B, HW, Cc, 1e-5, 1, None, P(ws), n_ws, P(mr), P(out), None)
        assert rc == 1 and b"bad size" in host.rnnpose_last_error(), (B, HW, Cc, rc, host.rnnpose_last_error())
        assert (out == 7.0).all() and (mr == 7.0).all() and (ws == 7.0).all()
    x, out = A(syn.normal("hostexec.in", (5, 96), 3)), np.zeros((5, 96), np.float32)     # the accepted sizes still run
    mr, ws = np.zeros((1, 96, 2), np.float32), np.zeros(96 * 2, np.float64)
    host.call("rnnpose_instnorm_nhwc_f32", P(x), 1, 5, 96, 1e-5, 0, None, P(ws), ws.nbytes, P(mr), P(out), None)
    want = (x - x.mean(0)) / np.sqrt(x.astype(np.float64).var(0) + 1e-5)
    assert np.abs(out - want).max() <= 2e-6
    assert host.rnnpose_instnorm_nhwc_f32(P(x), 1, 5, 40, 1e-5, 0, None, P(ws), ws.nbytes, P(mr), P(out), None) == 1
    assert b"C must be" in host.rnnpose_last_error()


# ---- the `-m gpu` parity tests themselves, against the host-executed kernels -------------------------------------------------------
# Excluded: sizes that take the emulation minutes (full BASELINE shapes, the long refinement loops but one), tests of hipGraph replay
# (no capture on the host) or of a real torch.cuda allocator; the strip-kernel tests are the second set (STRIP_IDS).
PARITY_K = ("not (full_size or full_shape or loop_480 or timed_configuration or config3 or linemod_crop or graph_replay or "
            "alternate_corr_block_vs_oracle or alternate_corr_odd or teacher or facade_stateful or context_prep_and_flow_to_coords or "
            "strip or stride2_strips or patch_tiling_equals_row_major or range_guard_is_visible or per_image_tiles or "
            "k_split_matches_single_pass or range_guard_counts_in_every or narrow_sources or zoom_pipeline_full_size or "
            "coverage_agrees_with_vertex_splat or (split_sources and not segs2) or encoder_split_output or nn_search_bit_exact or "
            # r06: the encoder-in-the-loop S1 fixture (4 min per case under emulation) and the 60 x 80 cases of the r06 kernel-variant tests
            "loop_S1_shipped or (lds_dma_operands and 60-80) or (fused_equals_the_two_kernels and 60-80) or (induced_coords_formed and 60-80))")
DESELECT = [
    "tests/test_gpu_parity.py::test_refinement_loop_golden[loop_128-shape0-1-3-1-True]",      # (the literal call sequence of the same loop stays)
    "tests/test_gpu_parity.py::test_refinement_loop_golden[loop_2x2-shape1-2-2-2-True]",
    "tests/test_gpu_parity.py::test_refinement_loop_golden[loop_2x2-shape1-2-2-2-False]",
    "tests/test_gpu_parity.py::test_refinement_loop_golden[loop_S1-shape2-1-3-1-True]",
    "tests/test_gpu_parity.py::test_refinement_loop_golden[loop_S1-shape2-1-3-1-False]",
    "tests/test_gpu_parity.py::test_update_engine_one_step[True-False-]",
    "tests/test_gpu_parity.py::test_update_engine_one_step[True-True-convc2=4,convf2=4,conv=4,zr=4,q=4,zr2=4,q2=4,heads=4,inp=4]",
    "tests/test_gpu_parity.py::test_update_engine_one_step[True-True-zr=3,zr2=3,heads=3,q=1,conv=2]",
    "tests/test_gpu_parity.py::test_update_engine_one_step[False-False-]",
    "tests/test_gpu_parity.py::test_update_engine_one_step[False-True-]",
    "tests/test_gpu_parity.py::test_update_engine_one_step[False-True-convc2=4,convf2=4,conv=4,zr=4,q=4,zr2=4,q2=4,heads=4,inp=4]",
    "tests/test_gpu_parity.py::test_update_engine_one_step[False-True-zr=3,zr2=3,heads=3,q=1,conv=2]",
]
FILES = ["tests/test_gpu_parity.py", "tests/test_gpu_conv.py", "tests/test_gpu_eval.py", "tests/test_zoom.py", "tests/test_raster.py",
         "tests/test_gpu_lm_geometry.py", "tests/test_gpu_raster_edges.py",      # (their large shapes carry `full_size` in their names: PARITY_K leaves them out)
         "tests/test_gpu_zoom_edges.py",                                         # (no large shapes: the whole module runs here)
         "tests/test_gpu_glue_edges.py", "tests/test_gpu_corr_edges.py",
         "tests/test_gpu_point_edges.py",                                        # (no large shapes either: 16384 x 40 x 70 takes the emulation under a second)
         "tests/test_gpu_range_guard.py",                                        # (at most 3 x 11 x 19 pixels per launch, one stride-2 layer of 20 x 32: the whole module)
         "tests/test_gpu_stem_mask_edges.py"]                                    # (at most 20 x 16 x 32 image pixels / 75 low-resolution pixels per launch: the whole module)

# The strip convolution kernels (LDS-DMA by inline assembly on the GPU; tests/host_exec/build_host.py gives their scratch copy host
# versions of the request / wait helpers): both strip heights, split-tensor (DMA) and fp32 (register-path) sources, 3x3 / 1x5 / 5x1,
# two column tiles per wave, GRU epilogues, tile statistics + fused input norm, the stride-2 forms over parity planes, single product.
_C = "tests/test_gpu_conv.py::"
STRIP_IDS = [_C + t for t in (
    "test_conv_strip_vs_fp64[auto-rows160-1-21-33-segs8-48-3-3-False]", "test_conv_strip_vs_fp64[auto-rows160-1-21-33-segs8-48-3-3-True]",
    "test_conv_strip_vs_fp64[auto-rows32-1-21-33-segs8-48-3-3-False]", "test_conv_strip_vs_fp64[auto-rows32-1-21-33-segs8-48-3-3-True]",
    "test_conv_strip_vs_fp64[auto-rows160-3-7-11-segs2-128-5-1-False]", "test_conv_strip_vs_fp64[auto-rows160-3-7-11-segs2-128-5-1-True]",
    "test_conv_strip_vs_fp64[auto-rows32-3-7-11-segs2-128-5-1-True]", "test_conv_strip_vs_fp64[auto-rows32-1-16-16-segs1-256-1-5-True]",
    "test_conv_strip_vs_fp64[two-tile-waves-rows160-2-13-29-segs6-320-1-5-True]",
    "test_conv_strip_vs_fp64[two-tile-waves-rows160-1-23-37-segs5-96-3-3-False]",
    "test_conv_strip_vs_fp64[auto-rows160-2-40-48-segs7-64-3-3-True]", "test_conv_strip_vs_fp64[auto-rows32-2-40-48-segs7-64-3-3-False]",
    "test_conv_strip_gru_epilogues[auto-rows160-1-5-True]", "test_conv_strip_gru_epilogues[auto-rows160-5-1-False]",
    "test_conv_strip_gru_epilogues[auto-rows32-1-5-False]", "test_conv_strip_gru_epilogues[auto-rows32-5-1-True]",
    "test_conv_strip_gru_epilogues[two-tile-waves-rows160-5-1-True]",
    "test_conv_strip_tile_stats_and_fused_input_norm[auto-rows160-2-40-48-64-64]",
    "test_conv_strip_tile_stats_and_fused_input_norm[auto-rows32-3-15-20-96-96]",
    "test_conv_strip_tile_stats_and_fused_input_norm[two-tile-waves-rows160-2-20-32-128-128]",
    "test_conv_stride2_strips_over_parity_planes[3-96-160-32-64-True-3]", "test_conv_stride2_strips_over_parity_planes[2-100-112-64-96-True-3]",
    "test_conv_stride2_strips_over_parity_planes[2-100-112-64-96-True-1]", "test_conv_stride2_strips_over_parity_planes[1-60-60-96-128-True-3]",
    "test_conv_stride2_strips_over_parity_planes[1-60-60-96-128-True-1]", "test_conv_stride2_strips_over_parity_planes[2-120-120-64-96-True-3]",
    "test_conv_strip_single_product_is_plain_fp16[1-40-48-segs2-64-3-3-True]", "test_conv_strip_single_product_is_plain_fp16[2-20-32-segs0-256-1-5-False]",
    # r06: 96-row strips (three MFMA row tiles per wave, 6 x 16 patches); the PERSISTENT form of the fp32-source kernels (the host "device" has 4
    # CUs: 8 / 16 resident workgroups walk 24-30 tiles, ragged ones included)
    "test_conv_strip_vs_fp64[auto-rows96-1-21-33-segs8-48-3-3-False]", "test_conv_strip_vs_fp64[auto-rows96-3-7-11-segs2-128-5-1-True]",
    "test_conv_strip_vs_fp64[auto-rows96-2-40-48-segs7-64-3-3-True]", "test_conv_strip_gru_epilogues[auto-rows96-1-5-True]",
    "test_conv_strip_tile_stats_and_fused_input_norm[auto-rows96-3-15-20-96-96]",
    "test_conv_strip_persistent_launch_is_bit_identical[2-64-64-40-48-True]", "test_conv_strip_persistent_launch_is_bit_identical[3-96-96-30-48-False]",
    "test_conv_strip_persistent_launch_is_bit_identical[2-128-128-50-33-True]",
)] + ["tests/test_gpu_parity.py::test_corr_lookup_convc1_fused_equals_the_two_kernels[" + t + "]" for t in ("False-2-16-24-0-2", "True-3-17-19-1-3", "False-4-30-30-2-3")]


def _subset(host_lib, args):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + ROOT, HOSTEXEC_DIR=os.path.dirname(host_lib))
    cmd = [sys.executable, "-m", "pytest", "-p", "host_exec.pytest_hostexec", "-m", "gpu", "-q", "-p", "no:cacheprovider"] + args
    try:                                   # (pytest-timeout is optional: without the plugin the flag would be a usage error -- ADVICE r05)
        import pytest_timeout  # noqa: F401
        cmd.insert(cmd.index("-q"), "--timeout=300")
    except ImportError:
        pass
    return subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _passed(proc, at_least):
    out = proc.communicate(timeout=1500)[0]
    tail = out[-3000:]
    m = re.search(r"(\d+) passed", tail)
    assert proc.returncode == 0 and m and " failed" not in tail.splitlines()[-1], tail
    assert int(m.group(1)) >= at_least, tail


def test_gpu_parity_tests_pass_on_the_host_executed_kernels(host_lib):
    """Two curated sets of the `-m gpu` tests (see the module docstring), UNMODIFIED, in subprocesses whose sessions run under
    tests/host_exec/hostmode.py: the Python front end drives the host library.  Every selected test must pass; the counts guard
    against a selection that silently shrinks.  (The two run side by side: the wall time is the longer one's.)"""
    a = _subset(host_lib, ["-k", PARITY_K] + [x for d in DESELECT for x in ("--deselect", d)] + FILES)
    b = _subset(host_lib, STRIP_IDS)
    _passed(b, len(STRIP_IDS))
    # 88: the small-shape cases of tests/test_gpu_lm_geometry.py, 70: those of tests/test_gpu_raster_edges.py, 94: all of tests/test_gpu_zoom_edges.py,
    # 90: those of tests/test_gpu_glue_edges.py, 52: those of tests/test_gpu_corr_edges.py (all but the four entries of its 48 x 56 volume),
    # 73: all of tests/test_gpu_point_edges.py, 93: all of tests/test_gpu_range_guard.py, 145: all of tests/test_gpu_stem_mask_edges.py
    _passed(a, 95 + 88 + 70 + 94 + 90 + 52 + 73 + 93 + 145)


def test_harness_model(tmp_path):
    """The execution model of tests/host_exec/harness.hpp on kernels of its own (tests/host_exec/selftest_kernels.hip.inc): one MFMA tile in
    the gfx950 register layout against a matrix product, threads that return before a barrier, shuffles among the remaining lanes,
    dynamic LDS, atomics across workgroups."""
    import build_host
    try:
        cxx = build_host.clang()
    except RuntimeError as e:
        pytest.skip(str(e))
    here = os.path.join(ROOT, "tests", "host_exec")
    src = open(os.path.join(here, "selftest_kernels.hip.inc")).read().replace("extern __shared__ float buf[];", "float* buf = reinterpret_cast<float*>(hostexec::dyn_lds());")
    (tmp_path / "selftest.hip").write_text(src)
    (tmp_path / "tu.cpp").write_text(f'#include "harness.hpp"\n#include "{tmp_path / "selftest.hip"}"\n')
    lib = str(tmp_path / "selftest.so")
    r = subprocess.run([cxx, "-x", "c++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-D__HIP_PLATFORM_AMD__", "-w", "-I", "/opt/rocm/include",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rnnpose_amd", "csrc"), "-I", here, str(tmp_path / "tu.cpp"),
                        os.path.join(here, "runtime_host.cpp"), "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    st = C.CDLL(lib)
    rng = np.random.default_rng(0)
    a = np.ascontiguousarray(rng.standard_normal((32, 16)).astype(np.float16).astype(np.float32))
    b = np.ascontiguousarray(rng.standard_normal((16, 32)).astype(np.float16).astype(np.float32))
    d = np.zeros((32, 32), np.float32)
    st.selftest_mfma(P(a), P(b), P(d))
    assert np.array_equal(d, (a.astype(np.float64) @ b.astype(np.float64) + 1.0).astype(np.float32))      # exact products, one rounding
    nblk = 5
    x = np.ascontiguousarray(rng.integers(-100, 100, nblk * 128).astype(np.int32))
    out = np.zeros(nblk * 2, np.int32)
    st.selftest_barrier_exit(P(x), P(out), nblk)
    xs = x.reshape(nblk, 128)
    want = np.array([[sum(int(xs[k, (t + 2) % 128]) for t in range(w * 64, w * 64 + 64, 2)) for w in (0, 1)] for k in range(nblk)], np.int32)
    assert np.array_equal(out.reshape(nblk, 2), want)
    f = np.ascontiguousarray(rng.standard_normal(7 * 64).astype(np.float32))
    y, cnt = np.zeros_like(f), np.zeros(1, np.uint64)
    st.selftest_dyn_lds(P(f), P(cnt), P(y), 7)
    assert np.array_equal(y.reshape(7, 64), f.reshape(7, 64)[:, ::-1]) and int(cnt[0]) == int((f > 0).sum())
