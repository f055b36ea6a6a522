#!/usr/bin/env python3
"""bench.py -- RNNPose recurrent pose-refinement throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 5 --warmup 2
    python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs bench_outputs   # + the last timed step's outputs as .npy
    python bench.py --gpus 1 --steps 5 --warmup 2 --full     # + CPU baseline and in-run parity against the CPU oracle
    python bench.py --gpus 8                       # no WORLD_SIZE in the environment: spawns the 8 ranks itself
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One STEP = one full refinement of one batch: 3 outer x 8 inner iterations of the loop body
(model/PoseRefiner.py:239-365) on synthetic 640x480 render+target pairs, batch 8 per GPU
(BASELINE.json configs[1]); per outer iteration: RAFT encoder + correlation volume/pyramid + context prep;
per inner iteration: induced flow -> pyramid lookup -> update block -> convex upsample -> descriptor
weight -> LM step.  The renderer is outside the path: views are synthetic and fixed.
Inputs are resident in HBM before the timed region.  value = refinement iterations/s (one iteration = the
loop body for one rank's batch of 8), summed over ranks (weak scaling: every rank refines its own batch).

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line; whatever needs runs of its own
(the CPU baseline and the parity gate, together about 85 s at the default size) is done only with --full, after the line's
figures are taken.  Rank 0 prints ONE JSON line (see the task contract) carrying
  roofline                   the dominant kernel (the implicit-GEMM convolution) against the fp16 MFMA peak, per launch,
                             measured live with HIP events on the launch stream;
  chip_level                 executed matrix-core flops of the WHOLE step / wall time of the step;
  correlation_volume_kernel  north_star's named kernel against the HBM roofline;
  kernels                    every C-ABI launch type: mean duration, share of the step, achieved GB/s from the bytes each
                             launch declared for its own arguments (a half-batch launch declares half the batch);
  cpu_baseline               --full only (null otherwise): the CPU oracle on the host cores: the full batch, 1 outer x `inner`
                             iterations (the 3x8 schedule repeats that unit, so iterations/s are directly comparable), median of
                             3 runs, N=1 only;
  parity                     --full only (null otherwise): the GPU refiner's first outer iteration against that oracle run's
                             outputs (identical inputs, both started from the reference's literal Tij = Ti * Ti^-1 -- the
                             shipped default since r06): pose within 1e-5 and first-iteration flow within 1e-4, or the line is
                             declared invalid; `exact_identity_start` = the same gate for the literal_legacy_pose=False option.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s measured achievable)
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 peak
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense fp16/bf16 MFMA peak (no sparsity)
DUMP_LIMIT_BYTES = 64 * 10**6  # --dump-outputs: all arrays together, .npy headers included
DUMP_SAMPLE_SEED = 0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--outer", type=int, default=3)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--optim-iters", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the CPU baseline and the parity gate against the CPU oracle (N=1 only); a plain "
                         "run leaves both out of the line (null)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline and the parity gate")
    ap.add_argument("--cpu-runs", type=int, default=3, help="--full: timed runs of the CPU baseline (median reported) after one warm-up run")
    ap.add_argument("--no-encoder", action="store_true", help="feed synthetic feature maps (kernel-only runs)")
    ap.add_argument("--unfused", action="store_true", help="literal reference call sequence through the facade")
    ap.add_argument("--no-graph", action="store_true", help="eager launches only (no hipGraph replay; for counter passes)")
    ap.add_argument("--mixed-precision", action="store_true",
                    help="cfg.raft.mixed_precision: single-product fp16 convolutions (the reference's GPU arithmetic) -- NOT the headline "
                         "arithmetic: the line says so in `dtype` / `config`, and its parity block is a distance, not a gate")
    ap.add_argument("--workload", choices=["cfg1", "cfg4"], default=None,
                    help="a BASELINE.json configuration verbatim: cfg1 = configs[1] (640x480, batch 8/GPU, 3x8: the default), cfg4 = "
                         "configs[4] (1280x960 high-res, batch 8/GPU = batch 64 over 8 GPUs, 3x8)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0) as DIR/<name>.npy (float32 / float64, "
                         f"at most {DUMP_LIMIT_BYTES // 10**6} MB in all: larger outputs are stored as a fixed, seeded sample)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.workload == "cfg4":
        args.batch, args.height, args.width, args.outer, args.inner = 8, 960, 1280, 3, 8
    elif args.workload == "cfg1":
        args.batch, args.height, args.width, args.outer, args.inner = 8, 480, 640, 3, 8
    return args


def step_outputs(out):
    """The arrays a caller of PoseRefiner.forward receives from one step, by name (the echoed inputs -- intrinsics, views --
    are left out).  Floating-point tensors keep float64 or become float32; masks and counters become float64/float32 numbers."""
    arrays = {"Ti_pred": out["Ti_pred"].G, "Tij": out["Tij"].G}
    for i, f in enumerate(out["flow"]):
        arrays[f"flow_{i}"] = f
    arrays.update(flow_last=out["flow_last"], weight=out["weight"], vmask=out["vmask"], f16x3_range_events=out["f16x3_range_events"])
    res = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        res[name] = a if a.dtype == "float64" else a.astype("float64" if a.dtype.kind in "iu" else "float32")
    return res


def dump_outputs(arrays, path, limit=DUMP_LIMIT_BYTES, seed=DUMP_SAMPLE_SEED):
    """Write every array as path/<name>.npy.  If they do not fit in `limit` bytes together, every array larger than 1 MB is
    replaced by the same fraction of its elements, flattened, at positions drawn once from a generator seeded with `seed` and
    the array's size (sorted): the sample depends only on the arguments, so two builds' dumps compare element for element.
    -> {name: {"shape", "dtype", "sampled"}}"""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    header = 256                                                       # bound on one .npy header (128 bytes for these shapes)
    big = {k for k, a in arrays.items() if a.nbytes > 2**20}
    fixed = sum(a.nbytes + header for k, a in arrays.items() if k not in big) + header * len(big)
    big_bytes = sum(arrays[k].nbytes for k in big)
    frac = 1.0 if fixed + big_bytes <= limit else max(0.0, (limit - fixed) / big_bytes)
    info = {}
    for name, a in arrays.items():
        sampled = name in big and frac < 1.0
        if sampled:
            k = int(a.size * frac)
            idx = np.sort(np.random.default_rng([seed, a.size]).choice(a.size, size=k, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))
        info[name] = {"shape": list(arrays[name].shape), "dtype": str(a.dtype), "sampled": (f"{a.size} of {arrays[name].size} elements"
                                                                                          if sampled else None)}
    return info


def spawn_ranks(n):
    """`python bench.py --gpus N` outside torchrun: launch the N ranks of one node ourselves (reference:
    tools/eval.py:224-225 spawns one process per GPU) and relay rank 0's JSON line."""
    import torch
    have = torch.cuda.device_count()
    if have < n and not os.environ.get("RNNPOSE_DIST_BACKEND"):       # (gloo override: several ranks share one GPU -- path test only)
        raise SystemExit(f"bench.py --gpus {n}: only {have} GPU(s) visible on this node")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def synth_views(B, H, W, device, seed, with_encoder):
    """Synthetic, fixed, already-cropped views in HBM (shapes/ranges of SURVEY.md section 8d)."""
    import torch
    from rnnpose_amd import ops
    from rnnpose_amd.pose_refiner import SyntheticRenderer
    from rnnpose_amd.synthetic import intrinsics
    g = torch.Generator(device=device)
    g.manual_seed(1234 + seed)
    rnd = lambda *s: torch.randn(*s, device=device, generator=g)
    uni = lambda *s: torch.rand(*s, device=device, generator=g)
    syn_img, image_crop = uni(B, 3, H, W), uni(B, 3, H, W)
    cfea = rnd(B, 256, H, W).mul_(0.1)
    g1, g2 = rnd(B, 32, H, W), rnd(B, 32, H, W)
    g1 /= g1.norm(dim=1, keepdim=True)
    g2 /= g2.norm(dim=1, keepdim=True)
    depth = uni(B, 1, H, W) * 0.3 + 0.9
    depth[:, :, : H // 4] = 0
    K = torch.from_numpy(intrinsics(B, H, W)).to(device)
    xi = rnd(B, 6) * 0.02
    G0 = ops.se3_exp(xi).reshape(B, 1, 4, 4)
    fm = (None, None) if with_encoder else (rnd(B, 256, H // 8, W // 8), rnd(B, 256, H // 8, W // 8))
    rend = SyntheticRenderer(syn_img=syn_img, image_crop=image_crop, cfea=cfea, geofea1=g1, geofea2_crop=g2,
                             syn_depth=depth, intrinsics_crop=K, fmap1=fm[0], fmap2=fm[1])
    return rend, K, G0


def cpu_baseline(refiner, rend, K, G0, args):
    """CPU oracle (oracle/rnnpose_oracle.py, kind 'port') on the SAME workload: the full batch, one outer iteration
    (encoder + volume build + context prep) followed by `inner` inner iterations -- the unit the 3x8 schedule repeats
    three times, so its iterations/s are the schedule's.  SURVEY 8d: one full warm-up refinement, then the median of 3
    timed runs.  The warm-up run also captures the oracle's outputs: -> (record, outputs) for the in-run parity check."""
    import statistics
    import torch
    from oracle import rnnpose_oracle as orc
    v = rend.views
    ncpu = os.cpu_count() or 1
    cores = int(os.environ.get("RNNPOSE_CPU_THREADS", min(ncpu, 64)))   # torch-CPU stops scaling well before 256 SMT threads
    torch.set_num_threads(cores)
    inp = {"ctx": v["cfea"], "g1": v["geofea1"], "g2": v["geofea2_crop"], "depth": v["syn_depth"], "K": K, "G0": G0,
           "sigma": refiner.sigma[0].detach()}
    W = {"upd": {k: p.detach().cpu().numpy() for k, p in refiner.cf_net.update_block.state_dict().items()}}
    if v["fmap1"] is None:
        inp["img_render"], inp["img_target"] = v["syn_img"], v["image_crop"]
        W["enc"] = {k: p.detach().cpu().numpy() for k, p in refiner.image_fea_enc.fnet.state_dict().items()}
    else:
        inp["fmap1"], inp["fmap2"] = v["fmap1"], v["fmap2"]
    inp = {k: t.detach().cpu().numpy() for k, t in inp.items()}
    t0 = time.perf_counter()
    # (r06: the shipped default -- GPU refiner and oracle -- starts every outer iteration from the reference's literal Tij = Ti * Ti^-1,
    #  model/PoseRefiner.py:243-244; the exact identity of r03-r05 is the option, gated below as parity.exact_identity_start)
    warm = orc.refine(inp, W, outer=1, inner=args.inner, optim_iters=args.optim_iters, fast=True, capture=True, literal_legacy_pose=True)   # warm-up + parity capture
    t_warm = time.perf_counter() - t0
    outputs = {"G": warm["G"], "Tij": [tr["Tij"] for tr in warm["trace"]], "flow_first": warm["trace"][0]["flow_up"],
               "flow_last": warm["flow_up"], "weight_last": warm["weight"]}
    del warm
    # the same unit started from the EXACT identity (the r03-r05 default, now the option), for parity.exact_identity_start
    t0 = time.perf_counter()
    leg = orc.refine(inp, W, outer=1, inner=args.inner, optim_iters=args.optim_iters, fast=True, capture=True, literal_legacy_pose=False)
    outputs["identity"] = {"G": leg["G"], "Tij": [tr["Tij"] for tr in leg["trace"]], "flow_first": leg["trace"][0]["flow_up"],
                         "flow_last": leg["flow_up"], "seconds": time.perf_counter() - t0}
    del leg
    # the same arithmetic in fp64 for the FIRST iteration: what both fp32 evaluations (this oracle's, the GPU's) approximate
    t0 = time.perf_counter()
    with orc.precision(torch.float64):
        truth = orc.refine(inp, W, outer=1, inner=1, optim_iters=args.optim_iters, fast=True, capture=True, literal_legacy_pose=True)
    outputs["flow_first_fp64"] = truth["trace"][0]["flow_up"]
    outputs["fp64_seconds"] = time.perf_counter() - t0
    del truth
    walls, tm = [], {}
    for _ in range(max(1, args.cpu_runs)):
        tm = {}
        t0 = time.perf_counter()
        orc.refine(inp, W, outer=1, inner=args.inner, optim_iters=args.optim_iters, stage_timer=tm, fast=True)
        walls.append(time.perf_counter() - t0)
    wall = statistics.median(walls)
    rec = {
        "value": round(args.inner / wall, 4), "unit": "iters/s", "cores": cores, "kind": "port",
        "runs": len(walls), "min": round(args.inner / max(walls), 4), "max": round(args.inner / min(walls), 4),
        "sample": (f"full batch ({args.batch} x {args.height}x{args.width}), 1 outer x {args.inner} inner iterations of the CPU "
                   f"oracle in its library-call form (grid_sample/unfold as the reference uses on CPU), encoder + volume build "
                   f"included; one full warm-up run ({t_warm:.1f} s, also the parity capture), then the MEDIAN of {len(walls)} timed runs "
                   f"({', '.join(f'{x:.1f}' for x in walls)} s); torch {torch.__version__} CPU with "
                   f"{cores} threads on {ncpu} logical CPUs.  The 3x8 schedule repeats this unit 3 times: same iterations/s"),
        "stages_s": {k: round(x, 3) for k, x in tm.items()},
    }
    return rec, outputs


# north_star: 1e-5 on the 6-DoF pose, 1e-4 on the correspondence field (identical inputs).
# The flow check has two legs.  (1) |GPU - CPU oracle| <= 1e-4 on the first iteration's field: the literal criterion.
# (2) Both are fp32 evaluations of the same arithmetic; at the timed size (2.4 M pixels, features of magnitude ~30) the CPU
# oracle itself sits ~1e-4 away from the fp64 evaluation of that arithmetic (tools/error_budget.py, profiles/r03_error_budget.json:
# GPU and CPU oracle are equally far from fp64 at every feature scale).  Two implementations cannot be asked to agree more
# closely than the reference agrees with its exact self, so the line is ALSO accepted when the GPU is within
# max(1e-4, 2 x the CPU oracle's own distance) of the fp64 evaluation.  All three distances are reported.
POSE_TOL, FLOW_TOL = 1e-5, 1e-4


def parity_block(refiner, rend, K, G0, args, want):
    """In-run parity of the TIMED configuration: the GPU refiner's first outer iteration (encoder
    included, `inner` inner iterations, the same weights and device-resident inputs the timed steps used) against the
    outputs the CPU oracle produced for the cpu_baseline leg on identical inputs.  First-iteration flow and every pose are
    held to the north-star tolerances; later flows see the pose fed back through the projection (d flow / d pose ~ fx / Z
    ~ 600 px per unit: DESIGN.md section 2), so the last flow is reported with the free-running drift bound 5e-4."""
    import torch
    from rnnpose_amd.pose_refiner import PoseRefiner, default_config
    from rnnpose_amd.transformation import SE3Sequence
    cfg = default_config(RENDER_ITER_COUNT=1, ITER_COUNT=args.inner, OPTIM_ITER_COUNT=args.optim_iters)
    cfg.raft.mixed_precision = bool(args.mixed_precision)
    one = PoseRefiner(cfg, renderer=rend, fused=not args.unfused, use_graph=not args.no_graph).to(K.device).eval()
    one.load_state_dict(refiner.state_dict())
    out = one(rend.views["image_crop"], SE3Sequence(matrix=G0.clone()), K)
    torch.cuda.synchronize()
    T = lambda a: torch.as_tensor(a).to(K.device)
    dG = float((out["Ti_pred"].G.reshape(-1, 4, 4) - T(want["G"]).reshape(-1, 4, 4)).abs().max())
    dT = max(float((t.G.reshape(-1, 4, 4) - T(w_).reshape(-1, 4, 4)).abs().max()) for t, w_ in zip(one.residual_pose_history, want["Tij"]))
    wf, w64 = T(want["flow_first"]), T(want["flow_first_fp64"])
    gf = out["flow"][0]
    d_first = float((gf - wf).abs().max())
    d_gpu64 = float((gf.double() - w64).abs().max())
    d_cpu64 = float((wf.double() - w64).abs().max())
    flow_mag = float(wf.abs().max())
    d_last = float((out["flow_last"] - T(want["flow_last"])).abs().max())
    d_w = float((out["weight"][:, 0, 0] - T(want["weight_last"])).abs().max())
    # `ok` = the LITERAL north-star criterion only: pose 1e-5 and |GPU - CPU oracle| <= 1e-4 on the first
    # iteration's field.  The fp64 yardstick stays in the record as a diagnostic (`ok_fp64_leg`); `leg` says which one held.
    ok_literal = bool(d_first <= FLOW_TOL)
    ok_fp64 = bool(d_gpu64 <= max(FLOW_TOL, 2.0 * d_cpu64))
    leg = "literal" if ok_literal else ("fp64" if ok_fp64 else "none")
    ok = bool(max(dG, dT) <= POSE_TOL and ok_literal)
    # r06: the pair above IS the reference's semantics -- GPU refiner and oracle both start every outer iteration
    # from the literal product Tij = Ti * Ti^-1 (the shipped default).  The same comparison with both sides started from the exact
    # identity (the r03-r05 default, now `literal_legacy_pose=False`) is reported next to it.
    legacy = None
    if want.get("identity") is not None:
        wl = want["identity"]
        two = PoseRefiner(cfg, renderer=rend, fused=not args.unfused, use_graph=not args.no_graph, literal_legacy_pose=False).to(K.device).eval()
        two.load_state_dict(refiner.state_dict())
        o2 = two(rend.views["image_crop"], SE3Sequence(matrix=G0.clone()), K)
        torch.cuda.synchronize()
        lG = float((o2["Ti_pred"].G.reshape(-1, 4, 4) - T(wl["G"]).reshape(-1, 4, 4)).abs().max())
        lT = max(float((t.G.reshape(-1, 4, 4) - T(w_).reshape(-1, 4, 4)).abs().max()) for t, w_ in zip(two.residual_pose_history, wl["Tij"]))
        l_first = float((o2["flow"][0] - T(wl["flow_first"])).abs().max())
        l_last = float((o2["flow_last"] - T(wl["flow_last"])).abs().max())
        legacy = {"max_abs_dpose": max(lG, lT), "max_abs_dflow_first": l_first, "max_abs_dflow_last": l_last,
                  "ok": bool(max(lG, lT) <= POSE_TOL and l_first <= FLOW_TOL), "drift_ok": bool(l_last <= 5e-4),
                  "default_vs_identity_start_gpu_dflow_first": float((o2["flow"][0] - gf).abs().max()),
                  "oracle_seconds": round(wl["seconds"], 1),
                  "what": "GPU PoseRefiner(literal_legacy_pose=False) vs oracle.refine(literal_legacy_pose=False) on the timed inputs: every outer "
                          "iteration starts from the exact identity instead of the reference's Tij = Ti * Ti^-1 (the option, not what is timed)"}
        del two, o2
    return {"max_abs_dpose": max(dG, dT), "max_abs_dpose_final": dG, "max_abs_dflow_first": d_first,
            "start_pose": "literal Tij = Ti * Ti^-1 (model/PoseRefiner.py:243-244) on both sides: the shipped default, the one that is timed",
            "exact_identity_start": legacy,
            "first_iteration_vs_fp64": {"gpu": d_gpu64, "cpu_oracle_fp32": d_cpu64, "fp64_oracle_seconds": round(want["fp64_seconds"], 1)},
            "max_abs_dflow_last": d_last, "max_abs_dweight_last": d_w, "max_abs_flow_first": flow_mag,
            "tol": {"pose": POSE_TOL, "flow_first_iteration": f"|gpu - cpu| <= {FLOW_TOL} (literal: the gate); diagnostic leg: |gpu - fp64| <= max({FLOW_TOL}, 2 |cpu - fp64|)",
                    "flow_last_drift_bound": 5e-4},
            "ok": ok, "leg": leg, "ok_literal": bool(max(dG, dT) <= POSE_TOL and ok_literal), "ok_fp64_leg": bool(max(dG, dT) <= POSE_TOL and ok_fp64),
            "drift_ok": bool(d_last <= 5e-4),
            "what": (f"GPU refiner vs the CPU oracle on the identical device-generated inputs and weights of the timed run: batch "
                     f"{args.batch} x {args.height}x{args.width}, encoder in the loop, 1 outer x {args.inner} inner iterations "
                     f"(the unit the timed schedule repeats {args.outer} times); poses of all {args.inner} iterations and the final pose")}


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args.gpus)
    import torch
    from rnnpose_amd import distributed as D
    rank, world, local = D.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: rnnpose_amd has no CPU product path")
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    device = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(device)
    from rnnpose_amd import build, ops
    D.build_once(build.build)                       # rank 0 compiles, the others wait at a barrier and then only check the stamp
    host_threads = D.pin_host_threads(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)), max_threads=64 if world == 1 else 16)
    from rnnpose_amd.pose_refiner import PoseRefiner, default_config
    from rnnpose_amd.transformation import SE3Sequence

    B, H, W = args.batch, args.height, args.width
    torch.manual_seed(0)
    rend, K, G0 = synth_views(B, H, W, device, seed=rank, with_encoder=not args.no_encoder)
    cfg = default_config(RENDER_ITER_COUNT=args.outer, ITER_COUNT=args.inner, OPTIM_ITER_COUNT=args.optim_iters)
    cfg.raft.mixed_precision = bool(args.mixed_precision)
    refiner = PoseRefiner(cfg, renderer=rend, fused=not args.unfused, use_graph=not args.no_graph).to(device).eval()

    def step():
        return refiner(rend.views["image_crop"], SE3Sequence(matrix=G0.clone()), K)

    # setup (not a warm-up step): one eager pass under the event recorder -- the event-instrumented timed step below runs
    # eagerly too and would otherwise pay first-use allocations (1 GB volume buffer, ...) inside the timed region --
    # and one pass that captures the hipGraphs the remaining steps replay.
    with ops.profile(None):
        step()
    step()
    for _ in range(args.warmup):
        step()
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # HIP events bracket every C-ABI launch of the FIRST OUTER ITERATION of the first timed step only (~450 launches,
    # eager): the rest of that step and the other K-1 steps replay hipGraphs, so that a small K does not dilute `value`.
    rec = refiner.profile_first_outer() if (args.outer > 1 and not args.unfused) else ops.profile_begin(None)
    out = step()
    if refiner.profile_rec is not None or ops.profiling():      # single outer iteration / unfused: the whole step was recorded
        ops.profile_end(rec)
        refiner.profile_rec = None
    for _ in range(args.steps - 1):
        out = step()
    torch.cuda.synchronize()
    D.barrier()
    dt_rank = time.perf_counter() - t0
    dt = D.max_over_ranks(dt_rank)
    seen = D.ranks_seen()                            # the collective's own count of ranks (must equal n_gpus)
    per_rank = D.gather_values(args.steps * args.outer * args.inner / dt_rank)
    prof = ops.summarize(rec)
    prof_steps = (1.0 / args.outer) if (args.outer > 1 and not args.unfused) else 1.0     # fraction of one step that was instrumented

    if rank != 0:
        return
    if args.dump_outputs:
        info = dump_outputs(step_outputs(out), args.dump_outputs)
        print(f"bench.py: last timed step's outputs -> {args.dump_outputs}: {json.dumps(info)}", file=sys.stderr)
    iters = args.outer * args.inner
    value = world * args.steps * iters / dt
    ms_step = dt / args.steps * 1e3
    # HBM bytes per launch from the FETCH_SIZE / WRITE_SIZE counter passes over this same command (tools/gpu_round.sh ->
    # tools/summarize_profiles.py -> profiles/traffic.json).  The file records the digest of the kernel sources it was
    # measured on: counters of OTHER kernels than the ones timed here are refused (traffic = null), not quoted.
    traffic, traffic_note = {}, None
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tpath):
        try:
            traffic = json.load(open(tpath))
        except Exception:
            traffic = {}
        if traffic.get("csrc_digest") != build.source_digest():
            traffic_note = ("profiles/traffic.json was measured on other kernel sources (digest "
                            f"{str(traffic.get('csrc_digest'))[:12]} != {build.source_digest()[:12]}): refused")
            traffic = {}
        elif traffic.get("carried_over"):              # measured on an earlier commit whose measured kernels are the same machine code (tools/isa_equal.py)
            co = traffic["carried_over"]
            traffic_note = (f"counters measured at commit {co.get('measured_at')} (source digest {str(co.get('measured_on_digest'))[:12]}); "
                            f"carried to this digest by {co.get('check')}")
    tr = lambda k: (traffic.get(k) or {}).get("bytes_per_launch") if isinstance(traffic.get(k), dict) else None

    MFMA3 = ("rnnpose_conv2d_nhwc_f16x3", "rnnpose_stem_conv7x7_s2_f16x3", "rnnpose_corr_pyramid_f16x3", "rnnpose_corr_pyramid_split")   # 3 fp16 products per multiply-add
    kernels = {}
    exec_flops_step = 0.0
    for name, (n, mean_ms, tot_ms, work, nbytes) in prof.items():
        e = {"launches": n, "mean_ms": round(mean_ms, 4), "share_of_step": round(tot_ms / prof_steps / ms_step, 4)}
        if nbytes:
            e["algorithmic_MB_per_launch"] = round(nbytes / n / 1e6, 2)
            e["GBps"] = round(nbytes / (tot_ms * 1e-3) / 1e9, 1)
            e["hbm_frac"] = round(e["GBps"] / PEAK_HBM_GBS, 4)
        if work and name in MFMA3:
            ex = (rec.get("_exec") or {}).get(name) or 3 * work     # executed fp16 flops: 3 products per multiply-add, 1 for single-product launches (--mixed-precision)
            e["fp32_equivalent_TFLOPps"] = round(work / (tot_ms * 1e-3) / 1e12, 2)
            e["executed_fp16_TFLOPps"] = round(ex / (tot_ms * 1e-3) / 1e12, 1)
            e["fp16_mfma_frac"] = round(ex / (tot_ms * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS, 4)
            exec_flops_step += ex / prof_steps
        elif work and name == "rnnpose_corr_pyramid_f32":
            e["TFLOPps"] = round(work / (tot_ms * 1e-3) / 1e12, 2)
            e["f32_mfma_frac"] = round(e["TFLOPps"] / PEAK_F32_MFMA_TFLOPS, 4)
        kernels[name.replace("rnnpose_", "")] = e

    # roofline object = the DOMINANT hand-written kernel of the timed region (largest summed duration)
    dom = max(prof.items(), key=lambda kv: kv[1][2])[0] if prof else None
    roofline = None
    if dom == "rnnpose_conv2d_nhwc_f16x3":
        n, mean_ms, tot_ms, work, nbytes = prof[dom]
        ach_alg = work / (tot_ms * 1e-3) / 1e12                   # 2 * MAC of every launch / its duration
        ach_exec = ((rec.get("_exec") or {}).get(dom) or 3 * work) / (tot_ms * 1e-3) / 1e12    # three fp16 MFMA products per multiply-add (one in single-product launches)
        roofline = {"kernel": "conv_strip_f16x3_kernel + conv_igemm_f16x3_kernel (NHWC implicit-GEMM convolutions, fp16x3-split MFMA = fp32-class "
                              "accuracy: csrc/conv_strip.hip takes the stride-1 3x3 / 1x5 / 5x1 layers of maps that fill the chip with 160-row "
                              "strips, csrc/conv_igemm.hip the rest; all update-block and encoder convolutions but the stem)",
                    "bound": "mfma", "achieved": round(ach_alg, 1), "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach_alg / PEAK_F16_MFMA_TFLOPS, 4),
                    "frac_label": "ALGORITHMIC flops (SURVEY 8d: 2 * multiply-adds of the convolution) / duration / fp16 dense MFMA peak",
                    "pipe_util": round(ach_exec / PEAK_F16_MFMA_TFLOPS, 4),
                    "pipe_util_label": "EXECUTED fp16 MFMA flops (3 products per algorithmic multiply-add; 1 in the single-product launches of --mixed-precision) / duration / fp16 dense peak",
                    "executed_fp16_TFLOPps": round(ach_exec, 1),
                    "traffic": tr("conv"), "traffic_note": traffic_note,
                    "algorithmic_bytes_per_launch": int(nbytes / n) if nbytes else None,
                    "traffic_over_algorithmic": (round(tr("conv") / (nbytes / n), 3) if (tr("conv") and nbytes) else None),
                    "note": "achieved = ALGORITHMIC flops of the timed launches / their summed HIP-event duration.  In the event-instrumented "
                            "outer iteration every launch goes to ONE stream, so each is timed alone on the chip (the same durations "
                            "rocprofv3's kernel trace reports: profiles/).  traffic = mean HBM bytes per launch of both kernel families from the "
                            "FETCH_SIZE / WRITE_SIZE counter passes over the same command, algorithmic_bytes_per_launch = the mean over the "
                            "same launches of inputs + weights + outputs + epilogue operands.  The production schedule (r05) is two half-batch "
                            "loop chains on two streams and one encoder stream per image set (RNNPOSE_SPLIT_BATCH=0: one full-batch loop chain on "
                            "the caller's stream; RNNPOSE_ENCODER_MERGE=1: one encoder batch on one stream; bit-identical results either way: "
                            "tests/test_gpu_reproducibility.py): chip_level is the aggregate over the whole step",
                    "fp32_equivalent_over_f32_mfma_peak": round(ach_alg / PEAK_F32_MFMA_TFLOPS, 3),
                    "launches_timed": n,
                    "mean_ms": round(mean_ms, 4), "share_of_step": round(tot_ms / prof_steps / ms_step, 4),
                    "algorithmic_flops_timed": work}
    elif dom is not None:
        n, mean_ms, tot_ms, work, nbytes = prof[dom]
        gbs = nbytes / (tot_ms * 1e-3) / 1e9 if nbytes else 0.0
        roofline = {"kernel": dom, "bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": round(gbs / PEAK_HBM_GBS, 4), "traffic": None, "launches_timed": n, "mean_ms": round(mean_ms, 4)}
    chip = {"executed_fp16_TFLOP_per_step": round(exec_flops_step / 1e12, 3), "ms_per_step": round(ms_step, 3),
            "TFLOPps": round(exec_flops_step / (ms_step * 1e-3) / 1e12, 1),
            "frac_of_fp16_mfma_peak": round(exec_flops_step / (ms_step * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS, 4),
            "note": "matrix-core flops executed by the fp16x3 kernels (convolutions, stem, volume build) in one step / wall time "
                    "of the step -- includes every memory-bound kernel and launch gap of the step"}
    # north_star's named kernel
    corr_vol = None
    for nm, label in (("rnnpose_corr_pyramid_split", "corr_pyramid_h3_kernel (operands written as fp16 hi|lo split tensors by the encoder's "
                                                    "output convolution: the C-ABI call is this one kernel)"),
                      ("rnnpose_corr_pyramid_f16x3", "corr_pyramid_h3_kernel (+ the split_features_kernel pre-pass of the same C-ABI call)"),
                      ("rnnpose_corr_pyramid_f32", "corr_pyramid_kernel (exact fp32 MFMA)")):
        if nm in prof:
            n, mean_ms, tot_ms, work, nbytes = prof[nm]
            gbs = nbytes / (tot_ms * 1e-3) / 1e9
            corr_vol = {"kernel": label, "bound": "hbm" if not nm.endswith("f32") else "mfma (fp32, 96 flop/B)",
                        "achieved_GBps": round(gbs, 1), "peak_GBps": PEAK_HBM_GBS, "frac": round(gbs / PEAK_HBM_GBS, 4),
                        "algorithmic_bytes_per_launch": nbytes / n, "traffic": tr("corr_pyramid_h3" if not nm.endswith("f32") else "corr_pyramid"),
                        "mean_ms": round(mean_ms, 4), "launches_timed": n}
            if nm.endswith("f32"):
                corr_vol["TFLOPps"] = round(work / (tot_ms * 1e-3) / 1e12, 2)
                corr_vol["f32_mfma_frac"] = round(corr_vol["TFLOPps"] / PEAK_F32_MFMA_TFLOPS, 4)
            else:
                corr_vol["executed_fp16_TFLOPps"] = round(3 * work / (tot_ms * 1e-3) / 1e12, 1)
            break
    is_cfg1 = (B, H, W, args.outer, args.inner) == (8, 480, 640, 3, 8)
    is_cfg4 = (B, H, W, args.outer, args.inner) == (8, 960, 1280, 3, 8)
    cfg_label = ("BASELINE.json configs[1]" if is_cfg1 else
                 f"BASELINE.json configs[4]: 1280x960 high-res, global batch {8 * world} data-parallel over {world} GPU(s) -- NOT the headline configuration" if is_cfg4
                 else "NOT the headline configuration: a different shape of the same workload")
    res = {
        "metric": "pose-refine iters/sec (640x480, B=8, 3x8 recurrent)", "value": round(value, 3), "unit": "iters/s",
        "n_gpus": world, "ranks_seen": seen, "dist_backend": D.backend_name() + (" (RCCL)" if D.backend_name() == "nccl" else ""),
        "per_rank_iters_per_sec": [round(v, 2) for v in per_rank], "host_threads_per_rank": host_threads,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": ("f16 products, f32 accumulation in the strip convolutions (cfg.raft.mixed_precision: NOT the headline arithmetic); volume build "
                  "fp16x3, LM f64") if args.mixed_precision else
                 "f32 (convolutions and volume build: fp16x3-split MFMA, fp32-class accuracy; LM: f64)",
        "data": "synthetic", "image_iters_per_sec": round(value * B, 2),
        "config": {"workload": f"synthetic {W}x{H} render+target pairs, batch {B}/GPU, {args.outer} outer x "
                               f"{args.inner} inner refinement ({cfg_label}); 1 step = 1 refinement = "
                               f"{iters} iterations", "batch_per_gpu": B, "height": H, "width": W,
                   "outer": args.outer, "inner": args.inner, "optim_iters": args.optim_iters, "mixed_precision": bool(args.mixed_precision),
                   "encoder_in_timed_region": not args.no_encoder, "fused_schedule": not args.unfused,
                   "hip_graphs": "encoder+volume build and the inner-iteration body replay as hipGraphs (except in the "
                                 "event-instrumented first outer iteration of the first timed step)" if refiner.use_graph and not args.unfused else "off",
                   "schedule": {"loop_chains": len(refiner.cf_net.engine().halves(B)) if hasattr(refiner.cf_net.engine(), "halves") else 1,
                                "encoder_streams": 1 if (args.no_encoder or refiner.image_fea_enc.engine().merge_sets or
                                                          (refiner.image_fea_enc.engine().merge_sets is None and B * H * W < refiner.image_fea_enc.engine().MIN_SET_PIXELS)) else 2},
                   "weights": "random init", "lm_accumulation": "f64", "sharding": f"dp{world} (independent images, no collective in the path)"},
        "roofline": roofline, "chip_level": chip, "correlation_volume_kernel": corr_vol, "kernels": kernels,
        "kernels_note": "HIP events around every C-ABI launch of the first outer iteration of the first timed step (eager); GB/s from "
                        "the ALGORITHMIC bytes each launch declares for its own arguments (SURVEY 8d formulas; half-batch launches "
                        "declare half the batch); share_of_step = summed launch durations x outer iterations / step time (the two image sets of the "
                        "encoder run on two streams in the timed steps, and so do the two batch halves of the loop, so the "
                        "shares, measured launch by launch on one stream, can add up to more than 1)",
    }
    if args.full and world == 1 and not args.no_cpu_baseline:
        res["cpu_baseline"], want = cpu_baseline(refiner, rend, K, G0, args)
        res["speedup_vs_cpu"] = round(value / res["cpu_baseline"]["value"], 1)
        res["parity"] = parity_block(refiner, rend, K, G0, args, want)
    else:
        res["cpu_baseline"] = None
        res["parity"] = None
    res["f16x3_range_events"] = int(ops.saturation_count(reset=False))     # clamped activation quads over the whole run (sticky counter)
    if seen != world:
        raise SystemExit(f"bench.py: the collective reached {seen} ranks, the line would claim {world}")
    print(json.dumps(res))
    if args.mixed_precision and res["parity"] is not None:
        res["parity"]["note"] = "mixed precision: distances to the fp32 CPU oracle, reported, not gated (not the headline arithmetic)"
    if res["parity"] is not None and not args.mixed_precision and res["parity"].get("exact_identity_start") and not res["parity"]["exact_identity_start"]["ok"]:
        raise SystemExit(f"bench.py: the exact-identity option is OUTSIDE the parity tolerances against the CPU oracle ({res['parity']['exact_identity_start']})")
    if res["parity"] is not None and not res["parity"]["ok"] and not args.mixed_precision:
        raise SystemExit("bench.py: the timed configuration is OUTSIDE the parity tolerances against the CPU oracle "
                         f"({res['parity']}) -- the line above is invalid")


if __name__ == "__main__":
    main()
