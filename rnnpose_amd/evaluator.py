"""LINEMOD pose evaluation on device ("next" rows): the per-sample metrics of
utils/eval_metric.py:102-192 (`LineMODEvaluator`) with model points resident on the GPU, plus the mirror of
thirdparty/nn/nn_utils.py:6-24 (`find_nearest_point_idx`) over the drop-in `findNearestPointIdxLauncher`.

Only the metric arithmetic is rebuilt; PLY loading, ICP refinement and visualisation stay outside (out of scope).

`BOPEvaluator`: the three BOP pose-error functions -- VSD, MSSD, MSPD -- and their recalls on device (csrc/eval_metrics.hip,
definitions in include/rnnpose_hip.h).  The reference has no code for them; parity with bop_toolkit is unpinned.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .distributed import METRICS, MetricAccumulator

SYMMETRIC_CLASSES = ("eggbox", "glue")                      # utils/eval_metric.py:329
LINEMOD_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], dtype=np.float32)
#                                                           data/linemod/linemod_config.py:23-25


def find_nearest_point_idx(ref_pts: np.ndarray, que_pts: np.ndarray) -> np.ndarray:
    """numpy in / numpy out, same contract as thirdparty/nn/nn_utils.py:6-24 (host buffers, synchronous)."""
    assert ref_pts.shape[1] == que_pts.shape[1] and 1 < que_pts.shape[1] <= 3
    pn1, pn2, dim = ref_pts.shape[0], que_pts.shape[0], ref_pts.shape[1]
    ref = np.ascontiguousarray(ref_pts[None], np.float32)
    que = np.ascontiguousarray(que_pts[None], np.float32)
    idxs = np.zeros([1, pn2], np.int32)
    _lib.load().findNearestPointIdxLauncher(ref.ctypes.data_as(C.c_void_p), que.ctypes.data_as(C.c_void_p),
                                           idxs.ctypes.data_as(C.c_void_p), 1, pn1, pn2, dim, 0)
    return idxs[0]


class LineMODEvaluator:
    """evaluate(pose_pred (B,3,4), pose_gt (B,3,4)) accumulates ADD(-S) @0.1/0.02/0.05 d, proj2d<5px, 5cm5deg."""

    def __init__(self, class_name: str, model_points, diameter: float, K=None, device="cuda"):
        self.class_name = class_name
        self.symmetric = class_name in SYMMETRIC_CLASSES
        self.model = torch.as_tensor(np.asarray(model_points, dtype=np.float32)).to(device)
        self.diameter = float(diameter)
        self.K = torch.as_tensor(LINEMOD_K if K is None else np.asarray(K, dtype=np.float32)).to(device)
        self.acc = MetricAccumulator((class_name,))
        self.last = None

    def evaluate(self, pose_pred, pose_gt, unique=None):
        m = ops.pose_metrics(self.model, pose_pred[..., :3, :].reshape(-1, 3, 4), pose_gt[..., :3, :].reshape(-1, 3, 4),
                             self.K, self.symmetric)
        self.last = m
        dist = m[:, 1] if self.symmetric else m[:, 0]
        flags = torch.stack([dist < 0.1 * self.diameter, dist < 0.02 * self.diameter, dist < 0.05 * self.diameter,
                             m[:, 2] < 5.0, (m[:, 3] < 5.0) & (m[:, 4] < 5.0)], 1).cpu().numpy()   # one D2H per batch
        for i, row in enumerate(flags):
            self.acc.update(self.class_name, dict(zip(METRICS, row.astype(float))),
                            unique=True if unique is None else bool(unique[i]))
        return m

    def summarize(self):
        """Cross-rank means (one RCCL all-reduce) with the reference's key names (utils/eval_metric.py:261-302)."""
        r = self.acc.reduce()[self.class_name]
        return {"proj2d": r["proj2d"], "add": r["add"], "add2": r["add2"], "add5": r["add5"], "cmd5": r["cmd5"],
                "seq_len": r["n"]}


# ---- BOP pose-error functions and their recalls ----------------------------------------------------------------------------
BOP_TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))          # VSD misalignment tolerances (fractions of the diameter)
BOP_THETAS = BOP_TAUS                                               # correctness thresholds of VSD; x diameter for MSSD
BOP_THETAS_PX = tuple(float(5 * k) for k in range(1, 11))           # MSPD thresholds in pixels of a 640-wide image
BOP_DELTA = 0.015                                                   # VSD visibility tolerance: 15 mm in metres


def bop_recalls(vsd, mssd, mspd, diameters, width, vsd_thetas=BOP_THETAS, mssd_thetas=BOP_THETAS, mspd_thetas=BOP_THETAS_PX):
    """Per-sample recalls of the BOP errors, host fp64: vsd (B,NT), mssd (B), mspd (B), diameters (B) or a number, width the image
    width in pixels -> (B,3) [AR_VSD, AR_MSSD, AR_MSPD]:
      AR_VSD  = mean over the NT taus and the thetas of  err_tau < theta
      AR_MSSD = mean over theta of  MSSD < theta * diameter
      AR_MSPD = mean over theta of  MSPD < theta * (width / 640)
    A NaN error is never below a threshold: it counts as a miss."""
    vsd = np.asarray(vsd, dtype=np.float64)
    vsd = vsd.reshape(vsd.shape[0], -1)
    B = vsd.shape[0]
    mssd, mspd = np.asarray(mssd, dtype=np.float64).reshape(B), np.asarray(mspd, dtype=np.float64).reshape(B)
    d = np.broadcast_to(np.asarray(diameters, dtype=np.float64).reshape(-1), (B,))
    tv, ts, tp = (np.asarray(t, dtype=np.float64) for t in (vsd_thetas, mssd_thetas, mspd_thetas))
    out = np.empty((B, 3), np.float64)
    out[:, 0] = (vsd[:, :, None] < tv[None, None, :]).mean((1, 2))
    out[:, 1] = (mssd[:, None] < ts[None, :] * d[:, None]).mean(1)
    out[:, 2] = (mspd[:, None] < tp[None, :] * (float(width) / 640.0)).mean(1)
    return out


class BOPAccumulator:
    """Per-key (class) running sums [sum AR_VSD, sum AR_MSSD, sum AR_MSPD, n] in fp64; reduce() is ONE all_reduce(SUM).  Its own
    buffer: distributed.METRICS and MetricAccumulator's packed layout are not involved."""

    def __init__(self, keys):
        self.keys = tuple(keys)
        self.sums = torch.zeros(len(self.keys), 4, dtype=torch.float64)

    def update(self, key, recalls, unique=True):
        if unique:
            r = self.keys.index(key)
            self.sums[r, :3] += torch.as_tensor(np.asarray(recalls, dtype=np.float64).reshape(3))
            self.sums[r, 3] += 1.0

    def reduce(self, device=None):
        """-> {key: {"ar_vsd", "ar_mssd", "ar_mspd", "ar" (the mean of the three), "n"}} plus "all": the same over every sample."""
        import torch.distributed as dist
        buf = self.sums.clone()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else "cpu"
            buf = buf.to(device)
            dist.all_reduce(buf, op=dist.ReduceOp.SUM)
            buf = buf.cpu()

        def row(v):
            n = float(v[3])
            m = [float(x) / n if n > 0 else float("nan") for x in v[:3]]
            return {"ar_vsd": m[0], "ar_mssd": m[1], "ar_mspd": m[2], "ar": (m[0] + m[1] + m[2]) / 3.0, "n": int(n)}
        out = {k: row(buf[r]) for r, k in enumerate(self.keys)}
        out["all"] = row(buf.sum(0))
        return out


class BOPEvaluator:
    """VSD / MSSD / MSPD of a batch of poses of any classes, on device.

        ev = BOPEvaluator(renderer, models)                  # renderer: the MeshRenderer that holds the meshes; models: {name: m}
        e = ev.errors(names, pose_est, pose_gt, K, depth_obs, src_index)
        r = ev.recalls(e, [models[n].diameter for n in names], width)
        ev.update(names, r); ev.summarize()

    models[name] has .verts or .eval_points (the model points of MSSD / MSPD), .diameter and optionally .symmetries (S,4,4) -- the
    discretised symmetry transformations, identity included; None = no symmetry (eval_epoch.ClassModel).
    delta is in the meshes' length unit (15 mm); VSD distances are normalised by the diameter."""

    def __init__(self, renderer, models, device="cuda", delta=BOP_DELTA, taus=BOP_TAUS, vsd_thetas=BOP_THETAS, mssd_thetas=BOP_THETAS,
                 mspd_thetas=BOP_THETAS_PX, near=0.1):
        self.renderer = renderer
        self.device = torch.device(device)
        self.delta, self.taus, self.near = float(delta), tuple(float(t) for t in taus), float(near)
        self.thetas = (tuple(vsd_thetas), tuple(mssd_thetas), tuple(mspd_thetas))
        self.points, self.sym, self.diameter = {}, {}, {}
        for n, m in models.items():
            pts = getattr(m, "eval_points", None)
            pts = m.verts if pts is None else pts
            self.points[n] = torch.as_tensor(np.ascontiguousarray(pts, dtype=np.float32)).to(self.device)
            sy = getattr(m, "symmetries", None)
            sy = np.eye(4, dtype=np.float32)[None] if sy is None else np.asarray(sy, dtype=np.float32).reshape(-1, 4, 4)
            if sy.shape[0] < 1:
                raise ValueError(f"BOPEvaluator: {n!r} has an empty symmetry set (pass the identity)")
            self.sym[n] = torch.as_tensor(np.ascontiguousarray(sy[:, :3, :])).to(self.device)
            self.diameter[n] = float(m.diameter)
        self.acc = BOPAccumulator(sorted(models))

    def errors(self, names, pose_est, pose_gt, K, depth_obs, src_index=None):
        """names: B class names; pose_est / pose_gt (B,3,4) or (B,4,4); K (3,3) or (B,3,3); depth_obs (H,W) or (S,H,W) observed
        depth in the meshes' unit; src_index (ops.SourceIndex, B integers or None): which observed map each sample is compared to
        (None: the only one, or sample b's own when S == B).
        Both model depth images are rendered at the frame size by the renderer's z-buffer path (empty pixels = -1).
        -> {"vsd" (B,NT) fp64, "mssd" (B) fp64, "mspd" (B) fp64 px, "counts" (B,2+NT) int64} on the device."""
        dev = self.device
        B = len(names)
        pe = torch.as_tensor(pose_est).to(dev).float().reshape(B, -1, 4)[:, :3].contiguous()
        pg = torch.as_tensor(pose_gt).to(dev).float().reshape(B, -1, 4)[:, :3].contiguous()
        K = torch.as_tensor(K).to(dev).float()
        K = (K.expand(B, 3, 3) if K.dim() == 2 else K).contiguous()
        obs = torch.as_tensor(depth_obs).to(dev).float()
        obs = (obs[None] if obs.dim() == 2 else obs.reshape(-1, obs.shape[-2], obs.shape[-1])).contiguous()
        S, H, W = obs.shape
        if src_index is None:
            if S not in (1, B):
                raise ValueError(f"BOPEvaluator.errors: {S} observed maps for {B} samples need a src_index")
            src_index = [0] * B if S == 1 else list(range(B))
        if not isinstance(src_index, ops.SourceIndex):
            src_index = ops.SourceIndex(src_index, S, dev)
        d_est = self.renderer.render_zbuf(names, pe, K, (H, W), near=self.near)[:, 0]
        d_gt = self.renderer.render_zbuf(names, pg, K, (H, W), near=self.near)[:, 0]
        diam = torch.tensor([self.diameter[n] for n in names], dtype=torch.float32, device=dev)
        vsd, counts = ops.bop_vsd(d_est, d_gt, obs, src_index, K, diam, self.delta, self.taus)
        sd = torch.empty(B, 2, dtype=torch.float64, device=dev)
        for c in sorted(set(names)):                                 # one launch pair per class of the batch
            rows = [j for j, n in enumerate(names) if n == c]
            r = torch.tensor(rows, dtype=torch.long, device=dev)
            sd[r] = ops.bop_sym_dist(self.points[c], self.sym[c], pe[r], pg[r], K[r])
        return {"vsd": vsd, "mssd": sd[:, 0], "mspd": sd[:, 1], "counts": counts}

    def recalls(self, errors, diameters, width):
        """errors of `errors()` (one device->host copy here) -> (B,3) fp64 numpy [AR_VSD, AR_MSSD, AR_MSPD] (bop_recalls)."""
        host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        return bop_recalls(host(errors["vsd"]), host(errors["mssd"]), host(errors["mspd"]), diameters, width, *self.thetas)

    def update(self, names, recalls, unique=None):
        for j, n in enumerate(names):
            self.acc.update(n, recalls[j], unique=True if unique is None else bool(unique[j]))

    def summarize(self, device=None):
        """Cross-rank per-class and overall mean recalls: ONE all_reduce of the (classes x 4) fp64 buffer."""
        return self.acc.reduce(device=device)
