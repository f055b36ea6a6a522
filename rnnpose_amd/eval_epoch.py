"""One evaluation epoch: what tools/eval.py does between `mp.spawn` and the printed per-class table.

    reference                                                         here
    tools/eval.py:224-225   one process per GPU (mp.spawn)            torchrun / bench-style spawn; rank, world from the env
    tools/eval.py:305-316   init_process_group("nccl")                distributed.init_from_env (RCCL; gloo on CPU)
    tools/eval.py:471       DistributedSequatialSampler               distributed.shard_indices (rank-strided, wrap-around
                            (utils/distributed_utils.py:150-169)      duplicates flagged so that they can be masked)
    model/RNNPose.py:157-222  one batch = ONE object class: views     batches of one class -> PoseRefiner(image, Ts, K, fea_3d,
                            from the class model, PoseRefiner(...)    Tj_gt, obj_cls, geofea_3d, geofea_2d) through its renderer
    utils/eval_metric.py:306-356  LineMODEvaluator.evaluate per       evaluator.LineMODEvaluator (csrc/eval_metrics.hip), batched
                            sample (ADD / ADD-S / proj2d / 5cm5deg)
    tools/train.py:725-741  two scalar all_gathers per metric         ONE all_reduce(SUM) of a packed fp64 vector at the end
    (tools/eval.py itself prints per-rank means, :560-562)            of the epoch (MetricAccumulator.reduce)

Datasets (`EXPDATA`) and trained weights are absent from this build: `synthetic_dataset` makes a closed-form stand-in
(ellipsoid meshes per class, ground-truth poses, perturbed initial poses, images rendered by the same HIP rasteriser at the
ground-truth pose) so that the whole epoch -- sharding, per-class batching, refinement, metrics, reduction -- runs end to end
on any number of ranks; `data_io` reads the reference's on-disk formats the day real data is supplied.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np
import torch

from . import distributed as D
from .distributed import METRICS, MetricAccumulator


@dataclass
class ClassModel:
    """What model/RNNPose.py:160-189 looks up per object class: mesh, per-vertex context / geometric features, diameter."""
    name: str
    verts: np.ndarray            # (P,3) float32, metres
    faces: np.ndarray            # (F,3) int32
    colors: np.ndarray           # (P,3) in [0,1]
    fea_3d: torch.Tensor         # (1,P,256) context features sampled on the vertices
    geofea_3d: torch.Tensor      # (1,P,32) geometric descriptors of the vertices
    diameter: float
    eval_points: np.ndarray = None   # model points of the metric (defaults to verts)
    verts_uvs: np.ndarray = None     # (U,2) texture coordinates of a textured model (mesh_io.load_obj), else None
    faces_uvs: np.ndarray = None     # (F,3) int32 uv rows of each face
    texture: np.ndarray = None       # (Ht,Wt,3) float32 in [0,1], the class's texture map
    symmetries: np.ndarray = None    # (S,4,4) symmetry transformations of the BOP errors, identity included (None: no symmetry)


@dataclass
class EvalItem:
    """One evaluation sample (data/linemod_dataset.py:311-343 after preprocessing)."""
    class_name: str
    image: torch.Tensor          # (3,H,W) observed image
    K: np.ndarray                # (3,3)
    pose_init: np.ndarray        # (4,4) initial pose (PoseCNN / PVNet in the reference); None: HipEpoch(init=...) finds one inside `bbox`
    pose_gt: np.ndarray          # (4,4)
    geofea_2d: torch.Tensor      # (32,H,W) descriptors of the observed image (None: HipEpoch(desc2d=...) computes them)
    frame_id: int | None = None  # camera frame the object was seen in: items of one frame share `image` / `geofea_2d` (None: its own)
    depth: torch.Tensor | None = None   # (H,W) observed depth of the frame in the meshes' unit, 0 = missing; shared like `image` (BOP VSD)
    object_id: object = None     # views of ONE physical object from several calibrated cameras share it (None: the item is its own object)
    cam_from_rig: np.ndarray | None = None   # (4,4) camera-from-rig transform of the item's camera (None: the identity)
    bbox: np.ndarray | None = None   # [xmin, ymin, xmax, ymax] inclusive pixels: the detector's box, where an item without pose_init is matched


class PackedEpochMetrics:
    """Initial-pose and refined-pose statistics of every class in ONE packed fp64 buffer -> one all_reduce per epoch."""

    def __init__(self, classes):
        self.classes = tuple(classes)
        self.init = MetricAccumulator(self.classes)
        self.refined = MetricAccumulator(self.classes)

    def reduce(self, device=None):
        both = MetricAccumulator(tuple(f"{k}/{c}" for k in ("init", "refined") for c in self.classes))
        both.sums = torch.cat([self.init.sums, self.refined.sums], 0)
        r = both.reduce(device=device)
        return {k: {c: r[f"{k}/{c}"] for c in self.classes} for k in ("init", "refined")}


def class_batches(items, indices, unique, batch_size):
    """The shard's samples as batches of ONE class each (model/RNNPose.py:158 asserts a single class per batch), in shard
    order: -> [(class, [item index], [unique flag])]."""
    out = []
    for i, u in zip(indices, unique):
        c = items[i].class_name
        if out and out[-1][0] == c and len(out[-1][1]) < batch_size:
            out[-1][1].append(i)
            out[-1][2].append(u)
        else:
            out.append((c, [i], [u]))
    return out


def frame_batches(items, indices, unique, batch_size):
    """The shard's samples as batches of ONE CAMERA FRAME each, whatever the classes of its objects, in shard order:
    consecutive shard items with the same non-None `frame_id` share a batch (a frame with more than batch_size objects is
    split); items without a frame id batch as class_batches does.  -> [(None | class, [item index], [unique flag])]: None
    marks a frame batch (mixed classes, one shared image)."""
    out, keys = [], []
    for i, u in zip(indices, unique):
        f = items[i].frame_id
        key = ("frame", f) if f is not None else ("class", items[i].class_name)
        if out and keys[-1] == key and len(out[-1][1]) < batch_size:
            out[-1][1].append(i)
            out[-1][2].append(u)
        else:
            out.append((None if f is not None else items[i].class_name, [i], [u]))
            keys.append(key)
    return out


def flags_from_metrics(m, diameter, symmetric):
    """(B,5) [ADD, ADD-S, proj2d px, translation cm, rotation deg] -> (B,5) 0/1 flags in METRICS order
    (utils/eval_metric.py:102-192: ADD(-S) < 10 % / 2 % / 5 % of the diameter, proj2d < 5 px, 5 cm 5 deg)."""
    m = np.asarray(m, dtype=np.float64)
    dist = m[:, 1] if symmetric else m[:, 0]
    return np.stack([dist < 0.1 * diameter, dist < 0.02 * diameter, dist < 0.05 * diameter, m[:, 2] < 5.0,
                     (m[:, 3] < 5.0) & (m[:, 4] < 5.0)], 1).astype(np.float64)


def run_epoch(items, models, refine_fn, metric_fn, rank=0, world=1, batch_size=8, symmetric=(), reduce_device=None, group="class",
              bop_fn=None):
    """items: list[EvalItem]; models: {class: ClassModel};
    refine_fn(class_name, [EvalItem]) -> (B,4,4) refined poses (numpy or tensor): one PoseRefiner call per batch;
    metric_fn(class_name, pose_pred (B,4,4), pose_gt (B,4,4)) -> (B,5) [ADD, ADD-S, proj2d, t cm, r deg].
    group="class": batches of one class (the reference's restriction).  group="frame": frame_batches -- the objects of one
    camera frame in one batch whatever their classes; refine_fn is then called as refine_fn(None, batch) (HipEpoch.refine_frame
    behind `lambda _, batch: epoch.refine_frame(batch)`) and every item's metrics are booked under its own class, with that
    class's diameter and symmetry.
    -> {"init": {cls: {metric: mean, "n": count}}, "refined": {...}} identical on every rank (wrap-around duplicates of the
    sampler are excluded from the sums).
    bop_fn(batch [EvalItem], poses (B,4,4)) -> (B,3) per-sample recalls [AR_VSD, AR_MSSD, AR_MSPD] (HipEpoch.bop_metrics): the
    result gains "bop": {"init" | "refined": {cls: {"ar_vsd", "ar_mssd", "ar_mspd", "ar", "n"}, "all": {...}}} from one more
    all_reduce of a (2 x classes x 4) fp64 buffer.  None (the default): no such entry and no such collective."""
    if group not in ("class", "frame"):
        raise ValueError(f"group must be 'class' or 'frame', got {group!r}")
    classes = sorted(models)
    idx, uniq = D.shard_indices(len(items), rank, world)
    acc = PackedEpochMetrics(classes)
    bop = None
    if bop_fn is not None:
        from .evaluator import BOPAccumulator
        bop = BOPAccumulator(tuple(f"{k}/{c}" for k in ("init", "refined") for c in classes))
    batches = class_batches(items, idx, uniq, batch_size) if group == "class" else frame_batches(items, idx, uniq, batch_size)
    for cls, ids, us in batches:
        batch = [items[i] for i in ids]
        gt = np.stack([it.pose_gt for it in batch]).astype(np.float32)
        init = np.stack([it.pose_init for it in batch]).astype(np.float32)
        pred = refine_fn(cls if group == "class" else None, batch)
        pred = pred.detach().cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
        pred = pred.reshape(-1, 4, 4)
        for c in sorted({it.class_name for it in batch}):           # one class in a class batch; per-item classes in a frame batch
            rows = [j for j, it in enumerate(batch) if it.class_name == c]
            sym = c in symmetric
            for which, poses in ((acc.init, init), (acc.refined, pred)):
                fl = flags_from_metrics(metric_fn(c, poses[rows], gt[rows]), models[c].diameter, sym)
                for row, j in zip(fl, rows):
                    which.update(c, dict(zip(METRICS, row)), unique=us[j])
        if bop is not None:
            for which, poses in (("init", init), ("refined", pred)):
                rec = np.asarray(bop_fn(batch, poses), dtype=np.float64).reshape(len(batch), 3)
                for j, it in enumerate(batch):
                    bop.update(f"{which}/{it.class_name}", rec[j], unique=us[j])
    result = acc.reduce(device=reduce_device)
    if bop is not None:
        r = bop.reduce(device=reduce_device)
        result["bop"] = {}
        for k in ("init", "refined"):
            per = {c: r[f"{k}/{c}"] for c in classes}
            n = sum(v["n"] for v in per.values())
            tot = [sum(v[m] * v["n"] for v in per.values() if v["n"]) / n if n else float("nan") for m in ("ar_vsd", "ar_mssd", "ar_mspd")]
            per["all"] = {"ar_vsd": tot[0], "ar_mssd": tot[1], "ar_mspd": tot[2], "ar": sum(tot) / 3.0, "n": n}
            result["bop"][k] = per
    return result


# ---- the GPU pieces behind refine_fn / metric_fn ---------------------------------------------------------------------
class HipEpoch:
    """PoseRefiner on the HIP mesh rasteriser + device metrics: the refine_fn / metric_fn pair of run_epoch."""

    def __init__(self, models, cfg=None, device="cuda", refiner=None, symmetric=("eggbox", "glue"), desc2d=None, occlusion=None,
                 occlusion_margin=0.0, depth_term=None, init=None, score=False, init_candidates=1, init_select="score"):
        """init_candidates = N > 1: an item without a pose gets the N best DISTINCT RANSAC hypotheses of its box
        (DescriptorPoseInitializer.candidates) instead of the cheapest one.  init_select="score": all n * N of them are scored against
        the frames in ONE PoseScorer call and every item starts from its highest-scoring valid one (the lowest slot on a tie).
        init_select="refined" (refine_frame only; `refine` and `initial_poses` select by the score): refine_frame refines ALL N starts
        of such an item in the same refiner call, scores the refined poses and returns the best valid one per item.  The record
        `last_init_info` gains candidates (n,N,4,4), candidate_scores (n,N), candidate_valid (n,N) and selected (n).  With
        init_candidates=1 (the default) nothing new runs.
        score: True or a pose_score.PoseScorer -- `refine` and `refine_frame` also score the poses they return against their frames
        (the object's descriptors and depth rendered under the pose, compared with the frame's descriptor map and,
        where every item has one, its observed depth) and leave the scores in `last_scores`, the record in `last_score_info`.  False (the
        default): nothing new runs and `last_scores` stays None; `score_poses` / `select_poses` work either way.
        init: "descriptors" or a pose_init.DescriptorPoseInitializer -- items whose pose_init is None get their start from the frame's
        descriptor map inside their `bbox` (2D-3D matches, P3P RANSAC, polish; `initial_poses`); the record of the
        last such call is in `last_init_info`.  None (the default): every item must bring its pose_init, and nothing new runs.
        depth_term (PoseRefiner's argument: True or a dict of depth_weight / depth_gate / edge_tol): `refine` and `refine_frame`
        hand the frames' observed depth (EvalItem.depth) to the refiner, whose LM steps then carry its 3-D residual; an item without
        depth raises ValueError.  The statistics of the last call are in `last_depth_stats`.
        occlusion="frame" (PoseRefiner's argument; occlusion_margin in the models' length unit): refine_frame masks the pixels of
        every object that another object of the same frame hides under the current pose estimates.  `refine` -- one class per
        batch, one image per object -- has no pairs and is unaffected.  With a ready-made `refiner`, set it there."""
        from .evaluator import LineMODEvaluator
        from .pose_refiner import PoseRefiner, default_config
        from .rasterizer import MeshRenderer
        self.models = models
        self.device = torch.device(device)
        # textured models render as the reference's SoftPhongShader does; without one, the flat vertex-colour path as before
        shading = "phong" if any(m.texture is not None for m in models.values()) else "flat"
        self.renderer = MeshRenderer({n: dict(verts=m.verts, faces=m.faces, colors=m.colors, verts_uvs=m.verts_uvs,
                                              faces_uvs=m.faces_uvs, texture=m.texture) for n, m in models.items()},
                                     device=device, shading=shading)
        self.cfg = cfg if cfg is not None else default_config()
        if refiner is not None and occlusion is not None:
            raise ValueError("HipEpoch(refiner=..., occlusion=...): construct the refiner with occlusion= instead")
        if refiner is not None and depth_term is not None:
            raise ValueError("HipEpoch(refiner=..., depth_term=...): construct the refiner with depth_term= instead")
        self.refiner = refiner if refiner is not None else \
            PoseRefiner(self.cfg, renderer=self.renderer, occlusion=occlusion, occlusion_margin=occlusion_margin,
                        depth_term=depth_term).to(self.device).eval()
        if isinstance(init, str):
            if init != "descriptors":
                raise ValueError(f"init must be None, 'descriptors' or a DescriptorPoseInitializer, got {init!r}")
            from .pose_init import DescriptorPoseInitializer
            init = DescriptorPoseInitializer(models, device=self.device, pixel_center=getattr(self.renderer, "pixel_center", 0.5),
                                             top_k=init_candidates)
        self.init = init
        self.init_candidates, self.init_select = int(init_candidates), init_select
        if init_select not in ("score", "refined"):
            raise ValueError(f"init_select must be 'score' or 'refined', got {init_select!r}")
        if self.init_candidates < 1 or (self.init_candidates > 1 and (init is None or getattr(init, "top_k", 1) != self.init_candidates)):
            raise ValueError(f"init_candidates={init_candidates} needs init='descriptors' or a DescriptorPoseInitializer(top_k={init_candidates})")
        self.last_init_info = None        # initial_poses / refine / refine_frame: the record of the LAST such call (None: it initialised nothing)
        if score is True:
            from .pose_score import PoseScorer
            score = PoseScorer(self.renderer, models, device=self.device)
        self.scorer = score or None       # refine / refine_frame score their results with it; None: they do not
        self._default_scorer = None       # score_poses / select_poses without one: made on their first call
        self.last_scores = None           # refine / refine_frame with a scorer: (B) fp64 scores of the poses they returned, in batch order
        self.last_score_info = None       # the record of the LAST scoring call (PoseScorer.__call__)
        self.last_depth_stats = None
        self.last_rig_poses = None        # refine_frame with multi-view items: T_rig (n_groups,4,4) of the last call, groups in order of first appearance
        self._view_groups = {}            # ops.ViewGroups by (layout, transforms): the same rig keeps its device arrays, so captured graphs replay
        self.symmetric = tuple(symmetric)
        # desc2d: a descriptor2d.SuperPoint2D -- items without geofea_2d get theirs from the batch image on the device, as
        # model/RNNPose.py:162 computes them (HybridNet.py:97 keeps the descriptors only)
        self.desc2d = desc2d
        self._frame_tables = None         # refine_frame: resident or per-object, decided on its first call
        self.evaluators = {n: LineMODEvaluator(n, m.eval_points if m.eval_points is not None else m.verts, m.diameter,
                                               device=device) for n, m in models.items()}
        for n, e in self.evaluators.items():
            e.symmetric = n in self.symmetric
        self.bop = None                   # bop_metrics: the BOPEvaluator, made on its first call

    def refine(self, cls, batch):
        from .transformation import SE3Sequence
        dev, m = self.device, self.models[cls]
        image = torch.stack([it.image for it in batch]).to(dev)
        missing = [j for j, it in enumerate(batch) if it.geofea_2d is None]
        if missing and self.desc2d is None:
            raise ValueError("items without geofea_2d need HipEpoch(desc2d=SuperPoint2D(...))")
        if missing:
            fresh = self.desc2d.descriptors(image.float() if len(missing) == len(batch) else image[missing].float())
            if len(missing) == len(batch):
                g2 = fresh
            else:
                given = iter(it.geofea_2d for it in batch if it.geofea_2d is not None)
                got = iter(fresh)
                g2 = torch.stack([next(got) if it.geofea_2d is None else next(given).to(dev) for it in batch])
        else:
            g2 = torch.stack([it.geofea_2d for it in batch]).to(dev)
        K = torch.as_tensor(np.stack([it.K for it in batch]).astype(np.float32)).to(dev)
        T0 = self._start_poses(batch, g2, list(range(len(batch))), K, firsts=batch)
        Tg = torch.as_tensor(np.stack([it.pose_gt for it in batch]).astype(np.float32)).to(dev)
        out = self.refiner(image, SE3Sequence(matrix=T0[:, None]), K, fea_3d=m.fea_3d.to(dev), Tj_gt=SE3Sequence(matrix=Tg[:, None]),
                           obj_cls=[cls] * len(batch), geofea_3d=m.geofea_3d.to(dev), geofea_2d=g2, **self._observed_depth(batch))
        self.last_depth_stats = out.get("depth_stats")
        poses = out["Ti_pred"].G.reshape(-1, 4, 4)
        self.last_scores = None if self.scorer is None else self.score_poses(batch, poses, scorer=self.scorer)
        return poses

    def _start_poses(self, batch, g2, index, K, skip=(), caller_row=None, firsts=None):
        """(B,4,4) start poses on the device: every item's pose_init; the items without one (rows in `skip` excepted: they get the
        identity, their start comes from elsewhere) are initialised from the descriptor maps g2 (S,32,H,W) through `index`.
        `last_init_info` becomes the record of this call -- its arrays in ascending order of `rows`, the rows of the CALLER's batch
        (caller_row[j] = the caller's row of item j, where the batch was regrouped) -- or None when nothing was initialised.
        firsts: the items the frames of g2 came from (their observed depth goes into the candidates' scores, init_candidates > 1)."""
        dev = self.device
        self.last_init_info = None
        need = [j for j, it in enumerate(batch) if it.pose_init is None and j not in skip]
        bad = [j for j in need if self.init is None or batch[j].bbox is None]
        if bad:
            raise ValueError(f"items {bad} have no pose_init: they need a bbox and HipEpoch(init='descriptors' or a DescriptorPoseInitializer)")
        eye = np.eye(4, dtype=np.float32)
        T0 = torch.as_tensor(np.stack([eye if it.pose_init is None else np.asarray(it.pose_init, np.float32) for it in batch])).to(dev)
        if need:
            boxes = np.stack([np.asarray(batch[j].bbox).astype(np.int32).reshape(4) for j in need])
            rows = torch.as_tensor(need, device=dev)
            args = ([batch[j].class_name for j in need], g2, [index[j] for j in need], K[rows].contiguous(), boxes)
            if self.init_candidates > 1:
                Ti, rec = self._select_by_score([batch[j] for j in need], *args, firsts)
            else:
                Ti, rec = self.init(*args)
            T0[rows] = Ti
            rows = np.asarray(need if caller_row is None else [caller_row[j] for j in need])
            by_row = np.argsort(rows, kind="stable")
            rec = {k: np.asarray(v)[by_row] for k, v in rec.items()}
            rec["rows"] = rows[by_row]
            self.last_init_info = rec
        return T0

    def _select_by_score(self, items, names, g2, index, K, boxes, firsts):
        """The N candidates of every item, all scored in ONE PoseScorer call on the frames' maps (with the observed depth where every
        frame has one) -> (the highest-scoring VALID candidate of every item, the lowest slot on a tie; the record of `candidates` with
        its per-slot arrays reduced to the selected slot, plus candidates, candidate_scores, candidate_valid, selected)."""
        cand, rec = self.init.candidates(names, g2, index, K, boxes)
        n, N = cand.shape[:2]
        depth = None if firsts is None or any(it.depth is None for it in firsts) else \
            torch.stack([it.depth for it in firsts]).to(self.device).float().contiguous()
        scores = self._score(items, cand.reshape(n * N, 4, 4), N, None, maps=(g2, index, depth)).reshape(n, N).cpu().numpy()
        sel = self._best_valid(scores, rec["valid"])
        pick = np.arange(n)
        out = dict(count=rec["count"], n_inliers=rec["n_inliers"][pick, sel], final_cost=rec["final_cost"][pick, sel], info=rec["info"][pick, sel],
                   fallback=rec["fallback"], candidates=cand.cpu().numpy(), candidate_scores=scores, candidate_valid=rec["valid"], selected=sel)
        return cand[torch.arange(n, device=self.device), torch.as_tensor(sel).to(self.device)], out

    @staticmethod
    def _best_valid(scores, valid):
        """(n) the first maximum of every row over its valid slots (slot 0 where none is valid: the fallback lives there)."""
        return np.argmax(np.where(valid, scores, -np.inf), axis=1)

    def _frames(self, batch):
        """-> (first item of every distinct frame, the frame index of every item): items with the same non-None frame_id share a frame."""
        src, index = {}, []
        for j, it in enumerate(batch):
            key = ("frame", it.frame_id) if it.frame_id is not None else ("item", j)
            index.append(src.setdefault(key, (len(src), it))[0])
        return [it for _, it in sorted(src.values(), key=lambda v: v[0])], index

    def _frame_maps(self, firsts, want_image=True):
        """-> images (S,3,H,W) and descriptor maps (S,32,H,W) of the frames, the latter computed where an item brings none.
        want_image=False: the images are stacked only if a descriptor map has to be computed from them (None otherwise)."""
        dev = self.device
        missing = [s for s, it in enumerate(firsts) if it.geofea_2d is None]
        image = torch.stack([it.image for it in firsts]).to(dev) if want_image or missing else None
        if missing and self.desc2d is None:
            raise ValueError("items without geofea_2d need HipEpoch(desc2d=SuperPoint2D(...))")
        fresh = iter(self.desc2d.descriptors(image[missing].float().contiguous())) if missing else iter(())
        return image, torch.stack([next(fresh) if it.geofea_2d is None else it.geofea_2d.to(dev) for it in firsts])

    def initial_poses(self, batch):
        """(B,4,4) start poses of the items of one or several frames, in batch order: an item with a `bbox` is initialised from its
        frame's descriptor map (whatever its pose_init), an item without one keeps its pose_init; neither raises ValueError.  The record
        (count, n_inliers, final_cost, info, fallback per initialised row, and `rows`, their rows in `batch`, ascending) is in
        `last_init_info`."""
        if self.init is None:
            raise ValueError("initial_poses needs HipEpoch(init='descriptors' or a DescriptorPoseInitializer)")
        firsts, index = self._frames(batch)
        _, g2 = self._frame_maps(firsts)
        K = torch.as_tensor(np.stack([it.K for it in batch]).astype(np.float32)).to(self.device)
        return self._start_poses([dataclasses.replace(it, pose_init=None) if it.bbox is not None else it for it in batch], g2, index, K,
                                 firsts=firsts)

    def score_poses(self, batch, poses, scorer=None):
        """Render-and-compare confidence of the poses `poses` (B,4,4) of the items of `batch` (any classes, one or several camera
        frames) -> (B) fp64 scores on the device, in batch order; `last_score_info` becomes the record
        (PoseScorer.__call__).  Every frame's descriptor map is held once, as refine_frame holds it, and every item reads its frame's
        through a source index; the observed depth (EvalItem.depth) is used where EVERY item has one.  No pose_gt is read.
        scorer: a pose_score.PoseScorer (None: the one of HipEpoch(score=...), or a default one)."""
        return self._score(batch, poses, 1, scorer)

    def select_poses(self, batch, candidates):
        """candidates (B,N,4,4): N pose hypotheses for every item of `batch`; all B * N are scored in ONE call.
        -> (poses (B,4,4) the best hypothesis of every item, index (B) int64 which one, scores (B,N) fp64), on the device; equal scores
        go to the LOWEST index.  `last_score_info` holds the record with its per-pose arrays reshaped to (B,N,...)."""
        cand = candidates if torch.is_tensor(candidates) else torch.as_tensor(np.asarray(candidates, np.float32))
        cand = cand.to(self.device, torch.float32)
        if cand.dim() != 4 or cand.shape[0] != len(batch) or cand.shape[1] < 1 or cand.shape[2:] != (4, 4):
            raise ValueError(f"select_poses: candidates must be ({len(batch)},N,4,4), got {tuple(cand.shape)}")
        B, N = cand.shape[:2]
        scores = self._score(batch, cand.reshape(B * N, 4, 4), N, None).reshape(B, N)
        self.last_score_info = {k: (np.asarray(v).reshape(B, N, *np.asarray(v).shape[1:]) if k != "window_size" else v)
                                for k, v in self.last_score_info.items()}
        index = torch.as_tensor(np.argmax(scores.cpu().numpy(), axis=1)).to(self.device)          # (numpy: the first maximum)
        return cand[torch.arange(B, device=self.device), index], index, scores

    def _score(self, batch, poses, reps, scorer, maps=None):
        """Scores of poses (B * reps,4,4): item j owns the rows [j reps, (j + 1) reps).  maps: (descriptor maps, the frame index of
        every item, observed depth or None) where the caller holds them already."""
        if scorer is None:
            scorer = self.scorer
        if scorer is None:
            if self._default_scorer is None:
                from .pose_score import PoseScorer
                self._default_scorer = PoseScorer(self.renderer, self.models, device=self.device)
            scorer = self._default_scorer
        if len(batch) < 1 or len(poses) != len(batch) * reps:
            raise ValueError(f"{len(poses)} poses for {len(batch)} items x {reps}")
        if maps is None:
            firsts, index = self._frames(batch)
            _, g2 = self._frame_maps(firsts, want_image=False)
            depth = None if any(it.depth is None for it in firsts) else torch.stack([it.depth for it in firsts]).to(self.device).float().contiguous()
        else:
            g2, index, depth = maps
        rows = [j for j in range(len(batch)) for _ in range(reps)]
        K = np.stack([batch[j].K for j in rows]).astype(np.float32)
        score, self.last_score_info = scorer([batch[j].class_name for j in rows], poses, K, g2.float().contiguous(), [index[j] for j in rows], depth)
        return score

    def _observed_depth(self, frames):
        """-> the refiner's depth= argument for these frames' items ({} when the depth term is off)."""
        if getattr(self.refiner, "depth_term", None) is None:
            return {}
        if any(it.depth is None for it in frames):
            raise ValueError("depth_term: every item needs the observed depth of its frame (EvalItem.depth)")
        return dict(depth=torch.stack([it.depth for it in frames]).to(self.device).float())

    def _resident_tables(self):
        """On the first refine_frame: lay every class's [context | descriptor] table out once in the refiner's renderer
        (MeshRenderer.set_vertex_attributes).  False when that renderer keeps no tables or the classes' channel counts differ:
        refine_frame then passes one table per object."""
        if self._frame_tables is None:
            ren = getattr(self.refiner.renderer, "renderer", None)
            tables = {n: torch.cat([m.fea_3d, m.geofea_3d], -1)[0] for n, m in self.models.items()}
            self._frame_tables = hasattr(ren, "set_vertex_attributes") and len({t.shape[1] for t in tables.values()}) == 1
            if self._frame_tables:
                ren.set_vertex_attributes(tables)
        return self._frame_tables

    def refine_frame(self, batch):
        """The objects of one or several camera frames, of any classes, in ONE PoseRefiner call: the image and its descriptor
        map are held once per distinct frame (items with the same non-None frame_id; an item without one is its own frame),
        `SuperPoint2D.descriptors` runs once per frame that carries no geofea_2d, and every object crops its frame through
        image_index.  -> (B,4,4) refined poses in batch order.
        Multi-view: items with the same non-None `object_id` are views of one object from cameras with the
        camera-from-rig transforms `cam_from_rig`; they are refined as one group (PoseRefiner.forward(view_groups=)): one increment per
        object, the poses tied by the rig.  The pose_init of a group's FIRST item (in batch order) is its start, the others' are
        ignored.  Items without object_id are groups of one.  `last_rig_poses` then holds T_rig per group.
        Items whose pose_init is None are initialised from their frame's descriptor map inside their `bbox` (HipEpoch(init=...),
        DESIGN.md section 20) -- of a multi-view group only the first view; the record goes to `last_init_info` (`rows` = rows of `batch` as the
        caller passed it; None when no item needed a start).  With every pose_init
        given nothing new runs."""
        from .transformation import SE3Sequence
        dev = self.device
        if self.init_candidates > 1 and self.init_select == "refined" and any(it.pose_init is None for it in batch):
            return self._refine_frame_candidates(batch)
        order = vgroups = None
        given = batch                                                             # (the caller's order: the scores are taken in it)
        if any(it.object_id is not None or it.cam_from_rig is not None for it in batch):
            from . import ops
            gid = {}
            for j, it in enumerate(batch):
                gid.setdefault(("obj", it.object_id) if it.object_id is not None else ("item", j), len(gid))
            gof = [gid[("obj", it.object_id) if it.object_id is not None else ("item", j)] for j, it in enumerate(batch)]
            order = sorted(range(len(batch)), key=lambda j: (gof[j], j))          # groups contiguous, first appearance first
            batch = [batch[j] for j in order]
            E = np.stack([np.eye(4, dtype=np.float32) if it.cam_from_rig is None else np.asarray(it.cam_from_rig, np.float32) for it in batch])
            key = (tuple(gof[j] for j in order), E.tobytes())
            vgroups = self._view_groups.get(key)
            if vgroups is None:
                if len(self._view_groups) >= 8:
                    self._view_groups.pop(next(iter(self._view_groups)))
                vgroups = self._view_groups[key] = ops.ViewGroups(key[0], E, len(batch), dev)
        firsts, index = self._frames(batch)
        image, g2 = self._frame_maps(firsts)
        K = torch.as_tensor(np.stack([it.K for it in batch]).astype(np.float32)).to(dev)
        # (multi-view: only the FIRST view of a group needs a start, the others are tied to it by the rig)
        tied = () if order is None else {j for j in range(1, len(batch)) if gof[order[j]] == gof[order[j - 1]]}
        T0 = self._start_poses(batch, g2, index, K, skip=tied, caller_row=order, firsts=firsts)
        Tg = torch.as_tensor(np.stack([it.pose_gt for it in batch]).astype(np.float32)).to(dev)
        names = [it.class_name for it in batch]
        fea = geo = None                                             # = the renderer's resident tables
        if not self._resident_tables():
            fea = [self.models[n].fea_3d.to(dev)[0] for n in names]
            geo = [self.models[n].geofea_3d.to(dev)[0] for n in names]
        out = self.refiner(image, SE3Sequence(matrix=T0[:, None]), K, fea_3d=fea, Tj_gt=SE3Sequence(matrix=Tg[:, None]),
                           obj_cls=names, geofea_3d=geo, geofea_2d=g2, image_index=index, **self._observed_depth(firsts),
                           **({} if vgroups is None else dict(view_groups=vgroups)))
        self.last_depth_stats = out.get("depth_stats")
        self.last_rig_poses = out.get("T_rig")
        poses = out["Ti_pred"].G.reshape(-1, 4, 4)
        if order is not None:
            back = torch.empty(len(order), dtype=torch.long)
            back[torch.tensor(order)] = torch.arange(len(order))                  # the caller's order
            if self.last_depth_stats is not None:
                self.last_depth_stats = self.last_depth_stats[back.to(dev)]
            poses = poses[back.to(dev)]
        # (multi-view items are scored view by view, each in its own camera and against its own frame)
        self.last_scores = None if self.scorer is None else self.score_poses(given, poses, scorer=self.scorer)
        return poses

    def _refine_frame_candidates(self, batch):
        """refine_frame with init_select="refined": every item without a pose becomes its N candidates (same frame, same class, so the
        frame's maps are still held once), all rows are refined in ONE refiner call and scored in one scorer call, and the best valid
        refined candidate is returned per item; `last_scores` holds the scores of the returned poses."""
        if getattr(self.refiner, "occlusion", None) == "frame":
            raise ValueError("init_select='refined' with occlusion='frame': the candidates of one object would hide each other")
        if any(it.object_id is not None or it.cam_from_rig is not None for it in batch):
            raise ValueError("init_select='refined' does not take multi-view groups")
        need = [j for j, it in enumerate(batch) if it.pose_init is None]
        bad = [j for j in need if batch[j].bbox is None]
        if bad:
            raise ValueError(f"items {bad} have no pose_init: they need a bbox")
        sub = [batch[j] for j in need]
        firsts, index = self._frames(sub)
        _, g2 = self._frame_maps(firsts, want_image=False)
        K = torch.as_tensor(np.stack([it.K for it in sub]).astype(np.float32)).to(self.device)
        boxes = np.stack([np.asarray(it.bbox).astype(np.int32).reshape(4) for it in sub])
        cand, rec = self.init.candidates([it.class_name for it in sub], g2, index, K, boxes)
        N, ch = cand.shape[1], cand.cpu().numpy()
        rows, first = [], []                                                      # the expanded batch and every item's first row in it
        slot = {j: i for i, j in enumerate(need)}
        for j, it in enumerate(batch):
            first.append(len(rows))
            rows += [dataclasses.replace(it, pose_init=ch[slot[j], k].copy()) for k in range(N)] if j in slot else [it]
        scorer, self.scorer = self.scorer, None                                   # (the rows are scored below, once)
        try:
            refined = self.refine_frame(rows)
        finally:
            self.scorer = scorer
        scores = self.score_poses(rows, refined, scorer=scorer)
        sc = scores.cpu().numpy()
        cs = np.stack([sc[first[j]:first[j] + N] for j in need])
        sel = self._best_valid(cs, rec["valid"])
        take = [first[j] + (int(sel[slot[j]]) if j in slot else 0) for j in range(len(batch))]
        pick = np.arange(len(need))
        self.last_init_info = dict(count=rec["count"], n_inliers=rec["n_inliers"][pick, sel], final_cost=rec["final_cost"][pick, sel],
                                   info=rec["info"][pick, sel], fallback=rec["fallback"], candidates=ch, candidate_scores=cs,
                                   candidate_valid=rec["valid"], selected=sel, rows=np.asarray(need))
        take = torch.as_tensor(take, device=self.device)
        if self.last_depth_stats is not None:
            self.last_depth_stats = self.last_depth_stats[take]
        self.last_scores = scores[take]
        return refined[take]

    def bop_metrics(self, batch, pose_pred, want_errors=False):
        """BOP recalls of the poses `pose_pred` (B,4,4) of the items of `batch` (any classes, one or several camera frames):
        -> (B,3) fp64 numpy [AR_VSD, AR_MSSD, AR_MSPD] per item  [, the error dictionary of BOPEvaluator.errors].
        The observed depth (EvalItem.depth) is held once per distinct frame, as refine_frame holds the image, and every item
        reads its frame's through a source index; an item without a frame id is its own frame.  The bop_fn of run_epoch."""
        from .evaluator import BOPEvaluator
        if self.bop is None:
            self.bop = BOPEvaluator(self.renderer, self.models, device=self.device)
        src, index = {}, []
        for j, it in enumerate(batch):
            if it.depth is None:
                raise ValueError("bop_metrics: every item needs the observed depth of its frame (EvalItem.depth)")
            key = ("frame", it.frame_id) if it.frame_id is not None else ("item", j)
            index.append(src.setdefault(key, (len(src), it))[0])
        firsts = [it for _, it in sorted(src.values(), key=lambda v: v[0])]
        depth = torch.stack([it.depth for it in firsts]).to(self.device)
        names = [it.class_name for it in batch]
        K = np.stack([it.K for it in batch]).astype(np.float32)
        gt = np.stack([it.pose_gt for it in batch]).astype(np.float32)
        pred = pose_pred if torch.is_tensor(pose_pred) else np.asarray(pose_pred, dtype=np.float32)
        err = self.bop.errors(names, pred, gt, K, depth, src_index=index)
        rec = self.bop.recalls(err, [self.models[n].diameter for n in names], depth.shape[-1])
        return (rec, err) if want_errors else rec

    def metrics(self, cls, pose_pred, pose_gt):
        ev = self.evaluators[cls]
        T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(self.device)
        return ev.evaluate(T(pose_pred), T(pose_gt)).cpu().numpy()


# ---- synthetic stand-in for EXPDATA ----------------------------------------------------------------------------------
def _ellipsoid(sub, scale):
    """Closed triangle mesh: subdivided icosahedron scaled to an ellipsoid (consistent outward winding)."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(sub):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * np.array(scale)).astype(np.float32), np.array(f, np.int32)


def synthetic_models(class_names=("ape", "cat", "glue"), sub=3, seed=0):
    """Ellipsoid 'objects' of LINEMOD-like size (5-10 cm half axes) with hash-generated vertex features."""
    from . import synthetic as syn
    models = {}
    for k, name in enumerate(class_names):
        scale = (0.05 + 0.015 * k, 0.04 + 0.01 * ((k + 1) % 3), 0.035 + 0.01 * ((k + 2) % 3))
        verts, faces = _ellipsoid(sub, scale)
        P = verts.shape[0]
        g3 = syn.normal(f"g3:{name}", (1, P, 32), seed)
        g3 /= np.linalg.norm(g3, axis=-1, keepdims=True) + 1e-12
        d = verts[:, None, :] - verts[None, :, :]
        models[name] = ClassModel(name=name, verts=verts, faces=faces, colors=syn.uniform(f"col:{name}", (P, 3), seed),
                                  fea_3d=torch.from_numpy(syn.normal(f"f3:{name}", (1, P, 256), seed, std=0.5)),
                                  geofea_3d=torch.from_numpy(g3.astype(np.float32)),
                                  diameter=float(np.sqrt((d * d).sum(-1)).max()))
    return models


def synthetic_dataset(models, n_items, image_size=(480, 640), seed=0, pose_sigma=(0.05, 0.01), renderer=None, device="cuda"):
    """n_items samples cycling through the classes in blocks (as a per-class LINEMOD sequence does): ground-truth pose in front
    of the camera, initial pose = exp(xi) * gt with xi ~ N(0, pose_sigma (rotation rad, translation m)); the observed image
    and its descriptors are RENDERED at the ground-truth pose by `renderer` (MeshRenderer) -- or hash noise when None (CPU)."""
    from . import synthetic as syn
    from .evaluator import LINEMOD_K
    H, W = image_size
    names = sorted(models)
    K = LINEMOD_K.copy()
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    items = []
    block = max(1, -(-n_items // len(names)))
    for i in range(n_items):
        cls = names[min(i // block, len(names) - 1)]
        g = syn.se3_exp_np(syn.normal(f"gt{i}", (1, 6), seed, std=0.6))[0]
        g[:3, 3] = syn.uniform(f"t{i}", (3,), seed, -0.03, 0.03) + np.array([0.0, 0.0, 0.8])
        xi = syn.normal(f"xi{i}", (1, 6), seed)[0] * np.array([pose_sigma[1]] * 3 + [pose_sigma[0]] * 3)
        init = syn.se3_exp_np(xi[None])[0] @ g
        items.append(EvalItem(cls, None, K.copy(), init.astype(np.float32), g.astype(np.float32), None))
    if renderer is None:
        for i, it in enumerate(items):
            it.image = torch.from_numpy(syn.uniform(f"img{i}", (3, H, W), seed) * 255.0)
            it.geofea_2d = torch.from_numpy(syn.normal(f"g2{i}", (32, H, W), seed))
        return items
    dev = torch.device(device)
    for cls in names:
        ids = [i for i, it in enumerate(items) if it.class_name == cls]
        m = models[cls]
        for a in range(0, len(ids), 8):
            sub_ids = ids[a:a + 8]
            Tg = torch.as_tensor(np.stack([items[i].pose_gt for i in sub_ids])).to(dev)
            Kt = torch.as_tensor(np.stack([items[i].K for i in sub_ids])).to(dev)
            out, _ = renderer([cls] * len(sub_ids), m.geofea_3d.to(dev), T=Tg, K=Kt, render_image_size=(H, W), render_tex=True)
            for j, i in enumerate(sub_ids):
                items[i].image = (out[j, :3] * 255.0).cpu()
                items[i].geofea_2d = out[j, 3:].cpu()
    return items


def synthetic_scenes(models, n_frames, objects_per_frame, image_size=(480, 640), seed=0, pose_sigma=(0.05, 0.01), renderer=None,
                     device="cuda", cameras=None):
    """n_frames camera frames with objects_per_frame objects each, of different classes (cycling through them), at separated
    image positions and depths: every object is rendered at its ground-truth pose by `renderer` (MeshRenderer) and the frame is
    composed by nearest depth in torch -- colour and rendered descriptors alike -- so nearer objects occlude farther ones.
    Every object becomes an EvalItem that SHARES the frame's image and geofea_2d tensors and carries its frame_id; items of a
    frame are consecutive, and `depth`, the composed nearest depth (0 on the background): the frame's observed depth for the BOP VSD.
    renderer=None (CPU): hash noise per frame instead of a render, and no depth.
    cameras: a list of (4,4) camera-from-rig matrices E_c -- every frame becomes len(cameras) images of the same objects (the poses
    above are then rig-frame poses): pose_gt = E_c g, frame_id = (f, c), object_id = (f, j), cam_from_rig = E_c, and ONE initial error
    per object, expressed in the rig frame (pose_init = E_c exp(xi) g).  Items of an image are consecutive, images in camera order."""
    from . import synthetic as syn
    from .evaluator import LINEMOD_K
    H, W = image_size
    names = sorted(models)
    K = LINEMOD_K.copy()
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    cols = int(np.ceil(np.sqrt(objects_per_frame)))
    rows = -(-objects_per_frame // cols)
    # grid cells of 0.8 x the image at 0.8 m, shrunk towards the centre so that the objects stay inside the frame
    dx, dy = 0.8 * W / K[0, 0] * 0.8 / max(cols, 1), 0.8 * H / K[1, 1] * 0.8 / max(rows, 1)
    items = []
    cams = [None] if cameras is None else [np.asarray(E, np.float64).reshape(4, 4) for E in cameras]
    for f, c in ((f, c) for f in range(n_frames) for c in range(len(cams))):
        frame = []
        for j in range(objects_per_frame):
            cls = names[(f + j) % len(names)]
            i = f * objects_per_frame + j
            g = syn.se3_exp_np(syn.normal(f"sgt{i}", (1, 6), seed, std=0.6))[0]
            cell = np.array([(j % cols - (cols - 1) / 2.0) * dx, (j // cols - (rows - 1) / 2.0) * dy, 0.8 + 0.06 * ((j * 5) % 7) / 7.0])
            g[:3, 3] = syn.uniform(f"st{i}", (3,), seed, -0.1, 0.1) * np.array([dx, dy, 0.05]) + cell      # jitter within the cell
            xi = syn.normal(f"sxi{i}", (1, 6), seed)[0] * np.array([pose_sigma[1]] * 3 + [pose_sigma[0]] * 3)
            init = syn.se3_exp_np(xi[None])[0] @ g
            if cameras is None:
                frame.append(EvalItem(cls, None, K.copy(), init.astype(np.float32), g.astype(np.float32), None, frame_id=f))
            else:
                frame.append(EvalItem(cls, None, K.copy(), (cams[c] @ init).astype(np.float32), (cams[c] @ g).astype(np.float32), None,
                                      frame_id=(f, c), object_id=(f, j), cam_from_rig=cams[c].astype(np.float32)))
        if renderer is None:
            tag = f"{f}" if cameras is None else f"{f}c{c}"
            image = torch.from_numpy(syn.uniform(f"simg{tag}", (3, H, W), seed) * 255.0)
            g2 = torch.from_numpy(syn.normal(f"sg2{tag}", (32, H, W), seed))
        else:
            dev = torch.device(device)
            Tg = torch.as_tensor(np.stack([it.pose_gt for it in frame])).to(dev)
            Kt = torch.as_tensor(np.stack([it.K for it in frame])).to(dev)
            out, depth = renderer([it.class_name for it in frame], [models[it.class_name].geofea_3d[0].to(dev) for it in frame],
                                  T=Tg, K=Kt, render_image_size=(H, W), render_tex=True)
            z = torch.where(depth > 0, depth, torch.full_like(depth, float("inf")))          # (n,1,H,W); -1 = empty
            near = z.argmin(0, keepdim=True)                                                 # nearest object per pixel
            comp = torch.gather(out, 0, near.expand(1, out.shape[1], H, W))[0]
            comp = comp * torch.isfinite(z.min(0).values).to(comp.dtype)                     # background stays 0
            image, g2 = (comp[:3] * 255.0).cpu(), comp[3:].cpu()
            zmin = z.min(0).values[0]                                                        # the frame's observed depth, 0 = background
            obs = torch.where(torch.isfinite(zmin), zmin, torch.zeros_like(zmin)).cpu()
        for it in frame:
            it.image, it.geofea_2d = image, g2
            it.depth = obs if renderer is not None else None
        items += frame
    return items
