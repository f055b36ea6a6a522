"""GPU tests of the BOP pose-error functions (csrc/eval_metrics.hip: rnnpose_bop_sym_dist_f64, rnnpose_bop_vsd_f64) against their
fp64 numpy restatement tests/bop_ref.py, and of the plumbing above them (ops, BOPEvaluator, HipEpoch.bop_metrics).

MSSD / MSPD are held to the tolerance tests/test_gpu_eval.py holds rnnpose_pose_metrics_f64 to (rtol 1e-6, atol 1e-9): the same
fp64 arithmetic on the same fp32 inputs.  The VSD counts are integers and must be EQUAL; err is then the same fp64 division of the
same integers, bit for bit.  That holds as long as no comparison of the input sits within rounding of its threshold: every VSD case
asserts, on the reference's own values, that no pixel is within a relative 1e-9 of delta or of a tau (fp64 differences between the
kernel and numpy are ~1e-16).

tests/test_bop_on_host.py runs this module on the host-executed kernels, all but the `full_size` and `end_to_end` tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import bop_ref as br
from rnnpose_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from rnnpose_amd import build, ops as _ops
    build.build()
    return _ops


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def npy(t):
    return t.detach().cpu().numpy()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ---- MSSD / MSPD ---------------------------------------------------------------------------------------------------------------------
def _poses(tag, n, seed, z=0.9):
    T = syn.se3_exp_np(syn.normal(tag, (n, 6), seed, std=0.8))
    T[:, :3, 3] = syn.uniform(tag + ".t", (n, 3), seed, -0.05, 0.05) + np.array([0.0, 0.0, z])
    return T


def _sym_case(P, S, B, seed):
    model = syn.uniform("bop.model", (P, 3), seed, -0.08, 0.08).astype(np.float32)
    sym = syn.se3_exp_np(syn.normal("bop.sym", (S, 6), seed, std=1.0) * np.array([0.01] * 3 + [1.0] * 3))
    sym[0] = np.eye(4)
    gt = _poses("bop.gt", B, seed)
    d = syn.normal("bop.dxi", (B, 6), seed) * np.array([0.01] * 3 + [0.08] * 3)
    est = syn.se3_exp_np(d) @ gt
    K = np.tile(np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]]), (B, 1, 1))
    K[:, 0, 0] += np.arange(B) * 3.0
    K[:, 1, 2] -= np.arange(B) * 1.5
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return model, f(sym[:, :3]), f(est[:, :3]), f(gt[:, :3]), f(K)


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("S", [1, 2, 6, 37])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 2562])
def test_sym_dist_vs_reference(ops, P, S, B):
    model, sym, est, gt, K = _sym_case(P, S, B, seed=P + 7 * S + B)
    got = npy(ops.bop_sym_dist(dev(model), dev(sym), dev(est), dev(gt), dev(K)))
    want = br.sym_dist(model, sym, est, gt, K)
    assert got.shape == (B, 2) and got.dtype == np.float64
    assert np.allclose(got, want, rtol=1e-6, atol=1e-9), np.abs(got - want).max()
    if B == 3:                                             # one shared K (3,3) is K repeated
        one = npy(ops.bop_sym_dist(dev(model), dev(sym), dev(est), dev(gt), dev(K[0])))
        assert np.allclose(one, br.sym_dist(model, sym, est, gt, K[0]), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("S,k", [(2, 1), (6, 4), (37, 36), (37, 0)])
def test_sym_dist_finds_the_planted_symmetry(ops, S, k):
    """est = gt * S_k (rounded to fp32): symmetry k gives ~1e-7, every other one centimetres -- the min over S, not the max, and
    not the first."""
    model, sym, _, gt, K = _sym_case(257, S, 3, seed=11 + S)
    h = lambda T: np.concatenate([T.astype(np.float64), np.tile([[[0.0, 0.0, 0.0, 1.0]]], (T.shape[0], 1, 1))], 1)
    est = np.ascontiguousarray((h(gt) @ h(sym[k:k + 1]))[:, :3], dtype=np.float32)
    allv = br.sym_dist_all(model, sym, est, gt, K)
    assert np.all(allv.argmin(1) == k) and (S == 1 or np.sort(allv[:, :, 0], 1)[:, 1].min() > 1e-3)
    got = npy(ops.bop_sym_dist(dev(model), dev(sym), dev(est), dev(gt), dev(K)))
    assert np.allclose(got, allv.min(1), rtol=1e-6, atol=1e-9)
    assert got[:, 0].max() < 1e-6 and got[:, 1].max() < 1e-3


# ---- VSD -----------------------------------------------------------------------------------------------------------------------------
DELTA = 0.015
EMPTY = (0.0, -1.0, np.nan)
MISSING = (0.0, -2.0, np.nan, np.inf)


def _taus(NT):
    return tuple(round(0.03 * (k + 1), 2) for k in range(NT))


def _vsd_case(H, W, B, S, seed, p_empty=0.3, p_missing=0.2):
    rng = np.random.default_rng(seed)
    gt = (0.8 + 0.1 * rng.random((B, H, W))).astype(np.float32)
    est = (gt + rng.uniform(-0.05, 0.05, (B, H, W))).astype(np.float32)
    obs = (0.85 + rng.uniform(-0.06, 0.06, (S, H, W))).astype(np.float32)
    for a, p, marks in ((gt, p_empty, EMPTY), (est, p_empty, EMPTY), (obs, p_missing, MISSING)):
        hole = rng.random(a.shape) < p
        a[hole] = rng.choice(np.array(marks, np.float32), size=int(hole.sum()))
    K = np.tile(np.array([[1.2 * W + 1.0, 0.0, W / 2.0 - 0.3], [0.0, 1.3 * W + 1.0, H / 2.0 + 0.2], [0.0, 0.0, 1.0]]), (B, 1, 1))
    K[:, 0, 0] += np.arange(B) * 0.5
    K[:, 0, 2] += np.arange(B) * 0.25
    src = [(3 * b + 1) % S for b in range(B)]
    return est, gt, obs, src, K.astype(np.float32)


def _diameters(mode, B):
    if mode == "pos":
        return (0.1 + 0.05 * np.arange(B)).astype(np.float32)
    if mode == "nonpos":
        return np.array([0.0, -0.3] * B, np.float32)[:B]
    return np.array([0.2, 0.0, 0.15, -1.0, 0.3] * B, np.float32)[:B]


def _check_vsd(ops, est, gt, obs, src, K, diam, delta, taus):
    err, counts = ops.bop_vsd(dev(est), dev(gt), dev(obs), src, dev(K), dev(diam), delta, taus)
    werr, wcounts, near = br.vsd(est, gt, obs, src, K, diam, delta, taus)
    assert near == 0, f"{near} comparisons of this input sit within 1e-9 of a threshold: pick another seed"
    err, counts = npy(err), npy(counts)
    assert counts.dtype == np.int64 and err.dtype == np.float64 and counts.shape == wcounts.shape and err.shape == werr.shape
    assert np.array_equal(counts, wcounts), (counts, wcounts)
    assert np.array_equal(err.view(np.int64), werr.view(np.int64))
    return err, counts


@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (37, 53), (64, 64), (65, 67)])
def test_vsd_counts_equal_the_reference(ops, H, W, B):
    """Every combination of one / two observed maps (mixed source index), NT in {1, 10, 16} and diameters > 0 / <= 0 / mixed.
    65 x 67 = 4355 pixels = two whole 2048-pixel workgroups and a ragged third; 64 x 64 = two exactly."""
    seen = 0
    for S in (1, 2):
        for NT in (1, 10, 16):
            for mode in ("pos", "nonpos", "mixed"):
                est, gt, obs, src, K = _vsd_case(H, W, B, S, seed=1000 * H + 10 * B + S + NT)
                _, counts = _check_vsd(ops, est, gt, obs, src, K, _diameters(mode, B), DELTA, _taus(NT))
                seen += int(counts[:, 1].sum())
    assert H * W < 30 or seen > 0


def test_vsd_full_size_frame(ops):
    est, gt, obs, src, K = _vsd_case(480, 640, 2, 2, seed=5)
    _, counts = _check_vsd(ops, est, gt, obs, src, K, _diameters("pos", 2), DELTA, _taus(10))
    assert counts[:, 1].min() > 50000 and counts[0, 2] > counts[0, 11] > 0


def test_vsd_edge_inputs(ops):
    H, W, B = 65, 67, 2
    est, gt, obs, src, K = _vsd_case(H, W, B, 2, seed=3, p_empty=0.1, p_missing=0.0)
    diam, taus = _diameters("pos", B), _taus(10)
    # everything empty: no union, err = 1
    e = np.stack([np.zeros((H, W), np.float32), np.full((H, W), np.nan, np.float32)])
    err, counts = _check_vsd(ops, e, -e, obs, src, K, diam, DELTA, taus)
    assert not counts.any() and np.all(err == 1.0)
    # est empty, gt not: union = vis_gt, no intersection, err = 1
    err, counts = _check_vsd(ops, e, gt, obs, src, K, diam, DELTA, taus)
    assert counts[:, 0].min() > 0 and not counts[:, 1:].any() and np.all(err == 1.0)
    # nothing observed: every non-empty model pixel is visible
    miss = np.stack([np.zeros((H, W), np.float32), np.full((H, W), np.inf, np.float32)])
    err, counts = _check_vsd(ops, est, gt, miss, src, K, diam, DELTA, taus)
    assert np.array_equal(counts[:, 0], ((est > 0) | (gt > 0)).sum((1, 2))) and np.array_equal(counts[:, 1], ((est > 0) & (gt > 0)).sum((1, 2)))
    # the observed surface in front of both models everywhere: nothing visible
    err, counts = _check_vsd(ops, est, gt, np.full((2, H, W), 0.5, np.float32), src, K, diam, DELTA, taus)
    assert not counts.any() and np.all(err == 1.0)


def test_vsd_comparisons_are_inclusive(ops):
    """Exactly `<=` on delta and `>=` on tau, on values that are exact in fp64: at the principal point of a 1 x 1 image the ray factor is 1,
    so gt 1.0 behind obs 0.75 is 0.25 = delta away (visible), and est 1.5 differs from gt by 0.5 = tau (counted)."""
    K = np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
    one = lambda v: np.full((1, 1, 1), v, np.float32)
    err, counts = ops.bop_vsd(dev(one(1.5)), dev(one(1.0)), dev(one(0.75)), [0], dev(K), 0.0, 0.25, (0.25, 0.5, 0.75))
    assert npy(counts).tolist() == [[1, 1, 1, 1, 0]] and npy(err).tolist() == [[1.0, 1.0, 0.0]]
    w = br.vsd(one(1.5), one(1.0), one(0.75), [0], K, 0.0, 0.25, (0.25, 0.5, 0.75))
    assert w[1].tolist() == [[1, 1, 1, 1, 0]] and w[2] == 2                    # (the reference agrees, and knows these two sit ON a threshold)
    err, counts = ops.bop_vsd(dev(one(1.5)), dev(one(1.0)), dev(one(0.75)), [0], dev(K), 0.0, 0.125, (0.5,))
    assert npy(counts).tolist() == [[0, 0, 0]] and npy(err).tolist() == [[1.0]]         # 0.25 > delta: hidden


def test_vsd_is_bit_identical_under_rerun_and_independent_of_the_batch(ops):
    H, W, B = 65, 67, 5
    est, gt, obs, src, K = _vsd_case(H, W, B, 2, seed=9)
    diam, taus = _diameters("mixed", B), _taus(16)
    a = [npy(t) for t in ops.bop_vsd(dev(est), dev(gt), dev(obs), src, dev(K), dev(diam), DELTA, taus)]
    b = [npy(t) for t in ops.bop_vsd(dev(est), dev(gt), dev(obs), src, dev(K), dev(diam), DELTA, taus)]
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1])
    for j in range(B):
        e1, c1 = ops.bop_vsd(dev(est[j:j + 1]), dev(gt[j:j + 1]), dev(obs), src[j:j + 1], dev(K[j:j + 1]), dev(diam[j:j + 1]), DELTA, taus)
        assert np.array_equal(npy(e1).view(np.int64), a[0][j:j + 1].view(np.int64)) and np.array_equal(npy(c1), a[1][j:j + 1])
    # a SourceIndex built once, a scalar diameter and a shared K are the same call
    si = ops.SourceIndex(src, 2, "cuda")
    e2, c2 = ops.bop_vsd(dev(est), dev(gt), dev(obs), si, dev(K[0]), 0.2, DELTA, taus)
    w2 = br.vsd(est, gt, obs, src, K[0], 0.2, DELTA, taus)
    assert w2[2] == 0 and np.array_equal(npy(c2), w2[1]) and np.array_equal(npy(e2), w2[0])


# ---- bad arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_on_the_host_before_any_launch(ops, monkeypatch):
    est, gt, obs, src, K = _vsd_case(7, 5, 2, 2, seed=1)
    model, sym, pe, pg, Ks = _sym_case(5, 2, 2, seed=1)

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    monkeypatch.setattr(ops, "_launch", no_launch)
    d = 0.1
    with pytest.raises(ValueError, match="taus"):
        ops.bop_vsd(dev(est), dev(gt), dev(obs), src, dev(K), d, DELTA, _taus(16) + (0.9,))
    with pytest.raises(ValueError, match="taus"):
        ops.bop_vsd(dev(est), dev(gt), dev(obs), src, dev(K), d, DELTA, ())
    for bad in ([0, 2], [-1, 0], [0], [0, 1, 1]):
        with pytest.raises(ValueError):
            ops.bop_vsd(dev(est), dev(gt), dev(obs), bad, dev(K), d, DELTA, _taus(2))
    with pytest.raises(ValueError):
        ops.bop_vsd(dev(est), dev(gt), dev(obs), ops.SourceIndex([0, 1, 2], 3, "cuda"), dev(K), d, DELTA, _taus(2))
    with pytest.raises(ValueError, match="depth_gt"):
        ops.bop_vsd(dev(est), dev(gt[:, :, :4]), dev(obs), src, dev(K), d, DELTA, _taus(2))
    with pytest.raises(ValueError, match="depth_obs"):
        ops.bop_vsd(dev(est), dev(gt), dev(obs[:, :6]), src, dev(K), d, DELTA, _taus(2))
    with pytest.raises(ValueError, match="K must"):
        ops.bop_vsd(dev(est), dev(gt), dev(obs), src, dev(K[:1].repeat(3, 0)), d, DELTA, _taus(2))
    with pytest.raises(ValueError, match="diameter"):
        ops.bop_vsd(dev(est), dev(gt), dev(obs), src, dev(K), [0.1, 0.2, 0.3], DELTA, _taus(2))
    with pytest.raises(ValueError, match="sym"):
        ops.bop_sym_dist(dev(model), dev(sym[:0]), dev(pe), dev(pg), dev(Ks))
    with pytest.raises(ValueError, match="sym"):
        ops.bop_sym_dist(dev(model), dev(sym[:, :, :3]), dev(pe), dev(pg), dev(Ks))
    with pytest.raises(ValueError, match="pose"):
        ops.bop_sym_dist(dev(model), dev(sym), dev(pe), dev(pg[:1]), dev(Ks))
    with pytest.raises(ValueError, match="model"):
        ops.bop_sym_dist(dev(model[:, :2]), dev(sym), dev(pe), dev(pg), dev(Ks))
    with pytest.raises(ValueError, match="K must"):
        ops.bop_sym_dist(dev(model), dev(sym), dev(pe), dev(pg), dev(Ks[:1].repeat(3, 0)))


def test_bad_arguments_through_the_c_abi_write_nothing(ops):
    from rnnpose_amd import _lib
    lib = _lib.load()
    H, W, B, S, NT = 7, 5, 2, 2, 3
    est, gt, obs, src, K = _vsd_case(H, W, B, S, seed=2)
    d_est, d_gt, d_obs, d_K, d_diam = dev(est), dev(gt), dev(obs), dev(K), dev(_diameters("pos", B))
    d_src = torch.tensor(src, dtype=torch.int32).cuda()
    taus = (C.c_double * 17)(*[0.03 * (k + 1) for k in range(17)])
    n = int(lib.rnnpose_bop_vsd_workspace_bytes(B, H, W, NT))
    assert n == B * 1 * (2 + NT) * 4 and lib.rnnpose_bop_vsd_workspace_bytes(B, 65, 67, 16) == B * 3 * 18 * 4
    assert lib.rnnpose_bop_vsd_workspace_bytes(B, H, W, 17) == 0 and lib.rnnpose_bop_vsd_workspace_bytes(0, H, W, 1) == 0
    ws = torch.zeros(64, dtype=torch.int32).cuda()
    counts = torch.full((B, 2 + 16), 7, dtype=torch.int64).cuda()
    err = torch.full((B, 16), 7.0, dtype=torch.float64).cuda()

    def vsd(de=d_est, dg=d_gt, do=d_obs, s_obs=S, si=d_src, b=B, h=H, w=W, tv=taus, nt=NT, wsp=ws, nb=n, cn=counts, er=err):
        tp = C.cast(tv, C.c_void_p) if tv is not None else C.c_void_p(0)
        rc = lib.rnnpose_bop_vsd_f64(ptr(de), ptr(dg), ptr(do), s_obs, ptr(si), ptr(d_K), ptr(d_diam), b, h, w, DELTA, tp, nt, ptr(wsp), nb,
                                     ptr(cn), ptr(er), ops._stream())
        torch.cuda.synchronize()
        return rc
    for kw, msg in ((dict(nt=17), b"NT"), (dict(nt=0), b"NT"), (dict(de=None), b"null"), (dict(tv=None), b"null"), (dict(er=None), b"null"),
                    (dict(nb=n - 1), b"workspace"), (dict(b=0), b"bad size"), (dict(h=0), b"bad size"), (dict(s_obs=0), b"bad size"),
                    (dict(b=65536, nb=1 << 30), b"bad size")):
        assert vsd(**kw) != 0 and msg in lib.rnnpose_last_error(), kw
    assert torch.all(counts == 7) and torch.all(err == 7.0) and not ws.any()              # refused before any launch
    # the kernel is the second fence: a sample whose index is out of range counts nothing and reports NaN, its neighbour is right
    for bad in (2, -1, 1 << 30):
        d_bad = torch.tensor([bad, src[1]], dtype=torch.int32).cuda()
        assert vsd(si=d_bad) == 0
        c, e = npy(counts), npy(err)
        _, wc, _ = br.vsd(est, gt, obs, src, K, _diameters("pos", B), DELTA, list(taus)[:NT])
        assert not c[0, :2 + NT].any() and np.all(np.isnan(e.reshape(-1)[:NT]))
        assert np.array_equal(c.reshape(-1)[2 + NT:2 * (2 + NT)], wc[1]) and not np.isnan(e.reshape(-1)[NT:2 * NT]).any()
    # sym_dist
    model, sym, pe, pg, Ks = (dev(a) for a in _sym_case(5, 2, 2, seed=1))
    ns = int(lib.rnnpose_bop_sym_dist_workspace_bytes(2, 2))
    assert ns == 2 * 2 * 2 * 8 and lib.rnnpose_bop_sym_dist_workspace_bytes(2, 0) == 0
    wsd = torch.zeros(16, dtype=torch.float64).cuda()
    out = torch.full((2, 2), 7.0, dtype=torch.float64).cuda()

    def sd(m=model, p=5, sy=sym, s=2, b=2, wsp=wsd, nb=ns, o=out):
        rc = lib.rnnpose_bop_sym_dist_f64(ptr(m), p, ptr(sy), s, ptr(pe), ptr(pg), ptr(Ks), b, ptr(wsp), nb, ptr(o), ops._stream())
        torch.cuda.synchronize()
        return rc
    for kw, msg in ((dict(s=0), b"S < 1"), (dict(s=-3), b"S < 1"), (dict(m=None), b"null"), (dict(o=None), b"null"), (dict(wsp=None), b"null"),
                    (dict(p=0), b"bad size"), (dict(b=0), b"bad size"), (dict(nb=ns - 1), b"workspace")):
        assert sd(**kw) != 0 and msg in lib.rnnpose_last_error(), kw
    assert torch.all(out == 7.0) and not wsd.any()
    assert sd() == 0 and torch.all(out != 7.0)


def test_torch_ops_are_the_same_kernels(ops):
    import rnnpose_amd.torch_ops  # noqa: F401
    est, gt, obs, src, K = _vsd_case(37, 53, 2, 2, seed=4)
    taus = list(_taus(10))
    err, counts = torch.ops.rnnpose.bop_vsd(dev(est), dev(gt), dev(obs), torch.tensor(src).cuda(), dev(K), dev(_diameters("pos", 2)), DELTA, taus)
    w = br.vsd(est, gt, obs, src, K, _diameters("pos", 2), DELTA, taus)
    assert w[2] == 0 and np.array_equal(npy(counts), w[1]) and np.array_equal(npy(err), w[0])
    model, sym, pe, pg, Ks = _sym_case(257, 6, 3, seed=2)
    got = npy(torch.ops.rnnpose.bop_sym_dist(dev(model), dev(sym), dev(pe), dev(pg), dev(Ks)))
    assert np.allclose(got, br.sym_dist(model, sym, pe, pg, Ks), rtol=1e-6, atol=1e-9)


# ---- end to end: BOPEvaluator on rendered frames, HipEpoch.bop_metrics ------------------------------------------------------------------
def test_end_to_end_on_synthetic_scenes(ops):
    from rnnpose_amd import eval_epoch as ee
    H, W = 120, 160
    models = ee.synthetic_models(("ape", "cat", "glue"), sub=2)
    assert models["ape"].verts.shape[0] == 162
    models["glue"].symmetries = np.stack([np.eye(4), np.diag([-1.0, -1.0, 1.0, 1.0])]).astype(np.float32)      # half a turn about z
    hip = ee.HipEpoch(models)
    items = ee.synthetic_scenes(models, 2, 3, image_size=(H, W), seed=3, renderer=hip.renderer)
    assert all(it.depth is items[0].depth for it in items[:3]) and items[3].depth is not items[0].depth
    assert tuple(items[0].depth.shape) == (H, W) and float(items[0].depth.min()) == 0.0 and float(items[0].depth.max()) > 0.5
    gt = np.stack([it.pose_gt for it in items])
    init = np.stack([it.pose_init for it in items])
    # ground-truth poses: no surface distance, no discrepancy wherever the object is visible at all; somebody is in front
    rec, e = hip.bop_metrics(items, gt, want_errors=True)
    counts, vsd = npy(e["counts"]), npy(e["vsd"])
    assert np.all(npy(e["mssd"]) == 0.0) and np.all(npy(e["mspd"]) == 0.0)
    names = [it.class_name for it in items]
    K = np.stack([it.K for it in items]).astype(np.float32)
    d_gt = npy(hip.renderer.render_zbuf(names, dev(gt), dev(K), (H, W)))[:, 0]
    cover = (d_gt > 0).sum((1, 2))
    assert cover.min() > 100 and np.all(counts[:, 0] == counts[:, 1]) and np.all(counts[:, 0] <= cover)
    frames = np.stack([npy(items[0].depth), npy(items[3].depth)])[[0, 0, 0, 1, 1, 1]]
    unoccluded = np.array([np.all(np.abs(frames[j] - d_gt[j])[d_gt[j] > 0] <= 1e-6) for j in range(6)])    # nearest on all of its pixels
    assert not unoccluded.all()                                  # (the objects of these small frames overlap and interpenetrate)
    assert np.all(counts[unoccluded, 0] == cover[unoccluded]) and np.all(rec[unoccluded] == 1.0)
    assert np.all(vsd[counts[:, 0] > 0] == 0.0) and np.all(counts[:, 0] > 0) and np.any(counts[:, 0] < cover)
    # an object alone in front of its own observed surface is unoccluded: every covered pixel visible, no discrepancy
    alone = hip.bop.errors(names[:1], gt[:1], gt[:1], K[:1], np.maximum(d_gt[0], 0.0))
    assert int(alone["counts"][0, 0]) == int(alone["counts"][0, 1]) == cover[0] and not npy(alone["counts"])[0, 2:].any()
    assert np.all(npy(alone["vsd"]) == 0.0)
    # initial poses: the evaluator == the reference fed with the same rendered depths
    rec, e = hip.bop_metrics(items, init, want_errors=True)
    d_est = npy(hip.renderer.render_zbuf(names, dev(init), dev(K), (H, W)))[:, 0]
    obs = np.stack([npy(items[0].depth), npy(items[3].depth)])
    src = [0, 0, 0, 1, 1, 1]
    diam = np.array([models[n].diameter for n in names], np.float32)
    werr, wcounts, near = br.vsd(d_est, d_gt, obs, src, K, diam, br.DELTA, br.TAUS)
    assert near == 0 and np.array_equal(npy(e["counts"]), wcounts) and np.array_equal(npy(e["vsd"]), werr)
    assert wcounts[:, 2].max() > 0
    for j, n in enumerate(names):
        sy = np.eye(4, dtype=np.float32)[None] if models[n].symmetries is None else models[n].symmetries
        w = br.sym_dist(models[n].verts, sy[:, :3], init[j:j + 1, :3], gt[j:j + 1, :3], K[j])
        assert np.allclose([float(e["mssd"][j]), float(e["mspd"][j])], w[0], rtol=1e-6, atol=1e-9)
    assert np.array_equal(rec, br.recalls(werr, npy(e["mssd"]), npy(e["mspd"]), [models[n].diameter for n in names], W))
    assert np.array_equal(rec, hip.bop.recalls(e, [models[n].diameter for n in names], W))
    # one call over both frames (shared observed depth, source index) == one call per object, bit for bit
    for j, it in enumerate(items):
        r1, e1 = hip.bop_metrics([it], init[j:j + 1], want_errors=True)
        assert np.array_equal(r1[0], rec[j]) and np.array_equal(npy(e1["counts"])[0], wcounts[j])
        for k in ("vsd", "mssd", "mspd"):
            assert np.array_equal(npy(e1[k]).reshape(-1).view(np.int64), npy(e[k])[j].reshape(-1).view(np.int64)), k
    # the evaluator's accumulator: per-class and overall means of what it was given
    hip.bop.update(names, rec)
    s = hip.bop.summarize()
    assert s["all"]["n"] == 6 and abs(s["all"]["ar"] - rec.mean()) < 1e-12 and s["ape"]["n"] == 2
    assert abs(s["glue"]["ar_vsd"] - rec[[j for j, n in enumerate(names) if n == "glue"], 0].mean()) < 1e-12
