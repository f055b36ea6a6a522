"""GPU tests of the top-K distinct RANSAC hypotheses: rnnpose_pnp_ransac_topk_f64 and the plumbing above it (ops,
torch.ops.rnnpose, DescriptorPoseInitializer.candidates, HipEpoch(init_candidates=...)), against the fp64 numpy restatement
tests/pnp_topk_ref.py.

Bounds: fp64 against fp64 -- the candidate poses, T and final_cost at the 1e-6 of test_gpu_pose_init.test_ransac_against_the_restatement;
everything discrete (hyp, n_found, masks, counts, info, dup_of) EQUAL.  Equality needs decisions that rounding cannot flip, so the
planted data is the first seed for which the restatement's own decisions keep their margins -- every distance the selection or dup_of
decides on more than 1e-4 diag from sep, every residual a polish step or the final mask decides on more than 1e-3 px from tau -- and the
margins are asserted again on the run that is compared (the selection then reads the DEVICE's cost array, which a separate assertion
holds to the restatement's at 1e-6 relative: near-ties in cost cannot reorder the comparison).

tests/test_pnp_topk_on_host.py runs the cases of this module that need no renderer on the host-executed kernels."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import pnp_ref as pr
import pnp_topk_ref as tr

pytestmark = pytest.mark.gpu

TAU, SEP, N_POLISH = 4.0, 0.25, 4
COUNTS, HYPS, KTS = [4, 57, 300], [1, 65, 256, 1100], [1, 2, 4, 16]
DIST_MARGIN, TAU_MARGIN = 1e-4, 1e-3
REC = np.dtype([("Rt", np.float64, (4, 12)), ("n", np.int32), ("best", np.int32)])      # pnp::HypRec
BOX = np.dtype([("lo", np.float64, 3), ("hi", np.float64, 3), ("sep", np.float64), ("diag", np.float64)])      # pnp::TopkBox
OUT_SPEC = (("T", torch.float32, -777.0), ("cost", torch.float64, -777.0), ("inliers", torch.int32, -777), ("hyp", torch.int32, -777),
            ("mask", torch.uint8, 77), ("n_inl", torch.int32, -777), ("fcost", torch.float64, -777.0), ("info", torch.int32, -777),
            ("dup_of", torch.int32, -777), ("n_found", torch.int32, -777))


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


def words(rnd):
    return dev(np.asarray(rnd).astype(np.int64), np.int64)


def margins_hold(refs):
    return all(r["select_margin"] > DIST_MARGIN * r["diag"] and r["dup_margin"] > DIST_MARGIN * r["diag"] and r["tau_margin"] > TAU_MARGIN for r in refs)


# ---- the planted two-mode data and its restatement, computed once ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_ref():
    """The first seed whose restatement keeps every margin at every Hyp of the grid (Kt = 16: the decisions of a smaller Kt are a prefix).
    -> (case, hyps): hyps[b] = (cost, inliers, poses) of object b at Hyp = 1100; a smaller Hyp is a prefix of it."""
    for seed in range(50):
        case = tr.two_mode_case(COUNTS, max(HYPS), seed)
        X, x, counts, K, rnd = case[:5]
        hyps = [tr.hypotheses(X[b], x[b], counts[b], K[b].astype(np.float64), rnd[b], TAU) for b in range(3)]
        if all(margins_hold(restate(case, hyps, Hyp, max(KTS))) for Hyp in HYPS):
            print(f"planted two-mode data: seed {seed}")
            return case, hyps
    raise AssertionError("no seed keeps the margins")


def restate(case, hyps, Hyp, Kt, sep_frac=SEP, min_inliers=0, cost=None, inliers=None):
    X, x, counts, K, rnd = case[:5]
    pre = [(h[0][:Hyp], h[1][:Hyp], h[2][:Hyp]) for h in hyps]
    return tr.topk(X, x, counts, K.astype(np.float64), rnd[:, :Hyp], TAU, N_POLISH, 4, Kt, sep_frac, min_inliers, hyps=pre, cost=cost, inliers=inliers)


def call_lib(case, Hyp, Kt, sep_frac=SEP, min_inliers=0, tau=TAU, n_polish=N_POLISH, guard=64):
    """The C entry point on guarded outputs and a guarded workspace.  -> (status, outputs as numpy by name, the workspace's candidate
    records (B,Hyp) with the extents (B) under the key "box" of the outputs, untouched(): every guard zone and the workspace behind its
    used bytes still hold their canaries)."""
    from rnnpose_amd import _lib, ops as _ops
    lib = _lib.load()
    X, x, counts, K, rnd = case[:5]
    B, M = X.shape[:2]
    shapes = dict(T=(B, Kt, 4, 4), cost=(B, Hyp), inliers=(B, Hyp), hyp=(B, Kt), mask=(B, Kt, M), n_inl=(B, Kt), fcost=(B, Kt), info=(B, Kt),
                  dup_of=(B, Kt), n_found=(B,))
    bufs, views = {}, {}
    for name, dt, fill in OUT_SPEC:
        n = int(np.prod(shapes[name]))
        bufs[name] = torch.full((n + 2 * guard,), fill, dtype=dt).cuda()
        views[name] = bufs[name][guard:guard + n].view(*shapes[name])
    n = int(lib.rnnpose_pnp_ransac_topk_workspace_bytes(B, Hyp, Kt))
    assert n == B * Hyp * 392 + B * Kt * 96 + B * 64 + (B * Hyp + 7) // 8 * 8
    ws = torch.full((n // 8 + guard,), -777, dtype=torch.int64).cuda()
    a = (dev(X), dev(x), dev(counts, np.int32), dev(K), _ops.random_words(words(rnd[:, :Hyp])))
    st = lib.rnnpose_pnp_ransac_topk_f64(ptr(a[0]), ptr(a[1]), ptr(a[2]), M, ptr(a[3]), ptr(a[4]), B, Hyp, tau, n_polish, 4, Kt, sep_frac, min_inliers,
                                         ptr(ws), n, *[ptr(views[name]) for name, _, _ in OUT_SPEC], None)
    torch.cuda.synchronize()

    def untouched():
        ok = bool((ws[n // 8:] == -777).all())
        for name, _, fill in OUT_SPEC:
            m = views[name].numel()
            ok = ok and bool((bufs[name][:guard] == fill).all()) and bool((bufs[name][guard + m:] == fill).all())
        return ok
    rec = npy(ws[:B * Hyp * 49]).view(REC).reshape(B, Hyp)
    out = {k: npy(v) for k, v in views.items()}
    out["box"] = npy(ws[B * Hyp * 49 + B * Kt * 12:][:B * 8]).view(BOX).reshape(B)
    return st, out, rec, untouched


def candidate_pose(rec):
    T = np.eye(4)
    T[:3] = rec["Rt"][rec["best"]].reshape(3, 4)
    return T


def check_against(case, hyps, out, rec, Hyp, Kt, sep_frac=SEP, min_inliers=0):
    """Every output of one call against the restatement (the selection on the device's cost and inlier arrays)."""
    counts = case[2]
    refs = restate(case, hyps, Hyp, Kt, sep_frac, min_inliers, cost=out["cost"], inliers=out["inliers"])
    assert margins_hold(refs), [(r["select_margin"] / r["diag"], r["dup_margin"] / r["diag"], r["tau_margin"]) for r in refs]
    for b, r in enumerate(refs):
        n = int(counts[b])
        box = out["box"][b]                                  # the extent: min / max are exact, diag and sep two roundings of the same formula
        assert np.array_equal(box["lo"], r["lo"]) and np.array_equal(box["hi"], r["hi"])
        assert abs(box["diag"] - r["diag"]) <= 1e-15 * r["diag"] and abs(box["sep"] - r["sep"]) <= 1e-15 * r["sep"]
        cost, fin = out["cost"][b], np.isfinite(r["cost"])
        both = fin & np.isfinite(cost)
        close = both.copy()
        close[both] = np.abs(cost[both] - r["cost"][both]) <= 1e-6 * np.abs(r["cost"][both])
        agree = close | (~fin & ~np.isfinite(cost))
        assert agree.mean() >= 0.99 and np.array_equal(out["inliers"][b][close], r["inliers"][close])
        assert out["n_found"][b] == r["n_found"] and np.array_equal(out["hyp"][b], r["hyp"]), (b, out["hyp"][b], r["hyp"])
        for k in range(Kt):
            h = int(r["hyp"][k])
            assert (out["mask"][b, k, n:] == 77).all()                          # rows behind count are not written
            if h < 0:
                assert out["info"][b, k] == -1 and (out["T"][b, k] == -777.0).all() and not out["mask"][b, k, :n].any() and out["n_inl"][b, k] == 0
                assert np.isinf(out["fcost"][b, k]) and out["dup_of"][b, k] == -1
                continue
            assert close[h] and np.abs(candidate_pose(rec[b, h]) - r["poses"][h]).max() <= 1e-6      # the start of the polish
            assert out["info"][b, k] == r["info"][k] and out["dup_of"][b, k] == r["dup_of"][k]
            assert np.array_equal(out["mask"][b, k, :n], r["inlier_mask"][k].astype(np.uint8))
            assert out["n_inl"][b, k] == r["n_inliers"][k]
            if r["info"][k] == 0:
                assert abs(out["fcost"][b, k] - r["final_cost"][k]) <= 1e-6 * r["final_cost"][k]
                assert np.abs(out["T"][b, k] - r["T"][k]).max() <= 1e-6 and out["T"][b, k, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
            else:
                assert (out["T"][b, k] == -777.0).all() and np.isinf(out["fcost"][b, k])
    return refs


@pytest.mark.parametrize("Kt", KTS)
@pytest.mark.parametrize("Hyp", HYPS)
def test_topk_against_the_restatement(ops, grid_ref, Hyp, Kt):
    """B = 3 objects with 4, 57 and 300 correspondences: one lane, a ragged wave, several passes of the 256-thread selection."""
    case, hyps = grid_ref
    st, out, rec, untouched = call_lib(case, Hyp, Kt)
    assert st == 0 and untouched()
    refs = check_against(case, hyps, out, rec, Hyp, Kt)
    print(f"Hyp {Hyp} Kt {Kt}: n_found {out['n_found'].tolist()}, margins / diag "
          f"{[float('%.2g' % (min(r['select_margin'], r['dup_margin']) / r['diag'])) for r in refs]}")


@pytest.mark.parametrize("Kt", KTS)
def test_slot_0_is_pnp_ransac(ops, grid_ref, Kt):
    """Slot 0 of every output is bit-identical to ops.pnp_ransac, whatever Kt; with Kt = 1 that is the whole output."""
    case, _ = grid_ref
    X, x, counts, K, rnd = case[:5]
    for Hyp in (65, 1100):
        a = (dev(X), dev(x), dev(counts, np.int32), dev(K), words(rnd[:, :Hyp]))
        T1, cost1, inl1, best, mask1, n1, f1, info1 = ops.pnp_ransac(*a, tau=TAU, n_polish=N_POLISH)
        T, cost, inl, hyp, mask, n_inl, fcost, info, dup_of, n_found = ops.pnp_ransac_topk(*a, tau=TAU, n_polish=N_POLISH, top_k=Kt, sep_frac=SEP)
        assert torch.equal(cost, cost1) and torch.equal(inl, inl1)
        assert torch.equal(T[:, 0], T1) and torch.equal(hyp[:, 0], best) and torch.equal(mask[:, 0], mask1) and torch.equal(n_inl[:, 0], n1)
        assert torch.equal(fcost[:, 0], f1) and torch.equal(info[:, 0], info1) and bool((dup_of[:, 0] == -1).all())
        assert tuple(T.shape) == (3, Kt, 4, 4) and tuple(mask.shape) == (3, Kt, X.shape[1]) and bool((n_found <= Kt).all())


# ---- planted cases ---------------------------------------------------------------------------------------------------------------------
def run_ops(ops, case, Hyp=None, **kw):
    X, x, counts, K, rnd = case[:5]
    kw = dict(dict(tau=TAU, n_polish=N_POLISH, top_k=4, sep_frac=SEP), **kw)
    out = ops.pnp_ransac_topk(dev(X), dev(x), dev(counts, np.int32), dev(K), words(rnd if Hyp is None else rnd[:, :Hyp]), **kw)
    return dict(zip(("T", "cost", "inliers", "hyp", "mask", "n_inl", "fcost", "info", "dup_of", "n_found"), out))


def test_every_slot_is_pnp_ransac_on_its_own_hypothesis(ops, grid_ref):
    """Slot k of every output is bit-identical to ops.pnp_ransac called with slot k's hypothesis as its ONLY one (rnd[b, hyp[b, k]]):
    with one hypothesis that call picks it, and both entry points polish with the one body (polish_body, csrc/pnp.cuh).  Against a
    vacuous pass: every object fills at least two slots, on the restatement first."""
    case, hyps = grid_ref
    X, x, counts, K, rnd = case[:5]
    Hyp, Kt = 65, 4
    assert all(r["n_found"] >= 2 for r in restate(case, hyps, Hyp, Kt)), "the planted case no longer fills two slots per object"
    o = run_ops(ops, case, Hyp=Hyp, top_k=Kt, T=torch.full((3, Kt, 4, 4), -777.0).cuda())
    hyp = o["hyp"].long()
    assert bool(((hyp >= 0).sum(1) >= 2).all()), hyp
    a, w, compared = (dev(X), dev(x), dev(counts, np.int32), dev(K)), words(rnd[:, :Hyp]), 0
    for k in range(Kt):
        rows = hyp[:, k] >= 0                                # (objects without a slot k: their hypothesis 0 runs and is not compared)
        h = hyp[:, k].clamp(min=0)
        one = w[torch.arange(3).cuda(), h][:, None].contiguous()
        T1, cost1, inl1, best, mask1, n1, f1, info1 = ops.pnp_ransac(*a, one, tau=TAU, n_polish=N_POLISH, T=torch.full((3, 4, 4), -777.0).cuda())
        assert tuple(one.shape) == (3, 1, 3) and bool((best[rows] == 0).all())
        assert torch.equal(cost1[rows, 0], o["cost"][rows, h[rows]]) and torch.equal(inl1[rows, 0], o["inliers"][rows, h[rows]])
        assert torch.equal(mask1[rows], o["mask"][rows, k]) and torch.equal(n1[rows], o["n_inl"][rows, k])
        assert torch.equal(f1[rows], o["fcost"][rows, k]) and torch.equal(info1[rows], o["info"][rows, k])
        written = rows & (info1 == 0)
        assert torch.equal(T1[written], o["T"][written, k])
        compared += int(rows.sum())
    assert compared >= 6 and compared == int((hyp >= 0).sum())


def test_two_modes_fill_slots_0_and_1(ops, grid_ref):
    case, _ = grid_ref
    Ta, Tb = case[5], case[6]
    o = {k: npy(v) for k, v in run_ops(ops, case, top_k=2).items()}
    for b in (1, 2):                                         # (57 and 300 correspondences; the 4 of object 0 are 2 + 2: no mode has 3)
        lo, hi, diag = tr.extent(case[0][b], case[2][b])
        assert o["n_found"][b] == 2 and o["info"][b].tolist() == [0, 0] and o["dup_of"][b].tolist() == [-1, -1]
        d = [[tr.distance(o["T"][b, k].astype(np.float64), T[b], lo, hi) / diag for T in (Ta, Tb)] for k in range(2)]
        assert d[0][0] < 0.1 and d[1][1] < 0.1 and d[0][1] > 1.0, d          # slot 0 = the wrong mode A (45 %), slot 1 = the truth B (35 %)


def test_sep_frac_and_min_inliers_gates(ops, grid_ref):
    case, hyps = grid_ref
    X, x, counts, K, rnd = case[:5]
    # sep_frac = 0: everything but exact duplicates is distinct; the same triple twice in rnd yields one slot
    twice = (X, x, counts, K, np.repeat(rnd[:, :8], 2, axis=1))
    o = {k: npy(v) for k, v in run_ops(ops, twice, top_k=16, sep_frac=0.0).items()}
    for b in range(3):
        kept = o["hyp"][b, :o["n_found"][b]]
        assert np.all(kept % 2 == 0) and len(set(kept.tolist())) == len(kept)          # the lower h of every pair, each once
        assert o["n_found"][b] == np.isfinite(o["cost"][b, ::2]).sum()                  # (these 8 triples give 8 different poses or none)
    # sep_frac huge: nothing is distinct from slot 0
    o = {k: npy(v) for k, v in run_ops(ops, case, top_k=4, sep_frac=1e6).items()}
    assert o["n_found"].tolist() == [1, 1, 1] and (o["hyp"][:, 1:] == -1).all() and (o["info"][:, 1:] == -1).all()
    # min_inliers above the second mode's support (35 %): slot 0 (45 %) is alone -- and slot 0 itself is exempt from the gate
    free = {k: npy(v) for k, v in run_ops(ops, case, top_k=4).items()}
    for b in (1, 2):
        second = int(free["inliers"][b, free["hyp"][b, 1]])
        first = int(free["inliers"][b, free["hyp"][b, 0]])
        assert second < first
        o = {k: npy(v) for k, v in run_ops(ops, case, top_k=4, min_inliers=(first + second + 1) // 2).items()}
        assert o["n_found"][b] == 1 and o["hyp"][b, 0] == free["hyp"][b, 0]
        o = {k: npy(v) for k, v in run_ops(ops, case, top_k=4, min_inliers=10 ** 6).items()}
        assert o["n_found"][b] == 1 and o["hyp"][b, 0] == free["hyp"][b, 0] and o["info"][b, 0] == 0


def test_fewer_distinct_modes_than_slots(ops, grid_ref):
    """Hyp = 64, Kt = 16 on clean single-mode data: the tail slots have hyp -1, info -1 and T untouched."""
    X, x, rnd, _ = pr.p3p_scenes(n_scenes=3, n_triples=64)
    K = np.tile(pr.P3P_K, (3, 1, 1)).astype(np.float32)
    Tc = torch.full((3, 16, 4, 4), -777.0).cuda()
    o = ops.pnp_ransac_topk(dev(X), dev(x), dev([64, 64, 64], np.int32), dev(K), words(rnd), tau=TAU, n_polish=N_POLISH, top_k=16, sep_frac=SEP, T=Tc)
    T, _, _, hyp, mask, n_inl, fcost, info, dup_of, n_found = [npy(t) for t in o]
    assert (n_found >= 1).all() and (n_found < 16).all()
    for b in range(3):
        nf = n_found[b]
        assert (hyp[b, nf:] == -1).all() and (info[b, nf:] == -1).all() and (T[b, nf:] == -777.0).all() and not mask[b, nf:].any()
        assert (n_inl[b, nf:] == 0).all() and np.isinf(fcost[b, nf:]).all() and (dup_of[b, nf:] == -1).all()
        assert info[b, 0] == 0 and n_inl[b, 0] == 64 and (hyp[b, :nf] >= 0).all()


def test_degenerate_inputs(ops, grid_ref):
    case, _ = grid_ref
    X, x, counts, K, rnd = case[:5]
    # count 0 and 3 (below min_count): nothing found, T untouched; a count beyond M is clamped
    Tc = torch.full((3, 4, 4, 4), -777.0).cuda()
    o = {k: npy(v) for k, v in run_ops(ops, (X, x, np.array([0, 3, 100000], np.int32), K, rnd), Hyp=256, T=Tc).items()}
    assert o["n_found"][:2].tolist() == [0, 0] and (o["hyp"][:2] == -1).all() and (o["info"][:2] == -1).all() and (o["T"][:2] == -777.0).all()
    assert np.isinf(o["cost"][:2]).all() and np.isinf(o["fcost"][:2]).all() and not o["mask"][:2].any() and (o["dup_of"][:2] == -1).all()
    assert o["n_found"][2] >= 1 and o["info"][2, 0] == 0
    # all X equal (diag = 0) and all-collinear points: never NaN, every slot either info -1 and untouched or a finite pose
    same = np.zeros_like(X)
    same[:] = np.array([0.02, -0.01, 0.03], np.float32)
    line = np.zeros_like(X)
    line[:] = np.linspace(-0.1, 0.1, X.shape[1])[None, :, None] * np.array([1.0, 0.4, -0.3])
    xl = np.stack([pr.project(np.eye(3), np.array([0.0, 0.0, 0.8]), pr.P3P_K, line[b].astype(np.float64))[0] for b in range(3)]).astype(np.float32)
    for Xc, xc in ((same, x), (line, xl)):
        Tc = torch.full((3, 4, 4, 4), -777.0).cuda()
        o = {k: npy(v) for k, v in run_ops(ops, (Xc, xc, counts, K, rnd), Hyp=256, T=Tc).items()}
        assert not np.isnan(o["cost"]).any() and not np.isnan(o["T"]).any() and not np.isnan(o["fcost"]).any()
        for b in range(3):
            nf = o["n_found"][b]
            assert 0 <= nf <= 4 and (o["hyp"][b, :nf] >= 0).all() and (o["hyp"][b, nf:] == -1).all() and len(set(o["hyp"][b, :nf].tolist())) == nf
            for k in range(4):
                assert (o["info"][b, k] == -1 and (o["T"][b, k] == -777.0).all()) or (o["info"][b, k] == 0 and np.isfinite(o["T"][b, k]).all() and k < nf)


def test_two_starts_that_polish_into_one_optimum(ops, grid_ref):
    """Clean single-mode data with a loose tau and a sep_frac small enough to separate the minimal solves of different triples (their
    fp32-rounding-sized differences): every start polishes into the one optimum, and dup_of says so."""
    X, x, rnd, poses = pr.p3p_scenes(n_scenes=3, n_triples=64)
    K = np.tile(pr.P3P_K, (3, 1, 1)).astype(np.float32)
    counts = np.array([64, 64, 64], np.int32)
    sep_frac = 1e-9
    o = {k: npy(v) for k, v in run_ops(ops, (X, x, counts, K, rnd), top_k=4, sep_frac=sep_frac, tau=8.0).items()}
    refs = tr.topk(X, x, counts, K.astype(np.float64), rnd, 8.0, N_POLISH, 4, 4, sep_frac, cost=o["cost"], inliers=o["inliers"])
    for b, r in enumerate(refs):
        assert o["n_found"][b] == 4 and o["info"][b].tolist() == [0, 0, 0, 0]
        assert o["dup_of"][b].tolist() == [-1, 0, 0, 0]
        if r["select_margin"] > DIST_MARGIN * r["diag"] * 1e-6 and r["dup_margin"] > 1e-12:      # (decisions at this scale: compared where the restatement is sure)
            assert np.array_equal(o["hyp"][b], r["hyp"]) and np.array_equal(o["dup_of"][b], r["dup_of"])
        assert np.abs(o["T"][b] - poses[b]).max() <= 1e-4


def test_reruns_and_batch_independence(ops, grid_ref):
    case, _ = grid_ref
    X, x, counts, K, rnd = case[:5]
    one, two = run_ops(ops, case, Hyp=300, top_k=4), run_ops(ops, case, Hyp=300, top_k=4)
    assert all(torch.equal(one[k], two[k]) for k in one)
    for b in range(3):                                       # every object alone == the object in the batch
        alone = run_ops(ops, (X[b:b + 1], x[b:b + 1], counts[b:b + 1], K[b:b + 1], rnd[b:b + 1]), Hyp=300, top_k=4)
        assert all(torch.equal(alone[k][0], one[k][b]) for k in one), b


def test_bad_arguments_return_1_and_write_nothing(ops, grid_ref):
    from rnnpose_amd import _lib
    lib = _lib.load()
    case, _ = grid_ref
    X, x, counts, K, rnd = case[:5]
    B, M, Hyp, Kt = 3, X.shape[1], 65, 4
    Xd, xd, cd, Kd, rd = dev(X), dev(x), dev(counts, np.int32), dev(K), ops.random_words(words(rnd[:, :Hyp]))
    n = int(lib.rnnpose_pnp_ransac_topk_workspace_bytes(B, Hyp, Kt))
    assert n > 0 and n % 8 == 0
    for bad in ((0, Hyp, Kt), (B, 0, Kt), (B, Hyp, 0), (B, Hyp, 17)):
        assert lib.rnnpose_pnp_ransac_topk_workspace_bytes(*bad) == 0
    ws = torch.zeros(n // 8, dtype=torch.int64).cuda()
    shapes = dict(T=(B, Kt, 4, 4), cost=(B, Hyp), inliers=(B, Hyp), hyp=(B, Kt), mask=(B, Kt, M), n_inl=(B, Kt), fcost=(B, Kt), info=(B, Kt),
                  dup_of=(B, Kt), n_found=(B,))
    outs = {name: torch.full(shapes[name], fill, dtype=dt).cuda() for name, dt, fill in OUT_SPEC}
    good = dict(X=ptr(Xd), x=ptr(xd), count=ptr(cd), M=M, K=ptr(Kd), rnd=ptr(rd), B=B, Hyp=Hyp, tau=TAU, n_polish=2, min_count=4, Kt=Kt, sep_frac=SEP,
                min_inliers=0, ws=ptr(ws), n=n, **{k: ptr(v) for k, v in outs.items()}, stream=None)
    bad = [dict(X=None), dict(x=None), dict(count=None), dict(K=None), dict(rnd=None), dict(ws=None)] + [{k: None} for k in outs] + \
          [dict(B=0), dict(M=0), dict(Hyp=0), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(n_polish=-1), dict(n_polish=65), dict(min_count=3),
           dict(Kt=0), dict(Kt=17), dict(Kt=-1), dict(sep_frac=-1e-9), dict(sep_frac=float("nan")), dict(sep_frac=float("inf")), dict(min_inliers=-1),
           dict(n=n - 8), dict(ws=C.c_void_p(ws.data_ptr() + 4))]
    for change in bad:
        assert lib.rnnpose_pnp_ransac_topk_f64(*dict(good, **change).values()) == 1, change
        assert len(lib.rnnpose_last_error()) > 0
    torch.cuda.synchronize()
    assert all(bool((outs[name] == fill).all()) for name, _, fill in OUT_SPEC) and not bool(ws.any())
    assert lib.rnnpose_pnp_ransac_topk_f64(*good.values()) == 0
    torch.cuda.synchronize()
    assert npy(outs["info"])[1:, 0].tolist() == [0, 0]


def test_ops_refusals(ops, grid_ref):
    case, _ = grid_ref
    X, x, counts, K, rnd = case[:5]
    a = [dev(X), dev(x), dev(counts, np.int32), dev(K), words(rnd[:, :65])]
    for bad in (dict(tau=0.0), dict(tau=float("nan")), dict(n_polish=-1), dict(min_count=3), dict(top_k=0), dict(top_k=17), dict(top_k=2.5),
                dict(sep_frac=-0.1), dict(sep_frac=float("nan")), dict(sep_frac=float("inf")), dict(min_inliers=-1),
                dict(T=torch.zeros(3, 3, 4, 4).cuda()), dict(T=torch.zeros(3, 4, 4, 4, dtype=torch.float64).cuda()),
                dict(T=torch.zeros(3, 4, 4, 8).cuda()[..., ::2])):
        with pytest.raises(ValueError):
            ops.pnp_ransac_topk(*a, **bad)
    swaps = [(0, a[0][:, :, :2].contiguous()), (0, X), (1, a[1][:, :-1].contiguous()), (2, a[2][:2].contiguous()), (2, a[2].to(torch.int64)),
             (2, torch.stack([a[2], a[2]], 1)[:, 0]), (3, a[3][:2].contiguous()), (4, a[4][:2].contiguous()), (4, a[4][:, :, :2].contiguous()),
             (4, a[4].double())]
    for i, t in swaps:
        with pytest.raises(ValueError):
            ops.pnp_ransac_topk(*[t if j == i else v for j, v in enumerate(a)])
    assert int(ops.pnp_ransac_topk(*a)[9].sum()) >= 3                        # the defaults run


def test_torch_ops_equal_ops_and_have_a_fake_kernel(ops, grid_ref):
    import rnnpose_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    case, _ = grid_ref
    X, x, counts, K, rnd = case[:5]
    a = (dev(X), dev(x), dev(counts, np.int32), dev(K), words(rnd[:, :256]))
    want = ops.pnp_ransac_topk(*a, tau=TAU, n_polish=N_POLISH, top_k=4, sep_frac=SEP, min_inliers=3)
    got = torch.ops.rnnpose.pnp_ransac_topk(*a, TAU, N_POLISH, 4, 4, SEP, 3)
    assert len(got) == 10 and all(torch.equal(p, q) for p, q in zip(got, want))
    with FakeTensorMode():
        e = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="cuda", dtype=dtype)
        f = torch.ops.rnnpose.pnp_ransac_topk(e(3, 300, 3), e(3, 300, 2), e(3, dtype=torch.int32), e(3, 3, 3), e(3, 256, 3, dtype=torch.int64), TAU,
                                              N_POLISH, 4, 4, SEP, 3)
        assert [(tuple(t.shape), t.dtype) for t in f] == [(tuple(t.shape), t.dtype) for t in got]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
WRONG_DEG = 60.0


@pytest.fixture(scope="module")
def scene(ops):
    """1 frame x 3 objects at 240 x 320 with 642 vertices each, and correspondences PLANTED from the scene's own vertices: 45 % project
    under a wrong pose (the ground truth rotated 60 degrees about the camera's z-axis), 35 % under the ground truth, 20 % are uniform
    in the frame; 0.5 px noise."""
    from oracle import rnnpose_oracle as orc
    from rnnpose_amd import eval_epoch as ee, synthetic as syn
    from rnnpose_amd.pose_refiner import default_config
    torch.manual_seed(0)
    models = ee.synthetic_models(sub=3)
    cfg = default_config(RENDER_ITER_COUNT=1, ITER_COUNT=2, OPTIM_ITER_COUNT=1, render_image_size=(240, 320), zoom_crop_size=(128, 128))
    Tt = lambda v: torch.from_numpy(v)

    def make(**kw):
        hip = ee.HipEpoch(models, cfg=cfg, **kw)
        hip.refiner.cf_net.update_block.load_state_dict({k: Tt(v) for k, v in syn.make_module_weights(orc.UPDATE_BLOCK_SHAPES, seed=0).items()})
        hip.refiner.image_fea_enc.fnet.load_state_dict({k: Tt(v) for k, v in syn.make_module_weights(orc.encoder_shapes(), seed=2).items()})
        return hip
    hip = make(init="descriptors", init_candidates=4)
    items = ee.synthetic_scenes(models, 1, 3, image_size=(240, 320), renderer=hip.renderer)
    names = [it.class_name for it in items]
    Tg = dev(np.stack([it.pose_gt for it in items]))
    K = dev(np.stack([it.K for it in items]))
    depth = hip.renderer.render_zbuf(names, Tg, K, (240, 320))
    boxes = npy(ops.mask_bbox(depth.float().contiguous())) + np.array([-8, -8, 8, 8], np.int32)
    for it, bb in zip(items, boxes):
        it.bbox = bb
    rng = np.random.default_rng(11)
    c, s = np.cos(np.deg2rad(WRONG_DEG)), np.sin(np.deg2rad(WRONG_DEG))
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    M = 642
    X, x, wrong = np.zeros((3, M, 3), np.float32), np.zeros((3, M, 2), np.float32), []
    for b, it in enumerate(items):
        v = models[it.class_name].verts.astype(np.float64)
        G = it.pose_gt.astype(np.float64)
        Wp = G.copy()
        Wp[:3, :3] = Rz @ G[:3, :3]                                           # (about the camera's z-axis THROUGH the object's centre)
        wrong.append(Wp)
        Kd = it.K.astype(np.float64)
        perm = rng.permutation(M)
        na, nb = int(round(0.45 * M)), int(round(0.35 * M))
        uv = np.stack([rng.uniform(0, 320, M), rng.uniform(0, 240, M)], 1)
        uv[perm[:na]] = pr.project(Wp[:3, :3], Wp[:3, 3], Kd, v[perm[:na]])[0] + rng.normal(0, 0.5, (na, 2))
        uv[perm[na:na + nb]] = pr.project(G[:3, :3], G[:3, 3], Kd, v[perm[na:na + nb]])[0] + rng.normal(0, 0.5, (nb, 2))
        X[b], x[b] = v, uv
    rnd = rng.integers(0, 2 ** 32, (3, 512, 3), dtype=np.uint64)
    return dict(hip=hip, make=make, models=models, items=items, boxes=boxes, X=X, x=x, rnd=rnd, wrong=np.stack(wrong))


def add_error(models, it, T):
    v = models[it.class_name].verts.astype(np.float64)
    T, G = np.asarray(T, np.float64), it.pose_gt.astype(np.float64)
    return np.linalg.norm((v @ T[:3, :3].T + T[:3, 3]) - (v @ G[:3, :3].T + G[:3, 3]), axis=1).mean() / models[it.class_name].diameter


def test_end_to_end_the_score_picks_the_true_mode(ops, scene):
    """On the planted correspondences ops.pnp_ransac returns the wrong mode; ops.pnp_ransac_topk + select_poses returns the ground-truth
    mode.  The ranking is asserted on the fp64 restatement of the score first, then on the device."""
    import score_ref as sr
    hip, models, items = scene["hip"], scene["models"], scene["items"]
    K = np.stack([it.K for it in items]).astype(np.float32)
    a = (dev(scene["X"]), dev(scene["x"]), dev([642] * 3, np.int32), dev(K), words(scene["rnd"]))
    T1 = npy(ops.pnp_ransac(*a, tau=TAU, n_polish=N_POLISH)[0])
    T, _, _, hyp, _, n_inl, _, info, dup_of, n_found = ops.pnp_ransac_topk(*a, tau=TAU, n_polish=N_POLISH, top_k=4, sep_frac=SEP)
    assert np.array_equal(npy(T[:, 0]), T1) and (npy(n_found) >= 2).all() and (npy(info)[:, :2] == 0).all() and (npy(dup_of)[:, :2] == -1).all()
    for b, it in enumerate(items):
        e_single, e0, e1 = add_error(models, it, T1[b]), add_error(models, it, npy(T)[b, 0]), add_error(models, it, npy(T)[b, 1])
        print(f"object {b}: ADD / diameter of pnp_ransac {e_single:.3f}, slot 0 {e0:.3f}, slot 1 {e1:.4f}; inliers {npy(n_inl)[b, :2].tolist()}")
        assert e_single > 0.1 and e1 < 0.1                                   # the cheapest fit is the wrong mode, slot 1 the truth
    cand = T[:, :2].contiguous()
    best, index, scores = hip.select_poses(items, cand)
    # the ranking on the fp64 restatement of the score (tests/score_ref.py), from the device's own renders
    names = [it.class_name for it in items for _ in range(2)]
    g2 = items[0].geofea_2d.cuda()[None].float().contiguous()
    obs = items[0].depth.cuda()[None].float().contiguous()
    scorer = hip._default_scorer if hip.scorer is None else hip.scorer
    rd, rdesc, window, _ = scorer.render(names, cand.reshape(6, 4, 4), np.repeat(K, 2, axis=0), (240, 320))
    ref_scores = sr.pose_score(npy(rd)[:, 0], npy(rdesc), npy(window), npy(g2), npy(obs), [0] * 6, scorer.depth_tol)[1].reshape(3, 2)
    assert (ref_scores[:, 1] > ref_scores[:, 0]).all(), ref_scores
    sc = npy(scores)
    assert (sc[:, 1] > sc[:, 0]).all() and npy(index).tolist() == [1, 1, 1] and np.abs(sc - ref_scores).max() <= 1e-9
    for b, it in enumerate(items):
        assert add_error(models, it, npy(best)[b]) < 0.1


def test_end_to_end_hip_epoch_selects_by_the_score(ops, scene):
    hip, make, models, items = scene["hip"], scene["make"], scene["models"], scene["items"]
    names = [it.class_name for it in items]
    g2 = items[0].geofea_2d.cuda()[None]
    K = dev(np.stack([it.K for it in items]))
    cand, rec = hip.init.candidates(names, g2, [0, 0, 0], K, dev(scene["boxes"], np.int32))
    assert tuple(cand.shape) == (3, 4, 4, 4) and rec["valid"][:, 0].all() and not rec["fallback"].any()
    assert np.array_equal(rec["valid"], (rec["info"] == 0) & (rec["dup_of"] < 0))
    for b in range(3):                                       # a slot that is not valid holds slot 0's pose
        for k in range(4):
            assert rec["valid"][b, k] or torch.equal(cand[b, k], cand[b, 0])
    _, _, scores = hip.select_poses(items, cand)
    sel = np.argmax(np.where(rec["valid"], npy(scores), -np.inf), axis=1)
    T0 = hip.initial_poses(items)
    info = hip.last_init_info
    assert torch.equal(T0, cand[torch.arange(3).cuda(), torch.as_tensor(sel).cuda()])
    assert info["selected"].tolist() == sel.tolist() and np.array_equal(info["candidates"], npy(cand)) and np.array_equal(info["candidate_valid"], rec["valid"])
    assert np.array_equal(info["candidate_scores"], npy(scores)) and info["rows"].tolist() == [0, 1, 2] and not info["fallback"].any()
    for b, it in enumerate(items):
        assert add_error(models, it, npy(T0)[b]) < 0.1
    # init_candidates = 1 is a HipEpoch without the argument, and the initializer's __call__ is what it was
    plain, one = make(init="descriptors"), make(init="descriptors", init_candidates=1)
    Tp, To = plain.initial_poses(items), one.initial_poses(items)
    assert torch.equal(Tp, To) and sorted(plain.last_init_info) == sorted(one.last_init_info) and "candidates" not in one.last_init_info
    assert torch.equal(Tp, cand[:, 0])                       # (slot 0 of the candidates is that pose)
    bare = [dataclasses.replace(it, pose_init=None) for it in items]
    assert torch.equal(plain.refine_frame(bare), one.refine_frame(bare))
    # refine_frame with init_select="score" starts from the selected poses
    given = [dataclasses.replace(it, pose_init=npy(T0)[b].copy(), bbox=None) for b, it in enumerate(items)]
    assert torch.equal(hip.refine_frame(bare), hip.refine_frame(given))
    # an empty box: the fallback in slot 0 and no valid slot
    empty = [bare[0], dataclasses.replace(bare[1], bbox=np.array([30, 30, 20, 20], np.int32)), bare[2]]
    Te = npy(hip.initial_poses(empty))
    info = hip.last_init_info
    assert info["fallback"].tolist() == [False, True, False] and not info["candidate_valid"][1].any() and info["selected"][1] == 0 and info["count"][1] == 0
    want = pr.fallback_pose(items[1].K, [30, 30, 20, 20], models[names[1]].diameter, (240, 320), hip.init.pixel_center)
    assert np.abs(Te[1] - want).max() <= 1e-6 and all(np.array_equal(info["candidates"][1, k], Te[1]) for k in range(4))
    with pytest.raises(ValueError):
        make(init="descriptors", init_candidates=0)
    with pytest.raises(ValueError):
        make(init_candidates=4)
    with pytest.raises(ValueError):
        make(init="descriptors", init_candidates=2, init_select="best")


def test_end_to_end_refined_selection(ops, scene):
    """init_select="refined" == the hand-made pipeline: expand the items into their candidates, refine_frame on the given poses,
    score_poses, the first maximum over the valid slots."""
    make, items = scene["make"], scene["items"]
    hip = make(init="descriptors", init_candidates=4, init_select="refined")
    names = [it.class_name for it in items]
    bare = [dataclasses.replace(it, pose_init=None) for it in items]
    mixed = [bare[0], items[1], bare[2]]                     # (item 1 brings its pose: it is not expanded)
    got = hip.refine_frame(mixed)
    info, got_scores = hip.last_init_info, hip.last_scores
    g2 = items[0].geofea_2d.cuda()[None]
    K = dev(np.stack([items[j].K for j in (0, 2)]))
    cand, rec = hip.init.candidates([names[0], names[2]], g2, [0, 0], K, dev(scene["boxes"][[0, 2]], np.int32))
    rows = [dataclasses.replace(bare[0], pose_init=npy(cand)[0, k].copy()) for k in range(4)] + [items[1]] + \
           [dataclasses.replace(bare[2], pose_init=npy(cand)[1, k].copy()) for k in range(4)]
    refined = hip.refine_frame(rows)
    scores = hip.score_poses(rows, refined)
    sc = npy(scores)
    cs = np.stack([sc[0:4], sc[5:9]])
    sel = np.argmax(np.where(rec["valid"], cs, -np.inf), axis=1)
    take = torch.as_tensor([int(sel[0]), 4, 5 + int(sel[1])]).cuda()
    assert torch.equal(got, refined[take]) and torch.equal(got_scores, scores[take])
    assert info["rows"].tolist() == [0, 2] and info["selected"].tolist() == sel.tolist() and np.array_equal(info["candidate_scores"], cs)
    assert np.array_equal(info["candidates"], npy(cand)) and np.array_equal(info["candidate_valid"], rec["valid"])
    with pytest.raises(ValueError):                          # one object's candidates would hide each other
        make(init="descriptors", init_candidates=4, init_select="refined", occlusion="frame").refine_frame(bare)
    eye = np.eye(4, dtype=np.float32)
    with pytest.raises(ValueError):                          # multi-view groups
        hip.refine_frame([dataclasses.replace(bare[0], object_id="a", cam_from_rig=eye), dataclasses.replace(bare[0], object_id="a", cam_from_rig=eye)])
