"""The LINEMOD metric kernels of csrc/eval_metrics.hip -- nn_search<2|3>, transform_points, pose_metrics -- and what stands on them
(ops.nn_search, ops.pose_metrics, the drop-in findNearestPointIdxLauncher, evaluator.LineMODEvaluator) at their edges (run with -m gpu on
an MI355X; the whole module also runs on the host-executed kernels, tests/test_eval_on_host.py).

tests/test_gpu_eval.py meets these kernels at a handful of convenient shapes and holds the fp64 columns to rtol 1e-6.  Here every shape is
in a table with the code path it is there for, and the yardsticks are the restatements of tests/eval_ref.py (checked on the CPU by
tests/test_eval_ref.py), which get the same fp32 arrays as the kernel.

Gates.  nn_search is exact: the index of the reference's serial loop (strict `<` from FLT_MAX over ascending indices, fp32 distance
(dx*dx + dy*dy) + dz*dz without contraction), for every batch element -- at the seams of the 1024-point LDS tile, on ties across a seam,
with exclude_self on global indices, on planted clouds whose winner changes under fp contraction, and on NaN / overflowing input, where
the loop takes nothing and np.argmin would.  The pose_metrics columns are fp64: they are held to the error another fp64 evaluation of
the same formula may have, derived per column in tests/eval_ref.py ((P + 2) u for the order of a sum of P terms, a few u per term, the
projection term absolute in u max|pixel|, the rotation compared as a cosine and as an angle only away from 0 and 180 degrees).  No gate is
taken from a kernel's output.  Each case prints `eval_edges <kernel> [<case>] err ... err/bound ...` (profiles/eval_edges_mutation.txt keeps
them).  The kernel tests go through the C ABI with their outputs and workspace pre-filled (index -7, 7.0, NaN) and guard cells behind
them: every cell must be written, none beyond.  No test here launches a kernel on mismatched buffers: the front end's refusals are
tested with the launch replaced by an exception."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_ref as er
from rnnpose_amd import synthetic as syn
from test_gpu_parity import ops  # noqa: F401  (the module-scoped build fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
SENT = 7.0
SENT_I = -7
GUARD = 16
K_LM = er.K_LM
_ids = lambda cases: [c[0] for c in cases]


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def lib_of():
    from rnnpose_amd import _lib
    return _lib.load()


def run_nn(ops, ref, que, exclude_self=False):
    """ref (B,n1,D), que (B,n2,D) numpy -> (B,n2) int32 through rnnpose_nn_search_f32, the index buffer pre-filled and guarded"""
    lib = lib_of()
    B, n1, dim = ref.shape
    n2 = que.shape[1]
    d_ref, d_que = D(ref), D(que)
    idx = torch.full((B * n2 + GUARD,), SENT_I, dtype=torch.int32).cuda()
    rc = lib.rnnpose_nn_search_f32(ptr(d_ref), ptr(d_que), ptr(idx), B, n1, n2, dim, int(exclude_self), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.rnnpose_last_error()
    got = N(idx)
    assert np.all(got[B * n2:] == SENT_I), "nn_search wrote beyond its B x pn2 indices"
    assert np.array_equal(N(d_ref), ref, equal_nan=True) and np.array_equal(N(d_que), que, equal_nan=True)
    return got[:B * n2].reshape(B, n2)


def gate_nn(case, got, ref, que, exclude_self=False):
    want = np.stack([er.nn_idx_serial(ref[b], que[b], exclude_self) for b in range(ref.shape[0])])
    bad = got != want
    print(f"eval_edges nn_search [{case}] err {int(bad.sum())} of {bad.size} indices differ, err/bound exact")
    if bad.any():
        b, q = (int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"nn_search [{case}]: {int(bad.sum())}/{bad.size} indices differ; first at batch {b} query {q}: got {got[b, q]} want {want[b, q]}")
    return want


def run_metrics(ops, model, pred, gt, K, sym):
    """-> (B,5) fp64 through rnnpose_pose_metrics_f64; out pre-filled with 7, two guard rows; the workspace NaN with a guarded tail"""
    lib = lib_of()
    P, B = model.shape[0], pred.shape[0]
    n = int(lib.rnnpose_pose_metrics_workspace_bytes(B, P))
    assert n == B * P * 28
    ws = torch.full((n // 4 + GUARD,), NAN, dtype=torch.float32).cuda()
    out = torch.full((B + 2, 5), SENT, dtype=torch.float64).cuda()
    d = [D(model), D(pred), D(gt), D(K)]
    rc = lib.rnnpose_pose_metrics_f64(ptr(d[0]), P, ptr(d[1]), ptr(d[2]), ptr(d[3]), B, int(sym), ptr(ws) if sym else C.c_void_p(0), n if sym else 0,
                                      ptr(out), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.rnnpose_last_error()
    o = N(out)
    assert np.all(o[B:] == SENT), "pose_metrics wrote beyond its B rows"
    assert torch.isnan(ws[n // 4:]).all() and (sym or torch.isnan(ws).all()), "pose_metrics wrote beyond (or, not symmetric, into) its workspace"
    return o[:B]


COLS = ("add", "adds", "proj", "trans")


def gate_metrics(case, got, r):
    """got (B,5) against eval_ref.pose_metrics_ref's dict: columns 0..3 within their bounds (the same inf / NaN where the restatement has
    one), the angle as a cosine everywhere and as an angle where its bound is defined; NaN where the restatement's is NaN."""
    cols, bound = r["cols"], r["bound"]
    assert got.shape == cols.shape
    fails = []
    for c, name in enumerate(COLS):
        fin = np.isfinite(cols[:, c])
        same_class = np.array_equal(got[~fin, c], cols[~fin, c], equal_nan=True)             # NaN where NaN, the same infinity where inf
        err = np.abs(got[fin, c] - cols[fin, c])
        bd = bound[fin, c]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bd > 0, err / np.where(bd > 0, bd, 1), np.where(err > 0, np.inf, 0.0))
        print(f"eval_edges pose_metrics.{name} [{case}] err {float(np.nanmax(err)) if err.size else 0.0:.3e} err/bound {float(np.nanmax(ratio)) if err.size else 0.0:.3f}")
        if not same_class or not np.all(err <= bd):
            fails.append(f"{name}: got {got[:, c]!r} want {cols[:, c]!r} bound {bound[:, c]!r}")
    nan = np.isnan(cols[:, 4])
    if not np.array_equal(np.isnan(got[:, 4]), nan):
        fails.append(f"angle NaN pattern: got {got[:, 4]!r} want {cols[:, 4]!r}")
    cerr = np.abs(np.cos(np.deg2rad(got[~nan, 4])) - r["cos"][~nan])
    print(f"eval_edges pose_metrics.cos [{case}] err {float(np.nanmax(cerr)) if cerr.size else 0.0:.3e} err/bound "
          f"{float(np.nanmax(cerr / r['cos_bound'][~nan])) if cerr.size else 0.0:.3f}")
    if not np.all(cerr <= r["cos_bound"][~nan]):
        fails.append(f"cosine of the angle: got {got[:, 4]!r} want {cols[:, 4]!r}")
    ang = ~np.isnan(bound[:, 4])
    aerr = np.abs(got[ang, 4] - cols[ang, 4])
    with np.errstate(divide="ignore", invalid="ignore"):
        ar = np.where(bound[ang, 4] > 0, aerr / np.where(bound[ang, 4] > 0, bound[ang, 4], 1), np.where(aerr > 0, np.inf, 0.0))
    print(f"eval_edges pose_metrics.angle [{case}] err {float(np.nanmax(aerr)) if aerr.size else 0.0:.3e} err/bound {float(np.nanmax(ar)) if aerr.size else 0.0:.3f}"
          f" ({int(ang.sum())} of {len(ang)} samples)")
    if not np.all(aerr <= bound[ang, 4]):
        fails.append(f"angle: got {got[:, 4]!r} want {cols[:, 4]!r} bound {bound[:, 4]!r}")
    assert not fails, f"pose_metrics [{case}]: " + "; ".join(fails)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ================================================================================================== A. nn_search
# (id, pn1, pn2, dim, B).  The reference points pass through LDS in tiles of 1024: pn1 = 1023 / 1024 / 1025 end a tile one short, full and
# one over; 2048 / 2049 the second.  256 queries per workgroup: pn2 = 255 / 256 / 257 / 513 leave a lane idle, fill a workgroup, start a
# second and a third with one query.  pn1 = 1 / 2: the tile holds less than a wave.  B = 3 with different clouds: the batch offsets.
NN_CASES = [
    ("n1_q1_d3_b1", 1, 1, 3, 1),
    ("n1_q257_d2_b3", 1, 257, 2, 3),
    ("n2_q255_d3_b3", 2, 255, 3, 3),
    ("n255_q256_d2_b1", 255, 256, 2, 1),
    ("n1023_q257_d3_b3", 1023, 257, 3, 3),
    ("n1024_q513_d2_b3", 1024, 513, 2, 3),
    ("n1024_q1_d3_b1", 1024, 1, 3, 1),
    ("n1025_q256_d3_b3", 1025, 256, 3, 3),
    ("n1025_q255_d2_b1", 1025, 255, 2, 1),
    ("n2048_q257_d3_b1", 2048, 257, 3, 1),
    ("n2048_q255_d2_b3", 2048, 255, 2, 3),
    ("n2049_q513_d3_b3", 2049, 513, 3, 3),
    ("n2049_q1_d2_b3", 2049, 1, 2, 3),
]


def clouds(name, B, n1, n2, dim, seed=0):
    return syn.uniform(name + "ref", (B, n1, dim), seed, -0.1, 0.1), syn.uniform(name + "que", (B, n2, dim), seed, -0.1, 0.1)


@pytest.mark.parametrize("name,n1,n2,dim,B", NN_CASES, ids=_ids(NN_CASES))
def test_nn_search_is_the_serial_loop(ops, name, n1, n2, dim, B):
    ref, que = clouds(name, B, n1, n2, dim)
    got = run_nn(ops, ref, que)
    want = gate_nn(name, got, ref, que)
    if B > 1 and n1 > 2:
        assert not np.array_equal(want[0], want[1])                  # the batch elements do differ: a dropped offset would show
    assert np.array_equal(N(ops.nn_search(D(ref), D(que))), got)      # the front end is the same launch


# (id, pn1, dim): the winners planted on the first and the last slot of every tile.  pn1 = 1030: tiles [0, 1024) and the ragged [1024, 1030);
# pn1 = 2049: a last tile of one slot, 2048, which is its first and its last.
PLANTED = [("n1030_d3", 1030, 3), ("n1030_d2", 1030, 2), ("n2049_d3", 2049, 3), ("n2049_d2", 2049, 2)]


@pytest.mark.parametrize("name,n1,dim", PLANTED, ids=_ids(PLANTED))
def test_nn_search_planted_winners_and_ties_across_a_seam(ops, name, n1, dim):
    B = 3
    ref, que = clouds("planted" + name, B, n1, 40, dim, seed=1)
    # batch 2 only: exact duplicates across the seam (1023, 1024) and one tile apart (5, 1029): the lower index wins
    ref[2, 1024] = ref[2, 1023]
    ref[2, 1029] = ref[2, 5]
    last_tile0 = (n1 - 1) // 1024 * 1024
    winners = [0, 1023, 1024, n1 - 1, last_tile0, 2047 if n1 > 2048 else 1029]
    for b in range(B):
        for k, w in enumerate(winners):                             # a unique nearest point: the query is the point, moved by far less than any spacing
            que[b, k] = ref[b, w] + F32(1e-7) * (b + 1)
    que[:, 10] = ref[:, 1023]
    que[:, 11] = ref[:, 5]
    que[:, 12] = ref[:, 1029]
    got = run_nn(ops, ref, que)
    gate_nn(name, got, ref, que)
    for b in range(B):
        dup = {1024: 1023, 1029: 5} if b == 2 else {}
        assert got[b, 10] == 1023 and got[b, 11] == 5 and got[b, 12] == dup.get(1029, 1029), (b, got[b, 10:13])
        for k, w in enumerate(winners):
            assert got[b, k] == dup.get(w, w), (b, w, got[b, k])


# (id, pn1, pn2, dim, B): p1i == p2i compares GLOBAL indices.  pn1 = 1025 > 1024: the self index 1024 lies in the second tile, where the
# tile-local index is 0; pn1 < pn2: queries beyond pn1 have no self; pn1 > pn2: reference points beyond pn2 are never a self.
SELF_CASES = [("n1025_q1030_d3_b3", 1025, 1030, 3, 3), ("n1025_q257_d2_b3", 1025, 257, 2, 3), ("n255_q513_d3_b3", 255, 513, 3, 3),
              ("n2049_q513_d2_b1", 2049, 513, 2, 1), ("n1_q1_d3_b1", 1, 1, 3, 1), ("n1_q3_d2_b3", 1, 3, 2, 3)]


@pytest.mark.parametrize("name,n1,n2,dim,B", SELF_CASES, ids=_ids(SELF_CASES))
def test_nn_search_exclude_self_on_global_indices(ops, name, n1, n2, dim, B):
    ref, que = clouds("self" + name, B, n1, n2, dim, seed=2)
    n = min(n1, n2)
    que[:, :n] = ref[:, :n]                                          # every query with a self sits ON it: not excluding it shows as the self
    got = run_nn(ops, ref, que, exclude_self=True)
    gate_nn(name, got, ref, que, exclude_self=True)
    if n1 == 1:
        assert not got.any()                                        # a lone point has nobody else: 0, as the reference
    else:
        assert np.all(got[:, :n] != np.arange(n)[None])
    plain = run_nn(ops, ref, que)
    assert np.array_equal(plain[:, :n], np.tile(np.arange(n), (B, 1)))
    assert np.array_equal(N(ops.nn_search(D(ref), D(que), exclude_self=True)), got)


@pytest.mark.parametrize("dim", [3, 2])
def test_nn_search_does_not_contract_the_distance(ops, dim):
    """the planted clouds of eval_ref.contraction_cloud: an fma anywhere in the distance changes more than 10 % of the winners"""
    ref, que = er.contraction_cloud(dim)
    plain = er.nn_idx_serial(ref, que)
    for form in ("fma_all", "fma_last"):                             # the condition on the input, asserted here as well
        assert np.mean(er.nn_idx_contracted(ref, que, form=form) != plain) >= 0.10
    refs, ques = np.stack([ref, ref[::-1].copy()]), np.stack([que, que])
    got = run_nn(ops, refs, ques)
    gate_nn(f"contraction_d{dim}", got, refs, ques)


def test_nn_search_non_finite_input(ops):
    nan, big = F32(NAN), F32(1e19)
    for dim in (3, 2):
        ref, que = clouds("nonfinite", 3, 1030, 300, dim, seed=3)
        # batch 0: NaN queries (whole and one component), NaN and inf reference points, index 0 among them
        ref[0, 0], ref[0, 7, 1], ref[0, 1023], ref[0, 1024, 0] = nan, nan, nan, F32(np.inf)
        que[0, 3], que[0, 9, dim - 1], que[0, 299, 0] = nan, nan, F32(-np.inf)
        # batch 1: every distance overflows
        ref[1], que[1] = (np.abs(ref[1]) + 1) * big, -(np.abs(que[1]) + 1) * big
        # batch 2: one finite candidate, 1027, behind NaN ones (the first tile holds none)
        ref[2] = nan
        ref[2, 1027] = syn.uniform("one", (dim,), 0, -0.1, 0.1)
        que[2, 5] = nan
        got = run_nn(ops, ref, que)
        gate_nn(f"non_finite_d{dim}", got, ref, que)
        assert got[0, 3] == 0 and got[0, 9] == 0 and got[0, 299] == 0          # a NaN / inf query takes nothing
        live = np.delete(np.arange(300), [3, 9, 299])
        assert not np.isin(got[0, live], (0, 7, 1023, 1024)).any()           # NaN / inf reference points are never chosen
        assert not got[1].any()
        assert np.all(np.delete(got[2], 5) == 1027) and got[2, 5] == 0
        ex = run_nn(ops, ref, que, exclude_self=True)
        gate_nn(f"non_finite_self_d{dim}", ex, ref, que, exclude_self=True)
        # a squared distance of EXACTLY FLT_MAX is not below the loop's start value: not taken (a loop that starts from infinity takes it)
        far = er.flt_max_point(dim)
        ref = np.stack([np.full(dim, nan), far, np.full(dim, big * 2), far])[None]
        que = np.zeros((1, 2, dim), F32)
        que[0, 1, 0] = F32(1.0)                                      # from here the same points are at an overflowing / a smaller distance
        assert er._dist_f32(ref[0], que[0])[0, 1] == er.FLT_MAX and er.nn_idx_serial(ref[0], que[0])[0] == 0
        got = run_nn(ops, ref, que)
        gate_nn(f"flt_max_d{dim}", got, ref, que)
        assert got[0, 0] == 0


def test_find_nearest_point_idx_launcher_on_host_pointers(ops):
    lib = lib_of()
    B, n1, n2, dim = 3, 1025, 300, 3
    ref, que = clouds("launcher", B, n1, n2, dim, seed=4)
    que[:, :n2] = ref[:, :n2]
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    for ex in (0, 1):
        r, q = ref.copy(), que.copy()
        idx = np.full(B * n2 + GUARD, SENT_I, np.int32)
        lib.findNearestPointIdxLauncher(hp(r), hp(q), hp(idx), B, n1, n2, dim, ex)
        assert np.all(idx[B * n2:] == SENT_I) and np.array_equal(r, ref) and np.array_equal(q, que)
        got = idx[:B * n2].reshape(B, n2)
        gate_nn(f"launcher_ex{ex}", got, ref, que, bool(ex))
        assert np.array_equal(got, run_nn(ops, ref, que, bool(ex)))
    # an invalid argument: idxs = -1 over its b x pn2 cells, nothing else touched, nothing read
    r4, q4 = syn.uniform("r4", (B, 5, 4), 0), syn.uniform("q4", (B, 6, 4), 0)
    r, q = r4.copy(), q4.copy()
    idx = np.full(B * 6 + GUARD, SENT_I, np.int32)
    lib.findNearestPointIdxLauncher(hp(r), hp(q), hp(idx), B, 5, 6, 4, 0)
    assert np.all(idx[:B * 6] == -1) and np.all(idx[B * 6:] == SENT_I) and np.array_equal(r, r4) and np.array_equal(q, q4)


# ================================================================================================== B. pose_metrics
# (id, P, B).  One workgroup of 256 threads = 4 waves per sample, a thread strides over the points: P = 1 / 63 / 64 / 65 one lane, a wave
# short of full, full, a second wave with one lane; 192 / 193: the fourth wave idle / with one term; 255 / 256 / 257: the stride's first
# wrap; 1025: the fifth round of the stride, and the inner search of ADD-S crosses a tile seam.  B = 70: more workgroups than a handful.
PM_CASES = [("p1_b3", 1, 3), ("p63_b1", 63, 1), ("p64_b3", 64, 3), ("p65_b70", 65, 70), ("p192_b3", 192, 3), ("p193_b1", 193, 1),
            ("p255_b3", 255, 3), ("p256_b1", 256, 1), ("p257_b70", 257, 70), ("p1025_b3", 1025, 3)]
SCALES = (1e-4, 1e-3, 1e-2, 1e-1)            # pose errors from sub-millimetre to decimetre


def pm_case(name, P, B):
    model = syn.uniform("model" + name, (P, 3), 3, -0.08, 0.08)
    pred, gt = er.pose_pair(name, B, SCALES[(P + B) % 4:] + SCALES[:(P + B) % 4], seed=P)
    return model, pred, gt


_REF = {}


def ref_of(key, model, pred, gt, sym):
    """the restatement of a case, computed once and shared (never modified)"""
    if (key, sym) not in _REF:
        _REF[key, sym] = er.pose_metrics_ref(model, pred, gt, K_LM, sym)
    return _REF[key, sym]


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "sym"])
@pytest.mark.parametrize("name,P,B", PM_CASES, ids=_ids(PM_CASES))
def test_pose_metrics_vs_fp64(ops, name, P, B, sym):
    model, pred, gt = pm_case(name, P, B)
    got = run_metrics(ops, model, pred, gt, K_LM, sym)
    gate_metrics(f"{name}_{'sym' if sym else 'plain'}", got, ref_of(name, model, pred, gt, sym))
    if not sym:
        assert np.all(got[:, 1] == -1.0)
    assert np.array_equal(bits(N(ops.pose_metrics(D(model), D(pred), D(gt), D(K_LM), sym))), bits(got))      # the front end is the same launch


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "sym"])
def test_pose_metrics_rows_do_not_depend_on_the_batch(ops, sym):
    model, pred, gt = pm_case("p257_b70", 257, 70)
    full = run_metrics(ops, model, pred, gt, K_LM, sym)
    assert np.array_equal(bits(run_metrics(ops, model, pred, gt, K_LM, sym)), bits(full))           # a second time
    for b in (0, 35, 69):
        alone = run_metrics(ops, model, pred[b:b + 1], gt[b:b + 1], K_LM, sym)
        assert np.array_equal(bits(alone[0]), bits(full[b])), (b, alone, full[b])


def planted_poses():
    """-> pred, gt (4,3,4): [pred == gt axis-aligned, pred == gt with a squared Frobenius norm above 3, an exact half turn about x,
    a pair whose trace lies below -1]"""
    t = np.array([0.01, -0.02, 0.9], F32)
    A = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    half = A * np.array([1, -1, -1], F32)[None]                      # A Rx(180 deg), exactly
    Ra, _ = er.rotation_with_trace("above3")
    Rp, Rg = er.rotation_with_trace("below-1")
    T = lambda R: np.concatenate([R, t[:, None]], 1)
    return np.stack([T(A), T(Ra), T(half), T(Rp)]), np.stack([T(A), T(Ra), T(A), T(Rg)])


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "sym"])
def test_pose_metrics_planted_rotations(ops, sym):
    model = syn.uniform("planted", (65, 3), 6, -0.08, 0.08)
    pred, gt = planted_poses()
    r = er.pose_metrics_ref(model, pred, gt, K_LM, sym)
    # the conditions on the input: the traces are outside [-1, 3] by more than any summation order moves them; the half turn is exact
    assert r["cos_raw"][1] - r["c_bound"][1] > 1.0 and r["cos_raw"][3] + r["c_bound"][3] < -1.0
    assert r["cos_raw"][0] == 1.0 and r["cos_raw"][2] == -1.0 and r["c_bound"][0] == 0.0 and r["c_bound"][2] == 0.0
    got = run_metrics(ops, model, pred, gt, K_LM, sym)
    gate_metrics(f"planted_{'sym' if sym else 'plain'}", got, r)
    for b in (0, 1):                                                 # pred == gt: every distance and the angle exactly 0 (row 1 through the clamp)
        want = [0.0, 0.0 if sym else -1.0, 0.0, 0.0, 0.0]
        assert np.array_equal(bits(got[b]), bits(np.array(want))), (b, got[b])
    assert abs(got[2, 4] - 180.0) <= 6 * er.U * 180.0 and got[2, 3] == 0.0
    assert np.isnan(got[3, 4]) and not np.isnan(got[3, :4]).any()   # a trace below -1: NaN, as the reference


def symmetric_model(n_pairs):
    """invariant under a half turn about z, exactly: (x, y, z) and (-x, -y, z) in fp32"""
    h = syn.uniform("sym_model", (n_pairs, 3), 8, -0.08, 0.08)
    h[:, 0] = np.abs(h[:, 0]) + F32(0.004)                          # no point on the axis: a point and its mirror image are distinct
    return np.concatenate([h, h * np.array([-1, -1, 1], F32)[None]], 0)


def test_pose_metrics_symmetric_cloud_and_direction(ops):
    model = symmetric_model(150)                                     # P = 300
    _, gt = er.pose_pair("symcloud", 3, (0.0,), seed=9)
    pred = gt.copy()
    pred[:, :, :2] = -pred[:, :, :2]                                 # gt Rz(180 deg), exactly
    r = er.pose_metrics_ref(model, pred, gt, K_LM, True)
    got = run_metrics(ops, model, pred, gt, K_LM, True)
    gate_metrics("symmetric_cloud", got, r)
    assert np.all(got[:, 0] > 0.02) and np.all(got[:, 1] < 1e-6)      # ADD at the scale of the model, ADD-S at the scale of fp32 rounding
    # a clustered, asymmetric model: the nearest PREDICTED point of every TARGET point; the swapped direction is another number
    model, pred, gt = er.clustered_case()
    r = er.pose_metrics_ref(model, pred, gt, K_LM, True)
    s = er.pose_metrics_ref(model, pred, gt, K_LM, True, swap_direction=True)
    assert np.all(np.abs(r["cols"][:, 1] - s["cols"][:, 1]) > 1e6 * r["bound"][:, 1])
    gate_metrics("clustered", run_metrics(ops, model, pred, gt, K_LM, True), r)


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "sym"])
def test_pose_metrics_nan_pose_stays_in_its_row(ops, sym):
    model, pred, gt = pm_case("nanrow", 193, 3)
    pred[1] = NAN
    got = run_metrics(ops, model, pred, gt, K_LM, sym)
    want = [True, sym, True, True, True]
    assert np.array_equal(np.isnan(got[1]), want) and (sym or got[1, 1] == -1.0), got[1]
    for b in (0, 2):
        alone = run_metrics(ops, model, pred[b:b + 1], gt[b:b + 1], K_LM, sym)
        assert np.array_equal(bits(alone[0]), bits(got[b])) and not np.isnan(got[b]).any()
    gate_metrics(f"nan_row_{'sym' if sym else 'plain'}", got, er.pose_metrics_ref(model, pred, gt, K_LM, sym))
    gt2 = gt.copy()
    gt2[1, 0, 3] = NAN                                               # one NaN entry of the other pose
    pred2 = pm_case("nanrow", 193, 3)[1]
    gate_metrics(f"nan_entry_{'sym' if sym else 'plain'}", run_metrics(ops, model, pred2, gt2, K_LM, sym), er.pose_metrics_ref(model, pred2, gt2, K_LM, sym))


def test_pose_metrics_points_at_and_behind_the_camera(ops):
    model = syn.uniform("depth", (5, 3), 10, -0.05, 0.05)
    I = np.eye(3, dtype=F32)
    T = lambda t: np.concatenate([I, np.asarray(t, F32)[:, None]], 1)
    m2 = model[2]
    pred = np.stack([T([0.01, 0.0, -m2[2]]),                         # point 2 at depth exactly 0, off the axis: x / 0 = inf
                     T([-m2[0], -m2[1], -m2[2]]),                    # point 2 at the camera centre: 0 / 0 = NaN
                     T([0.01, 0.0, -1.0])])                          # every point behind the camera: finite
    gt = np.stack([T([0.0, 0.0, 1.0])] * 3)
    r = er.pose_metrics_ref(model, pred, gt, K_LM, False)
    assert np.isinf(r["cols"][0, 2]) and np.isnan(r["cols"][1, 2]) and np.isfinite(r["cols"][2, 2])      # the conditions on the input
    got = run_metrics(ops, model, pred, gt, K_LM, False)
    gate_metrics("depth_0_and_behind", got, r)
    assert got[0, 2] == np.inf and np.isnan(got[1, 2]) and np.isfinite(got[:, [0, 3, 4]]).all()


# ================================================================================================== C. refusals
def test_bad_arguments_through_the_c_abi_write_nothing(ops):
    lib = lib_of()
    B, n1, n2 = 2, 5, 6
    ref, que = clouds("bad", B, n1, n2, 3)
    d_ref, d_que = D(ref), D(que)
    idx = torch.full((B * n2,), SENT_I, dtype=torch.int32).cuda()

    def nn(r=d_ref, q=d_que, i=idx, b=B, p1=n1, p2=n2, dim=3):
        rc = lib.rnnpose_nn_search_f32(ptr(r), ptr(q), ptr(i), b, p1, p2, dim, 0, ops._stream())
        torch.cuda.synchronize()
        return rc
    for kw, msg in ((dict(r=None), b"null"), (dict(q=None), b"null"), (dict(i=None), b"null"), (dict(b=0), b"bad size"), (dict(b=65536), b"bad size"),
                    (dict(b=-1), b"bad size"), (dict(p1=0), b"bad size"), (dict(p2=0), b"bad size"), (dict(dim=1), b"bad size"), (dict(dim=4), b"bad size")):
        assert nn(**kw) != 0 and msg in lib.rnnpose_last_error() and b"rnnpose_nn_search_f32" in lib.rnnpose_last_error(), kw
    assert torch.all(idx == SENT_I)                                  # refused before any launch
    assert nn() == 0 and torch.all(idx >= 0)

    P = 9
    model = syn.uniform("badm", (P, 3), 0, -0.05, 0.05)
    pred, gt = er.pose_pair("bad", B, (1e-2,))
    dm, dp, dg, dK = D(model), D(pred), D(gt), D(K_LM)
    n = int(lib.rnnpose_pose_metrics_workspace_bytes(B, P))
    assert n == B * P * 28 and lib.rnnpose_pose_metrics_workspace_bytes(70, 1025) == 70 * 1025 * 28
    for b, p in ((0, P), (-1, P), (B, 0), (B, -3)):
        assert lib.rnnpose_pose_metrics_workspace_bytes(b, p) == 0
    ws = torch.full((n // 4,), SENT, dtype=torch.float32).cuda()
    out = torch.full((B, 5), SENT, dtype=torch.float64).cuda()

    def pm(m=dm, p=P, pp=dp, pg=dg, k=dK, b=B, sym=1, w=ws, nb=n, o=out):
        rc = lib.rnnpose_pose_metrics_f64(ptr(m), p, ptr(pp), ptr(pg), ptr(k), b, sym, ptr(w), nb, ptr(o), ops._stream())
        torch.cuda.synchronize()
        return rc
    for kw, msg in ((dict(m=None), b"null"), (dict(pp=None), b"null"), (dict(pg=None), b"null"), (dict(k=None), b"null"), (dict(o=None), b"null"),
                    (dict(b=0), b"bad size"), (dict(b=65536, nb=1 << 30), b"bad size"), (dict(p=0), b"bad size"), (dict(w=None), b"workspace"),
                    (dict(nb=n - 1), b"workspace"), (dict(sym=0, b=0), b"bad size")):
        assert pm(**kw) != 0 and msg in lib.rnnpose_last_error() and b"rnnpose_pose_metrics_f64" in lib.rnnpose_last_error(), kw
    assert torch.all(out == SENT) and torch.all(ws == SENT)
    assert pm(sym=0, w=None, nb=0) == 0 and torch.all(ws == SENT) and torch.all(out[:, 1] == -1.0)          # not symmetric: no workspace needed
    assert pm() == 0 and torch.all(out != SENT) and torch.all(ws != SENT)


def test_front_end_refuses_mismatched_shapes_before_any_launch(ops, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a mismatched call reached a launch")
    monkeypatch.setattr(ops, "_launch", no_launch)
    z = lambda *s: torch.zeros(*s).cuda()
    for ref, que, word in ((z(2, 5, 3), z(3, 5, 3), "que_pts must be"),       # another batch
                           (z(2, 5, 3), z(2, 5, 2), "que_pts must be"),       # another dim
                           (z(2, 5, 3), z(2, 15), "que_pts must be"),         # not 3-D
                           (z(5, 3), z(5, 3), "ref_pts must be"),
                           (z(2, 5, 4), z(2, 5, 4), "ref_pts must be"),       # dim not in {2, 3}
                           (z(2, 5, 1), z(2, 5, 1), "ref_pts must be"),
                           (z(2, 0, 3), z(2, 5, 3), "ref_pts must be"),       # an empty cloud
                           (z(2, 5, 3), z(2, 0, 3), "que_pts must be"),
                           (z(0, 5, 3), z(0, 5, 3), "ref_pts must be")):
        with pytest.raises(ValueError, match=word):
            ops.nn_search(ref, que)
    m, p, K = z(7, 3), z(2, 3, 4), z(3, 3)
    for args, word in (((m, p, z(3, 3, 4), K), "pose_gt must be"),            # pose_gt differs from pose_pred
                       ((m, p, z(2, 4, 4), K), "pose_gt must be"),
                       ((m, z(2, 4, 4), z(2, 4, 4), K), "pose_pred must be"),  # not (B,3,4)
                       ((m, z(2, 12), z(2, 12), K), "pose_pred must be"),
                       ((m, z(0, 3, 4), z(0, 3, 4), K), "pose_pred must be"),
                       ((z(7, 2), p, p, K), "model must be"),
                       ((z(21), p, p, K), "model must be"),
                       ((z(0, 3), p, p, K), "model must be"),                  # P < 1
                       ((m, p, p, z(2, 3, 3)), "K must be"),
                       ((m, p, p, z(3, 4)), "K must be"),
                       ((m, p, p, z(9)), "K must be")):
        for sym in (False, True):
            with pytest.raises(ValueError, match=word):
                ops.pose_metrics(*args, sym)
    with pytest.raises(AssertionError, match="reached a launch"):      # the stand-in is in place: a well-formed call does get there
        ops.nn_search(z(2, 5, 3), z(2, 6, 3))
    with pytest.raises(AssertionError, match="reached a launch"):
        ops.pose_metrics(m, p, p, K, False)


# ================================================================================================== D. LineMODEvaluator
DIAMETER = 0.01            # thresholds of 1, 0.2 and 0.5 mm: far below the model's point spacing, so ADD-S of a small shift is the shift


def evaluator_case():
    """a model on a jittered grid (spacing >= 10 mm) that a half turn about z maps onto itself exactly (point pairs (x, y, z), (-x, -y, z)
    in fp32), and 14 samples: 0.9 x and 1.1 x of each threshold (ADD 0.1 d, 0.02 d, 0.05 d as shifts along x; 5 px as a shift; 5 cm as a
    shift; 5 degrees as a turn about z), the NaN-angle pair, and a half turn about z with a shift of 0.1 mm: its ADD is the size of
    the model, its ADD-S 0.1 mm, below every distance threshold -- the sample on which a symmetric and a plain class decide differently"""
    g = np.stack(np.meshgrid(np.arange(3) + 0.5, np.arange(6) - 2.5, np.arange(6) - 2.5, indexing="ij"), -1).reshape(-1, 3) * 0.016
    half = (g + syn.uniform("jitter", g.shape, 12, -0.003, 0.003)).astype(F32)
    model = np.concatenate([half, half * np.array([-1, -1, 1], F32)[None]], 0)
    I = np.eye(3)
    t0 = np.array([0.0, 0.0, 1.0])
    fx = float(K_LM[0, 0])
    pred = []
    for f in (0.9, 1.1):
        for thr in (0.1 * DIAMETER, 0.02 * DIAMETER, 0.05 * DIAMETER, 5.0 / fx, 0.05):
            pred.append(np.concatenate([I, (t0 + [f * thr, 0, 0])[:, None]], 1))
        a = np.deg2rad(5.0 * f)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        pred.append(np.concatenate([Rz, t0[:, None]], 1))
    gt = [np.concatenate([I, t0[:, None]], 1)] * (len(pred) + 2)
    Rp, Rg = er.rotation_with_trace("below-1")
    pred.append(np.concatenate([Rp, t0[:, None]], 1))
    gt[12] = np.concatenate([Rg, t0[:, None]], 1)
    pred.append(np.concatenate([np.diag([-1.0, -1.0, 1.0]), (t0 + [1e-4, 0, 0])[:, None]], 1))
    return model, np.stack(pred).astype(F32), np.stack(gt).astype(F32)


@pytest.mark.parametrize("cls", ["cat", "eggbox"])
def test_evaluator_decides_like_the_restatement(ops, cls):
    from rnnpose_amd.evaluator import LineMODEvaluator
    sym = cls == "eggbox"
    model, pred, gt = evaluator_case()
    n = len(pred)
    r = er.pose_metrics_ref(model, pred, gt, K_LM, sym)
    cols = r["cols"]
    want = er.flags(cols, DIAMETER, sym)
    # the conditions on the input: the deciding column of each planted sample sits 10 % (+- 2 %) off its threshold
    dist = cols[:, 1] if sym else cols[:, 0]
    for k, f in enumerate((0.9, 1.1)):
        for j, (val, thr) in enumerate(((dist, 0.1 * DIAMETER), (dist, 0.02 * DIAMETER), (dist, 0.05 * DIAMETER), (cols[:, 2], 5.0), (cols[:, 3], 5.0),
                                        (cols[:, 4], 5.0))):
            assert abs(val[6 * k + j] / thr - f) < 0.02, (cls, f, j, val[6 * k + j], thr)
    assert np.isnan(cols[12, 4]) and not want[12, 4]
    assert want[:, :4].any(0).all() and not want.all(0).any()         # every decision goes both ways in the batch
    # ... and on the half turn the two columns decide differently at every distance threshold: the symmetric class must read column 1
    both = er.pose_metrics_ref(model, pred[13:], gt[13:], K_LM, True)["cols"]
    assert not er.flags(both, DIAMETER, False)[0, :3].any() and er.flags(both, DIAMETER, True)[0, :3].all()
    assert np.array_equal(want[13, :3], [sym] * 3)
    ev = LineMODEvaluator(cls, model, diameter=DIAMETER)
    assert ev.symmetric == sym
    m = N(ev.evaluate(D(pred), D(gt)))                               # (the NaN sample does not raise)
    gate_metrics(f"evaluator_{cls}", m, r)
    keys = ("add", "add2", "add5", "proj2d", "cmd5")
    s = ev.summarize()
    assert s["seq_len"] == n
    assert [s[k] for k in keys] == [float(v) for v in want.mean(0)]
    # the evaluator's own decision for every sample: one sample per evaluator, its means are its flags
    for i in range(n):
        one = LineMODEvaluator(cls, model, diameter=DIAMETER)
        one.evaluate(D(pred[i:i + 1]), D(gt[i:i + 1]))
        si = one.summarize()
        assert si["seq_len"] == 1 and [si[k] for k in keys] == [float(v) for v in want[i]], (cls, i, si, want[i])
    # unique=[...]: masked samples stay out of the means and of seq_len
    mask = np.array([i % 3 != 1 for i in range(n)])
    ev2 = LineMODEvaluator(cls, model, diameter=DIAMETER)
    ev2.evaluate(D(pred), D(gt), unique=list(mask))
    ev2.evaluate(D(pred[:2]), D(gt[:2]), unique=[False, False])
    s2 = ev2.summarize()
    assert s2["seq_len"] == int(mask.sum())
    assert [s2[k] for k in keys] == [float(v) for v in want[mask].mean(0)]
