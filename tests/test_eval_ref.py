"""CPU checks of tests/eval_ref.py, the yardstick of tests/test_gpu_eval_edges.py: the vectorised serial loop against
oracle/eval_oracle.py (finite data) and against the loop written out (non-finite data, exclude_self); pose_metrics_ref against
oracle/eval_oracle.py on the `eval_metric` golden fixture, within the derived bounds; and the conditions the planted inputs of the GPU
tests must meet -- the contraction clouds change their winner under either contracted form in at least 10 % of the queries, the planted
rotations put the trace outside [-1, 3] by far more than a summation order can move it."""
import numpy as np
import pytest

import eval_ref as er
from oracle import eval_oracle as eo
from rnnpose_amd import synthetic as syn

F32 = np.float32


@pytest.mark.parametrize("n1,n2,dim", [(1, 1, 3), (7, 300, 3), (1025, 257, 3), (2049, 130, 2), (300, 300, 2)])
def test_nn_idx_serial_is_the_oracle_on_finite_data(n1, n2, dim):
    ref = syn.uniform("ref", (n1, dim), 11, -0.1, 0.1)
    que = syn.uniform("que", (n2, dim), 11, -0.1, 0.1)
    if n1 > 6:
        ref[6] = ref[2]
        que[0] = ref[2]                          # a tie at distance 0: the first index
    assert np.array_equal(er.nn_idx_serial(ref, que), eo.nn_idx(ref, que))
    if n1 > 6:
        assert er.nn_idx_serial(ref, que)[0] == 2
    assert np.array_equal(er.nn_idx_serial(ref, que, exclude_self=True), eo.nn_idx(ref, que, exclude_self=True))


def _small_clouds():
    big = F32(1e19)
    fm = er.FLT_MAX
    nan = F32("nan")
    inf = F32("inf")
    out = []
    for dim in (2, 3):
        for n1, n2 in ((1, 1), (1, 5), (5, 1), (17, 40), (40, 17), (33, 33)):
            ref = syn.uniform("r", (n1, dim), n1 + 100 * dim, -1, 1)
            que = syn.uniform("q", (n2, dim), n2 + 100 * dim, -1, 1)
            out.append((f"finite_{dim}_{n1}_{n2}", ref, que))
            if n1 >= 17 and n2 >= 17:
                r, q = ref.copy(), que.copy()
                r[12] = r[3]
                q[2] = r[3]
                out.append((f"tie_{dim}_{n1}_{n2}", r, q))
                r, q = ref.copy(), que.copy()
                r[0], r[5, 1], r[16, 0] = nan, nan, inf
                q[1], q[4, 0], q[7] = nan, inf, -inf
                out.append((f"nonfinite_{dim}_{n1}_{n2}", r, q))
                r, q = ref.copy(), que.copy()
                r[:9] = nan                       # one finite candidate behind NaN ones, for a far query
                r[10:] = nan
                out.append((f"one_finite_{dim}_{n1}_{n2}", r, q))
                out.append((f"overflow_{dim}_{n1}_{n2}", (np.abs(ref) + 1) * big, -(np.abs(que) + 1) * big))      # every dx*dx overflows: 0
                r, q = np.zeros_like(ref), np.zeros_like(que)
                r[:, 0] = np.sqrt(fm.astype(np.float64)).astype(F32)                         # squared distances about FLT_MAX itself
                r[3, 0] = np.nextafter(r[3, 0], F32(0))
                r[8, 0] = np.nextafter(r[8, 0], inf)
                out.append((f"near_flt_max_{dim}_{n1}_{n2}", r, q))
                r, q = np.full_like(ref, nan), np.zeros_like(que)
                r[4] = r[11] = er.flt_max_point(dim)                                         # a squared distance of exactly FLT_MAX: not taken
                q[1:, 0] = np.linspace(-3e12, 3e12, n2 - 1).astype(F32)
                out.append((f"exactly_flt_max_{dim}_{n1}_{n2}", r, q))
    return out


SMALL = _small_clouds()


@pytest.mark.parametrize("name,ref,que", SMALL, ids=[c[0] for c in SMALL])
def test_nn_idx_serial_is_the_loop_written_out(name, ref, que):
    for ex in (False, True):
        want = er.nn_idx_loop(ref, que, ex)
        assert np.array_equal(er.nn_idx_serial(ref, que, ex), want), (name, ex)
        if ex:
            n = min(len(ref), len(que))
            assert len(ref) == 1 or name.startswith(("nonfinite", "one_finite", "overflow", "near", "exactly")) or np.all(want[:n] != np.arange(n))
    if name.startswith("overflow"):
        assert not er.nn_idx_serial(ref, que).any()
    if name.startswith("one_finite"):
        assert np.all(er.nn_idx_serial(ref, que) == 9)
        assert np.all(np.delete(er.nn_idx_serial(ref, que, True), 9) == 9) and (len(que) <= 9 or er.nn_idx_serial(ref, que, True)[9] == 0)
    if name.startswith("exactly"):
        with np.errstate(over="ignore"):
            assert er._dist_f32(ref, que)[0, 4] == er.FLT_MAX and er.nn_idx_serial(ref, que)[0] == 0
    if name.startswith("nonfinite"):
        got = er.nn_idx_serial(ref, que)
        assert got[1] == 0 and got[4] == 0 and got[7] == 0 and not np.isin(got[[0, 2, 3, 5, 6]], (0, 5, 16)).any()
        with np.errstate(invalid="ignore"):
            assert eo.nn_idx(ref, que)[2] == 0 and got[2] != 0      # np.argmin picks the NaN at index 0: where the two differ


@pytest.mark.parametrize("dim", [3, 2])
def test_contraction_clouds_are_sensitive(dim):
    ref, que = er.contraction_cloud(dim)
    Q = len(que)
    assert Q == (512 if dim == 3 else 256) and ref.shape == (2 * Q, dim)
    plain = er.nn_idx_serial(ref, que)
    assert np.array_equal(plain % Q, np.arange(Q))                   # each query chooses between its own two candidates
    for form in ("fma_all", "fma_last"):
        flipped = float(np.mean(er.nn_idx_contracted(ref, que, form=form) != plain))
        print(f"eval_ref contraction cloud dim {dim} {form}: winner changes in {flipped:.3f} of {Q} queries")
        assert flipped >= 0.10, (dim, form, flipped)


@pytest.mark.parametrize("pre,sym", [("cat_", False), ("driller_", False), ("sym_eggbox_", True)])
def test_pose_metrics_ref_agrees_with_the_oracle_within_the_bounds(golden, pre, sym):
    g = golden("eval_metric")
    K = g["linemod_K"].astype(F32)
    r = er.pose_metrics_ref(g[pre + "model"], g[pre + "pred"], g[pre + "gt"], K, sym)
    want = eo.pose_metrics(g[pre + "model"], g[pre + "pred"], g[pre + "gt"], K, sym)
    cols, bound = r["cols"], r["bound"]
    for c, name in enumerate(("add", "adds", "proj", "trans")):
        err = np.abs(cols[:, c] - want[:, c])
        ratio = np.max(np.where(bound[:, c] > 0, err / np.where(bound[:, c] > 0, bound[:, c], 1), np.where(err > 0, np.inf, 0)))
        print(f"eval_ref vs oracle [{pre}{name}] err {err.max():.3e} err/bound {ratio:.3f}")
        assert np.all(err <= bound[:, c]), (name, err.max())
    cerr = np.abs(np.cos(np.deg2rad(want[:, 4])) - r["cos"])
    print(f"eval_ref vs oracle [{pre}cos] err {cerr.max():.3e} err/bound {np.max(cerr / r['cos_bound']):.3f}")
    assert np.all(cerr <= r["cos_bound"])
    ang = ~np.isnan(bound[:, 4])
    assert ang.sum() >= 10                                          # the fixture does have angles away from 0
    assert np.all(np.abs(cols[ang, 4] - want[ang, 4]) <= bound[ang, 4])
    assert np.array_equal(er.flags(cols, {"cat_": 0.152633, "driller_": 0.259425, "sym_eggbox_": 0.176364}[pre], sym), g[pre + "flags"])


def test_planted_rotations_meet_their_conditions():
    K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], F32)
    model = syn.uniform("m", (5, 3), 1, -0.05, 0.05)
    for kind in ("above3", "below-1"):
        Rp, Rg = er.rotation_with_trace(kind)
        t = np.array([[0.0], [0.0], [1.0]], F32)
        r = er.pose_metrics_ref(model, np.concatenate([Rp, t], 1)[None], np.concatenate([Rg, t], 1)[None], K, False)
        if kind == "above3":
            assert r["cos_raw"][0] - r["c_bound"][0] > 1.0 and r["cos"][0] == 1.0 and r["cols"][0, 4] == 0.0
        else:
            assert r["cos_raw"][0] + r["c_bound"][0] < -1.0 and np.isnan(r["cols"][0, 4]) and np.isnan(r["bound"][0, 4])
            assert not er.flags(r["cols"], 0.1, False)[0, 4]         # a NaN angle is a miss


def test_swapped_direction_is_another_number():
    """ADD-S is the nearest PREDICTED point of every TARGET point; on a clustered model the other direction is far from it."""
    model, pred, gt = er.clustered_case()
    r = er.pose_metrics_ref(model, pred, gt, er.K_LM, True)
    s = er.pose_metrics_ref(model, pred, gt, er.K_LM, True, swap_direction=True)
    assert np.all(np.abs(r["cols"][:, 1] - s["cols"][:, 1]) > 1e6 * r["bound"][:, 1])
    assert np.array_equal(r["cols"][:, [0, 2, 3, 4]], s["cols"][:, [0, 2, 3, 4]])
