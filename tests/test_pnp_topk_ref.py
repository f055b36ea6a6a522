"""The fp64 restatement of the top-K distinct RANSAC hypotheses (tests/pnp_topk_ref.py) tested on its own, on the CPU."""
import numpy as np
import pytest

import pnp_ref as pr
import pnp_topk_ref as tr

TAU = 4.0


@pytest.fixture(scope="module")
def planted():
    """Two-mode data (45 % wrong pose A, 35 % true pose B, 20 % random; 0.5 px noise), 57 and 300 correspondences, 256 hypotheses."""
    case = tr.two_mode_case([57, 300], 256, seed=1)
    X, x, counts, K, rnd = case[:5]
    hyps = [tr.hypotheses(X[b], x[b], counts[b], K[b].astype(np.float64), rnd[b], TAU) for b in range(2)]
    return case, hyps


def rot(axis, deg):
    return pr.se3_exp(np.concatenate([np.zeros(3), np.deg2rad(deg) * np.asarray(axis, np.float64)]))[0]


def test_distance_is_a_metric_on_the_box():
    rng = np.random.default_rng(0)
    lo, hi = np.array([-0.1, -0.05, -0.02]), np.array([0.1, 0.08, 0.03])
    P, Q = tr.pose_matrix(rot([0, 0, 1], 30), rng.normal(size=3)), tr.pose_matrix(rot([1, 0, 0], -50), rng.normal(size=3))
    assert tr.distance(P, P, lo, hi) == 0.0 and tr.distance(P, Q, lo, hi) == tr.distance(Q, P, lo, hi) > 0.0
    # a pure translation moves every corner alike; a rotation about z by a moves the farthest corner (in x, y) by 2 r sin(a / 2)
    S = P.copy()
    S[:3, 3] += [0.003, -0.004, 0.0]
    assert abs(tr.distance(P, S, lo, hi) - 0.005) < 1e-15
    I, Rz = np.eye(4), tr.pose_matrix(rot([0, 0, 1], 20), np.zeros(3))
    assert abs(tr.distance(I, Rz, lo, hi) - 2 * np.hypot(0.1, 0.08) * np.sin(np.deg2rad(10))) < 1e-15
    N = P.copy()
    N[0, 3] = np.nan
    assert np.isnan(tr.distance(P, N, lo, hi))
    assert tr.corners(lo, hi).shape == (8, 3) and len({tuple(c) for c in tr.corners(lo, hi)}) == 8
    lo0, hi0, d0 = tr.extent(np.zeros((5, 3)), 0)
    assert np.isinf(d0) and tr.extent(np.ones((5, 3)), 5)[2] == 0.0


def test_hypotheses_and_slot_0_are_pnp_ref_ransac(planted):
    case, hyps = planted
    X, x, counts, K, rnd = case[:5]
    ref = pr.ransac(X, x, counts, K.astype(np.float64), rnd, TAU, 4)
    for b in range(2):
        assert np.array_equal(hyps[b][0], ref[b]["cost"]) and np.array_equal(hyps[b][1], ref[b]["inliers"])
        for Kt in (1, 4):
            r = tr.topk_object(X[b], x[b], counts[b], K[b].astype(np.float64), rnd[b], TAU, 4, 4, Kt, 0.25, hyps=hyps[b])
            assert r["hyp"][0] == ref[b]["best"] and r["info"][0] == ref[b]["info"] == 0 and r["dup_of"][0] == -1
            assert np.array_equal(r["T"][0], ref[b]["T"]) and np.array_equal(r["inlier_mask"][0], ref[b]["inlier_mask"])
            assert r["n_inliers"][0] == ref[b]["n_inliers"] and r["final_cost"][0] == ref[b]["final_cost"]


def test_two_planted_modes_fill_slots_0_and_1(planted):
    case, hyps = planted
    X, x, counts, K, rnd, Ta, Tb = case[:7]
    for b in range(2):
        r = tr.topk_object(X[b], x[b], counts[b], K[b].astype(np.float64), rnd[b], TAU, 4, 4, 4, 0.25, hyps=hyps[b])
        assert r["n_found"] == 4 and r["info"][:2].tolist() == [0, 0]
        dA, dB = tr.distance(r["T"][0], Ta[b], r["lo"], r["hi"]) / r["diag"], tr.distance(r["T"][1], Tb[b], r["lo"], r["hi"]) / r["diag"]
        assert dA < 0.1 and dB < 0.1, (dA, dB)               # slot 0 = the wrong mode (more support), slot 1 = the truth
        chosen = [h for h in r["hyp"] if h >= 0]
        for i, h in enumerate(chosen):                        # the rule itself: pairwise distinct, costs ascending
            for g in chosen[:i]:
                assert tr.distance(r["poses"][h], r["poses"][g], r["lo"], r["hi"]) > r["sep"] and (r["cost"][g], g) < (r["cost"][h], h)
        # ... and nothing cheaper was passed over: every cheaper hypothesis lies within sep of an earlier slot
        for i, h in enumerate(chosen[1:], 1):
            cheaper = [g for g in range(len(r["cost"])) if (r["cost"][g], g) < (r["cost"][h], h) and g not in chosen[:i] and r["poses"][g] is not None]
            assert all(any(not tr.distance(r["poses"][g], r["poses"][j], r["lo"], r["hi"]) > r["sep"] for j in chosen[:i]) for g in cheaper)


def test_fewer_distinct_hypotheses_than_slots_and_the_gates(planted):
    case, hyps = planted
    X, x, counts, K, rnd = case[:5]
    b, Kd = 1, case[3][1].astype(np.float64)
    run = lambda **kw: tr.topk_object(X[b], x[b], counts[b], Kd, rnd[b], TAU, 4, 4, hyps=hyps[b], **dict(dict(Kt=16, sep_frac=0.25), **kw))
    r = run(sep_frac=1e6)
    assert r["n_found"] == 1 and r["hyp"].tolist() == [r["hyp"][0]] + [-1] * 15 and r["info"][1:].tolist() == [-1] * 15
    free = run(Kt=4)
    first, second = hyps[b][1][free["hyp"][0]], hyps[b][1][free["hyp"][1]]
    assert second < first
    r = run(Kt=4, min_inliers=int(second) + 1)
    assert all(hyps[b][1][h] > second for h in r["hyp"][1:] if h >= 0) and r["hyp"][0] == free["hyp"][0]
    r = run(Kt=4, min_inliers=10 ** 6)                       # the gate does not apply to slot 0
    assert r["n_found"] == 1 and r["hyp"][0] == free["hyp"][0] and r["info"][0] == 0
    # exact ties go to the lowest h: the same triples twice
    rnd2 = np.repeat(rnd[b][:8], 2, axis=0)
    r = tr.topk_object(X[b], x[b], counts[b], Kd, rnd2, TAU, 4, 4, 16, 0.0)
    kept = [h for h in r["hyp"] if h >= 0]
    assert all(h % 2 == 0 for h in kept) and len(kept) == np.isfinite(r["cost"][::2]).sum()
    # too few correspondences: nothing
    r = tr.topk_object(X[b], x[b], 3, Kd, rnd[b], TAU, 4, 4, 4, 0.25)
    assert r["n_found"] == 0 and r["hyp"].tolist() == [-1] * 4 and r["info"].tolist() == [-1] * 4


def test_dup_of_on_two_starts_of_one_mode():
    X, x, rnd, poses = pr.p3p_scenes(n_scenes=1, n_triples=32)
    K = pr.P3P_K
    r = tr.topk_object(X[0], x[0], 64, K, rnd[0], 8.0, 4, 4, 3, 1e-9)
    assert r["n_found"] == 3 and r["info"].tolist() == [0, 0, 0] and r["dup_of"].tolist() == [-1, 0, 0]
    assert all(np.abs(T - poses[0]).max() < 1e-4 for T in r["T"])
    far = tr.topk_object(X[0], x[0], 64, K, rnd[0], 8.0, 0, 4, 3, 1e-9)          # without a polish the starts stay apart
    assert far["dup_of"].tolist() == [-1, -1, -1]
