"""The fp64 restatement of the pose confidence (tests/score_ref.py) against its own definitions: the two count identities, every
classification rule on hand-made pixels, and score = 1 for a map compared with itself.  CPU only."""
import numpy as np

import score_ref as sr

D = 32
COL = {k: j for j, k in enumerate(sr.COLUMNS)}


def random_case(seed, h=9, w=11, H=12, W=10, S=2, B=3):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.4, 0.6, (B, h, w)).astype(np.float32)
    empty = rng.random(z.shape) < 0.3
    z[empty] = rng.choice(np.array([-1.0, 0.0, np.nan, np.inf], np.float32), int(empty.sum()))
    a = rng.normal(size=(B, D, h, w)).astype(np.float32)
    g = rng.normal(size=(S, D, H, W)).astype(np.float32)
    d = rng.uniform(0.4, 0.6, (S, H, W)).astype(np.float32)
    holes = rng.random(d.shape) < 0.2
    d[holes] = rng.choice(np.array([0.0, -0.3, np.nan, np.inf], np.float32), int(holes.sum()))
    a[0, 3, 2, 2] = np.nan
    g[1, 7, 5, 5] = np.inf
    window = np.array([[-3, -2], [4, 6], [1, 1]], np.int32)
    return z, a, window, g, d, [0, 1, 0]


def test_count_identities_hold_with_and_without_depth():
    for seed in range(4):
        z, a, window, g, d, src = random_case(seed)
        for depth in (None, d):
            stats, score = sr.pose_score(z, a, window, g, depth, src, 0.03)
            c = lambda k: stats[:, COL[k]]
            assert np.array_equal(c("n_rend"), c("n_out") + c("n_occ") + c("n_cons") + c("n_viol") + c("n_hole"))
            assert np.array_equal(c("n_desc") + c("n_bad"), c("n_cons") + c("n_viol") + c("n_hole"))
            assert (c("n_rend") > 0).all() and (c("n_out") > 0)[:2].all() and np.all((score >= 0) & (score <= 1))
            if depth is None:
                assert not c("n_occ").any() and not c("n_cons").any() and not c("n_viol").any() and np.array_equal(c("n_hole"), c("n_rend") - c("n_out"))
            else:
                assert c("n_occ").sum() > 0 and c("n_viol").sum() > 0 and c("n_hole").sum() > 0 and c("sum_abs_dd").sum() > 0


def one_pixel(z, d, a=None, g=None, window=(0, 0), tol=0.125, with_depth=True, s=0):
    e0 = np.eye(1, D, 5, dtype=np.float32)[0] * 3.0                          # |e0|^2 = 9: its cosine with itself is exactly 1
    a = e0 if a is None else np.asarray(a, np.float32)
    g = e0 if g is None else np.asarray(g, np.float32)
    stats, score = sr.pose_score(np.array([[[z]]], np.float32), a.reshape(1, D, 1, 1), np.array([window], np.int32), g.reshape(1, D, 1, 1),
                                 np.array([[[d]]], np.float32) if with_depth else None, [s], tol)
    return dict(zip(sr.COLUMNS, stats[0])), score[0]


def only(st, *names):
    """exactly the named count columns are 1, every other count 0"""
    counts = [k for k in sr.COLUMNS if k.startswith("n_")]
    return all(st[k] == (1.0 if k in names else 0.0) for k in counts)


def test_every_classification_rule_on_single_pixels():
    for z in (-1.0, 0.0, np.nan, np.inf, -np.inf):                           # not rendered: nothing is counted
        st, sc = one_pixel(z, 0.5)
        assert only(st) and sc == 0.0
    for win in ((1, 0), (-1, 0), (0, 1), (0, -1)):                           # rendered, outside the frame on each side
        st, sc = one_pixel(0.5, 0.5, window=win)
        assert only(st, "n_rend", "n_out") and sc == 0.0
    up, down = np.nextafter(np.float32(0.625), np.float32(np.inf)), np.nextafter(np.float32(0.375), np.float32(0))
    for d, cls in ((0.625, "n_cons"), (up, "n_viol"), (0.375, "n_cons"), (down, "n_occ"), (0.5, "n_cons"), (5.0, "n_viol"), (0.01, "n_occ")):
        st, sc = one_pixel(0.5, d)
        assert only(st, "n_rend", cls, *(() if cls == "n_occ" else ("n_desc",))), (d, st)
        assert st["sum_abs_dd"] == (abs(float(d) - 0.5) if cls == "n_cons" else 0.0)
        assert sc == {"n_cons": 1.0, "n_viol": 0.0, "n_occ": 0.0}[cls]
        assert st["sum_cos"] == (0.0 if cls == "n_occ" else 1.0)
    for d in (0.0, -0.5, np.nan, np.inf):                                    # no valid observation: a hole, compared all the same
        st, sc = one_pixel(0.5, d)
        assert only(st, "n_rend", "n_hole", "n_desc") and sc == 1.0
    st, sc = one_pixel(0.5, 0.5, with_depth=False)
    assert only(st, "n_rend", "n_hole", "n_desc") and sc == 1.0
    st, sc = one_pixel(0.5, 0.5, tol=0.0)                                    # tol = 0: equal depths are consistent
    assert only(st, "n_rend", "n_cons", "n_desc") and sc == 1.0
    st, sc = one_pixel(0.5, np.nextafter(np.float32(0.5), np.float32(1)), tol=0.0)
    assert only(st, "n_rend", "n_viol", "n_desc") and sc == 0.0
    st, sc = one_pixel(0.5, 0.5, s=1)                                        # a frame index outside [0, S): a zero row
    assert only(st) and sc == 0.0


def test_similarity_rules():
    e = np.zeros(D, np.float32)
    for a, g in ((e, None), (None, e), (e, e)):                              # a zero vector: cos 0, and it counts
        st, sc = one_pixel(0.5, 0.5, a=a, g=g)
        assert only(st, "n_rend", "n_cons", "n_desc") and st["sum_cos"] == 0.0 and sc == 0.0
    for bad in (np.nan, np.inf, -np.inf):
        for side in ("a", "g"):
            v = np.ones(D, np.float32)
            v[17] = bad
            st, sc = one_pixel(0.5, 0.5, **{side: v})
            assert only(st, "n_rend", "n_cons", "n_bad") and st["sum_cos"] == 0.0 and sc == 0.0
    rng = np.random.default_rng(0)
    a, g = rng.normal(size=D).astype(np.float32), rng.normal(size=D).astype(np.float32)
    st, _ = one_pixel(0.5, 0.5, a=a, g=g)
    want = float(a.astype(np.float64) @ g.astype(np.float64)) / (np.linalg.norm(a.astype(np.float64)) * np.linalg.norm(g.astype(np.float64)))
    assert abs(st["sum_cos"] - want) < 1e-15
    st, sc = one_pixel(0.5, 0.5, a=a, g=-a)                                  # a negative mean similarity scores 0, not below
    assert abs(st["sum_cos"] + 1.0) < 1e-15 and sc == 0.0
    tiny = np.zeros(D, np.float32)
    tiny[0] = 1e-20                                                          # |a| below the eps: the norm is floored, cos = 1e-20 / 1e-12
    st, _ = one_pixel(0.5, 0.5, a=tiny, g=np.eye(1, D, 0, dtype=np.float32)[0])
    assert abs(st["sum_cos"] - float(np.float32(1e-20)) / 1e-12) < 1e-22


def test_a_map_compared_with_itself_scores_one():
    rng = np.random.default_rng(1)
    H, W = 13, 17
    g = rng.normal(size=(1, D, H, W)).astype(np.float32)
    z = np.full((1, H, W), 0.7, np.float32)
    stats, score = sr.pose_score(z, g, np.zeros((1, 2), np.int32), g, None, [0], 0.015)
    st = dict(zip(sr.COLUMNS, stats[0]))
    assert st["n_rend"] == st["n_hole"] == st["n_desc"] == H * W and st["n_out"] == st["n_bad"] == 0
    assert abs(st["sum_cos"] - H * W) < 1e-12 * H * W and abs(score[0] - 1.0) < 1e-12
    # ... shifted by one pixel it does not, and the column that left the frame is counted as outside
    stats, score = sr.pose_score(z, g, np.array([[1, 0]], np.int32), g, None, [0], 0.015)
    assert stats[0, COL["n_out"]] == H and stats[0, COL["n_desc"]] == H * (W - 1) and score[0] < 0.5
