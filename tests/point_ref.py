"""Test-side fp64 (or exact integer) restatements of the point-cloud kernels of csrc/nhwc_ops.hip, one operation each, written for
tests/test_gpu_point_edges.py from the reference's definitions (thirdparty/kpconv/kpconv_blocks.py, model/descriptor3D.py; cited per
function).  numpy only; they share no code with rnnpose_amd.  Every function takes the SAME fp32 arrays the kernel gets and evaluates
in fp64; next to the value each floating-point one returns `bound`, the per-element error an fp32 evaluation of the same formula may
have (the derivation is in its docstring).  tests/test_point_ref.py checks these against torch's own operators and tests/golden/desc3d.npz.
The radius search and the grid subsampling are restated in tests/desc3d_fp64.py (np_radius, np_grid_subsample)."""
from __future__ import annotations

import numpy as np

SO = 1.01                           # every bound below is first order in u; this factor covers the (1 + u)^L - 1 - L u that is left out (L <= 300)
U = 2.0 ** -24 * SO                 # unit roundoff of fp32, round to nearest
U64 = 2.0 ** -53 * SO


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- row sums (kpconv_blocks.py:366-369: torch.sum(neighb_x, dim=-1)) --------------------------------------------------------------
def row_sum(x):
    """-> (sum, bound): an fp32 sum of c terms in any order is within (c - 1) u sum|x| of the exact one (each of the c - 1 additions
    rounds a partial sum that is at most sum|x|); the gate is c u sum|x|."""
    x = f64(x)
    return x.sum(1), x.shape[1] * U * np.abs(x).sum(1)


# ---- KPConv up to the weight product (kpconv_blocks.py:300-372; linear influence, sum aggregation) ---------------------------------
def kpconv_aggregate(q, s, nb, kp, extent, x):
    """q (n_q, 3), s (n_s, 3), nb (n_q, width) ids (anything outside 0..n_s-1 is the shadow: a point at 1e6 with a zero feature row),
    kp (K, 3), x (n_s, c) -> dict(wf (n_q, K, c), infl (n_q, width, K), count (n_q,), bound (n_q, K, c)).

    wf[q, k, c] = sum_j infl[q, j, k] x[nb[q, j], c] / max(1, #{j : sum_c x[nb[q, j], c] > 0}),  infl = max(0, 1 - |s_j - q - kp_k| / extent).

    bound, for an fp32 evaluation (u = 2^-24), with n = s - q and d = n - kp:
      * each component of n carries u |n_c|, each of d then u |n_c| + u |d_c|, so the distance |d| moves by at most
        u (|n|_1 + |d|_1); the squares, the two sums and the correctly rounded square root add at most 3 u |d| to it;
      * the division by the extent and the subtraction from 1 round once each (both results are at most ~ max(1, |d| / extent)), and
        max(., 0) is 1-Lipschitz:    dinfl <= u ((|n|_1 + |d|_1 + 4 |d|) / extent + 2);
      * the FMA chain over the `width` neighbours: width u sum_j |infl x|; the final division one more u |wf|.
    bound = (sum_j dinfl |x| + (width + 1) u sum_j |infl x|) / count.  Beyond the extent both sides clamp to exactly 0 unless |d| is
    within dinfl of it, which the bound covers as well."""
    q, s, kp, x = f64(q), f64(s), f64(kp), f64(x)
    nb = np.asarray(nb, dtype=np.int64)
    n_s = s.shape[0]
    nb = np.where((nb < 0) | (nb >= n_s), n_s, nb)
    s_ = np.concatenate([s, np.full((1, 3), 1e6)])
    x_ = np.concatenate([x, np.zeros((1, x.shape[1]))])
    n = s_[nb] - q[:, None, :]                                   # (n_q, w, 3)
    d = n[:, :, None, :] - kp[None, None]                        # (n_q, w, K, 3)
    dist = np.sqrt((d ** 2).sum(-1))
    infl = np.maximum(1.0 - dist / extent, 0.0)
    nx = x_[nb]                                                  # (n_q, w, c)
    count = np.maximum(1, (x_.sum(1)[nb] > 0).sum(1))
    wf = np.einsum("qjk,qjc->qkc", infl, nx) / count[:, None, None]
    dinfl = U * ((np.abs(n).sum(-1)[:, :, None] + np.abs(d).sum(-1) + 4 * dist) / extent + 2)
    dinfl = np.where((nb == n_s)[:, :, None], 0.0, dinfl)        # the shadow is skipped: it adds exactly nothing
    width = nb.shape[1]
    bound = (np.einsum("qjk,qjc->qkc", dinfl, np.abs(nx)) + (width + 1) * U * np.einsum("qjk,qjc->qkc", infl, np.abs(nx))) / count[:, None, None]
    return dict(wf=wf, infl=infl, count=count, bound=bound)


def sum_margin(x):
    """|sum x| / sum|x| per row (1 for an all-zero row): the positive-sum decision is the same in fp32 and fp64 when this is 0 exactly
    or far above c u."""
    x = f64(x)
    a = np.abs(x).sum(1)
    return np.where(a > 0, np.abs(x.sum(1)) / np.where(a > 0, a, 1), 1.0)


# ---- dense product (UnaryBlock :505, Conv1d bottle / proj_gnn) ------------------------------------------------------------------------
def linear(a, w, bias=None):
    """-> (a @ w + bias, bound).  One fp32 FMA chain of k terms: k u sum_k |a w|; the bias addition rounds once: u |out|."""
    a, w = f64(a), f64(w)
    y = a @ w
    mag = np.abs(a) @ np.abs(w)
    if bias is not None:
        y = y + f64(bias)
        mag = mag + np.abs(f64(bias))
    return y, (a.shape[1] + 1) * U * mag


# ---- instance norm over all rows (BatchNormBlock = InstanceNorm1d on (1, C, N), kpconv_blocks.py:456-473) ------------------------------
def norm_stats(x, eps=1e-5):
    """-> dict(mean (c,), rstd (c,), var, mean_bound, rstd_rel_bound).  mean, biased variance, rstd = 1 / sqrt(var + fp32(eps)).

    The kernel sums x and x^2 in fp64 and takes var = E[x^2] - mean^2, then stores fp32.
      * mean: n fp64 additions, n u64 mean|x|, and the fp32 store, u |mean|;
      * E[x^2] and mean^2 each carry (n + 2) u64 E[x^2] (sums, product, division), so dvar <= 2 (n + 2) u64 E[x^2]: the cancellation of
        a large mean against a small spread is why the sums are fp64.  rstd moves by dvar / (2 (var + eps)) relative to itself, plus
        the fp32 store u and the fp64 square root and division (2 u64)."""
    x = f64(x)
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    e = float(np.float32(eps))
    rstd = 1.0 / np.sqrt(var + e)
    ex2 = (x ** 2).mean(0)
    mean_bound = n * U64 * np.abs(x).mean(0) + U * np.abs(mean)
    rstd_rel_bound = U + 2 * U64 + (n + 2) * U64 * ex2 / (var + e)
    return dict(mean=mean, rstd=rstd, var=var, mean_bound=mean_bound, rstd_rel_bound=rstd_rel_bound)


def norm_apply(x, mr, res=None, mr_res=None, leaky=True, slope=0.1):
    """-> (out, bound).  y = (x - mean) rstd [+ res, as (res - mean_r) rstd_r when mr_res]; LeakyReLU: y if y > 0 else slope y
    (UnaryBlock :514-519, ResnetBottleneckBlock :686).  mr, mr_res: (c, 2) fp32 (mean, rstd), used as given.
    fp32 without contraction: the subtraction and the product round once each, 2 u |y|; the same for the residual term, 2 u |s|; the
    sum u |y + s|; the slope product u |out|.  LeakyReLU is 1-Lipschitz, so a sign that differs at a value within the bound of 0 stays
    inside it."""
    x, mr = f64(x), f64(mr)
    y = (x - mr[:, 0]) * mr[:, 1]
    b = 2 * U * np.abs(y)
    if res is not None:
        s = f64(res)
        if mr_res is not None:
            mrr = f64(mr_res)
            s = (s - mrr[:, 0]) * mrr[:, 1]
            b = b + 2 * U * np.abs(s)
        b = b + U * np.abs(y + s)
        y = y + s
    if leaky:
        y = np.where(y > 0, y, slope * y)
        b = b + U * np.abs(y)
    return y, b


# ---- max_pool (:88-104) and closest_pool (:73-85): exact ----------------------------------------------------------------------------------
def maxpool(x, idx):
    """max over the rows idx[q, :] of x with a zero shadow row (any id outside 0..n_s-1); a NaN among them comes out, as torch.max gives"""
    x = np.asarray(x)
    n_s = x.shape[0]
    idx = np.asarray(idx, dtype=np.int64)
    idx = np.where((idx < 0) | (idx >= n_s), n_s, idx)
    x_ = np.concatenate([x, np.zeros((1, x.shape[1]), x.dtype)])
    return x_[idx].max(1)                                       # (np.max propagates NaN)


def gather_rows(x, idx):
    x = np.asarray(x)
    n_s = x.shape[0]
    i0 = np.asarray(idx, dtype=np.int64)[:, 0]
    i0 = np.where((i0 < 0) | (i0 >= n_s), n_s, i0)
    return np.concatenate([x, np.zeros((1, x.shape[1]), x.dtype)])[i0]


# ---- F.normalize(p=2, dim=1, eps=1e-12) (model/descriptor3D.py:134-136) ---------------------------------------------------------------
def l2_normalize(x):
    """-> (x / max(|x|_2, fp32(1e-12)), bound).  The kernel's sum of squares is an FMA chain of ceil(c / 64) terms per lane and six
    pairwise wave additions, L = ceil(c / 64) + 6 roundings on a sum of non-negative terms: relative L u, halved by the square root,
    which rounds once itself; the division rounds once:   bound = (L / 2 + 2) u |out|."""
    x = f64(x)
    nrm = np.maximum(np.sqrt((x ** 2).sum(1, keepdims=True)), float(np.float32(1e-12)))
    out = x / nrm
    L = -(-x.shape[1] // 64) + 6
    return out, (L / 2 + 2) * U * np.abs(out)


# ---- voxel keys of grid subsampling (grid_subsampling.cpp:50-56), fp32 as the reference computes them ----------------------------------
def voxel_keys(p, dl):
    """one cloud p (n, 3) fp32 -> (keys int64 (n,), origin fp32 (3,), (nx, ny)): origin = floor(min / dl) dl, i = floor((p - origin) / dl),
    key = ix + nx iy + nx ny iz, every step in fp32"""
    p = np.asarray(p, dtype=np.float32)
    dl = np.float32(dl)
    inv = np.float32(1) / dl
    origin = np.floor(p.min(0) * inv).astype(np.float32) * dl
    ijk = np.floor((p - origin) / dl).astype(np.int64)
    nxy = np.floor((p.max(0) - origin) / dl).astype(np.int64) + 1
    return ijk[:, 0] + nxy[0] * ijk[:, 1] + nxy[0] * nxy[1] * ijk[:, 2], origin, (int(nxy[0]), int(nxy[1]))
