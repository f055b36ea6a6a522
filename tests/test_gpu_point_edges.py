"""The KPConv half of csrc/nhwc_ops.hip -- row_sum, kpconv_aggregate<1|2|4>, point_linear<16|64>, norm_partial / norm_final / norm_apply,
point_maxpool, point_gather, radius<0|1>, l2_rows, grid_keys: the kernels behind KPSuperpoint3Dv2 and its input pyramid -- against fp64
at their edges (run with -m gpu on an MI355X; every case whose test name does not contain `full_size` also runs on the host-executed
kernels, tests/test_kernels_on_host.py).

tests/test_gpu_desc3d.py meets these kernels through two whole networks and at one shape each.  Here every shape is in a table with the
code path it is there for.  References are the plain fp64 / exact-integer restatements of tests/point_ref.py and the numpy pyramid of
tests/desc3d_fp64.py (checked on the CPU by tests/test_point_ref.py); they get the same fp32 arrays as the kernel.

Gates.  Selection and integer kernels -- max-pool, gather, radius search, voxel keys and grid subsampling -- and every "same result by
another route" statement (strided == contiguous, in place == out of place, 64-row tile == 16-row tile, negative id == shadow) are exact.
The floating-point kernels are held to the error an fp32 evaluation of the same formula can have, derived per operation in
tests/point_ref.py (an FMA chain of L terms: L 2^-24 sum|terms|; KPConv adds the influence's own error from the fp32 coordinate
differences divided by the extent; the norm statistics are fp64 sums whose cancellation term is (n + 2) 2^-53 E[x^2] / (var + eps)).
No gate is taken from a kernel's output.  Each case prints its largest error and the largest error / bound ratio
(profiles/point_edges_mutation.txt keeps them).  Destinations are pre-filled (NaN, or 7 where NaN is a legitimate value) and sources that
are channel slices lie between NaN columns: every cell of the window must be written, none beyond, and nothing outside a source window
may be read."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import desc3d_fp64 as R
import point_ref as pr
from test_gpu_parity import ops  # noqa: F401  (the module-scoped build fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
SENT = 7.0
_ids = lambda cases: [c[0] for c in cases]


def D(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    return t if dt is None else t.to(dt)


def N(t):
    return t.detach().cpu().numpy()


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def src_slice(x, left=3, right=5):
    """x (n, c) as a channel slice of a wider buffer whose other columns are NaN"""
    n, c = x.shape
    buf = torch.full((n, c + left + right), NAN, device="cuda")
    buf[:, left:left + c] = D(x)
    return buf[:, left:left + c]


def dst_slice(n, c, fill=NAN, left=2, right=6):
    buf = torch.full((n, c + left + right), fill, device="cuda")
    return buf, buf[:, left:left + c]


def pads_untouched(buf, c, fill=NAN, left=2):
    pad = torch.cat([buf[:, :left], buf[:, left + c:]], 1)
    return bool(torch.isnan(pad).all()) if fill != fill else bool((pad == fill).all())


def gate(kernel, case, got, ref, bound):
    """|got - ref| <= bound at every element (a NaN fails); prints the largest error and the largest error / bound"""
    g = N(got).astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref, bound = np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(ref))
    assert g.shape == ref.shape, f"{kernel} [{case}]: shape {g.shape} vs {ref.shape}"
    err = np.abs(g - ref)
    bad = ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    print(f"point_edges {kernel} [{case}] err {float(np.nanmax(err)) if err.size else 0.0:.3e} err/bound {float(np.nanmax(ratio)) if err.size else 0.0:.3f}")
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{kernel} [{case}]: {int(bad.sum())}/{bad.size} elements beyond the bound; first at {i}: got {g[i]!r} want {ref[i]!r} "
                             f"bound {bound[i]:.3e}")


# ================================================================================================== 1. row sums
# (id, n, c, strided).  One wave per row, four rows per workgroup: n = 7 leaves one wave of the second workgroup without a row.
ROW_SUM = [("c1", 7, 1, False), ("c63_slice", 7, 63, True), ("c64", 5, 64, False), ("c65_slice", 7, 65, True), ("c256", 7, 256, False),
           ("n1_c65", 1, 65, False)]


@pytest.mark.parametrize("name,n,c,strided", ROW_SUM, ids=_ids(ROW_SUM))
def test_row_sum_vs_fp64(ops, name, n, c, strided):
    x = rng_of("rs" + name).normal(0.2, 1.0, (n, c)).astype(F32)
    buf = torch.full((n + 8,), NAN, device="cuda")
    got = ops.point_row_sum(src_slice(x) if strided else D(x), out=buf[:n])
    assert torch.isnan(buf[n:]).all(), "row_sum wrote beyond its n outputs"
    ref, bound = pr.row_sum(x)
    gate("row_sum", name, got, ref, bound)


# ================================================================================================== 2. KPConv aggregation
# (id, width, K, c_in, n_q).  64 neighbours per chunk: widths 65, 128, 130 take a second / third chunk, 63 and 130 a partial one.
# c_in <= 64 / <= 128 / else selects 1 / 2 / 4 channels per lane: 63, 65, 129, 200 leave the last slot partly masked.  K = 16 = KP_MAX.
# Four queries per workgroup: n_q = 1, 3 leave waves of the only workgroup inactive, n_q = 5 those of the second.
KPCONV = [
    ("w1_k1_c1_q1", 1, 1, 1, 1),
    ("w63_k15_c63_q3", 63, 15, 63, 3),
    ("w64_k16_c64_q5", 64, 16, 64, 5),
    ("w65_k15_c65_q1", 65, 15, 65, 1),
    ("w128_k15_c128_q3", 128, 15, 128, 3),
    ("w130_k16_c129_q5", 130, 16, 129, 5),
    ("w130_k15_c200_q3", 130, 15, 200, 3),
    ("w130_k16_c256_q5", 130, 16, 256, 5),
    ("w65_k1_c256_q1", 65, 1, 256, 1),
    ("w130_k15_c1_q5", 130, 15, 1, 5),
    ("w64_k1_c129_q3", 64, 1, 129, 3),
    ("w1_k16_c200_q5", 1, 16, 200, 5),
    ("w128_k16_c63_q1", 128, 16, 63, 1),
    ("w63_k1_c128_q5", 63, 1, 128, 5),
]
KP_NS, KP_EXTENT = 48, 0.125
FAR, ZERO_SUM, NEG_SUM = range(1, 4), range(4, 10), range(10, 16)       # support rows by role; row 0 coincides with a kernel point of query 2


def kpconv_case(name, width, K, c_in, n_q):
    """Supports: row 0 sits exactly on kernel point K-1 of query 2 (dyadic coordinates: the differences are exact, influence 1);
    rows 1-3 lie 5 units away (influence exactly 0); rows 4-9 have features that sum to exactly 0 in any order (multiples of 1/4 and
    their negatives); rows 10-15 sum to a negative number; the rest to a positive one.
    Neighbour rows by query: 0: duplicates, the shadow in the first, a middle and the last column; 1: all shadow; 2: support 0 only;
    3: only far, zero-sum and negative-sum supports (count 0 -> divisor 1); 4: all real, no shadow."""
    rng = rng_of("kp" + name)
    kp = (rng.integers(-5, 6, (K, 3)) / 64.0).astype(F32)
    kp[0] = 0
    s = rng.uniform(-0.15, 0.15, (KP_NS, 3)).astype(F32)
    s[1:4] += 5.0
    q = (s[20:20 + n_q] + rng.normal(0, 0.01, (n_q, 3))).astype(F32)
    x = rng.normal(0.5, 1.0, (KP_NS, c_in)).astype(F32)
    h = c_in // 2
    for r in ZERO_SUM:
        v = rng.integers(1, 9, h) / 4.0
        x[r] = 0
        x[r, :h], x[r, h:2 * h] = v, -v
    x[10:16] = -np.abs(x[10:16]) - 0.01
    x[1:4] = -np.abs(x[1:4]) - 0.01                             # (the far rows too: query 3 then has no positive-sum neighbour at all)
    x[0] = np.abs(x[0]) + 0.1
    for r in range(16, KP_NS):
        while abs(float(x[r].astype(np.float64).sum())) < 1e-2 * float(np.abs(x[r]).sum()):
            x[r, 0] += 1.0
    nb = np.full((n_q, width), KP_NS, np.int64)
    for i in range(n_q):
        if i == 0:
            nb[i] = rng.integers(0, KP_NS, width)
            if width >= 5:
                nb[i, 2] = nb[i, 3] = nb[i, 1]
                nb[i, 0] = nb[i, width // 2] = nb[i, width - 1] = KP_NS
        elif i == 2:
            q[i] = rng.integers(-8, 9, 3) / 64.0
            s[0] = q[i] + kp[K - 1]
            nb[i, 0] = 0
        elif i == 3:
            nb[i] = rng.integers(1, 16, width)
        elif i == 4:
            nb[i] = rng.integers(0, KP_NS, width)
    return q, s, nb, kp, x


@pytest.mark.parametrize("name,width,K,c_in,n_q", KPCONV, ids=_ids(KPCONV))
def test_kpconv_aggregate_vs_fp64(ops, name, width, K, c_in, n_q):
    q, s, nb, kp, x = kpconv_case(name, width, K, c_in, n_q)
    # a condition on the inputs: every row sum is exactly 0 or at least 1e-3 sum|x| away from it, so fp32 and fp64 count alike
    sums, margin = x.astype(np.float64).sum(1), pr.sum_margin(x)
    assert all(sums[r] == 0 for r in ZERO_SUM) and all(sums[r] < 0 for r in NEG_SUM) and ((sums == 0) | (margin >= 1e-3)).all()
    ref = pr.kpconv_aggregate(q, s, nb, kp, KP_EXTENT, x)
    t = ops.neighbor_table(D(nb), KP_NS)
    n_out = n_q * K * c_in
    buf = torch.full((n_out + 64,), NAN, device="cuda")
    wf = ops.kpconv_aggregate(D(q), D(s), t, D(kp), KP_EXTENT, D(x), out=buf[:n_out].view(n_q, K * c_in))
    assert torch.isnan(buf[n_out:]).all(), "kpconv_aggregate wrote beyond its (n_q, K c_in) output"
    gate("kpconv_aggregate", name, wf.view(n_q, K, c_in), ref["wf"], ref["bound"])
    got = N(wf).reshape(n_q, K, c_in)
    if n_q > 1:
        assert not got[1].any(), "an all-shadow row must give exactly zero"
    if n_q > 2:                                                 # influence exactly 1, count 1: the features themselves
        assert ref["infl"][2, 0, K - 1] == 1.0 and ref["count"][2] == 1 and np.array_equal(got[2, K - 1], x[0])
    if n_q > 3:                                                 # no positive-sum neighbour: the divisor clamps to 1, far supports add exactly 0
        far = np.isin(nb[3], list(FAR))
        assert ref["count"][3] == 1 and not ref["infl"][3][far].any()
    # a channel slice of a wider buffer as the source: bit for bit
    wf2 = ops.kpconv_aggregate(D(q), D(s), t, D(kp), KP_EXTENT, src_slice(x))
    assert torch.equal(wf, wf2)


def test_kpconv_negative_ids_are_refused_in_python_and_are_the_shadow_in_the_kernel(ops):
    from rnnpose_amd import _lib
    name, width, K, c_in, n_q = KPCONV[5]
    q, s, nb, kp, x = kpconv_case(name, width, K, c_in, n_q)
    with pytest.raises(ValueError, match="shadow"):
        ops.neighbor_table(D(np.where(nb == KP_NS, -1, nb)), KP_NS)
    dq, ds, dk, dx = D(q), D(s), D(kp), D(x)
    want = ops.kpconv_aggregate(dq, ds, ops.neighbor_table(D(nb), KP_NS), dk, KP_EXTENT, dx)
    rs = ops.point_row_sum(dx)
    lib = _lib.load()
    for neg in (-1, -2 ** 31):
        t = D(np.where(nb == KP_NS, neg, nb).astype(np.int32))
        out = torch.full_like(want, NAN)
        rc = lib.rnnpose_kpconv_aggregate_f32(ops._ptr(dq), n_q, ops._ptr(ds), KP_NS, ops._ptr(t), width, ops._ptr(dk), K, KP_EXTENT, ops._ptr(dx),
                                              c_in, c_in, ops._ptr(rs), ops._ptr(out), ops._stream())
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(out, want), neg


# ================================================================================================== 3. dense product
# (id, n, k, m, bias).  16 x 64 tiles (n < 16384), K in steps of 16: k = 15, 17, 40 leave a K tail, m = 1, 63, 65, 130 an M tail over one
# to three column tiles, n = 1, 15, 17 a row tail.  a and out are channel slices: lda > k, ldo > m.
LINEAR = [("n1_k1_m1", 1, 1, 1, False), ("n15_k15_m63_bias", 15, 15, 63, True), ("n16_k16_m64", 16, 16, 64, False),
          ("n17_k17_m65_bias", 17, 17, 65, True), ("n17_k40_m130_bias", 17, 40, 130, True), ("n16_k17_m1_bias", 16, 17, 1, True),
          ("n1_k40_m130", 1, 40, 130, False), ("n15_k1_m65_bias", 15, 1, 65, True)]


def _linear_inputs(name, n, k, m, bias):
    rng = rng_of("lin" + name)
    a = rng.normal(0, 1, (n, k)).astype(F32)
    w = rng.normal(0, 0.3, (k, m)).astype(F32)
    b = rng.uniform(-0.5, 0.5, m).astype(F32) if bias else None
    return a, w, b


@pytest.mark.parametrize("name,n,k,m,bias", LINEAR, ids=_ids(LINEAR))
def test_point_linear_vs_fp64(ops, name, n, k, m, bias):
    a, w, b = _linear_inputs(name, n, k, m, bias)
    buf, out = dst_slice(n, m)
    got = ops.point_linear(src_slice(a), D(w), None if b is None else D(b), out=out)
    assert pads_untouched(buf, m), "point_linear wrote outside its channel slice"
    ref, bound = pr.linear(a, w, b)
    gate("point_linear", name, got, ref, bound)


def test_point_linear_tile_height_independence(ops):
    """n = 16384 rows take the 64-row tile, the same rows in two calls of 8192 the 16-row tile: one FMA chain per output either way, so the
    results are bit-identical (K tail 40 = 2 x 16 + 8, M tail 70 = 64 + 6, lda > k, ldo > m, bias)."""
    n, k, m = 16384, 40, 70
    a, w, b = _linear_inputs("bm", n, k, m, True)
    da, dw, db = src_slice(a), D(w), D(b)
    buf, out = dst_slice(n, m)
    ops.point_linear(da, dw, db, out=out)
    assert pads_untouched(buf, m)
    buf2, out2 = dst_slice(n, m)
    ops.point_linear(da[:n // 2], dw, db, out=out2[:n // 2])
    ops.point_linear(da[n // 2:], dw, db, out=out2[n // 2:])
    assert pads_untouched(buf2, m) and torch.equal(out, out2)
    ref, bound = pr.linear(a, w, b)
    gate("point_linear", "bm64_n16384_k40_m70", out, ref, bound)


# ================================================================================================== 4. instance norm
# (id, n, c, strided).  512 rows per chunk, four row phases, 64 channels per workgroup; the final kernel 256 channels per workgroup.
# Column 0 has mean 1e3 and std 1e-2 (E[x^2] - mean^2 cancels ten digits: the reason the sums are fp64); column 1 is the constant 1.0 and
# column 2 the constant 1e10 (variance 0; the clamp fmax(var, 0) applies where the fp64 sum of squares rounds).
NORM = [("n1_c1", 1, 1, False), ("n2_c63_slice", 2, 63, True), ("n511_c64", 511, 64, False), ("n512_c65_slice", 512, 65, True),
        ("n513_c130", 513, 130, False), ("n1025_c5_slice", 1025, 5, True), ("n513_c1", 513, 1, False), ("n1_c130_slice", 1, 130, True)]


def _norm_inputs(name, n, c):
    rng = rng_of("norm" + name)
    x = rng.normal(0.3, 1.5, (n, c)).astype(F32)
    x[:, 0] = (1e3 + 1e-2 * rng.normal(0, 1, n)).astype(F32)
    if c > 1:
        x[:, 1] = 1.0
    if c > 2:
        x[:, 2] = 1e10
    return x


@pytest.mark.parametrize("name,n,c,strided", NORM, ids=_ids(NORM))
def test_point_norm_stats_vs_fp64(ops, name, n, c, strided):
    x = _norm_inputs(name, n, c)
    dx = src_slice(x) if strided else D(x)
    mr = ops.point_norm_stats(dx, 1e-5)
    assert tuple(mr.shape) == (c, 2) and torch.isfinite(mr).all() and (mr[:, 1] > 0).all()
    st = pr.norm_stats(x, 1e-5)
    got = N(mr).astype(np.float64)
    gate("norm_stats.mean", name, got[:, 0], st["mean"], st["mean_bound"])
    # the sum of squares of 1e10 is not exact in fp64 beyond 94 rows per phase: the derived bound says so, and only the output (below) is held
    derived = np.ones(c, bool)
    derived[2:3] = n == 1
    gate("norm_stats.rstd_rel", name, got[derived, 1] / st["rstd"][derived], np.ones(int(derived.sum())), st["rstd_rel_bound"][derived])
    assert (got[:, 1] <= (1 + 2 * pr.U) / np.sqrt(float(F32(1e-5)))).all()               # never above 1 / sqrt(eps)
    const = [j for j in range(c) if n == 1 or j in (1, 2)]
    assert all(st["var"][j] == 0 for j in const)
    for leaky in (False, True):
        buf, out = dst_slice(n, c)
        ops.point_norm_apply(dx, mr, leaky=leaky, out=out)
        assert pads_untouched(buf, c) and not torch.isnan(out).any()
        assert not N(out)[:, const].any(), "a constant column must come out exactly 0"
        ref, bound = pr.norm_apply(x, N(mr), leaky=leaky)
        gate("norm_apply.own_stats", f"{name}-leaky{int(leaky)}", out, ref, bound)


# (id, res, res_mean_rstd, leaky)
APPLY = [("plain", False, False, False), ("leaky", False, False, True), ("res", True, False, False), ("res_leaky", True, False, True),
         ("res_norm", True, True, False), ("res_norm_leaky", True, True, True)]


def _apply_inputs(name, n=37, c=65):
    rng = rng_of("apply" + name)
    x, r = rng.normal(0.3, 1.5, (n, c)).astype(F32), rng.normal(-0.2, 2.0, (n, c)).astype(F32)
    mr = np.stack([rng.normal(0.3, 0.5, c), rng.uniform(0.5, 2.0, c)], 1).astype(F32)
    mrr = np.stack([rng.normal(-0.2, 0.5, c), rng.uniform(0.5, 2.0, c)], 1).astype(F32)
    mr[3, 1] = -1.5                                               # (x - mean) = +0 times a negative factor: -0
    x[5], x[6] = mr[:, 0], mr[:, 0]                               # rows that land exactly on zero
    return x, r, mr, mrr


@pytest.mark.parametrize("name,res,res_mr,leaky", APPLY, ids=_ids(APPLY))
def test_point_norm_apply_variants_vs_fp64(ops, name, res, res_mr, leaky):
    x, r, mr, mrr = _apply_inputs(name)
    if res:
        r[5] = r[6] = mrr[:, 0] if res_mr else 0.0
    n, c = x.shape
    kw = dict(leaky=leaky, res=src_slice(r) if res else None, res_mean_rstd=D(mrr) if res_mr else None)
    buf, out = dst_slice(n, c)
    ops.point_norm_apply(src_slice(x), D(mr), out=out, **kw)
    assert pads_untouched(buf, c), "norm_apply wrote outside its channel slice"
    ref, bound = pr.norm_apply(x, mr, r if res else None, mrr if res_mr else None, leaky=leaky)
    gate("norm_apply", name, out, ref, bound)
    assert not N(out)[5:7].any() and not ref[5:7].any(), "(x - mean) = 0 [+ 0] must give exactly 0 (either sign)"
    # in place, as the network calls it (out = y): bit-identical, on a contiguous x and on a channel slice
    plain = ops.point_norm_apply(D(x), D(mr), **kw)
    assert torch.equal(plain, out)
    xi = D(x).clone()
    assert ops.point_norm_apply(xi, D(mr), out=xi, **kw) is xi and torch.equal(xi, plain)
    xs = src_slice(x)
    ops.point_norm_apply(xs, D(mr), out=xs, **kw)
    assert torch.equal(xs, plain)
    if res:                                                       # and with out = res
        rs = D(r).clone()
        ops.point_norm_apply(D(x), D(mr), out=rs, **dict(kw, res=rs))
        assert torch.equal(rs, plain)


# ================================================================================================== 5. max-pool and gather (exact)
# (id, c, width).  All features negative: the zero shadow row wins where, and only where, a shadow entry is present.
POOL = [("c1_w1", 1, 1), ("c65_w1", 65, 1), ("c1_w6", 1, 6), ("c65_w6", 65, 6), ("c300_w3", 300, 3)]
POOL_NS = 20


def _pool_inputs(name, c, width, with_nan=False):
    rng = rng_of("pool" + name)
    x = (-np.abs(rng.normal(0, 1, (POOL_NS, c))) - 0.1).astype(F32)
    idx = rng.integers(0, POOL_NS, (9, width))
    idx[1, 0] = POOL_NS                                           # the shadow in column 0
    idx[2] = POOL_NS                                              # all shadow
    idx[3, width - 1] = POOL_NS                                   # the shadow in the last column
    if with_nan:
        x[7, c // 2] = NAN
        x[8, 0] = NAN
        idx[idx == 7] = 6
        idx[4, 0], idx[5, width // 2], idx[6, width - 1] = 7, 7, 7        # the NaN row first, in the middle, last
        idx[1, width - 1] = 7 if width > 1 else POOL_NS                  # and next to a shadow entry
    return x, idx


@pytest.mark.parametrize("name,c,width", POOL, ids=_ids(POOL))
def test_maxpool_and_gather_exact(ops, name, c, width):
    x, idx = _pool_inputs(name, c, width)
    t = ops.neighbor_table(D(idx), POOL_NS)
    buf, out = dst_slice(9, c, fill=SENT)
    ops.point_maxpool(src_slice(x), t, out=out)
    want = pr.maxpool(x, idx)
    assert pads_untouched(buf, c, SENT) and np.array_equal(N(out), want)
    shadow = (idx == POOL_NS).any(1)
    assert (N(out)[~shadow] < 0).all() and not N(out)[shadow].any()
    assert torch.equal(ops.point_maxpool(D(x), t), out)
    # gather: column 0 of a table with idx_ld = width
    buf, out = dst_slice(9, c, fill=SENT)
    ops.point_gather_rows(src_slice(x), t, out=out)
    assert pads_untouched(buf, c, SENT) and np.array_equal(N(out), pr.gather_rows(x, idx))
    assert not N(out)[1].any() and not N(out)[2].any() and np.array_equal(N(out)[0], x[idx[0, 0]])
    assert torch.equal(ops.point_gather_rows(D(x), t), out)


@pytest.mark.parametrize("name,c,width", POOL, ids=_ids(POOL))
def test_maxpool_propagates_nan_like_the_reference(ops, name, c, width):
    """kpconv_blocks.py:103 pools with torch.max, which returns NaN when a pooled row holds one: a poisoned feature stays visible at
    every strided block instead of turning into the maximum of the others."""
    x, idx = _pool_inputs(name, c, width, with_nan=True)
    t = ops.neighbor_table(D(idx), POOL_NS)
    got = N(ops.point_maxpool(D(x), t))
    want = pr.maxpool(x, idx)
    assert np.array_equal(got, want, equal_nan=True)
    for row in (4, 5, 6) + ((1,) if width > 1 else ()):
        assert np.isnan(got[row, c // 2]), row
    assert np.isnan(got).sum() == np.isnan(want).sum()
    g = N(ops.point_gather_rows(D(x), t))
    assert np.array_equal(g, pr.gather_rows(x, idx), equal_nan=True) and np.isnan(g[4, c // 2])


# ================================================================================================== 6. L2 normalise
L2 = [("c1", 1), ("c32", 32), ("c65", 65), ("c256", 256)]


@pytest.mark.parametrize("name,c", L2, ids=_ids(L2))
def test_l2_normalize_vs_fp64(ops, name, c):
    x = rng_of("l2" + name).normal(0, 1, (9, c)).astype(F32)
    x[2] = 0                                                      # an all-zero row
    x[3] = 0
    x[3, c // 2] = 1e-13                                          # norm below the 1e-12 clamp: divided by the clamp, not by the norm
    x[4] = 1e-15 * x[5]                                           # squares near 1e-30: above the fp32 subnormals, the norm below the clamp
    buf, out = dst_slice(9, c)
    ops.point_l2_normalize(src_slice(x), out=out)
    assert pads_untouched(buf, c)
    ref, bound = pr.l2_normalize(x)
    gate("l2_normalize", name, out, ref, bound)
    got = N(out)
    assert not got[2].any() and abs(got[3, c // 2] - 0.1) < 1e-6
    plain = ops.point_l2_normalize(D(x))
    xi = D(x).clone()
    assert ops.point_l2_normalize(xi, out=xi) is xi and torch.equal(xi, plain) and torch.equal(plain, out)
    xs = src_slice(x)
    ops.point_l2_normalize(xs, out=xs)
    assert torch.equal(xs, plain)


# ================================================================================================== 7. radius search (exact)
def lattice(rng, n, span=12):
    """coordinates k / 32: with radius 0.125, r^2 = 2^-6 and d^2 = 16 / 1024 occur exactly -- pairs that `d2 < r2` must exclude -- and many
    distances tie; points repeat (ties at d2 = 0)"""
    p = (rng.integers(0, span, (n, 3)) / 32.0).astype(F32)
    if n > 1:
        p[1] = p[0]
    return p


def _forty(rng):
    return [int(v) for v in rng.integers(5, 21, 40)]


# id -> (q_lengths, s_lengths, queries are the supports).  256 queries per workgroup, supports staged 256 at a time over the union of the
# clouds of the workgroup's queries.
RADIUS = {
    "gaps_in_queries": ([0, 120, 0, 90], [30, 150, 20, 100], False),             # clouds without queries between the others
    "cloud_without_supports": ([40, 50, 30], [60, 0, 45], False),                # queries whose cloud is empty: count 0
    "empty_cloud_in_the_middle": ([40, 0, 30], [50, 0, 45], False),              # neither queries nor supports
    "forty_tiny_clouds": (None, None, True),                                     # dozens of clouds inside one workgroup's 256 queries
    "q257_s255": ([257], [255], False), "q257_s256": ([257], [256], False), "q257_s257": ([257], [257], False),
    "q256_s257": ([256], [257], False),
}


def _radius_inputs(name):
    rng = rng_of("rad" + name)
    ql, sl, same = RADIUS[name]
    if same:
        ql = sl = _forty(rng)
        s = lattice(rng, sum(sl), span=6)
        return s, s, ql, sl
    return lattice(rng, sum(ql)), lattice(rng, sum(sl)), ql, sl


def _radius_check(ops, q, s, ql, sl, radius, limit):
    got = ops.radius_neighbors(D(q), D(s), ql, sl, radius, limit)
    want = R.np_radius(q, s, ql, sl, radius, limit)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape and np.array_equal(N(got), want), (radius, limit)
    return want


@pytest.mark.parametrize("name", list(RADIUS))
def test_radius_search_layouts_exact(ops, name):
    q, s, ql, sl = _radius_inputs(name)
    r = np.float32(0.125)
    on_sphere, qs, ss = 0, 0, 0
    for a, b in zip(ql, sl):                                      # pairs at exactly d2 == r2 exist and are excluded by the strict test
        d = q[qs:qs + a, None, :] - s[None, ss:ss + b, :]
        on_sphere += int((((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) == r * r).sum())
        qs, ss = qs + a, ss + b
    assert on_sphere > 0
    widths = []
    for limit in (None, 0, 1, 10 ** 6):
        widths.append(_radius_check(ops, q, s, ql, sl, 0.125, limit).shape[1])
    assert widths[0] == widths[1] == widths[3] > 1 and widths[2] == 1
    assert _radius_check(ops, q, s, ql, sl, 0.0, None).shape == (len(q), 0)              # radius 0: every count is zero
    assert _radius_check(ops, q + F32(10.0), s, ql, sl, 0.125, 5).shape == (len(q), 0)   # nothing in reach


def test_radius_search_self_matches_and_duplicates(ops):
    """a radius below the lattice step: only coincident points remain (d2 = 0 ties, ordered by index)"""
    s, _, ql, sl = _radius_inputs("forty_tiny_clouds")
    want = _radius_check(ops, s, s, ql, sl, 1e-3, None)
    assert want.shape[1] >= 2 and (want[:, 0] <= np.arange(len(s))).all() and want[1, 0] == 0 and want[1, 1] == 1
    assert _radius_check(ops, s, s, ql, sl, 1e-3, 1).shape[1] == 1


# ================================================================================================== 8. grid subsampling (exact)
def _grid_cases():
    out = {}
    rng = rng_of("grid")
    out["faces_dl_2^-4"] = ((rng.integers(-8, 9, (200, 3)) * 2.0 ** -4).astype(F32), [120, 80], 2.0 ** -4)        # every point on a voxel corner
    neg = rng.uniform(-0.4, 0.3, (301, 3)).astype(F32)
    out["negative_dl_0.05"] = (neg, [1, 0, 300], 0.05)                                                         # one point, an empty cloud, 300
    out["negative_dl_0.1"] = (neg, [1, 0, 300], 0.1)
    out["one_voxel"] = (rng.uniform(0.01, 0.04, (300, 3)).astype(F32), [300], 0.05)
    big = rng.uniform(0, 1, (64, 3)).astype(F32)
    big[0], big[1] = 0.0, 1.0
    out["keys_above_2^32"] = (big, [64], 2.0 ** -11)
    return out


GRID = _grid_cases()


@pytest.mark.parametrize("name", list(GRID))
def test_grid_keys_and_subsampling_exact(ops, name):
    from rnnpose_amd.descriptor3d import grid_subsample
    pts, lengths, dl = GRID[name]
    start, kmax = 0, 0
    for ln in lengths:
        p = pts[start:start + ln]
        start += ln
        if ln == 0:
            continue
        keys, origin, (nx, ny) = pr.voxel_keys(p, dl)
        got = ops.grid_voxel_keys(D(p), origin, F32(dl), nx, ny)
        assert got.dtype == torch.int64 and np.array_equal(N(got), keys)
        kmax = max(kmax, int(keys.max()))
    got, gl = grid_subsample(D(pts), lengths, dl)
    want, wl = R.np_grid_subsample(pts, lengths, dl)
    assert np.array_equal(gl.numpy(), wl) and np.array_equal(N(got), want)
    if name == "keys_above_2^32":
        assert kmax > 2 ** 32                                     # why the keys are 64-bit
    if name == "one_voxel":
        assert list(wl) == [1]
    if name.startswith("negative"):
        assert wl[0] == 1 and wl[1] == 0 and np.array_equal(want[0], pts[0]) and (pts < 0).any()
    if name.startswith("faces"):
        assert (pts < 0).any() and np.array_equal(pts / F32(dl), np.round(pts / F32(dl)))


# ================================================================================================== 9. refused arguments
def test_bad_arguments_through_the_c_abi_write_nothing(ops):
    """one broken size rule per call, every one refused by the entry point's own checks before any launch: return code 1, a message, and
    every output buffer keeps its sentinel"""
    from rnnpose_amd import _lib
    lib = _lib.load()
    P, st = ops._ptr, ops._stream()
    x = torch.full((8, 300), 3.0, device="cuda")
    pts = torch.zeros(8, 3, device="cuda")
    kp = torch.zeros(17, 3, device="cuda")
    nb = torch.zeros(8, 4, dtype=torch.int32, device="cuda")
    starts = torch.tensor([0, 8], dtype=torch.int32, device="cuda")
    offs = torch.zeros(8, dtype=torch.int64, device="cuda")
    w = torch.ones(300, 8, device="cuda")
    mr = torch.ones(300, 2, device="cuda")
    out = torch.full((8 * 17 * 300,), SENT, device="cuda")
    ws = torch.full((4096,), SENT, dtype=torch.float64, device="cuda")
    iout = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    lout = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    z = C.c_void_p(0)
    calls = [
        ("row_sum ldx < c", lib.rnnpose_point_row_sum_f32, (P(x), 8, 4, 3, P(out), st), b"bad size"),
        ("row_sum c = 0", lib.rnnpose_point_row_sum_f32, (P(x), 8, 0, 4, P(out), st), b"bad size"),
        ("kpconv K = 17", lib.rnnpose_kpconv_aggregate_f32, (P(pts), 2, P(pts), 8, P(nb), 3, P(kp), 17, 0.1, P(x), 4, 300, P(x), P(out), st), b"K must"),
        ("kpconv K = 0", lib.rnnpose_kpconv_aggregate_f32, (P(pts), 2, P(pts), 8, P(nb), 3, P(kp), 0, 0.1, P(x), 4, 300, P(x), P(out), st), b"K must"),
        ("kpconv c_in = 257", lib.rnnpose_kpconv_aggregate_f32, (P(pts), 2, P(pts), 8, P(nb), 3, P(kp), 15, 0.1, P(x), 257, 300, P(x), P(out), st), b"c_in"),
        ("kpconv extent = 0", lib.rnnpose_kpconv_aggregate_f32, (P(pts), 2, P(pts), 8, P(nb), 3, P(kp), 15, 0.0, P(x), 4, 300, P(x), P(out), st), b"extent"),
        ("kpconv ldx < c_in", lib.rnnpose_kpconv_aggregate_f32, (P(pts), 2, P(pts), 8, P(nb), 3, P(kp), 15, 0.1, P(x), 4, 3, P(x), P(out), st), b"c_in"),
        ("kpconv width = 0", lib.rnnpose_kpconv_aggregate_f32, (P(pts), 2, P(pts), 8, P(nb), 0, P(kp), 15, 0.1, P(x), 4, 300, P(x), P(out), st), b"bad size"),
        ("linear m = 0", lib.rnnpose_point_linear_f32, (P(x), 8, 4, 300, P(w), 0, z, P(out), 8, st), b"bad size"),
        ("linear lda < k", lib.rnnpose_point_linear_f32, (P(x), 8, 4, 3, P(w), 8, z, P(out), 8, st), b"bad size"),
        ("linear ldo < m", lib.rnnpose_point_linear_f32, (P(x), 8, 4, 300, P(w), 8, z, P(out), 7, st), b"bad size"),
        ("linear n = 0", lib.rnnpose_point_linear_f32, (P(x), 0, 4, 300, P(w), 8, z, P(out), 8, st), b"bad size"),
        ("norm_stats ldx < c", lib.rnnpose_point_norm_stats_f32, (P(x), 8, 4, 3, 1e-5, P(ws), ws.numel() * 8, P(out), st), b"bad size"),
        ("norm_stats workspace", lib.rnnpose_point_norm_stats_f32, (P(x), 8, 4, 300, 1e-5, P(ws), 4 * 2 * 8 - 1, P(out), st), b"workspace"),
        ("norm_apply ldo < c", lib.rnnpose_point_norm_apply_f32, (P(x), 8, 4, 300, P(mr), z, 0, z, 1, 0.1, P(out), 3, st), b"bad size"),
        ("norm_apply ldr < c", lib.rnnpose_point_norm_apply_f32, (P(x), 8, 4, 300, P(mr), P(x), 3, z, 1, 0.1, P(out), 4, st), b"bad size"),
        ("norm_apply stats without res", lib.rnnpose_point_norm_apply_f32, (P(x), 8, 4, 300, P(mr), z, 0, P(mr), 1, 0.1, P(out), 4, st), b"without res"),
        ("maxpool width = 0", lib.rnnpose_point_maxpool_f32, (P(x), 8, 4, 300, P(nb), 8, 0, P(out), 4, st), b"bad size"),
        ("maxpool ldo < c", lib.rnnpose_point_maxpool_f32, (P(x), 8, 4, 300, P(nb), 8, 4, P(out), 3, st), b"bad size"),
        ("gather idx_ld = 0", lib.rnnpose_point_gather_rows_f32, (P(x), 8, 4, 300, P(nb), 8, 0, P(out), 4, st), b"bad size"),
        ("gather ldx < c", lib.rnnpose_point_gather_rows_f32, (P(x), 8, 4, 3, P(nb), 8, 4, P(out), 4, st), b"bad size"),
        ("l2 ldx < c", lib.rnnpose_point_l2_normalize_f32, (P(x), 8, 4, 3, P(out), 4, st), b"bad size"),
        ("l2 ldo < c", lib.rnnpose_point_l2_normalize_f32, (P(x), 8, 4, 300, P(out), 3, st), b"bad size"),
        ("keys dl = 0", lib.rnnpose_grid_voxel_keys_f32, (P(pts), 8, 0.0, 0.0, 0.0, 0.0, 4, 4, P(lout), st), b"bad size"),
        ("keys nx = 0", lib.rnnpose_grid_voxel_keys_f32, (P(pts), 8, 0.0, 0.0, 0.0, 0.1, 0, 4, P(lout), st), b"bad size"),
        ("radius_count clouds = 0", lib.rnnpose_radius_count_f32, (P(pts), 8, P(pts), P(starts), P(starts), 0, 0.1, P(iout), st), b"bad size"),
        ("radius_count n_q = 0", lib.rnnpose_radius_count_f32, (P(pts), 0, P(pts), P(starts), P(starts), 1, 0.1, P(iout), st), b"bad size"),
        ("radius_neighbors width = 0", lib.rnnpose_radius_neighbors_f32,
         (P(pts), 8, P(pts), P(starts), P(starts), 1, 0.1, P(offs), P(iout), P(out), 0, P(iout), st), b"bad size"),
    ]
    for label, fn, args, msg in calls:
        rc = fn(*args)
        torch.cuda.synchronize()
        assert rc == 1 and msg in lib.rnnpose_last_error(), (label, rc, lib.rnnpose_last_error())
    assert (out == SENT).all() and (ws == SENT).all() and (iout == 7).all() and (lout == 7).all()
    assert lib.rnnpose_point_norm_workspace_bytes(513, 4) == 2 * 4 * 2 * 8 and lib.rnnpose_point_norm_workspace_bytes(0, 4) == 0
