"""csrc/pnp_math.cuh -- the text the P3P RANSAC kernels call -- compiled with the HOST compiler behind a C shim and compared with the fp64
restatement tests/pnp_ref.py (CPU; nothing is preloaded, no sanitizer): the minimal solver on the P3P test distribution, the score of
one correspondence, the Gauss-Newton terms, the 6x6 Cholesky solve and the SE(3) left increment."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pnp_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "pnp_math.cuh"
extern "C" {
int shim_quartic(const double* c, double* x) { return pnpm::quartic_real_roots(c, x); }
int shim_p3p(const double* Xw, const double* xn, double* Rt) {
  double A[3][3], b[3][2], o[4][12];
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) A[i][k] = Xw[3 * i + k];
    for (int k = 0; k < 2; ++k) b[i][k] = xn[2 * i + k];
  }
  const int n = pnpm::p3p_solve(A, b, o);
  for (int s = 0; s < n; ++s)
    for (int e = 0; e < 12; ++e) Rt[12 * s + e] = o[s][e];
  return n;
}
int shim_score(const double* Rt, const double* cam, const double* X, const double* x, double tau2, double* cost) {
  const pnpm::Cam k{cam[0], cam[1], cam[2], cam[3]};
  return pnpm::score_point(Rt, k, X, x, tau2, cost) ? 1 : 0;
}
void shim_gn(const double* Rt, const double* cam, const double* X, const double* x, double* H, double* g) {
  const pnpm::Cam k{cam[0], cam[1], cam[2], cam[3]};
  pnpm::gn_accumulate(Rt, k, X, x, H, g);
}
int shim_chol6(const double* H, const double* g, double* xi) { return pnpm::chol6_solve(H, g, xi) ? 1 : 0; }
void shim_update(const double* xi, double* Rt) { pnpm::se3_left_update(xi, Rt); }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx is None and os.path.exists(c):
            cxx = c
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pnp_math")
    src, so = d / "shim.cpp", d / "libpnp_math_shim.so"
    src.write_text(SHIM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "rnnpose_amd", "csrc"),
                        str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    lib.shim_quartic.argtypes, lib.shim_quartic.restype = [dp, dp], C.c_int
    lib.shim_p3p.argtypes, lib.shim_p3p.restype = [dp, dp, dp], C.c_int
    lib.shim_score.argtypes, lib.shim_score.restype = [dp, dp, dp, dp, C.c_double, dp], C.c_int
    lib.shim_gn.argtypes, lib.shim_gn.restype = [dp] * 6, None
    lib.shim_chol6.argtypes, lib.shim_chol6.restype = [dp, dp, dp], C.c_int
    lib.shim_update.argtypes, lib.shim_update.restype = [dp, dp], None
    return lib


def P(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def A(a):
    return np.ascontiguousarray(np.asarray(a, np.float64))


CAM = A([pr.P3P_K[0, 0], pr.P3P_K[1, 1], pr.P3P_K[0, 2], pr.P3P_K[1, 2]])


def test_quartic_roots(shim):
    rng = np.random.default_rng(3)
    for _ in range(300):
        roots = rng.uniform(-3, 3, 4)
        kind = rng.integers(0, 3)
        if kind == 0:                                     # four real roots
            c = np.poly(roots)
            want = np.sort(roots)
        elif kind == 1:                                   # two real, one complex pair
            c = np.polymul(np.poly(roots[:2]), [1.0, -2 * roots[2], roots[2] ** 2 + roots[3] ** 2 + 0.1])
            want = np.sort(roots[:2])
        else:                                             # none
            c = np.polymul([1.0, -2 * roots[0], roots[0] ** 2 + roots[1] ** 2 + 0.1], [1.0, -2 * roots[2], roots[2] ** 2 + roots[3] ** 2 + 0.1])
            want = np.zeros(0)
        c = A(c[::-1] * rng.uniform(0.5, 2.0))            # ascending powers, any leading coefficient
        if want.size > 1 and np.diff(want).min() < 1e-3:
            continue                                      # (near-double roots are legitimately ill-conditioned)
        x = np.zeros(4)
        n = shim.shim_quartic(P(c), P(x))
        assert n == want.size, (c, x[:n], want)
        assert np.abs(np.sort(x[:n]) - want).max(initial=0.0) < 1e-9


def _solve(shim, Xw, xn):
    out = np.zeros(48)
    n = shim.shim_p3p(P(A(Xw)), P(A(xn)), P(out))
    return [(out[12 * s:12 * s + 12].reshape(3, 4)[:, :3].copy(), out[12 * s:12 * s + 12].reshape(3, 4)[:, 3].copy()) for s in range(n)]


def test_p3p_solver_against_the_restatement(shim):
    """The P3P distribution of the GPU test (fp32-rounded inputs, 20 scenes x 40 triples).  Every solution reprojects its samples and is a
    rotation; for at least 99 % of the triples (the issue's cap: near-double roots are in the mix) the two solvers give the same poses."""
    X, x, rnd, poses = pr.p3p_scenes(n_scenes=20, n_triples=40)
    K = pr.P3P_K
    n = agree = truth = 0
    worst_px = worst_rot = 0.0
    for s in range(X.shape[0]):
        Xs, xs = X[s].astype(np.float64), x[s].astype(np.float64)
        for h in range(rnd.shape[1]):
            i = [int(r) % 64 for r in rnd[s, h]]
            if len(set(i)) < 3:
                xr = np.stack([(xs[i, 0] - K[0, 2]) / K[0, 0], (xs[i, 1] - K[1, 2]) / K[1, 1]], 1)
                assert _solve(shim, Xs[i], xr) == []          # a repeated sample point: a degenerate triangle, no candidate
                continue
            xn = np.stack([(xs[i, 0] - K[0, 2]) / K[0, 0], (xs[i, 1] - K[1, 2]) / K[1, 1]], 1)
            got, want = _solve(shim, Xs[i], xn), pr.p3p(Xs[i], xn)
            n += 1
            for R, t in got:
                worst_px = max(worst_px, np.abs(pr.project(R, t, K, Xs[i])[0] - xs[i]).max())
                worst_rot = max(worst_rot, np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0))
            ok = all(min((max(np.abs(R - Rg).max(), np.abs(t - tg).max()) for Rg, tg in got), default=np.inf) < 1e-7 for R, t in want)
            ok = ok and all(min((max(np.abs(R - Rg).max(), np.abs(t - tg).max()) for R, t in want), default=np.inf) < 1e-7 for Rg, tg in got)
            agree += ok
            truth += min((np.abs(pr.project(R, t, K, Xs)[0] - xs).max() for R, t in got), default=np.inf) < 1e-3
    print(f"{n} triples: same poses on {agree}, true pose found on {truth}; worst sample reprojection {worst_px:.2e} px, rotation defect {worst_rot:.2e}")
    assert n > 700 and worst_px < 1e-9 and worst_rot < 1e-12
    assert agree >= 0.99 * n and truth >= 0.99 * n


def test_degenerate_samples_give_no_candidate_and_no_nan(shim):
    line = np.outer([0.0, 1.0, 2.5], [0.03, 0.01, -0.02])
    assert _solve(shim, line, [[0.0, 0.0], [0.01, 0.0], [0.02, 0.0]]) == []
    same = np.tile([0.01, 0.02, 0.03], (3, 1))
    assert _solve(shim, same, [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]) == []
    tri = np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.05, 0.0]])
    for xn in ([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], [[np.nan, 0.0], [0.1, 0.0], [0.0, 0.1]], [[1e30, 0.0], [0.1, 0.0], [0.0, 0.1]]):
        for R, t in _solve(shim, tri, xn):
            assert np.isfinite(R).all() and np.isfinite(t).all()


def test_score_gn_terms_cholesky_and_update(shim):
    rng = np.random.default_rng(4)
    R, _ = pr.se3_exp(np.concatenate([np.zeros(3), rng.normal(0, 1, 3)]))
    t = np.array([0.03, -0.02, 0.7])
    Rt = A(np.concatenate([R, t[:, None]], 1).reshape(-1))
    X = rng.uniform(-0.1, 0.1, (50, 3))
    X[0] = R.T @ (np.array([0.0, 0.0, 1e-6]) - t)          # at Z = 1e-6 (or a rounding below): an outlier
    X[1] = R.T @ (np.array([0.01, 0.0, -0.5]) - t)         # behind the camera
    x = pr.project(R, t, pr.P3P_K, X)[0] + rng.normal(0, 3.0, (50, 2))
    x[:2] = 100.0
    tau = 4.0
    r2 = pr.residuals2(R, t, pr.P3P_K, X, x)
    assert np.isinf(r2[1])
    H, g = np.zeros(21), np.zeros(6)
    for i in range(50):
        c = np.zeros(1)
        inl = shim.shim_score(P(Rt), P(CAM), P(A(X[i])), P(A(x[i])), tau * tau, P(c))
        assert inl == int(r2[i] < tau * tau) and abs(c[0] - min(r2[i], tau * tau)) <= 1e-12 * tau * tau
        if i >= 2:
            shim.shim_gn(P(Rt), P(CAM), P(A(X[i])), P(A(x[i])), P(H), P(g))
    r, J = pr.jacobian(R, t, pr.P3P_K, X[2:], x[2:])
    J2 = J.reshape(-1, 6)
    Hw, gw = J2.T @ J2, J2.T @ r.reshape(-1)
    Hf = np.zeros((6, 6))
    Hf[np.triu_indices(6)] = H
    assert np.abs(np.triu(Hw) - Hf).max() <= 1e-12 * np.abs(Hw).max() and np.abs(gw - g).max() <= 1e-12 * np.abs(gw).max()
    xi = np.zeros(6)
    assert shim.shim_chol6(P(H), P(g), P(xi)) == 1
    want = -np.linalg.solve(Hw, gw)
    assert np.abs(xi - want).max() <= 1e-9 * np.abs(want).max()
    Hs = H.copy()
    Hs[0] = -1.0
    assert shim.shim_chol6(P(Hs), P(g), P(xi)) == 0                          # not positive definite
    v = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    sing = np.outer(v, v)[np.triu_indices(6)]
    assert shim.shim_chol6(P(A(sing)), P(g), P(xi)) == 0                     # rank one
    for xi in (np.array([0.01, -0.02, 0.03, 0.3, -0.2, 0.5]), np.array([0.01, -0.02, 0.03, 1e-10, 0.0, 0.0]), np.zeros(6)):
        got = Rt.copy()
        shim.shim_update(P(A(xi)), P(got))
        Rw, tw = pr.left_update(xi, R, t)
        assert np.abs(got.reshape(3, 4)[:, :3] - Rw).max() < 1e-14 and np.abs(got.reshape(3, 4)[:, 3] - tw).max() < 1e-14
