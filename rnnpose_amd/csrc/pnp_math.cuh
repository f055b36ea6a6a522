// The arithmetic of the descriptor-based pose initialiser, fp64, as plain functions: the P3P minimal solver,
// the score of one correspondence, the Gauss-Newton terms of one correspondence, the 6x6 Cholesky solve and the SE(3) left increment.
// No intrinsics, no HIP types: csrc/pnp.cuh calls these from its kernels, and tests/test_pnp_math_host.py compiles exactly this text
// with the host compiler behind a C shim.  (The including file decides about fma contraction; csrc/eval_metrics.hip turns it off.)
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
#define PNP_HD __host__ __device__ inline
#else
#define PNP_HD inline
#endif

namespace pnpm {

constexpr double kMinZ = 1e-6;      // a point at or behind this depth is an outlier

PNP_HD bool finite_d(double v) { return v - v == 0.0; }

// ---- polynomial roots ---------------------------------------------------------------------------------------------------------
// monic cubic z^3 + A z^2 + B z + C: all real roots, DESCENDING, each polished by two Newton steps -> their number (1 or 3)
PNP_HD int cubic_real_roots(double A, double B, double C, double z[3]) {
  const double P = B - A * A / 3.0, Q = 2.0 * A * A * A / 27.0 - A * B / 3.0 + C;
  const double disc = Q * Q / 4.0 + P * P * P / 27.0;
  int n;
  if (disc > 0.0) {
    const double sd = sqrt(disc);
    z[0] = cbrt(-Q / 2.0 + sd) + cbrt(-Q / 2.0 - sd);
    n = 1;
  } else if (!(P < 0.0)) {
    z[0] = z[1] = z[2] = 0.0;
    n = 3;
  } else {
    const double rr = 2.0 * sqrt(-P / 3.0);
    double arg = 3.0 * Q / (P * rr);
    arg = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);
    const double th = acos(arg);
    for (int k = 0; k < 3; ++k) z[k] = rr * cos((th - 2.0 * 3.14159265358979323846 * k) / 3.0);
    n = 3;       // k = 0 is the largest; k = 1, 2 are then sorted below
    if (z[1] < z[2]) {
      const double s = z[1];
      z[1] = z[2];
      z[2] = s;
    }
  }
  for (int k = 0; k < n; ++k) {
    double x = z[k] - A / 3.0;
    for (int it = 0; it < 2; ++it) {
      const double f = ((x + A) * x + B) * x + C, d = (3.0 * x + 2.0 * A) * x + B;
      if (d != 0.0 && finite_d(f / d)) x -= f / d;
    }
    z[k] = x;
  }
  return n;
}

// c[0] + c[1] x + ... + c[4] x^4 = 0: the real roots by Ferrari's factorisation into two quadratics (largest root of the resolvent
// cubic), each polished by three Newton steps on the quartic itself -> their number (0..4).  ROOT ORDER (the tie rule of the P3P
// candidates): first quadratic y^2 + m y + s1 with +sqrt then -sqrt, then y^2 - m y + s2 likewise; the biquadratic case w+ (+, -), w- (+, -).
PNP_HD int quartic_real_roots(const double c[5], double x[4]) {
  double big = 0.0;
  for (int i = 0; i < 5; ++i) big = fabs(c[i]) > big ? fabs(c[i]) : big;
  if (!(big > 0.0) || !finite_d(big)) return 0;
  int n = 0;
  if (fabs(c[4]) <= 1e-13 * big) {                      // the leading term vanishes: a cubic (or nothing this solver follows)
    if (fabs(c[3]) <= 1e-13 * big) return 0;
    n = cubic_real_roots(c[2] / c[3], c[1] / c[3], c[0] / c[3], x);
    return n;
  }
  const double a = c[3] / c[4], b = c[2] / c[4], cc = c[1] / c[4], d = c[0] / c[4];
  const double p = b - 3.0 * a * a / 8.0, q = cc - a * b / 2.0 + a * a * a / 8.0;
  const double r = d - a * cc / 4.0 + a * a * b / 16.0 - 3.0 * a * a * a * a / 256.0;
  double z[3];
  cubic_real_roots(2.0 * p, p * p - 4.0 * r, -q * q, z);
  const double zz = z[0];
  const double scale = fabs(p) + sqrt(fabs(r)) + 1e-300;
  double y[4];
  if (!(zz > 1e-14 * scale)) {                          // q = 0: biquadratic in y
    double disc = p * p - 4.0 * r;
    if (disc < 0.0 && disc > -1e-9 * (p * p + 4.0 * fabs(r))) disc = 0.0;
    if (disc >= 0.0) {
      const double sd = sqrt(disc), w[2] = {(-p + sd) / 2.0, (-p - sd) / 2.0};
      for (int k = 0; k < 2; ++k) {
        double wk = w[k];
        if (wk < 0.0 && wk > -1e-9 * scale) wk = 0.0;
        if (wk >= 0.0) {
          y[n++] = sqrt(wk);
          y[n++] = -sqrt(wk);
        }
      }
    }
  } else {
    const double m = sqrt(zz), h = (p + zz) / 2.0, g = q / (2.0 * m);
    const double s[2] = {h - g, h + g}, sg[2] = {-1.0, 1.0};
    for (int k = 0; k < 2; ++k) {
      double disc = zz - 4.0 * s[k];
      if (disc < 0.0 && disc > -1e-9 * (zz + 4.0 * fabs(s[k]))) disc = 0.0;
      if (disc >= 0.0) {
        const double sd = sqrt(disc);
        y[n++] = (sg[k] * m + sd) / 2.0;
        y[n++] = (sg[k] * m - sd) / 2.0;
      }
    }
  }
  for (int k = 0; k < n; ++k) {
    double v = y[k] - a / 4.0;
    for (int it = 0; it < 3; ++it) {
      const double f = (((c[4] * v + c[3]) * v + c[2]) * v + c[1]) * v + c[0];
      const double df = ((4.0 * c[4] * v + 3.0 * c[3]) * v + 2.0 * c[2]) * v + c[1];
      if (df != 0.0 && finite_d(f / df)) v -= f / df;
    }
    x[k] = v;
  }
  return n;
}

// ---- P3P ------------------------------------------------------------------------------------------------------------------------
PNP_HD void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
PNP_HD double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// orthonormal frame (columns e1, e2, e3 as rows of F) of the triangle p0 p1 p2; false when it is degenerate
PNP_HD bool tri_frame(const double p0[3], const double p1[3], const double p2[3], double F[3][3]) {
  double d1[3], d2[3], n[3];
  for (int k = 0; k < 3; ++k) {
    d1[k] = p1[k] - p0[k];
    d2[k] = p2[k] - p0[k];
  }
  cross3(d1, d2, n);
  const double l1 = dot3(d1, d1), l2 = dot3(d2, d2), ln = dot3(n, n);
  if (!(ln > 1e-20 * l1 * l2) || !finite_d(ln)) return false;
  const double i1 = 1.0 / sqrt(l1), in = 1.0 / sqrt(ln);
  for (int k = 0; k < 3; ++k) {
    F[0][k] = d1[k] * i1;
    F[2][k] = n[k] * in;
  }
  cross3(F[2], F[0], F[1]);
  return true;
}

// Xw: the three model points; xn: their image points in NORMALISED coordinates ((u - cx) / fx, (v - cy) / fy).
// -> number of solutions (0..4); Rt[s] = rows of [R | t] (12 values).  Grunert's elimination: with the distances s2 = u s1, s3 = v s1,
// u is a rational function N(v) / D(v) of v and v a root of a quartic whose coefficients are formed here by polynomial arithmetic;
// every root with u, v > 0 gives the three distances, which three Newton steps on the three distance equations polish; the pose is
// the rigid alignment of the two (then congruent) triangles, a rotation by construction.  Kept: finite, all three depths > 0.
PNP_HD int p3p_solve(const double Xw[3][3], const double xn[3][2], double Rt[4][12]) {
  double j[3][3];
  for (int i = 0; i < 3; ++i) {
    const double l = 1.0 / sqrt(xn[i][0] * xn[i][0] + xn[i][1] * xn[i][1] + 1.0);
    j[i][0] = xn[i][0] * l;
    j[i][1] = xn[i][1] * l;
    j[i][2] = l;
  }
  double Fp[3][3];
  if (!tri_frame(Xw[0], Xw[1], Xw[2], Fp)) return 0;
  double e[3];
  for (int k = 0; k < 3; ++k) e[k] = Xw[1][k] - Xw[2][k];
  const double a2 = dot3(e, e);
  for (int k = 0; k < 3; ++k) e[k] = Xw[0][k] - Xw[2][k];
  const double b2 = dot3(e, e);
  for (int k = 0; k < 3; ++k) e[k] = Xw[0][k] - Xw[1][k];
  const double c2 = dot3(e, e);
  if (!(a2 > 0.0) || !(b2 > 0.0) || !(c2 > 0.0)) return 0;
  const double ca = dot3(j[1], j[2]), cb = dot3(j[0], j[2]), cg = dot3(j[0], j[1]);
  const double q = (a2 - c2) / b2, cr = c2 / b2;
  const double N[3] = {q + 1.0, -2.0 * q * cb, q - 1.0}, D[2] = {2.0 * cg, -2.0 * ca}, W[3] = {1.0, -2.0 * cb, 1.0};
  double D2[3] = {D[0] * D[0], 2.0 * D[0] * D[1], D[1] * D[1]};
  double Q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) Q[i + k] += N[i] * N[k] - cr * W[i] * D2[k];
  for (int i = 0; i < 3; ++i) Q[i] += D2[i];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 2; ++k) Q[i + k] -= 2.0 * cg * N[i] * D[k];
  double vs[4];
  const int nr = quartic_real_roots(Q, vs);
  int ns = 0;
  for (int r = 0; r < nr; ++r) {
    const double v = vs[r];
    if (!(v > 0.0) || !finite_d(v)) continue;
    const double Wv = 1.0 + v * v - 2.0 * cb * v;
    if (!(Wv > 0.0)) continue;
    const double Nv = (N[2] * v + N[1]) * v + N[0], Dv = D[1] * v + D[0];
    double u;
    if (fabs(Dv) > 1e-12) {
      u = Nv / Dv;
    } else {                                             // u is a root of u^2 - 2 cg u + 1 - cr W(v): the one that satisfies the other equation
      double disc = cg * cg - (1.0 - cr * Wv);
      if (disc < 0.0) disc = 0.0;
      const double u0 = cg + sqrt(disc), u1 = cg - sqrt(disc);
      const double r0 = fabs(b2 * (u0 * u0 + v * v - 2.0 * u0 * v * ca) - a2 * Wv), r1 = fabs(b2 * (u1 * u1 + v * v - 2.0 * u1 * v * ca) - a2 * Wv);
      u = r0 <= r1 ? u0 : u1;
    }
    if (!(u > 0.0) || !finite_d(u)) continue;
    double s[3];
    s[0] = sqrt(b2 / Wv);
    s[1] = u * s[0];
    s[2] = v * s[0];
    for (int it = 0; it < 3; ++it) {                     // Newton on the three distance equations
      const double f0 = s[1] * s[1] + s[2] * s[2] - 2.0 * s[1] * s[2] * ca - a2;
      const double f1 = s[0] * s[0] + s[2] * s[2] - 2.0 * s[0] * s[2] * cb - b2;
      const double f2 = s[0] * s[0] + s[1] * s[1] - 2.0 * s[0] * s[1] * cg - c2;
      const double J[3][3] = {{0.0, 2.0 * (s[1] - s[2] * ca), 2.0 * (s[2] - s[1] * ca)},
                              {2.0 * (s[0] - s[2] * cb), 0.0, 2.0 * (s[2] - s[0] * cb)},
                              {2.0 * (s[0] - s[1] * cg), 2.0 * (s[1] - s[0] * cg), 0.0}};
      const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                         J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
      if (!(fabs(det) > 1e-300)) break;
      const double d0 = (f0 * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (f1 * J[2][2] - J[1][2] * f2) + J[0][2] * (f1 * J[2][1] - J[1][1] * f2)) / det;
      const double d1 = (J[0][0] * (f1 * J[2][2] - J[1][2] * f2) - f0 * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) + J[0][2] * (J[1][0] * f2 - f1 * J[2][0])) / det;
      const double d2 = (J[0][0] * (J[1][1] * f2 - f1 * J[2][1]) - J[0][1] * (J[1][0] * f2 - f1 * J[2][0]) + f0 * (J[1][0] * J[2][1] - J[1][1] * J[2][0])) / det;
      if (!finite_d(d0) || !finite_d(d1) || !finite_d(d2)) break;
      if (fabs(d0) > 0.5 * s[0] || fabs(d1) > 0.5 * s[1] || fabs(d2) > 0.5 * s[2]) break;      // not a polish any more: keep the root's distances
      s[0] -= d0;
      s[1] -= d1;
      s[2] -= d2;
    }
    if (!(s[0] > 0.0) || !(s[1] > 0.0) || !(s[2] > 0.0)) continue;
    double Qc[3][3], Fq[3][3];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) Qc[i][k] = s[i] * j[i][k];
    if (!tri_frame(Qc[0], Qc[1], Qc[2], Fq)) continue;
    double* o = Rt[ns];
    bool ok = true;
    for (int rr = 0; rr < 3; ++rr)
      for (int cc = 0; cc < 3; ++cc) {
        o[4 * rr + cc] = Fq[0][rr] * Fp[0][cc] + Fq[1][rr] * Fp[1][cc] + Fq[2][rr] * Fp[2][cc];
        ok = ok && finite_d(o[4 * rr + cc]);
      }
    for (int rr = 0; rr < 3; ++rr) {                     // t = centroid(Q) - R centroid(P)
      double t = 0.0;
      for (int i = 0; i < 3; ++i) t += Qc[i][rr] - (o[4 * rr] * Xw[i][0] + o[4 * rr + 1] * Xw[i][1] + o[4 * rr + 2] * Xw[i][2]);
      o[4 * rr + 3] = t / 3.0;
      ok = ok && finite_d(o[4 * rr + 3]);
    }
    for (int i = 0; i < 3; ++i)                          // all three sample depths > 0 under the pose itself
      ok = ok && (o[8] * Xw[i][0] + o[9] * Xw[i][1] + o[10] * Xw[i][2] + o[11] > 0.0);
    if (ok) ++ns;
  }
  return ns;
}

// ---- scoring and Gauss-Newton terms of one correspondence --------------------------------------------------------------------
struct Cam {
  double fx, fy, cx, cy;
};

// squared re-projection residual of X under Rt against x; false (and r2 untouched) for a point at Z <= kMinZ: an outlier
PNP_HD bool reproj_r2(const double Rt[12], const Cam& k, const double X[3], const double x[2], double* r2) {
  const double Z = Rt[8] * X[0] + Rt[9] * X[1] + Rt[10] * X[2] + Rt[11];
  if (!(Z > kMinZ)) return false;
  const double Xc = Rt[0] * X[0] + Rt[1] * X[1] + Rt[2] * X[2] + Rt[3], Yc = Rt[4] * X[0] + Rt[5] * X[1] + Rt[6] * X[2] + Rt[7];
  const double du = k.fx * Xc / Z + k.cx - x[0], dv = k.fy * Yc / Z + k.cy - x[1];
  *r2 = du * du + dv * dv;
  return true;
}

// MSAC term and inlier flag of one correspondence: cost += min(r2, tau2); inlier iff r2 < tau2
PNP_HD bool score_point(const double Rt[12], const Cam& k, const double X[3], const double x[2], double tau2, double* cost) {
  double r2;
  if (!reproj_r2(Rt, k, X, x, &r2) || !(r2 < tau2)) {
    *cost = tau2;
    return false;
  }
  *cost = r2;
  return true;
}

// r = proj(X1) - x and its 2 x 6 Jacobian with respect to a left increment xi = (translation, rotation): J = J_proj [I | -[X1]x]
PNP_HD void gn_jacobian(const double Rt[12], const Cam& k, const double X[3], const double x[2], double r[2], double J[2][6]) {
  const double Xc = Rt[0] * X[0] + Rt[1] * X[1] + Rt[2] * X[2] + Rt[3], Yc = Rt[4] * X[0] + Rt[5] * X[1] + Rt[6] * X[2] + Rt[7];
  const double Z = Rt[8] * X[0] + Rt[9] * X[1] + Rt[10] * X[2] + Rt[11], iz = 1.0 / Z;
  r[0] = k.fx * Xc * iz + k.cx - x[0];
  r[1] = k.fy * Yc * iz + k.cy - x[1];
  const double P[2][3] = {{k.fx * iz, 0.0, -k.fx * Xc * iz * iz}, {0.0, k.fy * iz, -k.fy * Yc * iz * iz}};
  for (int a = 0; a < 2; ++a) {
    J[a][0] = P[a][0];
    J[a][1] = P[a][1];
    J[a][2] = P[a][2];
    // -[X1]x = [[0, Z, -Y], [-Z, 0, X], [Y, -X, 0]]
    J[a][3] = -P[a][1] * Z + P[a][2] * Yc;
    J[a][4] = P[a][0] * Z - P[a][2] * Xc;
    J[a][5] = -P[a][0] * Yc + P[a][1] * Xc;
  }
}

// upper triangle of J^T J (21 values, row-major: (0,0) (0,1) .. (0,5) (1,1) ..) and J^T r (6 values) of one correspondence, ADDED
PNP_HD void gn_accumulate(const double Rt[12], const Cam& k, const double X[3], const double x[2], double H[21], double g[6]) {
  double r[2], J[2][6];
  gn_jacobian(Rt, k, X, x, r, J);
  int e = 0;
  for (int a = 0; a < 6; ++a) {
    for (int b = a; b < 6; ++b) H[e++] += J[0][a] * J[0][b] + J[1][a] * J[1][b];
    g[a] += J[0][a] * r[0] + J[1][a] * r[1];
  }
}

// H (upper triangle, 21 values) xi = -g by Cholesky; false when H is not positive definite (a pivot not above 1e-13 of its diagonal
// entry, or not finite)
PNP_HD bool chol6_solve(const double H[21], const double g[6], double xi[6]) {
  double A[6][6], L[6][6];
  int e = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = H[e++];
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) L[a][b] = 0.0;
  for (int c = 0; c < 6; ++c) {
    double d = A[c][c];
    for (int k = 0; k < c; ++k) d -= L[c][k] * L[c][k];
    if (!(d > 1e-13 * A[c][c]) || !finite_d(d)) return false;
    L[c][c] = sqrt(d);
    for (int r = c + 1; r < 6; ++r) {
      double s = A[r][c];
      for (int k = 0; k < c; ++k) s -= L[r][k] * L[c][k];
      L[r][c] = s / L[c][c];
    }
  }
  double y[6];
  for (int r = 0; r < 6; ++r) {
    double s = -g[r];
    for (int k = 0; k < r; ++k) s -= L[r][k] * y[k];
    y[r] = s / L[r][r];
  }
  for (int r = 5; r >= 0; --r) {
    double s = y[r];
    for (int k = r + 1; k < 6; ++k) s -= L[k][r] * xi[k];
    xi[r] = s / L[r][r];
    if (!finite_d(xi[r])) return false;
  }
  return true;
}

// Rt <- exp(xi) Rt, xi = (translation, rotation): R' = E R, t' = E t + V v with E = exp([w]x), V the left Jacobian of SO(3)
PNP_HD void se3_left_update(const double xi[6], double Rt[12]) {
  const double wx = xi[3], wy = xi[4], wz = xi[5], th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  double A, B, C;
  if (th < 1e-8) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
    C = 1.0 / 6.0 - th2 / 120.0;
  } else {
    A = sin(th) / th;
    B = (1.0 - cos(th)) / th2;
    C = (th - sin(th)) / (th2 * th);
  }
  const double Wm[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  double W2[3][3], E[3][3], V[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) W2[r][c] = Wm[r][0] * Wm[0][c] + Wm[r][1] * Wm[1][c] + Wm[r][2] * Wm[2][c];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double I = r == c ? 1.0 : 0.0;
      E[r][c] = I + A * Wm[r][c] + B * W2[r][c];
      V[r][c] = I + B * Wm[r][c] + C * W2[r][c];
    }
  double o[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c) o[4 * r + c] = E[r][0] * Rt[c] + E[r][1] * Rt[4 + c] + E[r][2] * Rt[8 + c];
    o[4 * r + 3] += V[r][0] * xi[0] + V[r][1] * xi[1] + V[r][2] * xi[2];
  }
  for (int i = 0; i < 12; ++i) Rt[i] = o[i];
}

}  // namespace pnpm
