// P3P RANSAC with MSAC scoring and a Gauss-Newton polish, fp64.  Three launches:
//   pnp_solve_kernel   one thread per (object, hypothesis): the minimal solve (csrc/pnp_math.cuh), up to four candidates into the workspace
//   pnp_score_kernel   one wave per (object, hypothesis): every candidate against all correspondences; the cheapest one is the hypothesis
//   pnp_polish_kernel  one wave per object: the cheapest hypothesis (lowest h on a tie), n_polish Gauss-Newton steps, final inlier set
// The polish is polish_body, which pnp_topk_polish_kernel (csrc/pnp_topk.cuh) runs on its slots too.
// Sums go over the lanes' strided partial sums and then through a fixed xor butterfly, counts are integers: two launches are bit-identical.
// Included by csrc/eval_metrics.hip (the entry points are there, next to the evaluator's other per-object fp64 kernels).
#pragma once
#include "common.hpp"
#include "pnp_math.cuh"

namespace pnp {

struct HypRec {
  double Rt[4][12];
  int n, best;          // candidates; the cheapest one (set by the scoring pass)
};

__device__ __forceinline__ pnpm::Cam load_cam(const float* __restrict__ K, int b) {
  const float* k = K + 9 * b;
  return pnpm::Cam{static_cast<double>(k[0]), static_cast<double>(k[4]), static_cast<double>(k[2]), static_cast<double>(k[5])};
}

__device__ __forceinline__ int clamp_count(const int* __restrict__ count, int b, int M) { return max(0, min(count[b], M)); }

__device__ __forceinline__ double inf_d() { return __longlong_as_double(0x7ff0000000000000ll); }

__global__ __launch_bounds__(64) void pnp_solve_kernel(const float* __restrict__ X, const float* __restrict__ x, const int* __restrict__ count,
                                                      int M, const float* __restrict__ K, const unsigned* __restrict__ rnd, int B, int Hyp,
                                                      int min_count, HypRec* __restrict__ rec) {
  const int b = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
  if (h >= Hyp) return;
  HypRec* out = rec + static_cast<size_t>(b) * Hyp + h;
  out->n = 0;
  out->best = -1;
  const int cnt = clamp_count(count, b, M);
  if (cnt < min_count || cnt < 3) return;
  const unsigned* r = rnd + (static_cast<size_t>(b) * Hyp + h) * 3;
  const int i0 = static_cast<int>(r[0] % static_cast<unsigned>(cnt)), i1 = static_cast<int>(r[1] % static_cast<unsigned>(cnt)),
            i2 = static_cast<int>(r[2] % static_cast<unsigned>(cnt));
  if (i0 == i1 || i0 == i2 || i1 == i2) return;
  const pnpm::Cam cam = load_cam(K, b);
  const int idx[3] = {i0, i1, i2};
  double Xw[3][3], xn[3][2];
  for (int s = 0; s < 3; ++s) {
    const float* p = X + (static_cast<size_t>(b) * M + idx[s]) * 3;
    const float* q = x + (static_cast<size_t>(b) * M + idx[s]) * 2;
    for (int k = 0; k < 3; ++k) Xw[s][k] = static_cast<double>(p[k]);
    xn[s][0] = (static_cast<double>(q[0]) - cam.cx) / cam.fx;
    xn[s][1] = (static_cast<double>(q[1]) - cam.cy) / cam.fy;
  }
  double Rt[4][12];
  const int n = pnpm::p3p_solve(Xw, xn, Rt);
  for (int c = 0; c < n; ++c)
    for (int e = 0; e < 12; ++e) out->Rt[c][e] = Rt[c][e];
  out->n = n;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o >= 1; o >>= 1) v += rp::shfl_xor_f64(v, o);
  return v;
}

__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void load_corr(const float* __restrict__ X, const float* __restrict__ x, size_t row, double P[3], double p[2]) {
  P[0] = static_cast<double>(X[row * 3]);
  P[1] = static_cast<double>(X[row * 3 + 1]);
  P[2] = static_cast<double>(X[row * 3 + 2]);
  p[0] = static_cast<double>(x[row * 2]);
  p[1] = static_cast<double>(x[row * 2 + 1]);
}

__global__ __launch_bounds__(256) void pnp_score_kernel(const float* __restrict__ X, const float* __restrict__ x, const int* __restrict__ count,
                                                       int M, const float* __restrict__ K, int B, int Hyp, double tau, HypRec* __restrict__ rec,
                                                       double* __restrict__ cost, int* __restrict__ inliers) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, h = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (h >= Hyp) return;                                  // (a whole wave leaves)
  HypRec* hr = rec + static_cast<size_t>(b) * Hyp + h;
  const int n = hr->n, cnt = clamp_count(count, b, M);
  const pnpm::Cam cam = load_cam(K, b);
  const double tau2 = tau * tau;
  double best_cost = inf_d();
  int best_inl = 0, best_c = -1;
  for (int c = 0; c < n; ++c) {
    double Rt[12];
    for (int e = 0; e < 12; ++e) Rt[e] = hr->Rt[c][e];
    double s = 0.0;
    int ni = 0;
    for (int i = lane; i < cnt; i += 64) {
      double P[3], p[2], t;
      load_corr(X, x, static_cast<size_t>(b) * M + i, P, p);
      ni += pnpm::score_point(Rt, cam, P, p, tau2, &t) ? 1 : 0;
      s += t;
    }
    s = wave_sum(s);
    ni = wave_sum_i(ni);
    if (s < best_cost) {                                 // strict: a tie keeps the lower root order
      best_cost = s;
      best_inl = ni;
      best_c = c;
    }
  }
  if (lane == 0) {
    cost[static_cast<size_t>(b) * Hyp + h] = best_cost;
    inliers[static_cast<size_t>(b) * Hyp + h] = best_inl;
    hr->best = best_c;
  }
}

// the better of two (cost, hypothesis) keys: the lower cost, the lower h on a tie; h < 0 is no key
__device__ __forceinline__ void better_key(double& bc, int& bh, double oc, int oh) {
  if (oh >= 0 && (bh < 0 || oc < bc || (oc == bc && oh < bh))) {
    bc = oc;
    bh = oh;
  }
}

// the cheapest candidate of hypothesis h of object b -> Rt; false, and Rt as it was, when h is no hypothesis or has no candidate
__device__ __forceinline__ bool load_candidate(const HypRec* __restrict__ rec, int b, int Hyp, int h, double Rt[12]) {
  if (h < 0 || h >= Hyp) return false;
  const HypRec* hr = rec + static_cast<size_t>(b) * Hyp + h;
  const int c = hr->best;
  if (c < 0 || c >= 4) return false;
  for (int e = 0; e < 12; ++e) Rt[e] = hr->Rt[c][e];
  return true;
}

// One wave polishes hypothesis h of object b (h < 0: none) and writes the outputs of `row` (the object, or its slot): n_polish
// Gauss-Newton steps on the inliers of the current pose, the finite test, the final inlier set and MSAC cost.  T is written only
// where info is 0.  kPol: the polished pose also goes to pol[row] in fp64 (the top-K path's dup_of reads it).
template <bool kPol>
__device__ __forceinline__ void polish_body(const float* __restrict__ X, const float* __restrict__ x, const int* __restrict__ count, int M,
                                            const float* __restrict__ K, int b, double tau, int n_polish, const HypRec* __restrict__ rec,
                                            int Hyp, int h, size_t row, float* __restrict__ T, unsigned char* __restrict__ inlier_mask,
                                            int* __restrict__ n_inliers, double* __restrict__ final_cost, int* __restrict__ info,
                                            double* __restrict__ pol) {
  const int lane = threadIdx.x;
  const int cnt = clamp_count(count, b, M);
  const pnpm::Cam cam = load_cam(K, b);
  const double tau2 = tau * tau;
  double Rt[12];
  for (int e = 0; e < 12; ++e) Rt[e] = 0.0;
  bool ok = load_candidate(rec, b, Hyp, h, Rt);
  for (int it = 0; it < n_polish && ok; ++it) {          // (ok is the same in every lane: the control flow stays wave-uniform)
    double H[21], g[6];
    for (int e = 0; e < 21; ++e) H[e] = 0.0;
    for (int e = 0; e < 6; ++e) g[e] = 0.0;
    for (int i = lane; i < cnt; i += 64) {
      double P[3], p[2], r2;
      load_corr(X, x, static_cast<size_t>(b) * M + i, P, p);
      if (pnpm::reproj_r2(Rt, cam, P, p, &r2) && r2 < tau2) pnpm::gn_accumulate(Rt, cam, P, p, H, g);
    }
    for (int e = 0; e < 21; ++e) H[e] = wave_sum(H[e]);
    for (int e = 0; e < 6; ++e) g[e] = wave_sum(g[e]);
    double xi[6];
    ok = pnpm::chol6_solve(H, g, xi);
    if (ok) pnpm::se3_left_update(xi, Rt);
  }
  for (int e = 0; e < 12; ++e) ok = ok && pnpm::finite_d(Rt[e]);
  // the final inlier set and MSAC cost, under the final pose
  double s = 0.0;
  int ni = 0;
  for (int i = lane; i < cnt; i += 64) {
    double P[3], p[2], t = 0.0;
    bool in = false;
    if (ok) {
      load_corr(X, x, static_cast<size_t>(b) * M + i, P, p);
      in = pnpm::score_point(Rt, cam, P, p, tau2, &t);
    }
    inlier_mask[row * M + i] = in ? 1 : 0;
    ni += in ? 1 : 0;
    s += t;
  }
  s = wave_sum(s);
  ni = wave_sum_i(ni);
  if (lane < 16 && ok) {
    const int r = lane >> 2, c = lane & 3;
    T[16 * row + lane] = r < 3 ? static_cast<float>(Rt[4 * r + c]) : (c == 3 ? 1.f : 0.f);
  }
  if (lane == 0) {
    n_inliers[row] = ok ? ni : 0;
    final_cost[row] = ok ? s : inf_d();
    info[row] = ok ? 0 : -1;
    if (kPol)
      for (int e = 0; e < 12; ++e) pol[row * 12 + e] = Rt[e];
  }
}

__global__ __launch_bounds__(64) void pnp_polish_kernel(const float* __restrict__ X, const float* __restrict__ x, const int* __restrict__ count,
                                                       int M, const float* __restrict__ K, int B, int Hyp, double tau, int n_polish,
                                                       const HypRec* __restrict__ rec, const double* __restrict__ cost, float* __restrict__ T,
                                                       int* __restrict__ best, unsigned char* __restrict__ inlier_mask,
                                                       int* __restrict__ n_inliers, double* __restrict__ final_cost, int* __restrict__ info) {
  const int b = blockIdx.x, lane = threadIdx.x;
  // the cheapest hypothesis with a cost below +inf, the lowest h on a tie
  double bc = inf_d();
  int bh = -1;
  for (int h = lane; h < Hyp; h += 64) {
    const double c = cost[static_cast<size_t>(b) * Hyp + h];
    if (c < inf_d()) better_key(bc, bh, c, h);
  }
  for (int o = 32; o >= 1; o >>= 1) better_key(bc, bh, rp::shfl_xor_f64(bc, o), __shfl_xor(bh, o));
  if (lane == 0) best[b] = bh;
  polish_body<false>(X, x, count, M, K, b, tau, n_polish, rec, Hyp, bh, b, T, inlier_mask, n_inliers, final_cost, info, nullptr);
}

inline size_t workspace_bytes(int B, int Hyp) {
  if (B <= 0 || Hyp <= 0) return 0;
  return static_cast<size_t>(B) * Hyp * sizeof(HypRec);
}

}  // namespace pnp
