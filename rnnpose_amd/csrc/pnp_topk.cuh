// The K best DISTINCT hypotheses of the P3P RANSAC.  After pnp_solve_kernel and pnp_score_kernel (csrc/pnp.cuh):
//   pnp_topk_select_kernel  one workgroup per object: the extent of its correspondences, then Kt greedy rounds -- the cheapest live
//                           hypothesis (lowest h on a tie), then every hypothesis within `sep` of it dies
//   pnp_topk_polish_kernel  one wave per (object, slot): the polish body of pnp_polish_kernel (polish_body, csrc/pnp.cuh) on its hypothesis
//   pnp_topk_dup_kernel     one wave per object: slots whose POLISHED poses lie within `sep` of an earlier polished slot
// The distance of two poses is the largest displacement of a corner of the extent box.  Thread t of the selection owns the hypotheses
// h = t (mod 256) in every pass, so the live flags need no synchronisation; minima meet through the fixed xor butterfly and four LDS
// slots read in ascending wave order.  No atomics: two launches are bit-identical, and an object alone gives the bits it gives in a batch.
// Included by csrc/eval_metrics.hip after pnp.cuh (fma contraction is off there).
#pragma once
#include "pnp.cuh"

namespace pnp {

constexpr int kTopkMax = 16;
constexpr int kSelThreads = 256;

struct TopkBox {
  double lo[3], hi[3], sep, diag;
};

// max over the 8 corners c of [lo, hi] of |P c - Q c|; NaN as soon as one corner's displacement is NaN
__device__ __forceinline__ double pose_distance(const double* P, const double* Q, const double* lo, const double* hi) {
  double m = 0.0;
  for (int c = 0; c < 8; ++c) {
    const double cx = (c & 1) ? hi[0] : lo[0], cy = (c & 2) ? hi[1] : lo[1], cz = (c & 4) ? hi[2] : lo[2];
    double n2 = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double p = P[4 * r] * cx + P[4 * r + 1] * cy + P[4 * r + 2] * cz + P[4 * r + 3];
      const double q = Q[4 * r] * cx + Q[4 * r + 1] * cy + Q[4 * r + 2] * cz + Q[4 * r + 3];
      n2 += (p - q) * (p - q);
    }
    const double n = sqrt(n2);
    if (n > m || n != n) m = n;                          // (once m is NaN it stays: no later n compares greater)
  }
  return m;
}

__global__ __launch_bounds__(kSelThreads) void pnp_topk_select_kernel(const float* __restrict__ X, const int* __restrict__ count, int M, int Hyp,
                                                                     int Kt, double sep_frac, int min_inliers, const HypRec* __restrict__ rec,
                                                                     const double* __restrict__ cost, const int* __restrict__ inliers,
                                                                     unsigned char* __restrict__ live, TopkBox* __restrict__ box,
                                                                     int* __restrict__ hyp, int* __restrict__ n_found) {
  __shared__ double s_ext[4][6];
  __shared__ double s_cost[4];
  __shared__ int s_h[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = clamp_count(count, b, M);
  const size_t row = static_cast<size_t>(b) * Hyp;
  // the extent: min / max of the first cnt points (exact, whatever the order; the order is fixed all the same)
  double lo[3] = {inf_d(), inf_d(), inf_d()}, hi[3] = {-inf_d(), -inf_d(), -inf_d()};
  for (int i = tid; i < cnt; i += kSelThreads)
    for (int a = 0; a < 3; ++a) {
      const double v = static_cast<double>(X[(static_cast<size_t>(b) * M + i) * 3 + a]);
      lo[a] = v < lo[a] ? v : lo[a];
      hi[a] = v > hi[a] ? v : hi[a];
    }
  for (int o = 32; o >= 1; o >>= 1)
    for (int a = 0; a < 3; ++a) {
      const double ol = rp::shfl_xor_f64(lo[a], o), oh = rp::shfl_xor_f64(hi[a], o);
      lo[a] = ol < lo[a] ? ol : lo[a];
      hi[a] = oh > hi[a] ? oh : hi[a];
    }
  if (lane == 0)
    for (int a = 0; a < 3; ++a) {
      s_ext[wave][a] = lo[a];
      s_ext[wave][3 + a] = hi[a];
    }
  __syncthreads();
  for (int a = 0; a < 3; ++a) {
    lo[a] = s_ext[0][a];
    hi[a] = s_ext[0][3 + a];
    for (int w = 1; w < 4; ++w) {
      lo[a] = s_ext[w][a] < lo[a] ? s_ext[w][a] : lo[a];
      hi[a] = s_ext[w][3 + a] > hi[a] ? s_ext[w][3 + a] : hi[a];
    }
  }
  const double diag = sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
  const double sep = sep_frac * diag;
  if (tid == 0) {
    TopkBox* o = box + b;
    for (int a = 0; a < 3; ++a) {
      o->lo[a] = lo[a];
      o->hi[a] = hi[a];
    }
    o->sep = sep;
    o->diag = diag;
  }
  for (int h = tid; h < Hyp; h += kSelThreads) live[row + h] = cost[row + h] < inf_d() ? 1 : 0;      // slot 0: exactly pnp_polish_kernel's rule
  int found = 0;
  for (int k = 0; k < Kt; ++k) {
    double bc = inf_d();
    int bh = -1;
    for (int h = tid; h < Hyp; h += kSelThreads)
      if (live[row + h]) better_key(bc, bh, cost[row + h], h);
    for (int o = 32; o >= 1; o >>= 1) better_key(bc, bh, rp::shfl_xor_f64(bc, o), __shfl_xor(bh, o));
    __syncthreads();                                     // (the previous round's readers of s_cost / s_h are done)
    if (lane == 0) {
      s_cost[wave] = bc;
      s_h[wave] = bh;
    }
    __syncthreads();
    bc = s_cost[0];
    bh = s_h[0];
    for (int w = 1; w < 4; ++w) better_key(bc, bh, s_cost[w], s_h[w]);
    if (bh < 0) break;                                   // (the same in every thread)
    if (tid == 0) hyp[b * Kt + k] = bh;
    ++found;
    double P[12], Q[12];
    if (!load_candidate(rec, b, Hyp, bh, P))               // (a pick without a candidate: every distance to it is NaN)
      for (int e = 0; e < 12; ++e) P[e] = __longlong_as_double(0x7ff8000000000000ll);
    for (int h = tid; h < Hyp; h += kSelThreads) {
      if (!live[row + h]) continue;
      bool keep = load_candidate(rec, b, Hyp, h, Q);
      if (keep && k == 0) keep = pnpm::finite_d(cost[row + h]) && inliers[row + h] >= min_inliers;      // the gates of the slots k >= 1
      if (keep) keep = pose_distance(Q, P, lo, hi) > sep;  // must be TRUE: a NaN distance is never distinct; the pick itself has d = 0
      if (!keep) live[row + h] = 0;
    }
  }
  if (tid == 0) {
    for (int k = found; k < Kt; ++k) hyp[b * Kt + k] = -1;
    n_found[b] = found;
  }
}

// polish_body (csrc/pnp.cuh) on the hypothesis hyp[b][k] (-1: none), its outputs at (b, k); the polished pose also goes to `pol` in fp64
__global__ __launch_bounds__(64) void pnp_topk_polish_kernel(const float* __restrict__ X, const float* __restrict__ x, const int* __restrict__ count,
                                                            int M, const float* __restrict__ K, int Hyp, int Kt, double tau, int n_polish,
                                                            const HypRec* __restrict__ rec, const int* __restrict__ hyp, float* __restrict__ T,
                                                            unsigned char* __restrict__ inlier_mask, int* __restrict__ n_inliers,
                                                            double* __restrict__ final_cost, int* __restrict__ info, double* __restrict__ pol) {
  const int b = blockIdx.y;
  const size_t slot = static_cast<size_t>(b) * Kt + blockIdx.x;
  polish_body<true>(X, x, count, M, K, b, tau, n_polish, rec, Hyp, hyp[slot], slot, T, inlier_mask, n_inliers, final_cost, info, pol);
}

__global__ __launch_bounds__(64) void pnp_topk_dup_kernel(int Kt, const TopkBox* __restrict__ box, const double* __restrict__ pol,
                                                         const int* __restrict__ info, int* __restrict__ dup_of) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= Kt) return;
  const size_t base = static_cast<size_t>(b) * Kt;
  int dup = -1;
  if (info[base + k] == 0) {
    const TopkBox bx = box[b];
    double P[12];
    for (int e = 0; e < 12; ++e) P[e] = pol[(base + k) * 12 + e];
    for (int j = 0; j < k && dup < 0; ++j) {
      if (info[base + j] != 0) continue;
      double Q[12];
      for (int e = 0; e < 12; ++e) Q[e] = pol[(base + j) * 12 + e];
      if (!(pose_distance(P, Q, bx.lo, bx.hi) > bx.sep)) dup = j;
    }
  }
  dup_of[base + k] = dup;
}

// the candidates of every hypothesis | the polished fp64 poses | the extents | the live flags
inline size_t topk_live_offset(int B, int Hyp, int Kt) {
  return workspace_bytes(B, Hyp) + static_cast<size_t>(B) * Kt * 12 * sizeof(double) + static_cast<size_t>(B) * sizeof(TopkBox);
}

inline size_t topk_workspace_bytes(int B, int Hyp, int Kt) {
  if (B <= 0 || Hyp <= 0 || Kt < 1 || Kt > kTopkMax) return 0;
  return topk_live_offset(B, Hyp, Kt) + (static_cast<size_t>(B) * Hyp + 7) / 8 * 8;
}

}  // namespace pnp
