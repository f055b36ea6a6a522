// SURVEY.md section 8(f2,f3) "next" rows: the evaluator's per-sample metrics on device.
//   f3  brute-force nearest neighbour for ADD-S      thirdparty/nn/src/nearest_neighborhood.cu:48-163 (the only CUDA
//       kernel of the reference) + its cffi C ABI findNearestPointIdxLauncher (thirdparty/nn/src/ext.h:1-10)
//   f2  ADD / ADD-S / 2-D projection / 5cm-5deg       utils/eval_metric.py:28-37,102-192
// The reference kernel runs one thread per query with a serial loop over ALL reference points straight from global
// memory and re-mallocs / re-uploads every call.  Here reference points are staged through LDS in tiles shared by a
// 256-query workgroup (each reference point is read from HBM once per workgroup instead of once per thread), points
// stay device-resident, and the metric reductions happen in the same call.
// Semantics kept bit-exact for the index: strict '<' over ascending reference index (first minimum wins), fp32
// distance with the reference's operation order (no fma contraction).
#include "common.hpp"

#include <cfloat>
#include <cstdio>
#include <cstring>

#pragma clang fp contract(off)

// the pose initialiser: descriptor matcher and P3P RANSAC.  Their kernels live in headers of their own; the entry
// points are at the end of this file, so that the host-executed test tier (which builds a fixed list of sources) carries them too.
#include "desc_match.cuh"
#include "pnp.cuh"
#include "pnp_topk.cuh"
// the pose confidence, placed the same way
#include "pose_score.cuh"
// object onboarding: exact diameter and farthest-point sampling, placed the same way
#include "model_prep.cuh"

namespace {

constexpr int NN_TILE = 1024;

template <int DIM>
__global__ __launch_bounds__(256) void nn_search_kernel(const float* __restrict__ ref, const float* __restrict__ que,
                                                        int* __restrict__ idxs, int pn1, int pn2, int exclude_self) {
  __shared__ float tile[NN_TILE * DIM];
  const int bi = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;
  const bool live = q < pn2;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    const float* p = que + (static_cast<long long>(bi) * pn2 + q) * DIM;
    qx = p[0];
    qy = p[1];
    if (DIM == 3) qz = p[2];
  }
  float best = FLT_MAX;
  int best_i = 0;
  const float* rb = ref + static_cast<long long>(bi) * pn1 * DIM;
  for (int t0 = 0; t0 < pn1; t0 += NN_TILE) {
    const int n = min(NN_TILE, pn1 - t0);
    __syncthreads();
    for (int e = threadIdx.x; e < n * DIM; e += 256) tile[e] = rb[static_cast<long long>(t0) * DIM + e];
    __syncthreads();
    if (live) {
      for (int j = 0; j < n; ++j) {
        const int p1i = t0 + j;
        if (exclude_self && p1i == q) continue;
        const float dx = tile[j * DIM + 0] - qx, dy = tile[j * DIM + 1] - qy;
        float d = dx * dx + dy * dy;
        if (DIM == 3) {
          const float dz = tile[j * DIM + 2] - qz;
          d = d + dz * dz;
        }
        if (d < best) {
          best = d;
          best_i = p1i;
        }
      }
    }
  }
  if (live) idxs[static_cast<long long>(bi) * pn2 + q] = best_i;
}

// model (P,3) fp32, pose (B,3,4) fp32 -> pts (B,P,3) fp32 = float(R x + t computed in fp64)   (eval_metric.py:117-119)
__global__ __launch_bounds__(256) void transform_points_kernel(const float* __restrict__ model, const float* __restrict__ pose,
                                                               float* __restrict__ pts, int P) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float* T = pose + 12 * b;
  const double x = model[3 * i], y = model[3 * i + 1], z = model[3 * i + 2];
  float* o = pts + (static_cast<long long>(b) * P + i) * 3;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o[r] = static_cast<float>(static_cast<double>(T[4 * r]) * x + static_cast<double>(T[4 * r + 1]) * y +
                              static_cast<double>(T[4 * r + 2]) * z + static_cast<double>(T[4 * r + 3]));
}

__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int d = 32; d >= 1; d >>= 1) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_down(lo, d);
    hi = __shfl_down(hi, d);
    v += __hiloint2double(hi, lo);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < 4; ++w) s += red[w];
  return s;
}

// one workgroup per sample -> out (B,5) fp64: [ADD mean distance, ADD-S mean distance (or -1), mean 2-D projection
// error (px), translation error (cm), rotation error (deg)]
__global__ __launch_bounds__(256) void pose_metrics_kernel(const float* __restrict__ model, int P,
                                                           const float* __restrict__ pose_pred,
                                                           const float* __restrict__ pose_gt, const float* __restrict__ K,
                                                           const float* __restrict__ pts_pred, const float* __restrict__ pts_gt,
                                                           const int* __restrict__ nn_idx, double* __restrict__ out) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  const float* Tp = pose_pred + 12 * b;
  const float* Tg = pose_gt + 12 * b;
  double add = 0.0, adds = 0.0, proj = 0.0;
  for (int i = threadIdx.x; i < P; i += 256) {
    const double x = model[3 * i], y = model[3 * i + 1], z = model[3 * i + 2];
    double pp[3], pg[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      pp[r] = static_cast<double>(Tp[4 * r]) * x + static_cast<double>(Tp[4 * r + 1]) * y + static_cast<double>(Tp[4 * r + 2]) * z + static_cast<double>(Tp[4 * r + 3]);
      pg[r] = static_cast<double>(Tg[4 * r]) * x + static_cast<double>(Tg[4 * r + 1]) * y + static_cast<double>(Tg[4 * r + 2]) * z + static_cast<double>(Tg[4 * r + 3]);
    }
    add += sqrt((pp[0] - pg[0]) * (pp[0] - pg[0]) + (pp[1] - pg[1]) * (pp[1] - pg[1]) + (pp[2] - pg[2]) * (pp[2] - pg[2]));
    // project(): xyz K^T, divide by z (eval_metric.py:34-36)
    double up[3], ug[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      up[r] = static_cast<double>(K[3 * r]) * pp[0] + static_cast<double>(K[3 * r + 1]) * pp[1] + static_cast<double>(K[3 * r + 2]) * pp[2];
      ug[r] = static_cast<double>(K[3 * r]) * pg[0] + static_cast<double>(K[3 * r + 1]) * pg[1] + static_cast<double>(K[3 * r + 2]) * pg[2];
    }
    const double ex = up[0] / up[2] - ug[0] / ug[2], ey = up[1] / up[2] - ug[1] / ug[2];
    proj += sqrt(ex * ex + ey * ey);
    if (nn_idx) {   // ADD-S: nearest PREDICTED point of every TARGET point (eval_metric.py:121-125)
      const float* a = pts_pred + (static_cast<long long>(b) * P + nn_idx[static_cast<long long>(b) * P + i]) * 3;
      const float* g = pts_gt + (static_cast<long long>(b) * P + i) * 3;
      const double dx = static_cast<double>(a[0]) - g[0], dy = static_cast<double>(a[1]) - g[1], dz = static_cast<double>(a[2]) - g[2];
      adds += sqrt(dx * dx + dy * dy + dz * dz);
    }
  }
  add = block_sum(add, red);
  proj = block_sum(proj, red);
  adds = block_sum(adds, red);
  if (threadIdx.x == 0) {
    const double tx = static_cast<double>(Tp[3]) - Tg[3], ty = static_cast<double>(Tp[7]) - Tg[7], tz = static_cast<double>(Tp[11]) - Tg[11];
    double tr = 0.0;                                             // trace(R_pred R_gt^T)   (eval_metric.py:183-186)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) tr += static_cast<double>(Tp[4 * r + c]) * Tg[4 * r + c];
    if (tr > 3.0) tr = 3.0;
    out[5 * b + 0] = add / P;
    out[5 * b + 1] = nn_idx ? adds / P : -1.0;
    out[5 * b + 2] = proj / P;
    out[5 * b + 3] = sqrt(tx * tx + ty * ty + tz * tz) * 100.0;
    out[5 * b + 4] = acos((tr - 1.0) / 2.0) * (180.0 / 3.14159265358979323846);
  }
}

// max over the workgroup with a NaN that sticks (np.max semantics): the shape of block_sum
__device__ __forceinline__ double nan_max(double m, double v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ double block_max(double v, double* red) {
  for (int d = 32; d >= 1; d >>= 1) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_down(lo, d);
    hi = __shfl_down(hi, d);
    v = nan_max(v, __hiloint2double(hi, lo));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double m = red[0];
  for (int w = 1; w < 4; ++w) m = nan_max(m, red[w]);
  return m;
}

// ---- BOP pose-error functions (Hodan et al., BOP challenge 2019/2020): MSSD / MSPD and VSD -----------------------------------
// MSSD = min_s max_i |T_est x_i - T_gt S_s x_i|, MSPD the same with both points projected by the sample's K.
// One workgroup per (s, b): T_gt S_s is formed once (12 threads -> LDS), the threads stride over the P model points, block max of
// both distances -> partial (B,S,2).  No atomics: bop_sym_min_kernel takes the min over S.
__global__ __launch_bounds__(256) void bop_sym_dist_kernel(const float* __restrict__ model, int P, const float* __restrict__ sym, int S,
                                                           const float* __restrict__ pose_est, const float* __restrict__ pose_gt,
                                                           const float* __restrict__ K, double* __restrict__ partial) {
  __shared__ double M[12];
  __shared__ double red[4];
  const int s = blockIdx.x, b = blockIdx.y;
  const float* Te = pose_est + 12 * b;
  if (threadIdx.x < 12) {
    const float* Tg = pose_gt + 12 * b;
    const float* Ss = sym + 12 * static_cast<long long>(s);
    const int r = threadIdx.x >> 2, c = threadIdx.x & 3;
    double v = static_cast<double>(Tg[4 * r]) * Ss[c] + static_cast<double>(Tg[4 * r + 1]) * Ss[4 + c] + static_cast<double>(Tg[4 * r + 2]) * Ss[8 + c];
    if (c == 3) v = v + static_cast<double>(Tg[4 * r + 3]);
    M[threadIdx.x] = v;
  }
  __syncthreads();
  const double fx = K[9 * b], cx = K[9 * b + 2], fy = K[9 * b + 4], cy = K[9 * b + 5];
  double m3 = 0.0, m2 = 0.0;
  for (int i = threadIdx.x; i < P; i += 256) {
    const double x = model[3 * i], y = model[3 * i + 1], z = model[3 * i + 2];
    double pe[3], pg[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      pe[r] = static_cast<double>(Te[4 * r]) * x + static_cast<double>(Te[4 * r + 1]) * y + static_cast<double>(Te[4 * r + 2]) * z + static_cast<double>(Te[4 * r + 3]);
      pg[r] = M[4 * r] * x + M[4 * r + 1] * y + M[4 * r + 2] * z + M[4 * r + 3];
    }
    const double dx = pe[0] - pg[0], dy = pe[1] - pg[1], dz = pe[2] - pg[2];
    m3 = nan_max(m3, sqrt(dx * dx + dy * dy + dz * dz));
    const double ex = (fx * pe[0] / pe[2] + cx) - (fx * pg[0] / pg[2] + cx), ey = (fy * pe[1] / pe[2] + cy) - (fy * pg[1] / pg[2] + cy);
    m2 = nan_max(m2, sqrt(ex * ex + ey * ey));
  }
  m3 = block_max(m3, red);
  m2 = block_max(m2, red);
  if (threadIdx.x == 0) {
    double* o = partial + (static_cast<long long>(b) * S + s) * 2;
    o[0] = m3;
    o[1] = m2;
  }
}

__global__ __launch_bounds__(256) void bop_sym_min_kernel(const double* __restrict__ partial, int B, int S, double* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double* p = partial + static_cast<long long>(b) * S * 2;
  double m3 = p[0], m2 = p[1];
  for (int s = 1; s < S; ++s) {
    const double a = p[2 * s], c = p[2 * s + 1];
    m3 = (a < m3 || a != a) ? a : m3;
    m2 = (c < m2 || c != c) ? c : m2;
  }
  out[2 * b] = m3;
  out[2 * b + 1] = m2;
}

// VSD.  Every workgroup takes BOP_TILE consecutive pixels of one sample: pixel = tile start + k * 256 + thread, so the lanes of a
// wave read 64 consecutive floats of each of the three depth images.  Per thread 2 + NT int32 counters [union, inter, n_tau...],
// reduced by wave shuffles, then LDS, then ONE partial record per workgroup; bop_vsd_finalize_kernel sums the records in int64.
constexpr int BOP_TILE = 2048;
constexpr int BOP_MAX_NT = 16;
constexpr int BOP_NC = 2 + BOP_MAX_NT;

struct BopTaus {
  double v[BOP_MAX_NT];
};

__global__ __launch_bounds__(256) void bop_vsd_kernel(const float* __restrict__ depth_est, const float* __restrict__ depth_gt,
                                                      const float* __restrict__ depth_obs, int S_obs, const int* __restrict__ src_index,
                                                      const float* __restrict__ K, const float* __restrict__ diameter, int H, int W,
                                                      double delta, BopTaus taus, int NT, int* __restrict__ partial) {
  __shared__ int red[4][BOP_NC];
  const int b = blockIdx.y;
  const int src = src_index[b];
  const int HW = H * W;
  int cnt[BOP_NC];
#pragma unroll
  for (int c = 0; c < BOP_NC; ++c) cnt[c] = 0;
  if (src >= 0 && src < S_obs) {          // (a sample whose index is out of range counts nothing: the finalize writes NaN errors)
    const float* pe = depth_est + static_cast<long long>(b) * HW;
    const float* pg = depth_gt + static_cast<long long>(b) * HW;
    const float* po = depth_obs + static_cast<long long>(src) * HW;
    const double fx = K[9 * b], cx = K[9 * b + 2], fy = K[9 * b + 4], cy = K[9 * b + 5];
    const double diam = diameter[b];
    const bool normalise = diam > 0.0;
    const int p0 = blockIdx.x * BOP_TILE + threadIdx.x;
    for (int k = 0; k < BOP_TILE / 256; ++k) {
      const int p = p0 + k * 256;
      if (p >= HW) break;
      const float fe = pe[p], fg = pg[p], fo = po[p];
      const int v = p / W, u = p - v * W;
      const double rx = (u - cx) / fx, ry = (v - cy) / fy;
      const double ray = sqrt(rx * rx + ry * ry + 1.0);
      const double de = static_cast<double>(fe) * ray, dg = static_cast<double>(fg) * ray, dob = static_cast<double>(fo) * ray;
      const bool empty_e = !(fe > 0.f), empty_g = !(fg > 0.f);
      const bool missing = !(fo > 0.f) || !(fabsf(fo) <= FLT_MAX);
      const bool vis_g = !empty_g && (missing || dg - dob <= delta);
      const bool vis_e = (!empty_e && (missing || de - dob <= delta)) || (vis_g && !empty_e);
      const bool inter = vis_g && vis_e;
      cnt[0] += (vis_g || vis_e) ? 1 : 0;
      cnt[1] += inter ? 1 : 0;
      double e = fabs(dg - de);
      if (normalise) e = e / diam;
#pragma unroll
      for (int t = 0; t < BOP_MAX_NT; ++t) cnt[2 + t] += (t < NT && inter && e >= taus.v[t]) ? 1 : 0;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < BOP_NC; ++c) {
    int x = cnt[c];
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d);
    if (lane == 0) red[wave][c] = x;
  }
  __syncthreads();
  if (threadIdx.x < 2 + NT)
    partial[(static_cast<long long>(b) * gridDim.x + blockIdx.x) * (2 + NT) + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// one workgroup per sample: thread c < 2 + NT sums counter c over the sample's records (int64), then err_tau of the definitions
__global__ __launch_bounds__(64) void bop_vsd_finalize_kernel(const int* __restrict__ partial, int nblk, int S_obs,
                                                              const int* __restrict__ src_index, int NT, long long* __restrict__ counts,
                                                              double* __restrict__ err) {
  __shared__ long long tot[BOP_NC];
  const int b = blockIdx.x, c = threadIdx.x;
  const int src = src_index[b];
  const bool ok = src >= 0 && src < S_obs;
  if (c < 2 + NT) {
    long long s = 0;
    const int* p = partial + static_cast<long long>(b) * nblk * (2 + NT) + c;
    if (ok)
      for (int k = 0; k < nblk; ++k) s += p[static_cast<long long>(k) * (2 + NT)];
    tot[c] = s;
    counts[static_cast<long long>(b) * (2 + NT) + c] = s;
  }
  __syncthreads();
  if (c < NT) {
    double e = 1.0;
    if (!ok)
      e = __longlong_as_double(0x7ff8000000000000ll);
    else if (tot[0] > 0)
      e = static_cast<double>(tot[2 + c] + tot[0] - tot[1]) / static_cast<double>(tot[0]);
    err[static_cast<long long>(b) * NT + c] = e;
  }
}

int launch_nn(const float* ref, const float* que, int* idxs, int b, int pn1, int pn2, int dim, int exclude_self,
              hipStream_t st) {
  dim3 grid(rp::cdiv(pn2, 256), b), block(256);
  if (dim == 3)
    hipLaunchKernelGGL(nn_search_kernel<3>, grid, block, 0, st, ref, que, idxs, pn1, pn2, exclude_self);
  else
    hipLaunchKernelGGL(nn_search_kernel<2>, grid, block, 0, st, ref, que, idxs, pn1, pn2, exclude_self);
  return 0;
}

}  // namespace

extern "C" {

int rnnpose_nn_search_f32(const float* ref_pts, const float* que_pts, int* idxs, int b, int pn1, int pn2, int dim,
                          int exclude_self, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_nn_search_f32";
  RP_REQUIRE(ref_pts && que_pts && idxs, fn, "null pointer");
  RP_REQUIRE(b > 0 && b < 65536 && pn1 > 0 && pn2 > 0 && (dim == 2 || dim == 3), fn, "bad size (dim must be 2 or 3)");
  launch_nn(ref_pts, que_pts, idxs, b, pn1, pn2, dim, exclude_self, rp::as_stream(stream));
  return rp::check_launch(fn);
}

size_t rnnpose_pose_metrics_workspace_bytes(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return static_cast<size_t>(B) * P * (2 * 3 * sizeof(float) + sizeof(int));
}

int rnnpose_pose_metrics_f64(const float* model, int P, const float* pose_pred, const float* pose_gt, const float* K, int B,
                             int symmetric, void* workspace, size_t workspace_bytes, double* out, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_pose_metrics_f64";
  RP_REQUIRE(model && pose_pred && pose_gt && K && out, fn, "null pointer");
  RP_REQUIRE(B > 0 && B < 65536 && P > 0, fn, "bad size");
  hipStream_t st = rp::as_stream(stream);
  float *pp = nullptr, *pg = nullptr;
  int* idx = nullptr;
  if (symmetric) {
    RP_REQUIRE(workspace && workspace_bytes >= rnnpose_pose_metrics_workspace_bytes(B, P), fn, "workspace too small");
    pp = static_cast<float*>(workspace);
    pg = pp + static_cast<size_t>(B) * P * 3;
    idx = reinterpret_cast<int*>(pg + static_cast<size_t>(B) * P * 3);
    hipLaunchKernelGGL(transform_points_kernel, dim3(rp::cdiv(P, 256), B), dim3(256), 0, st, model, pose_pred, pp, P);
    hipLaunchKernelGGL(transform_points_kernel, dim3(rp::cdiv(P, 256), B), dim3(256), 0, st, model, pose_gt, pg, P);
    launch_nn(pp, pg, idx, B, P, P, 3, 0, st);      // ref = predicted points, queries = target points
  }
  hipLaunchKernelGGL(pose_metrics_kernel, dim3(B), dim3(256), 0, st, model, P, pose_pred, pose_gt, K, pp, pg, idx, out);
  return rp::check_launch(fn);
}

size_t rnnpose_bop_sym_dist_workspace_bytes(int B, int S) {
  if (B <= 0 || S <= 0) return 0;
  return static_cast<size_t>(B) * S * 2 * sizeof(double);
}

int rnnpose_bop_sym_dist_f64(const float* model, int P, const float* sym, int S, const float* pose_est, const float* pose_gt,
                             const float* K, int B, void* workspace, size_t workspace_bytes, double* out, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_bop_sym_dist_f64";
  RP_REQUIRE(model && sym && pose_est && pose_gt && K && workspace && out, fn, "null pointer");
  RP_REQUIRE(S >= 1, fn, "S < 1: an object without symmetries passes the identity");
  RP_REQUIRE(B > 0 && B < 65536 && P > 0, fn, "bad size");
  RP_REQUIRE(workspace_bytes >= rnnpose_bop_sym_dist_workspace_bytes(B, S), fn, "workspace too small");
  hipStream_t st = rp::as_stream(stream);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(bop_sym_dist_kernel, dim3(S, B), dim3(256), 0, st, model, P, sym, S, pose_est, pose_gt, K, partial);
  hipLaunchKernelGGL(bop_sym_min_kernel, dim3(rp::cdiv(B, 256)), dim3(256), 0, st, partial, B, S, out);
  return rp::check_launch(fn);
}

size_t rnnpose_bop_vsd_workspace_bytes(int B, int H, int W, int NT) {
  if (B <= 0 || H <= 0 || W <= 0 || NT < 1 || NT > BOP_MAX_NT || static_cast<long long>(H) * W > 0x7fffffffll - BOP_TILE) return 0;
  return static_cast<size_t>(B) * rp::cdiv(static_cast<long long>(H) * W, BOP_TILE) * (2 + NT) * sizeof(int);
}

int rnnpose_bop_vsd_f64(const float* depth_est, const float* depth_gt, const float* depth_obs, int S_obs, const int* src_index,
                        const float* K, const float* diameter, int B, int H, int W, double delta, const double* taus, int NT,
                        void* workspace, size_t workspace_bytes, long long* counts, double* err, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_bop_vsd_f64";
  RP_REQUIRE(depth_est && depth_gt && depth_obs && src_index && K && diameter && taus && workspace && counts && err, fn, "null pointer");
  RP_REQUIRE(NT >= 1 && NT <= BOP_MAX_NT, fn, "NT must lie in [1, 16]");
  RP_REQUIRE(B > 0 && B < 65536 && H > 0 && W > 0 && S_obs > 0 && static_cast<long long>(H) * W <= 0x7fffffffll - BOP_TILE, fn, "bad size");
  RP_REQUIRE(workspace_bytes >= rnnpose_bop_vsd_workspace_bytes(B, H, W, NT), fn, "workspace too small");
  hipStream_t st = rp::as_stream(stream);
  BopTaus tv;
  for (int t = 0; t < BOP_MAX_NT; ++t) tv.v[t] = t < NT ? taus[t] : 0.0;
  const int nblk = rp::cdiv(static_cast<long long>(H) * W, BOP_TILE);
  int* partial = static_cast<int*>(workspace);
  hipLaunchKernelGGL(bop_vsd_kernel, dim3(nblk, B), dim3(256), 0, st, depth_est, depth_gt, depth_obs, S_obs, src_index, K, diameter, H, W,
                     delta, tv, NT, partial);
  hipLaunchKernelGGL(bop_vsd_finalize_kernel, dim3(B), dim3(64), 0, st, static_cast<const int*>(partial), nblk, S_obs, src_index, NT, counts, err);
  return rp::check_launch(fn);
}

// Drop-in for the reference's cffi symbol (thirdparty/nn/src/ext.h:1-10): HOST buffers, synchronous.  The reference
// exit()s on any CUDA error; this one reports on stderr and fills idxs with -1.
void findNearestPointIdxLauncher(float* ref_pts, float* que_pts, int* idxs, int b, int pn1, int pn2, int dim, int exclude_self) {
  const size_t nr = static_cast<size_t>(b) * pn1 * dim * sizeof(float), nq = static_cast<size_t>(b) * pn2 * dim * sizeof(float);
  const size_t ni = static_cast<size_t>(b) * pn2 * sizeof(int);
  float *dr = nullptr, *dq = nullptr;
  int* di = nullptr;
  hipError_t e = hipSuccess;
  bool ok = b > 0 && pn1 > 0 && pn2 > 0 && (dim == 2 || dim == 3) && ref_pts && que_pts && idxs;
  if (ok) ok = (e = hipMalloc(reinterpret_cast<void**>(&dr), nr)) == hipSuccess;
  if (ok) ok = (e = hipMalloc(reinterpret_cast<void**>(&dq), nq)) == hipSuccess;
  if (ok) ok = (e = hipMalloc(reinterpret_cast<void**>(&di), ni)) == hipSuccess;
  if (ok) ok = (e = hipMemcpy(dr, ref_pts, nr, hipMemcpyHostToDevice)) == hipSuccess;
  if (ok) ok = (e = hipMemcpy(dq, que_pts, nq, hipMemcpyHostToDevice)) == hipSuccess;
  if (ok) {
    launch_nn(dr, dq, di, b, pn1, pn2, dim, exclude_self, nullptr);
    ok = (e = hipGetLastError()) == hipSuccess;
  }
  if (ok) ok = (e = hipMemcpy(idxs, di, ni, hipMemcpyDeviceToHost)) == hipSuccess;
  if (!ok) {
    fprintf(stderr, "findNearestPointIdxLauncher: %s\n", e == hipSuccess ? "invalid argument" : hipGetErrorString(e));
    if (idxs && b > 0 && pn2 > 0) memset(idxs, 0xff, ni);
  }
  if (dr) (void)hipFree(dr);
  if (dq) (void)hipFree(dq);
  if (di) (void)hipFree(di);
}

// ---- pose initialiser: descriptor matcher + P3P RANSAC (csrc/desc_match.cuh, csrc/pnp.cuh) ---------------------------------------
size_t rnnpose_desc_match_workspace_bytes(int total_points, int B, int H, int W, int step) {
  return dm::workspace_bytes(total_points, B, H, W, step);
}

int rnnpose_desc_match_f32(const float* desc3d, const float* points, const int* pt_off, int total_points, int max_points,
                           const float* desc2d, int S, int D, int H, int W, const int* src_index, const int* bbox, int B, int step,
                           float min_sim, int mutual, float pixel_center, int M, void* workspace, size_t workspace_bytes, float* X,
                           float* x, float* sim, int* point_idx, int* count, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_desc_match_f32";
  RP_REQUIRE(desc3d && points && pt_off && desc2d && src_index && bbox && workspace && X && x && sim && point_idx && count, fn, "null pointer");
  RP_REQUIRE(D == dm::kD, fn, "D must be 32");
  RP_REQUIRE(B > 0 && B < 65536 && S > 0 && H > 0 && W > 0 && total_points > 0 && max_points > 0 && max_points <= total_points && M > 0, fn,
             "bad size");
  RP_REQUIRE(static_cast<long long>(H) * W < (1ll << 31) && static_cast<long long>(B) * M < (1ll << 31), fn, "bad size (too large)");
  RP_REQUIRE(step >= 1, fn, "step must be >= 1");
  RP_REQUIRE(mutual == 0 || mutual == 1, fn, "mutual must be 0 or 1");
  RP_REQUIRE(reinterpret_cast<uintptr_t>(desc3d) % 16 == 0 && reinterpret_cast<uintptr_t>(workspace) % 8 == 0, fn,
             "desc3d must be 16-byte aligned, workspace 8-byte aligned");
  RP_REQUIRE(workspace_bytes >= dm::workspace_bytes(total_points, B, H, W, step), fn, "workspace too small");
  const int cap = dm::pixel_capacity(H, W, step);
  RP_REQUIRE(rp::cdiv(cap, dm::kFwdChunk) < 65536 && rp::cdiv(max_points, dm::kBwdChunk) < 65536, fn, "bad size (too large)");
  hipStream_t st = rp::as_stream(stream);
  unsigned long long* fwd = static_cast<unsigned long long*>(workspace);
  unsigned long long* bwd = fwd + total_points;
  const size_t nkeys = static_cast<size_t>(total_points) + static_cast<size_t>(B) * cap;
  hipLaunchKernelGGL(dm::dm_clear_kernel, dim3(rp::cdiv(nkeys, 256)), dim3(256), 0, st, fwd, nkeys);
  hipLaunchKernelGGL(dm::dm_forward_kernel, dim3(rp::cdiv(max_points, 256), rp::cdiv(cap, dm::kFwdChunk), B), dim3(256), 0, st, desc3d, pt_off,
                     total_points, max_points, desc2d, S, H, W, src_index, bbox, step, fwd);
  hipLaunchKernelGGL(dm::dm_backward_kernel, dim3(rp::cdiv(cap, 256), rp::cdiv(max_points, dm::kBwdChunk), B), dim3(256), 0, st, desc3d, pt_off,
                     total_points, max_points, desc2d, S, H, W, src_index, bbox, step, cap, bwd);
  hipLaunchKernelGGL(dm::dm_select_kernel, dim3(B), dim3(256), 0, st, points, pt_off, total_points, max_points, S, H, W, src_index, bbox, step,
                     cap, min_sim, mutual, pixel_center, M, fwd, bwd, X, x, sim, point_idx, count);
  return rp::check_launch(fn);
}

// The argument checks both RANSAC entry points make, in their order; Kt = 1 for the single pose.  -> 0, or 1 with the error set for `fn`.
static int pnp_check_args(const char* fn, bool pointers, int B, int M, int Hyp, int Kt, double tau, int n_polish, int min_count) {
  RP_REQUIRE(pointers, fn, "null pointer");
  RP_REQUIRE(B > 0 && B < 65536 && M > 0 && Hyp > 0 && Hyp <= (1 << 22), fn, "bad size");
  RP_REQUIRE(Kt >= 1 && Kt <= pnp::kTopkMax, fn, "Kt must lie in [1, 16]");
  RP_REQUIRE(static_cast<long long>(B) * M * Kt < (1ll << 31), fn, "bad size (too large)");
  RP_REQUIRE(tau > 0.0 && tau - tau == 0.0, fn, "tau must be positive and finite");
  RP_REQUIRE(n_polish >= 0 && n_polish <= 64, fn, "n_polish must lie in [0, 64]");
  RP_REQUIRE(min_count >= 4, fn, "min_count must be >= 4");
  return 0;
}

// The minimal solves and their scores: the head of the workspace holds every hypothesis's candidates afterwards.
static pnp::HypRec* pnp_solve_and_score(const float* X, const float* x, const int* count, int M, const float* K, const unsigned* rnd, int B, int Hyp,
                                        double tau, int min_count, void* workspace, double* cost, int* inliers, hipStream_t st) {
  pnp::HypRec* rec = static_cast<pnp::HypRec*>(workspace);
  hipLaunchKernelGGL(pnp::pnp_solve_kernel, dim3(rp::cdiv(Hyp, 64), B), dim3(64), 0, st, X, x, count, M, K, rnd, B, Hyp, min_count, rec);
  hipLaunchKernelGGL(pnp::pnp_score_kernel, dim3(rp::cdiv(Hyp, 4), B), dim3(256), 0, st, X, x, count, M, K, B, Hyp, tau, rec, cost, inliers);
  return rec;
}

size_t rnnpose_pnp_ransac_workspace_bytes(int B, int Hyp) { return pnp::workspace_bytes(B, Hyp); }

int rnnpose_pnp_ransac_f64(const float* X, const float* x, const int* count, int M, const float* K, const unsigned* rnd, int B, int Hyp,
                           double tau, int n_polish, int min_count, void* workspace, size_t workspace_bytes, float* T, double* cost,
                           int* inliers, int* best, unsigned char* inlier_mask, int* n_inliers, double* final_cost, int* info,
                           rnnpose_stream_t stream) {
  const char* fn = "rnnpose_pnp_ransac_f64";
  if (pnp_check_args(fn, X && x && count && K && rnd && workspace && T && cost && inliers && best && inlier_mask && n_inliers && final_cost && info,
                     B, M, Hyp, 1, tau, n_polish, min_count))
    return 1;
  RP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, fn, "workspace must be 8-byte aligned");
  RP_REQUIRE(workspace_bytes >= pnp::workspace_bytes(B, Hyp), fn, "workspace too small");
  hipStream_t st = rp::as_stream(stream);
  pnp::HypRec* rec = pnp_solve_and_score(X, x, count, M, K, rnd, B, Hyp, tau, min_count, workspace, cost, inliers, st);
  hipLaunchKernelGGL(pnp::pnp_polish_kernel, dim3(B), dim3(64), 0, st, X, x, count, M, K, B, Hyp, tau, n_polish, rec, cost, T, best, inlier_mask,
                     n_inliers, final_cost, info);
  return rp::check_launch(fn);
}

// ---- pose confidence: render-and-compare score of a pose against its frame (csrc/pose_score.cuh) ----------------------------------------
size_t rnnpose_pose_score_workspace_bytes(int B, int h, int w) { return ps::workspace_bytes(B, h, w); }

int rnnpose_pose_score_f64(const float* rend_depth, const float* rend_desc, const int* window, const float* desc2d, const float* depth_obs,
                           const int* src_index, int B, int S, int D, int h, int w, int H, int W, double depth_tol, void* workspace,
                           size_t workspace_bytes, double* stats, double* score, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_pose_score_f64";
  RP_REQUIRE(rend_depth && rend_desc && window && desc2d && src_index && workspace && stats && score, fn, "null pointer");
  RP_REQUIRE(D == ps::kD, fn, "D must be 32");
  RP_REQUIRE(B > 0 && S > 0 && h > 0 && w > 0 && H > 0 && W > 0, fn, "bad size");
  RP_REQUIRE(static_cast<long long>(H) * W < (1ll << 31) && ps::workspace_bytes(B, h, w) > 0, fn, "bad size (too large)");
  RP_REQUIRE(depth_tol >= 0.0 && depth_tol - depth_tol == 0.0, fn, "depth_tol must be non-negative and finite");
  RP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, fn, "workspace must be 8-byte aligned");
  RP_REQUIRE(workspace_bytes >= ps::workspace_bytes(B, h, w), fn, "workspace too small");
  hipStream_t st = rp::as_stream(stream);
  const int nchunk = ps::chunks(h, w);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(ps::ps_partial_kernel, dim3(B * nchunk), dim3(256), 0, st, rend_depth, rend_desc, window, desc2d, depth_obs, src_index, S, h,
                     w, H, W, nchunk, depth_tol, partial);
  hipLaunchKernelGGL(ps::ps_final_kernel, dim3(B), dim3(64), 0, st, static_cast<const double*>(partial), nchunk, stats, score);
  return rp::check_launch(fn);
}

// ---- the K best distinct RANSAC hypotheses, each polished (csrc/pnp_topk.cuh) --------------------------------------------------------------
size_t rnnpose_pnp_ransac_topk_workspace_bytes(int B, int Hyp, int Kt) { return pnp::topk_workspace_bytes(B, Hyp, Kt); }

int rnnpose_pnp_ransac_topk_f64(const float* X, const float* x, const int* count, int M, const float* K, const unsigned* rnd, int B, int Hyp,
                                double tau, int n_polish, int min_count, int Kt, double sep_frac, int min_inliers, void* workspace,
                                size_t workspace_bytes, float* T, double* cost, int* inliers, int* hyp, unsigned char* inlier_mask,
                                int* n_inliers, double* final_cost, int* info, int* dup_of, int* n_found, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_pnp_ransac_topk_f64";
  if (pnp_check_args(fn, X && x && count && K && rnd && workspace && T && cost && inliers && hyp && inlier_mask && n_inliers && final_cost && info &&
                             dup_of && n_found,
                     B, M, Hyp, Kt, tau, n_polish, min_count))
    return 1;
  RP_REQUIRE(sep_frac >= 0.0 && sep_frac - sep_frac == 0.0, fn, "sep_frac must be non-negative and finite");
  RP_REQUIRE(min_inliers >= 0, fn, "min_inliers must be >= 0");
  RP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, fn, "workspace must be 8-byte aligned");
  RP_REQUIRE(workspace_bytes >= pnp::topk_workspace_bytes(B, Hyp, Kt), fn, "workspace too small");
  hipStream_t st = rp::as_stream(stream);
  pnp::HypRec* rec = pnp_solve_and_score(X, x, count, M, K, rnd, B, Hyp, tau, min_count, workspace, cost, inliers, st);
  double* pol = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + pnp::workspace_bytes(B, Hyp));
  pnp::TopkBox* box = reinterpret_cast<pnp::TopkBox*>(pol + static_cast<size_t>(B) * Kt * 12);
  unsigned char* live = static_cast<unsigned char*>(workspace) + pnp::topk_live_offset(B, Hyp, Kt);
  hipLaunchKernelGGL(pnp::pnp_topk_select_kernel, dim3(B), dim3(pnp::kSelThreads), 0, st, X, count, M, Hyp, Kt, sep_frac, min_inliers,
                     static_cast<const pnp::HypRec*>(rec), static_cast<const double*>(cost), static_cast<const int*>(inliers), live, box, hyp, n_found);
  hipLaunchKernelGGL(pnp::pnp_topk_polish_kernel, dim3(Kt, B), dim3(64), 0, st, X, x, count, M, K, Hyp, Kt, tau, n_polish,
                     static_cast<const pnp::HypRec*>(rec), static_cast<const int*>(hyp), T, inlier_mask, n_inliers, final_cost, info, pol);
  hipLaunchKernelGGL(pnp::pnp_topk_dup_kernel, dim3(B), dim3(64), 0, st, Kt, static_cast<const pnp::TopkBox*>(box), static_cast<const double*>(pol),
                     static_cast<const int*>(info), dup_of);
  return rp::check_launch(fn);
}

// ---- object onboarding: exact diameter and farthest-point sampling of a point set (csrc/model_prep.cuh) ------------------------------------
size_t rnnpose_point_diameter_workspace_bytes(int total_points, int B) { return mp::diameter_workspace_bytes(total_points, B); }

int rnnpose_point_diameter_f64(const float* points, const int* pt_off, int total_points, int B, void* workspace, size_t workspace_bytes,
                               double* d2, double* diameter, int* pair, float* bounds, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_point_diameter_f64";
  RP_REQUIRE(points && pt_off && workspace && d2 && diameter && pair && bounds, fn, "null pointer");
  RP_REQUIRE(total_points >= 0 && B > 0 && B < 65536, fn, "bad size");
  RP_REQUIRE(mp::diameter_workspace_bytes(total_points, B) > 0, fn, "bad size (too large: at most 1 048 576 points a call)");
  RP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, fn, "workspace must be 8-byte aligned");
  RP_REQUIRE(workspace_bytes >= mp::diameter_workspace_bytes(total_points, B), fn, "workspace too small");
  hipStream_t st = rp::as_stream(stream);
  const long long cap = mp::tile_pairs(mp::tiles_of(total_points));
  mp::Partial* partial = static_cast<mp::Partial*>(workspace);
  hipLaunchKernelGGL(mp::mp_diameter_pairs_kernel, dim3(static_cast<unsigned>(cap), B), dim3(256), 0, st, points, pt_off, total_points, cap, partial);
  hipLaunchKernelGGL(mp::mp_diameter_final_kernel, dim3(B), dim3(256), 0, st, points, pt_off, total_points, cap,
                     static_cast<const mp::Partial*>(partial), d2, diameter, pair, bounds);
  return rp::check_launch(fn);
}

size_t rnnpose_fps_workspace_bytes(int total_points, int B) { return mp::fps_workspace_bytes(total_points, B); }

int rnnpose_fps_f64(const float* points, const int* pt_off, int total_points, int B, int n, const int* start, void* workspace,
                    size_t workspace_bytes, int* idx, double* dist2, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_fps_f64";
  RP_REQUIRE(points && pt_off && start && workspace && idx && dist2, fn, "null pointer");
  RP_REQUIRE(total_points >= 0 && B > 0 && n > 0, fn, "bad size");
  RP_REQUIRE(static_cast<long long>(B) * n < (1ll << 31), fn, "bad size (too large)");
  RP_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, fn, "workspace must be 8-byte aligned");
  RP_REQUIRE(workspace_bytes >= mp::fps_workspace_bytes(total_points, B), fn, "workspace too small");
  hipLaunchKernelGGL(mp::mp_fps_kernel, dim3(B), dim3(mp::kFpsThreads), 0, rp::as_stream(stream), points, pt_off, total_points, n, start,
                     static_cast<double*>(workspace), idx, dist2);
  return rp::check_launch(fn);
}

}  // extern "C"
