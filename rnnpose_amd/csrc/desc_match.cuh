// 2D-3D descriptor matcher: s(i, j) = sum_k d3[i][k] d2[j][k] over the points of an object and the pixels of its
// box, reduced on the fly to every point's best pixel (forward) and every pixel's best point (backward); the similarity matrix is never
// stored.  Plain fp32 VALU form: one fmaf chain over k = 0..31 from +0 per pair, the same chain in both passes, so the two directions see
// the same bits.  A thread keeps the running maximum of the pairs it walks in ascending index order (strict >: the first one stays) and
// hands it over with ONE 64-bit integer atomicMax on a packed key (orderable similarity bits << 32 | ~index): order-independent, so the
// result is bit-identical from run to run, and the lowest index wins among equal similarities.  No floating-point atomics.
// Included by csrc/eval_metrics.hip, where the entry point is.
#pragma once
#include "common.hpp"

namespace dm {

constexpr int kD = 32;            // descriptor channels
constexpr int kFwdChunk = 1024;   // box pixels one forward workgroup walks
constexpr int kFwdTile = 128;     // ... staged in LDS at a time
constexpr int kFwdPitch = 36;     // floats per staged pixel (16-byte aligned rows, 4-way instead of 64-way bank conflicts on the staging stores)
constexpr int kBwdChunk = 512;    // points one backward workgroup walks
constexpr int kBwdTile = 128;

struct Roi {
  int x0, y0, nx, ny, src;        // clamped box corner, grid size (nx * ny pixels, step apart), source image; nx = 0: nothing to match
};

__device__ __forceinline__ Roi load_roi(const int* __restrict__ bbox, const int* __restrict__ src_index, int b, int S, int H, int W, int step) {
  const int* bb = bbox + 4 * b;
  Roi r;
  r.x0 = max(bb[0], 0);
  r.y0 = max(bb[1], 0);
  const int x1 = min(bb[2], W - 1), y1 = min(bb[3], H - 1);
  r.src = src_index[b];
  const bool ok = r.src >= 0 && r.src < S && x1 >= r.x0 && y1 >= r.y0;
  r.nx = ok ? (x1 - r.x0) / step + 1 : 0;
  r.ny = ok ? (y1 - r.y0) / step + 1 : 0;
  return r;
}

// the points of object b: [off, off + P) of the concatenated arrays; P = 0 when the offsets do not fit the arrays
__device__ __forceinline__ int load_points(const int* __restrict__ pt_off, int b, int total_points, int max_points, int* off) {
  const int o = pt_off[b], e = pt_off[b + 1];
  *off = o;
  if (o < 0 || e < o || e > total_points || e - o > max_points) return 0;
  return e - o;
}

__device__ __forceinline__ unsigned long long pack_key(float s, unsigned idx) {
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (static_cast<unsigned long long>(u) << 32) | (0xFFFFFFFFu - idx);
}
__device__ __forceinline__ float key_sim(unsigned long long k) {
  unsigned u = static_cast<unsigned>(k >> 32);
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  return __uint_as_float(u);
}
__device__ __forceinline__ unsigned key_idx(unsigned long long k) { return 0xFFFFFFFFu - static_cast<unsigned>(k); }

__global__ __launch_bounds__(256) void dm_clear_kernel(unsigned long long* __restrict__ keys, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) keys[i] = 0ull;         // 0 = no candidate (every packed key is > 0)
}

// forward: a thread owns a point (its 32 channels in registers) and walks a chunk of the box's pixels staged in LDS
__global__ __launch_bounds__(256) void dm_forward_kernel(const float* __restrict__ desc3d, const int* __restrict__ pt_off, int total_points,
                                                        int max_points, const float* __restrict__ desc2d, int S, int H, int W,
                                                        const int* __restrict__ src_index, const int* __restrict__ bbox, int step,
                                                        unsigned long long* __restrict__ fwd) {
  __shared__ __attribute__((aligned(16))) float tile[kFwdTile * kFwdPitch];
  __shared__ int tile_lin[kFwdTile];
  const int b = blockIdx.z, tid = threadIdx.x;
  const Roi roi = load_roi(bbox, src_index, b, S, H, W, step);
  int off;
  const int P = load_points(pt_off, b, total_points, max_points, &off);
  const int N = roi.nx * roi.ny, n0 = blockIdx.y * kFwdChunk, n1 = min(n0 + kFwdChunk, N);
  if (n0 >= N || static_cast<int>(blockIdx.x) * 256 >= P) return;          // (the whole workgroup)
  const int i = blockIdx.x * 256 + tid;
  const bool live = i < P;
  float a[kD];
#pragma unroll
  for (int k = 0; k < kD; k += 4) {
    const float4 v = live ? *reinterpret_cast<const float4*>(desc3d + (static_cast<size_t>(off) + i) * kD + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    a[k] = v.x;
    a[k + 1] = v.y;
    a[k + 2] = v.z;
    a[k + 3] = v.w;
  }
  const float* img = desc2d + static_cast<size_t>(roi.src) * kD * H * W;
  float best = -__builtin_inff();
  int best_lin = -1;
  for (int t0 = n0; t0 < n1; t0 += kFwdTile) {
    const int cnt = min(kFwdTile, n1 - t0);
    __syncthreads();
    for (int e = tid; e < kFwdTile * kD; e += 256) {
      const int j = e % kFwdTile, k = e / kFwdTile;
      float v = 0.f;
      if (j < cnt) {
        const int n = t0 + j, gy = n / roi.nx, gx = n - gy * roi.nx;
        const int lin = (roi.y0 + gy * step) * W + roi.x0 + gx * step;
        v = img[static_cast<size_t>(k) * H * W + lin];
        if (k == 0) tile_lin[j] = lin;
      }
      tile[j * kFwdPitch + k] = v;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float4* row = reinterpret_cast<const float4*>(tile + j * kFwdPitch);
      float s = 0.f;
#pragma unroll
      for (int k4 = 0; k4 < kD / 4; ++k4) {
        const float4 v = row[k4];
        s = fmaf(a[4 * k4], v.x, s);
        s = fmaf(a[4 * k4 + 1], v.y, s);
        s = fmaf(a[4 * k4 + 2], v.z, s);
        s = fmaf(a[4 * k4 + 3], v.w, s);
      }
      if (s > best) {
        best = s;
        best_lin = tile_lin[j];
      }
    }
  }
  if (live && best_lin >= 0) atomicMax(fwd + off + i, pack_key(best, static_cast<unsigned>(best_lin)));
}

// backward: a thread owns a pixel of the box (its 32 channels in registers) and walks a chunk of the object's points staged in LDS
__global__ __launch_bounds__(256) void dm_backward_kernel(const float* __restrict__ desc3d, const int* __restrict__ pt_off, int total_points,
                                                         int max_points, const float* __restrict__ desc2d, int S, int H, int W,
                                                         const int* __restrict__ src_index, const int* __restrict__ bbox, int step, int cap,
                                                         unsigned long long* __restrict__ bwd) {
  __shared__ __attribute__((aligned(16))) float tile[kBwdTile * kD];
  const int b = blockIdx.z, tid = threadIdx.x;
  const Roi roi = load_roi(bbox, src_index, b, S, H, W, step);
  int off;
  const int P = load_points(pt_off, b, total_points, max_points, &off);
  const int N = roi.nx * roi.ny, p0 = blockIdx.y * kBwdChunk, p1 = min(p0 + kBwdChunk, P);
  if (p0 >= P || static_cast<int>(blockIdx.x) * 256 >= N) return;          // (the whole workgroup)
  const int n = blockIdx.x * 256 + tid;
  const bool live = n < N;
  float c[kD];
  {
    const int gy = live ? n / roi.nx : 0, gx = live ? n - gy * roi.nx : 0;
    const float* px = desc2d + static_cast<size_t>(roi.src) * kD * H * W + static_cast<size_t>(roi.y0 + gy * step) * W + roi.x0 + gx * step;
#pragma unroll
    for (int k = 0; k < kD; ++k) c[k] = live ? px[static_cast<size_t>(k) * H * W] : 0.f;
  }
  float best = -__builtin_inff();
  int best_i = -1;
  for (int t0 = p0; t0 < p1; t0 += kBwdTile) {
    const int cnt = min(kBwdTile, p1 - t0);
    __syncthreads();
    for (int e = tid; e < cnt * kD; e += 256) tile[e] = desc3d[(static_cast<size_t>(off) + t0) * kD + e];
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const float4* row = reinterpret_cast<const float4*>(tile + i * kD);
      float s = 0.f;
#pragma unroll
      for (int k4 = 0; k4 < kD / 4; ++k4) {
        const float4 v = row[k4];
        s = fmaf(v.x, c[4 * k4], s);
        s = fmaf(v.y, c[4 * k4 + 1], s);
        s = fmaf(v.z, c[4 * k4 + 2], s);
        s = fmaf(v.w, c[4 * k4 + 3], s);
      }
      if (s > best) {
        best = s;
        best_i = t0 + i;
      }
    }
  }
  if (live && best_i >= 0) atomicMax(bwd + static_cast<size_t>(b) * cap + n, pack_key(best, static_cast<unsigned>(best_i)));
}

// one workgroup per object: threshold, mutual check, compaction in ascending point index
__global__ __launch_bounds__(256) void dm_select_kernel(const float* __restrict__ points, const int* __restrict__ pt_off, int total_points,
                                                       int max_points, int S, int H, int W, const int* __restrict__ src_index,
                                                       const int* __restrict__ bbox, int step, int cap, float min_sim, int mutual,
                                                       float pixel_center, int M, const unsigned long long* __restrict__ fwd,
                                                       const unsigned long long* __restrict__ bwd, float* __restrict__ X, float* __restrict__ x,
                                                       float* __restrict__ sim, int* __restrict__ point_idx, int* __restrict__ count) {
  __shared__ int wave_tot[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Roi roi = load_roi(bbox, src_index, b, S, H, W, step);
  int off;
  const int P = roi.nx > 0 ? load_points(pt_off, b, total_points, max_points, &off) : 0;
  int running = 0;
  for (int base = 0; base < P; base += 256) {
    const int i = base + tid;
    bool flag = false;
    float s = 0.f;
    unsigned lin = 0;
    if (i < P) {
      const unsigned long long key = fwd[off + i];
      if (key != 0ull) {
        s = key_sim(key);
        lin = key_idx(key);
        flag = s >= min_sim;
        if (flag && mutual) {
          const int u = static_cast<int>(lin % static_cast<unsigned>(W)), v = static_cast<int>(lin / static_cast<unsigned>(W));
          const int n = ((v - roi.y0) / step) * roi.nx + (u - roi.x0) / step;
          const unsigned long long bk = bwd[static_cast<size_t>(b) * cap + n];
          flag = bk != 0ull && key_idx(bk) == static_cast<unsigned>(i);
        }
      }
    }
    int incl = flag ? 1 : 0;                               // inclusive prefix count within the wave
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    __syncthreads();
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int rank = running + incl - (flag ? 1 : 0);
    for (int w = 0; w < wave; ++w) rank += wave_tot[w];
    if (flag && rank < M) {
      const size_t row = static_cast<size_t>(b) * M + rank;
      const float* p = points + (static_cast<size_t>(off) + i) * 3;
      X[row * 3] = p[0];
      X[row * 3 + 1] = p[1];
      X[row * 3 + 2] = p[2];
      x[row * 2] = static_cast<float>(static_cast<int>(lin % static_cast<unsigned>(W))) + pixel_center;
      x[row * 2 + 1] = static_cast<float>(static_cast<int>(lin / static_cast<unsigned>(W))) + pixel_center;
      sim[row] = s;
      point_idx[row] = i;
    }
    running += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
  }
  if (tid == 0) count[b] = min(running, M);
}

inline int pixel_capacity(int H, int W, int step) { return rp::cdiv(H, step) * rp::cdiv(W, step); }

inline size_t workspace_bytes(int total_points, int B, int H, int W, int step) {
  if (total_points <= 0 || B <= 0 || H <= 0 || W <= 0 || step < 1) return 0;
  return (static_cast<size_t>(total_points) + static_cast<size_t>(B) * pixel_capacity(H, W, step)) * sizeof(unsigned long long);
}

}  // namespace dm
