// Pose confidence: the render-and-compare score of a pose against its frame.  The caller renders the object's
// per-vertex descriptors and z-buffer into a window of the frame (principal point shifted by the window's integer corner, so window
// pixel (x, y) IS frame pixel (x0 + x, y0 + y): no resampling); these kernels classify every rendered pixel against the observed
// depth, compare its descriptor with the frame's by the cosine, and reduce both to ten fp64 statistics and one score per pose.
// Two launches:
//   ps_partial_kernel  a lane owns one window pixel (linear index, so every channel plane of rend_desc is read contiguously), a
//                      256-thread workgroup a 256-pixel chunk of one pose; the grid is flat over B x chunks.  Lane values go through a
//                      fixed xor butterfly, the four wave sums are added in wave order: one partial row per workgroup.
//   ps_final_kernel    one workgroup per pose: column c's partial rows added in ascending chunk order, then the score.
// All arithmetic fp64 on values converted from fp32, no fma contraction, no atomics, no tickets: two runs are bit-identical, and a
// pose's row depends on nothing but its own window (alone == in a batch).
// Included by csrc/eval_metrics.hip, where the entry point is.
#pragma once
#include "common.hpp"

namespace ps {

constexpr int kD = 32;        // descriptor channels
constexpr int kChunk = 256;   // window pixels per workgroup = threads per workgroup
constexpr int kNS = 10;       // statistics per pose
// columns of a statistics row
enum { N_REND = 0, N_OUT, N_OCC, N_CONS, N_VIOL, N_HOLE, N_DESC, SUM_COS, SUM_ADD, N_BAD };

constexpr double kNormEps = 1e-12;

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

inline int chunks(int h, int w) { return rp::cdiv(static_cast<long long>(h) * w, kChunk); }

__global__ __launch_bounds__(256) void ps_partial_kernel(const float* __restrict__ rend_depth, const float* __restrict__ rend_desc,
                                                         const int* __restrict__ window, const float* __restrict__ desc2d,
                                                         const float* __restrict__ depth_obs, const int* __restrict__ src_index, int S,
                                                         int h, int w, int H, int W, int nchunk, double tol, double* __restrict__ partial) {
  __shared__ double red[4][kNS];
  const int b = blockIdx.x / nchunk, c = blockIdx.x - b * nchunk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hw = h * w;
  const int p = c * kChunk + tid;
  const int src = src_index[b];
  double st[kNS];
#pragma unroll
  for (int i = 0; i < kNS; ++i) st[i] = 0.0;
  if (p < hw && src >= 0 && src < S) {
    const double z = static_cast<double>(rend_depth[static_cast<size_t>(b) * hw + p]);
    if (finite_d(z) && z > 0.0) {
      st[N_REND] = 1.0;
      const int y = p / w, x = p - y * w;
      const long long u = static_cast<long long>(window[2 * b]) + x, v = static_cast<long long>(window[2 * b + 1]) + y;
      if (u < 0 || u >= W || v < 0 || v >= H) {
        st[N_OUT] = 1.0;
      } else {
        const size_t HW = static_cast<size_t>(H) * W, pix = static_cast<size_t>(v) * W + static_cast<size_t>(u);
        bool occluded = false;
        if (depth_obs != nullptr) {
          const double d = static_cast<double>(depth_obs[static_cast<size_t>(src) * HW + pix]);
          if (finite_d(d) && d > 0.0) {
            const double dd = d - z;
            if (dd < -tol) {
              occluded = true;
              st[N_OCC] = 1.0;
            } else if (dd <= tol) {
              st[N_CONS] = 1.0;
              st[SUM_ADD] = fabs(dd);
            } else {
              st[N_VIOL] = 1.0;
            }
          } else {
            st[N_HOLE] = 1.0;
          }
        } else {
          st[N_HOLE] = 1.0;
        }
        if (!occluded) {
          const float* pa = rend_desc + static_cast<size_t>(b) * kD * hw + p;
          const float* pg = desc2d + static_cast<size_t>(src) * kD * HW + pix;
          double dot = 0.0, na = 0.0, ng = 0.0;
          bool bad = false;
          for (int k = 0; k < kD; ++k) {
            const double a = static_cast<double>(pa[static_cast<size_t>(k) * hw]), g = static_cast<double>(pg[static_cast<size_t>(k) * HW]);
            bad = bad || !finite_d(a) || !finite_d(g);
            dot += a * g;
            na += a * a;
            ng += g * g;
          }
          if (bad) {
            st[N_BAD] = 1.0;
          } else {
            st[N_DESC] = 1.0;
            st[SUM_COS] = dot / (fmax(sqrt(na), kNormEps) * fmax(sqrt(ng), kNormEps));
          }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kNS; ++i) {
    double s = st[i];
    for (int o = 32; o >= 1; o >>= 1) s += rp::shfl_xor_f64(s, o);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (tid < kNS) partial[static_cast<size_t>(blockIdx.x) * kNS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(64) void ps_final_kernel(const double* __restrict__ partial, int nchunk, double* __restrict__ stats,
                                                      double* __restrict__ score) {
  __shared__ double tot[kNS];
  const int b = blockIdx.x, c = threadIdx.x;
  if (c < kNS) {
    const double* p = partial + static_cast<size_t>(b) * nchunk * kNS + c;
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += p[static_cast<size_t>(k) * kNS];
    tot[c] = s;
    stats[static_cast<size_t>(b) * kNS + c] = s;
  }
  __syncthreads();
  if (c == 0) {
    double sc = 0.0;
    if (tot[N_DESC] > 0.0) {
      const double den = tot[N_CONS] + tot[N_VIOL];
      const double depth_factor = den > 0.0 ? tot[N_CONS] / den : 1.0;
      sc = fmax(tot[SUM_COS] / tot[N_DESC], 0.0) * depth_factor;
    }
    score[b] = sc;
  }
}

inline size_t workspace_bytes(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0 || static_cast<long long>(h) * w > 0x7fffffffll - kChunk) return 0;
  const long long rows = static_cast<long long>(B) * chunks(h, w);
  if (rows > 0x7fffffffll) return 0;
  return static_cast<size_t>(rows) * kNS * sizeof(double);
}

}  // namespace ps
