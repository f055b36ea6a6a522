// Object onboarding: the exact diameter of a point set and farthest-point sampling, on the layout of the
// rasteriser and the matcher -- points (total_points,3) fp32, object b owns the rows [pt_off[b], pt_off[b+1]).
//   mp_diameter_pairs_kernel   a tiled upper-triangular sweep: workgroup (k, b) takes tile pair k = (ti <= tj) of object b, a thread owns
//                              point i of tile ti and walks tile tj staged in LDS (every read a broadcast); on the diagonal tile it starts
//                              at i + 1.  One partial (d2, i, j) per tile pair goes to the workspace.
//   mp_diameter_final_kernel   one workgroup per object: the partials and the bounds reduced under an order-independent comparison.
//   mp_fps_kernel              one workgroup per object, n dependent arg-max rounds, ONE barrier per round: every thread updates its strided
//                              slice with the last centre and keeps its best, a wave butterfly on (d2, index), the wave winners with the
//                              winner's coordinates in a double-buffered LDS slot array, and every thread reads all slots itself.
// All arithmetic fp64 on values converted from fp32, d2 = (dx dx + dy dy) + dz dz without fma contraction; no atomics: bit-identical from
// run to run and independent of B.  A point with a non-finite coordinate takes part in nothing.
// Included by csrc/eval_metrics.hip, where the entry points are.
#pragma once
#include "common.hpp"

namespace mp {

constexpr int kTile = 256;            // points per diameter tile = threads per workgroup
constexpr int kMaxTiles = 4096;       // tiles per call (total_points <= 1 048 576): the pair grid stays inside the launch limits
constexpr int kFpsThreads = 1024;     // threads of an FPS workgroup
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsReg = 8;            // points a thread keeps in registers: objects up to kFpsThreads * kFpsReg points never re-read memory

struct Partial {
  double d2;                          // -1: no pair
  int i, j;
};

__device__ __forceinline__ bool finite3(float x, float y, float z) { return x - x == 0.f && y - y == 0.f && z - z == 0.f; }

__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// the points of object b: [off, off + P); P = 0 when the range does not fit the array
__device__ __forceinline__ int load_range(const int* __restrict__ pt_off, int b, int total_points, int* off) {
  const int o = pt_off[b], e = pt_off[b + 1];
  *off = o;
  if (o < 0 || e < o || e > total_points) return 0;
  return e - o;
}

__host__ __device__ inline long long tile_pairs(int nt) { return static_cast<long long>(nt) * (nt + 1) / 2; }
__host__ __device__ inline int tiles(int points) { return (points + kTile - 1) / kTile; }
inline int tiles_of(int total_points) { return total_points > 0 ? tiles(total_points) : 1; }

// a is a better diameter pair than b: d2 larger, then i lower, then j lower (a total order: any reduction tree gives the same answer)
__device__ __forceinline__ bool better_pair(double ad, int ai, int aj, double bd, int bi, int bj) {
  return ad > bd || (ad == bd && (ai < bi || (ai == bi && aj < bj)));
}

__device__ __forceinline__ void wave_best_pair(double& d, int& i, int& j) {
  for (int o = 32; o >= 1; o >>= 1) {
    const double od = rp::shfl_xor_f64(d, o);
    const int oi = __shfl_xor(i, o), oj = __shfl_xor(j, o);
    if (better_pair(od, oi, oj, d, i, j)) {
      d = od;
      i = oi;
      j = oj;
    }
  }
}

__global__ __launch_bounds__(256) void mp_diameter_pairs_kernel(const float* __restrict__ points, const int* __restrict__ pt_off,
                                                                int total_points, long long pair_cap, Partial* __restrict__ partial) {
  __shared__ float tile[kTile * 3];
  __shared__ Partial red[4];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int off;
  const int P = load_range(pt_off, b, total_points, &off);
  const int nt = tiles(P);
  const long long k = blockIdx.x;
  if (k >= tile_pairs(nt)) return;                       // (the whole workgroup)
  // k = ti nt - ti (ti - 1) / 2 + (tj - ti), ti <= tj: the row from the root, set right by whole steps
  const double s = 2.0 * nt + 1.0;
  int ti = static_cast<int>((s - sqrt(s * s - 8.0 * static_cast<double>(k))) * 0.5);
  ti = min(max(ti, 0), nt - 1);
  auto row_start = [nt](int t) { return static_cast<long long>(t) * nt - static_cast<long long>(t) * (t - 1) / 2; };
  while (ti + 1 < nt && row_start(ti + 1) <= k) ++ti;
  while (ti > 0 && row_start(ti) > k) --ti;
  const int tj = ti + static_cast<int>(k - row_start(ti));
  const float* base = points + static_cast<size_t>(off) * 3;
  const int j0 = tj * kTile, cnt = min(kTile, P - j0);
  for (int e = tid; e < cnt; e += 256) {                 // a point that is not finite is staged as NaN: no comparison with it is true
    const float x = base[static_cast<size_t>(j0 + e) * 3], y = base[static_cast<size_t>(j0 + e) * 3 + 1], z = base[static_cast<size_t>(j0 + e) * 3 + 2];
    const bool ok = finite3(x, y, z);
    tile[3 * e] = ok ? x : __builtin_nanf("");
    tile[3 * e + 1] = y;
    tile[3 * e + 2] = z;
  }
  __syncthreads();
  const int i = ti * kTile + tid;
  double best = -1.0;
  int best_j = 0x7fffffff;
  if (i < P) {
    const float xf = base[static_cast<size_t>(i) * 3], yf = base[static_cast<size_t>(i) * 3 + 1], zf = base[static_cast<size_t>(i) * 3 + 2];
    if (finite3(xf, yf, zf)) {
      const double x = xf, y = yf, z = zf;
      for (int e = (ti == tj ? tid + 1 : 0); e < cnt; ++e) {
        const double d2 = dist2(x, y, z, static_cast<double>(tile[3 * e]), static_cast<double>(tile[3 * e + 1]), static_cast<double>(tile[3 * e + 2]));
        if (d2 > best) {                                   // strict: the lowest j stays
          best = d2;
          best_j = j0 + e;
        }
      }
    }
  }
  int bi = best < 0.0 ? 0x7fffffff : i;
  wave_best_pair(best, bi, best_j);
  if (lane == 0) red[wave] = Partial{best, bi, best_j};
  __syncthreads();
  if (tid == 0) {
    Partial p = red[0];
    for (int w = 1; w < 4; ++w)
      if (better_pair(red[w].d2, red[w].i, red[w].j, p.d2, p.i, p.j)) p = red[w];
    partial[static_cast<size_t>(b) * pair_cap + k] = p;
  }
}

__global__ __launch_bounds__(256) void mp_diameter_final_kernel(const float* __restrict__ points, const int* __restrict__ pt_off,
                                                                int total_points, long long pair_cap, const Partial* __restrict__ partial,
                                                                double* __restrict__ d2_out, double* __restrict__ diameter,
                                                                int* __restrict__ pair, float* __restrict__ bounds) {
  __shared__ Partial red[4];
  __shared__ float lo[4][3], hi[4][3];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int off;
  const int P = load_range(pt_off, b, total_points, &off);
  const long long np = tile_pairs(tiles(P));
  double best = -1.0;
  int bi = 0x7fffffff, bj = 0x7fffffff;
  for (long long k = tid; k < np; k += 256) {
    const Partial p = partial[static_cast<size_t>(b) * pair_cap + k];
    if (better_pair(p.d2, p.i, p.j, best, bi, bj)) {
      best = p.d2;
      bi = p.i;
      bj = p.j;
    }
  }
  wave_best_pair(best, bi, bj);
  float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int i = tid; i < P; i += 256) {
    const float* p = points + (static_cast<size_t>(off) + i) * 3;
    if (finite3(p[0], p[1], p[2])) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        mn[c] = fminf(mn[c], p[c]);
        mx[c] = fmaxf(mx[c], p[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    for (int o = 32; o >= 1; o >>= 1) {
      mn[c] = fminf(mn[c], __shfl_xor(mn[c], o));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o));
    }
  if (lane == 0) {
    red[wave] = Partial{best, bi, bj};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[wave][c] = mn[c];
      hi[wave][c] = mx[c];
    }
  }
  __syncthreads();
  if (tid == 0) {
    Partial p = red[0];
    for (int w = 1; w < 4; ++w)
      if (better_pair(red[w].d2, red[w].i, red[w].j, p.d2, p.i, p.j)) p = red[w];
    const bool any = p.d2 >= 0.0;
    d2_out[b] = any ? p.d2 : 0.0;
    diameter[b] = any ? sqrt(p.d2) : 0.0;
    pair[2 * b] = any ? p.i : -1;
    pair[2 * b + 1] = any ? p.j : -1;
  }
  if (tid < 3) {
    bounds[6 * b + tid] = fminf(fminf(lo[0][tid], lo[1][tid]), fminf(lo[2][tid], lo[3][tid]));
    bounds[6 * b + 3 + tid] = fmaxf(fmaxf(hi[0][tid], hi[1][tid]), fmaxf(hi[2][tid], hi[3][tid]));
  }
}

// ---- farthest-point sampling ---------------------------------------------------------------------------------------------------------------
// Running distance of a point: >= 0 pickable; -1 picked; -2 not finite (never picked, never updated).
struct FpsSlot {
  double d2;
  int idx;                            // -1: the wave has no pickable point
  float x, y, z;
};

// a is a better pick than b: d2 larger, then the index lower; idx < 0 is no candidate
__device__ __forceinline__ bool better_pick(double ad, int ai, double bd, int bi) {
  if (ai < 0) return false;
  if (bi < 0) return true;
  return ad > bd || (ad == bd && ai < bi);
}

// one point of a thread's slice: the update with the last centre (have_c), then the candidacy.  first_given: round 0 of a given start
__device__ __forceinline__ void fps_visit(int i, float x, float y, float z, double& d, bool have_c, int last, double cx, double cy, double cz,
                                          bool first_given, int st, double& best, int& best_i, float& bx, float& by, float& bz) {
  if (have_c) {
    if (i == last) {
      d = -1.0;                                            // a picked point is never picked again
    } else if (d >= 0.0) {
      const double nd = dist2(static_cast<double>(x), static_cast<double>(y), static_cast<double>(z), cx, cy, cz);
      if (nd < d) d = nd;
    }
  }
  const bool cand = first_given ? (i == st && d >= 0.0) : (d >= 0.0);
  if (cand && (best_i < 0 || d > best)) {                  // strict, ascending i: the lowest index stays
    best = d;
    best_i = i;
    bx = x;
    by = y;
    bz = z;
  }
}

__global__ __launch_bounds__(kFpsThreads) void mp_fps_kernel(const float* __restrict__ points, const int* __restrict__ pt_off, int total_points,
                                                             int n, const int* __restrict__ start, double* __restrict__ run,
                                                             int* __restrict__ idx, double* __restrict__ dist2_out) {
  __shared__ FpsSlot slot[2][kFpsWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int off;
  int P = load_range(pt_off, b, total_points, &off);
  const int st = start[b];
  if (st < -1 || st >= P) P = 0;                           // a start outside the object: the object is empty
  const float* base = points + static_cast<size_t>(off) * 3;
  double* dg = run + off;                                  // the running distances of an object too large for the registers
  const bool in_regs = P <= kFpsThreads * kFpsReg;
  const double init = st >= 0 ? static_cast<double>(__builtin_inff()) : 0.0;
  float px[kFpsReg], py[kFpsReg], pz[kFpsReg];
  double pd[kFpsReg];
  if (in_regs) {
#pragma unroll
    for (int r = 0; r < kFpsReg; ++r) {
      const int i = tid + r * kFpsThreads;
      px[r] = py[r] = pz[r] = 0.f;
      pd[r] = -2.0;
      if (i < P) {
        px[r] = base[static_cast<size_t>(i) * 3];
        py[r] = base[static_cast<size_t>(i) * 3 + 1];
        pz[r] = base[static_cast<size_t>(i) * 3 + 2];
        if (finite3(px[r], py[r], pz[r]))
          pd[r] = st >= 0 ? init : dist2(static_cast<double>(px[r]), static_cast<double>(py[r]), static_cast<double>(pz[r]), 0.0, 0.0, 0.0);
      }
    }
  } else {
    for (int i = tid; i < P; i += kFpsThreads) {
      const float x = base[static_cast<size_t>(i) * 3], y = base[static_cast<size_t>(i) * 3 + 1], z = base[static_cast<size_t>(i) * 3 + 2];
      dg[i] = !finite3(x, y, z) ? -2.0 : st >= 0 ? init : dist2(static_cast<double>(x), static_cast<double>(y), static_cast<double>(z), 0.0, 0.0, 0.0);
    }
  }
  int last = -1;
  double cx = 0.0, cy = 0.0, cz = 0.0;
  int k = 0;
  for (; k < n; ++k) {
    const bool have_c = k > 0, first_given = k == 0 && st >= 0;
    double best = -1.0;
    int best_i = -1;
    float bx = 0.f, by = 0.f, bz = 0.f;
    if (in_regs) {
#pragma unroll
      for (int r = 0; r < kFpsReg; ++r) {
        const int i = tid + r * kFpsThreads;
        if (i < P) fps_visit(i, px[r], py[r], pz[r], pd[r], have_c, last, cx, cy, cz, first_given, st, best, best_i, bx, by, bz);
      }
    } else {
      for (int i = tid; i < P; i += kFpsThreads) {
        const float x = base[static_cast<size_t>(i) * 3], y = base[static_cast<size_t>(i) * 3 + 1], z = base[static_cast<size_t>(i) * 3 + 2];
        double d = dg[i];
        const double was = d;
        fps_visit(i, x, y, z, d, have_c, last, cx, cy, cz, first_given, st, best, best_i, bx, by, bz);
        if (d != was) dg[i] = d;
      }
    }
    double wd = best;
    int wi = best_i;
    for (int o = 32; o >= 1; o >>= 1) {
      const double od = rp::shfl_xor_f64(wd, o);
      const int oi = __shfl_xor(wi, o);
      if (better_pick(od, oi, wd, wi)) {
        wd = od;
        wi = oi;
      }
    }
    // the lane that owns the wave's winner publishes it with its coordinates; a wave without a candidate publishes that (lane 0)
    FpsSlot* mine = slot[k & 1];
    if (wi < 0 ? lane == 0 : wi == best_i) mine[wave] = FpsSlot{wd, wi, bx, by, bz};
    __syncthreads();                                       // (the only barrier of a round: the other buffer is written two rounds apart)
    FpsSlot w = mine[0];
#pragma unroll
    for (int v = 1; v < kFpsWaves; ++v) {
      const FpsSlot s = mine[v];
      if (better_pick(s.d2, s.idx, w.d2, w.idx)) w = s;
    }
    if (w.idx < 0) break;                                  // (the whole workgroup) nothing left to pick
    if (tid == 0) {
      idx[static_cast<size_t>(b) * n + k] = w.idx;
      dist2_out[static_cast<size_t>(b) * n + k] = w.d2;
    }
    last = w.idx;
    cx = static_cast<double>(w.x);
    cy = static_cast<double>(w.y);
    cz = static_cast<double>(w.z);
  }
  for (int r = k + tid; r < n; r += kFpsThreads) {
    idx[static_cast<size_t>(b) * n + r] = -1;
    dist2_out[static_cast<size_t>(b) * n + r] = -1.0;
  }
}

inline size_t diameter_workspace_bytes(int total_points, int B) {
  if (total_points < 0 || B <= 0 || B >= 65536) return 0;
  const int nt = tiles_of(total_points);
  if (nt > kMaxTiles) return 0;
  return static_cast<size_t>(B) * static_cast<size_t>(tile_pairs(nt)) * sizeof(Partial);
}

inline size_t fps_workspace_bytes(int total_points, int B) {
  if (total_points < 0 || B <= 0) return 0;
  return static_cast<size_t>(total_points > 0 ? total_points : 1) * sizeof(double);
}

}  // namespace mp
