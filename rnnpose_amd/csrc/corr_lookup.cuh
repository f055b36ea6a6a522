// The window lookup, written once: shared by corr_lookup.hip (a3: the lookup as a kernel of its own, r01-r05 and r06 forms) and
// corr_convc1.hip (r06: the lookup as the staging phase of BasicMotionEncoder.convc1 -- the 324 window features of a pixel tile go
// straight into the convolution's LDS ring).  Here: the pyramid layout record and its host-side fill, the coordinate prologue, the
// cooperative footprint fetch of NP pixels of one level by one wave, the two-row sliding-window tap loop and the NHWC row store.
// Reference: CorrBlock.__call__ + bilinear_sampler (thirdparty/raft/corr.py:36-57, thirdparty/raft/utils/utils.py:57-71).
#pragma once
#ifndef RP_CONTRACT_LOCAL
#define RP_CONTRACT_LOCAL 1      // (geometry.cuh / induced.cuh: no fma contraction inside THEIR functions only -- the taps below contract in every includer alike)
#endif
#include "common.hpp"
#include "induced.cuh"

#ifndef RPL_LB
#define RPL_LB 8          // pixels whose footprint loads are in flight together (measurement: 16)
#endif

namespace rplookup {

constexpr int R = 4;
constexpr int WIN = 2 * R + 1;      // 9
constexpr int FP = WIN + 1;         // 10: footprint side
constexpr int FS = FP * FP + 1;     // 101: per-pixel LDS stride (odd -> conflict-free lane-per-pixel reads)
constexpr int PIX = 16;             // pixels per wave and round

struct LookupInfo {
  long long off[RNNPOSE_MAX_LEVELS];
  int hl[RNNPOSE_MAX_LEVELS];
  int wl[RNNPOSE_MAX_LEVELS];
  int n_px, n_patch;          // level 0 is stored j-patch-major: [image][8 x 16 patch][i][8][16] (csrc/corr_pyramid.hip)
};

// Host side of every lookup launch: the images [b0, b1) of a pyramid built for B_total images of h x w pixels.
inline int lookup_info(const char* fn, int B_total, int b0, int b1, int h, int w, int levels, LookupInfo& info) {
  RP_REQUIRE(b0 >= 0 && b0 < b1 && b1 <= B_total, fn, "image range must satisfy 0 <= b0 < b1 <= B");
  int64_t offs[RNNPOSE_MAX_LEVELS + 1];
  if (int e = rnnpose_corr_pyramid_layout(B_total, h, w, levels, offs, info.hl, info.wl)) return e;
  info.n_px = rp::cdiv(w, 16);
  info.n_patch = rp::cdiv(h, 8) * info.n_px;
  for (int l = 0; l < levels; ++l) {
    info.off[l] = offs[l];
    // the reference divides by (W_l - 1): a 1-wide level yields inf/NaN there
    RP_REQUIRE(info.hl[l] >= 2 && info.wl[l] >= 2, fn, "every pyramid level must be at least 2x2");
  }
  return 0;
}

// flat pixel index (b, Y, X) of a batch of N-pixel maps -> image and pixel inside it
__device__ __forceinline__ void decode_px(long long p, int N, int& b, int& pix) {
  b = static_cast<int>(p / N);
  pix = static_cast<int>(p - static_cast<long long>(b) * N);
}

// window centre of pixel `pix` of image b, at level-0 scale, from a (B, 2, h, w) coordinate tensor
__device__ __forceinline__ float2 read_centre(const float* coords, int b, int pix, int N) {
  return make_float2(coords[(static_cast<long long>(b) * 2 + 0) * N + pix], coords[(static_cast<long long>(b) * 2 + 1) * N + pix]);
}

// Coordinate prologue of the two lookup kernels for flat pixel p of a launch of `total` pixels: its image and pixel (b, pix; 0 when not
// `live`), its row in the pyramid (image bg of the WHOLE batch the pyramid was built for, pixel pixg inside it; pixels past the end repeat
// the last one) and its window centre (cx, cy) at the scale of level `lvl` (0 when not live).  The centre is read from `coords` or -- r06,
// isrc.depth set -- formed HERE (induced.cuh: the very function of induced_coords_lowres_kernel) instead of being read from the output of a
// launch of its own; the lanes with `writer` set (one per pixel), at level 0, write it out for the later consumers.
struct Centre {
  float cx, cy;
  int b, pix, bg, pixg;
};
__device__ __forceinline__ Centre lookup_centre(const float* coords, const rp::InducedSrc& isrc, float* coords_out, bool writer, long long p,
                                                long long total, bool live, int h, int w, long long p_off, int lvl) {
  const int N = h * w;
  const float inv = 1.0f / static_cast<float>(1 << lvl);
  float cx = 0.f, cy = 0.f;
  int b = 0, pix = 0, bg, pixg;
  decode_px(p_off + (p < total ? p : total - 1), N, bg, pixg);
  if (live) {
    decode_px(p, N, b, pix);
    if (isrc.depth) {
      const int Y = pix / w, X = pix - Y * w;
      const float2 c = rp::induced_coords_at(isrc.depth + static_cast<long long>(b) * isrc.H * isrc.W, X, Y, isrc.H, isrc.W, h, w, isrc.eps,
                                             rp::load_intr(isrc.K, b), rp::load_pose(isrc.G, b));
      if (lvl == 0 && coords_out && writer) {
        coords_out[(static_cast<long long>(b) * 2 + 0) * N + pix] = c.x;
        coords_out[(static_cast<long long>(b) * 2 + 1) * N + pix] = c.y;
      }
      cx = c.x * inv;
      cy = c.y * inv;
    } else {
      const float2 c = read_centre(coords, b, pix, N);
      cx = c.x * inv;
      cy = c.y * inv;
    }
  }
  return Centre{cx, cy, b, pix, bg, pixg};
}

// Integer base and fractional offsets of the 10 x 10 footprint of a pixel whose window centre is (cx, cy) at this level's scale.
// Non-finite / far-away coordinates sample only padding -> zeros.
__device__ __forceinline__ void footprint_base(float cx, float cy, int& bx, int& by, float& ax, float& ay) {
  const bool sane = (cx > -1.0e6f) && (cx < 1.0e6f) && (cy > -1.0e6f) && (cy < 1.0e6f);
  const float fx0 = floorf(cx), fy0 = floorf(cy);
  bx = sane ? static_cast<int>(fx0) - R : -1000000;
  by = sane ? static_cast<int>(fy0) - R : -1000000;
  ax = sane ? cx - fx0 : 0.f;
  ay = sane ? cy - fy0 : 0.f;
}

// ---- footprint fetch ------------------------------------------------------------------------------------------------------------
// One wave fetches the footprints of `npix` (<= NP) pixels of one level into foot[q * FS + t] (t = 10 ty + tx), zeros outside the level.
// Lane q < NP holds its pixel's footprint base (bx, by); where a pixel's map lies and how a texel of it is addressed is the ADDRESS POLICY
// `a` (below).  Every load is UNCONDITIONAL (texels outside the level read element 0 of the pixel's map and are zeroed on the way into
// LDS; pixel slots past npix repeat the last pixel) and the loads of LB pixels are issued before the first LDS store: with the bounds
// test around the load the compiler waited vmcnt(0) after every pixel -- 16 dependent memory round trips per wave (r02: 46 us per
// half-batch launch, latency-bound).  (NP = 16: corr_lookup.hip; 8: corr_convc1.hip.)
template <int NP, class Addr>
__device__ __forceinline__ void gather_batches(const Addr& a, int lane, int npix, int bx, int by, float* foot) {
  const int t0 = lane, t1 = lane + 64;
  const int ty0 = t0 / FP, tx0 = t0 - ty0 * FP;
  const int ty1 = t1 / FP, tx1 = t1 - ty1 * FP;
  constexpr int LB = RPL_LB < NP ? RPL_LB : NP;
  const bool has1 = t1 < FP * FP;
#pragma unroll
  for (int qb = 0; qb < NP; qb += LB) {
    float v0[LB], v1[LB];
    unsigned ok = 0u;
#pragma unroll
    for (int j = 0; j < LB; ++j) {
      const int q = qb + j;
      const int qq = q < npix ? q : npix - 1;
      const auto px = a.pixel(bx, by, qq);
      const int xa = px.bx + tx0, ya = px.by + ty0, xb = px.bx + tx1, yb = px.by + ty1;
      const bool oka = a.inside(xa, ya);
      const bool okb = has1 && a.inside(xb, yb);
      v0[j] = a.texel(px, xa, ya, oka);
      v1[j] = a.texel(px, xb, yb, okb);
      ok |= (oka ? 1u : 0u) << (2 * j) | (okb ? 2u : 0u) << (2 * j);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < LB; ++j) {
      const int q = qb + j;
      foot[q * FS + t0] = (ok >> (2 * j)) & 1u ? v0[j] : 0.f;
      if (has1) foot[q * FS + t1] = (ok >> (2 * j)) & 2u ? v1[j] : 0.f;
    }
  }
}

// What both address policies know of the wave: the level and its maps, lane q's image in the pyramid (bg) and its pixel index inside
// it (pixg), and `first_row` = pyramid row (= p_off + flat pixel index) of pixel 0 of the NP.
struct WaveMaps {
  const float* lvl_base;
  int lvl, n_px, n_patch, N, hl, wl, bg, pixg;
  long long first_row;
};
__device__ __forceinline__ WaveMaps wave_maps(const float* __restrict__ pyr, const LookupInfo& info, int lvl, int N, int bg, int pixg, long long first_row) {
  return WaveMaps{pyr + info.off[lvl], lvl, info.n_px, info.n_patch, N, info.hl[lvl], info.wl[lvl], bg, pixg, first_row};
}

// r01-r05 (corr_lookup_kernel, the fused kernel): any level, any map size.  Level 0 is j-patch-major: texel (y, x) of pixel i = patch
// ((y >> 3) n_px + (x >> 4)), row i, cell (y & 7, x & 15); the other levels are row-major maps per pixel.  Both forms as SELECTS on the
// (wave-uniform) level, not as a branch: a branch around the loads brought the one-wait-per-load form back (tests/test_isa_guard.py: 24
// vmcnt(0) waits for 50 loads)
struct AddrSelect {
  WaveMaps m;
  struct Px {
    int bx, by;
    const float* src;
  };
  __device__ __forceinline__ Px pixel(int bx, int by, int qq) const {
    const int qbx = __shfl(bx, qq), qby = __shfl(by, qq);
    const int qbg = __shfl(m.bg, qq), qpix = __shfl(m.pixg, qq);
    const long long img = static_cast<long long>(m.hl) * m.wl;
    return Px{qbx, qby, m.lvl_base + (m.lvl == 0 ? (static_cast<long long>(qbg) * m.n_patch * m.N + qpix) * 128 : (m.first_row + qq) * img)};
  }
  __device__ __forceinline__ bool inside(int x, int y) const { return x >= 0 && x < m.wl && y >= 0 && y < m.hl; }
  __device__ __forceinline__ float texel(const Px& px, int x, int y, bool ok) const {
    const long long pstride = static_cast<long long>(m.N) * 128;
    const long long e = m.lvl == 0 ? ((y >> 3) * m.n_px + (x >> 4)) * pstride + (y & 7) * 16 + (x & 15) : static_cast<long long>(y * m.wl + x);
    return px.src[ok ? e : 0];
  }
};

// r06: the same fetch with a third of the instructions (the lookup is bound by INSTRUCTIONS per wave, not by a pipe: ~1600 per 16 pixels of one
// level, ~1000 of them here -- per load a 64-bit patch-stride multiply, both address forms evaluated and selected, four bpermutes per pixel):
//   * L0 (level 0, j-patch-major) or not is a TEMPLATE parameter: one address form, chosen by one wave-uniform branch around the whole body;
//   * the pixel's footprint base / image / index come from v_readlane (the pixel slot is wave-uniform): scalars, and the pixel's map base is a
//     scalar 64-bit address; a lane's texel is an unsigned 32-bit BYTE offset from it (a level-0 image is N^2 floats <= 1.5 GB at 120 x 160);
//   * bounds tests as unsigned compares.
// Same texels into the same LDS slots: the results do not change by a bit.
template <bool L0>
struct AddrFast {
  WaveMaps m;
  struct Px {
    int bx, by;
    const char* src;
  };
  __device__ __forceinline__ Px pixel(int bx, int by, int qq) const {                 // (qq is wave-uniform)
    const int qbx = __builtin_amdgcn_readlane(bx, qq), qby = __builtin_amdgcn_readlane(by, qq);
    const char* const base = reinterpret_cast<const char*>(m.lvl_base);
    if constexpr (L0) {
      const int qbg = __builtin_amdgcn_readlane(m.bg, qq), qpix = __builtin_amdgcn_readlane(m.pixg, qq);
      return Px{qbx, qby, base + (static_cast<long long>(qbg) * m.n_patch * m.N + qpix) * 512};
    } else {
      const unsigned img_b = static_cast<unsigned>(m.hl * m.wl) * 4u;                     // bytes of one pixel's map (levels >= 1)
      return Px{qbx, qby, base + (m.first_row + qq) * static_cast<long long>(img_b)};
    }
  }
  __device__ __forceinline__ bool inside(int x, int y) const {
    return static_cast<unsigned>(x) < static_cast<unsigned>(m.wl) && static_cast<unsigned>(y) < static_cast<unsigned>(m.hl);
  }
  __device__ __forceinline__ float texel(const Px& px, int x, int y, bool ok) const {
    unsigned e;
    if constexpr (L0) {     // texel (y, x) of pixel i = patch ((y >> 3) n_px + (x >> 4)), row i, cell (y & 7, x & 15)
      const unsigned pstride = static_cast<unsigned>(m.N) * 128u;                       // floats from one j patch to the next
      e = (static_cast<unsigned>((y >> 3) * m.n_px + (x >> 4)) * pstride + static_cast<unsigned>(((y & 7) << 4) | (x & 15))) * 4u;
    } else {
      e = static_cast<unsigned>(y * m.wl + x) * 4u;
    }
    return *reinterpret_cast<const float*>(px.src + (ok ? e : 0u));
  }
};

// ---- taps ---------------------------------------------------------------------------------------------------------------------------
// The bilinear taps of a pixel over ROWS window rows (the first `nrows` of them: run-time in the fused kernel): f = the pixel's footprint
// at its first window row, (ax, ay) = the fractional offsets of its centre.  A two-row register window slides over footprint rows jj,
// jj + 1 (y offset) and columns i, i + 1 (x offset i - 4); emit(i, jj, value) receives the tap of window column i, row jj.
template <int ROWS, class Emit>
__device__ __forceinline__ void window_taps(const float* f, float ax, float ay, int nrows, Emit emit) {
  const float w00 = (1.f - ax) * (1.f - ay), w10 = ax * (1.f - ay), w01 = (1.f - ax) * ay, w11 = ax * ay;
  float prev[FP], cur[FP];
#pragma unroll
  for (int x = 0; x < FP; ++x) prev[x] = f[x];
#pragma unroll
  for (int jj = 0; jj < ROWS; ++jj) {
    if (jj < nrows) {
#pragma unroll
      for (int x = 0; x < FP; ++x) cur[x] = f[(jj + 1) * FP + x];
#pragma unroll
      for (int i = 0; i < WIN; ++i) emit(i, jj, w00 * prev[i] + w10 * prev[i + 1] + w01 * cur[i] + w11 * cur[i + 1]);
#pragma unroll
      for (int x = 0; x < FP; ++x) prev[x] = cur[x];
    }
  }
}

// ---- NHWC rows ----------------------------------------------------------------------------------------------------------------------
// (B, h, w, L*81): rows[q * 81 + c] (LDS) holds the 81 values of pixel q of the wave's npix at this level; every pixel's values leave as
// one contiguous 324-byte run.  `first` = flat index of pixel 0.
__device__ __forceinline__ void store_rows_nhwc(float* __restrict__ out, const float* rows, long long first, int npix, int levels, int lvl, int lane) {
  const int ctot = levels * WIN * WIN;
  float* o = out + first * ctot + lvl * (WIN * WIN);
  for (int q = 0; q < npix; ++q) {
    o[static_cast<long long>(q) * ctot + lane] = rows[q * (WIN * WIN) + lane];
    if (lane < WIN * WIN - 64) o[static_cast<long long>(q) * ctot + 64 + lane] = rows[q * (WIN * WIN) + 64 + lane];
  }
}

}  // namespace rplookup
