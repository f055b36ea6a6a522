// The 32-pixel x 256-column output tile of the resident 1x1 convolution, shared by conv1x1_resident.hip (activation tile split once into
// LDS) and corr_convc1.hip (activation blocks computed level by level into an LDS ring): a workgroup of 4 waves owns 32 consecutive pixels
// and ALL 256 output columns -- 4 column tiles x 2 pixel tiles of v_mfma_f32_16x16x32_f16 per wave.  Here: the weight-record load, the
// 24-MFMA step of one 32-channel block, the epilogue with its destination record, and the host-side checks and fill of that record.
#pragma once
#include "common.hpp"
#include "f16x3.cuh"

namespace rptile {

using rp::h4; using rp::h8;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MQ = 32;          // pixels per workgroup (= threads / 8)
constexpr int CT = 4;           // 16-column tiles per wave: Cout = 4 waves x 4 x 16 = 256
constexpr int RSF = 260;        // epilogue staging row stride in floats (256 + 4: conflict-free)

struct TileOut {
  const float* bias;            // (256)
  float a_scale, out_scale;
  float* dst;                   // (M, dcs): channels [dco, dco + 256)
  int dcs, dco, relu;
  long long M;
  unsigned long long* sat;
  int dst_hl;                   // write the output as a SPLIT tensor (fp16 hi|lo per 8-channel group, rnnpose_hip.h) for the next convolution
};

// B fragments of channel block cb for this wave's column tiles, (hi, lo) each, straight from the packed array: record
// (cb * 16 + column tile) * 128 + part * 64 + lane
__device__ __forceinline__ void load_weights(uint4 (&bq)[CT][2], const uint4* wpk, int cb, int wave, int lane) {
  const uint4* rec = wpk + (static_cast<long long>(cb) * 16 + wave * CT) * 128 + lane;
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    bq[j][0] = rec[j * 128];
    bq[j][1] = rec[j * 128 + 64];
  }
}

// One 32-channel block: A fragments of the two pixel tiles from the block's hi and lo planes (row * 32 + swizzled chunk * 8 + e; lane ->
// row 16 t + l15, chunk phys), then 4 column tiles x 2 pixel tiles x 3 split products = 24 MFMAs
__device__ __forceinline__ void block_step(f32x4 (&acc)[2][CT], const _Float16* hi, const _Float16* lo, const uint4 (&bq)[CT][2], int l15, int phys) {
  h8 ah[2], al[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    ah[t] = *reinterpret_cast<const h8*>(hi + (16 * t + l15) * 32 + phys * 8);
    al[t] = *reinterpret_cast<const h8*>(lo + (16 * t + l15) * 32 + phys * 8);
  }
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    const h8 bh = __builtin_bit_cast(h8, bq[j][0]), bl = __builtin_bit_cast(h8, bq[j][1]);
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t][j] = rp::mfma16_c32(al[t], bh, acc[t][j]);
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t][j] = rp::mfma16_c32(ah[t], bl, acc[t][j]);
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t][j] = rp::mfma16_c32(ah[t], bh, acc[t][j]);
  }
}

// Epilogue: accumulators (C layout of the 16x16 tile: col = lane & 15, row = 4 (lane >> 4) + e) -> LDS tile S (MQ x RSF floats, aliasing
// the activations: every wave must be done reading them) -> 16-byte stores, a whole 1-KB output row per 64 lanes.  Straight from the
// registers it was 32 4-byte stores per lane in 64-byte runs: the store path, not the arithmetic, set the kernel's time.
__device__ __forceinline__ void tile_epilogue(const TileOut o, const f32x4 (&acc)[2][CT], float* S, long long m0, int tid) {
  const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    const int col = 64 * wave + 16 * j + l15;
    const float b = o.bias[col];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float y = acc[t][j][e] * o.out_scale + b;
        if (o.relu) y = fmaxf(y, 0.f);
        S[(16 * t + 4 * lq + e) * RSF + col] = y;
      }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int idx = tid + 256 * k;
    const int row = idx >> 6, cq = (idx & 63) * 4;
    const long long m = m0 + row;
    if (m >= o.M) continue;
    const float4 y = *reinterpret_cast<const float4*>(S + row * RSF + cq);
    if (o.dst_hl) {               // quad cq of the row -> 8 bytes of the hi plane + 8 bytes of the lo plane of its 8-channel group
      h4 hi, lo;
      rp::split4(y, o.a_scale, hi, lo);
      if (o.sat && rp::quad_saturates(y, o.a_scale)) atomicAdd(o.sat, 1ull);
      const int ch = o.dco + cq;
      float* ph = o.dst + m * o.dcs + (ch & ~7) + ((ch >> 2) & 1) * 2;
      *reinterpret_cast<h4*>(ph) = hi;
      *reinterpret_cast<h4*>(ph + 4) = lo;
    } else {
      *reinterpret_cast<float4*>(o.dst + m * o.dcs + o.dco + cq) = y;
    }
  }
}

// Host side: the destination and scale checks of an entry whose output is this tile (`also16`: a further pointer that must be 16-byte
// aligned under the destination's message) ...
inline int check_tile_out(const char* fn, const float* dst, int dst_c_stride, int dst_c_offset, int dst_split, float a_scale, float w_scale,
                          const void* also16 = nullptr) {
  if (dst_split) RP_REQUIRE(dst_c_stride % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 32 == 0, fn, "split-form dst: channel stride multiple of 8, 32-byte aligned");
  RP_REQUIRE(dst_c_offset >= 0 && dst_c_offset + 256 <= dst_c_stride && dst_c_offset % 4 == 0 && dst_c_stride % 4 == 0 &&
                 reinterpret_cast<uintptr_t>(dst) % 16 == 0 && reinterpret_cast<uintptr_t>(also16) % 16 == 0, fn,
             "the 256 output channels must lie inside the row, 16-byte aligned");
  RP_REQUIRE(a_scale > 0.f && w_scale > 0.f, fn, "scales must be positive");
  return 0;
}

// ... and the record itself
inline TileOut tile_out(const float* bias, float a_scale, float w_scale, int relu, float* dst, int dst_c_stride, int dst_c_offset, int dst_split,
                        long long n_pixels) {
  return TileOut{bias, a_scale, 1.0f / (a_scale * w_scale), dst, dst_c_stride, dst_c_offset, relu, n_pixels, rp::sat_counter(), dst_split};
}

}  // namespace rptile
