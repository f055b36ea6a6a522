// Shared by the two implicit-GEMM convolution kernel families (conv_igemm.hip: 128-row tiles, 4 waves, weights straight to
// registers; conv_strip.hip: 160-row strips, operands by LDS-DMA): the launch parameter block, which rnnpose_conv2d_nhwc_f16x3
// fills once from the public descriptor, and the split-form output store.
#pragma once
#include "common.hpp"
#include "f16x3.cuh"

namespace rpconv {

constexpr int BK = 32;                  // channels per block (one 128-byte line of an NHWC pixel)
constexpr int MAX_CB = 24;

using rp::h8; using rp::h4; using rp::h2; using rp::f32x2; using rp::f32x16; using rp::u32x2; using rp::split4;

struct Seg {
  const float* ptr;
  int cstride, coff, ccount;
};

struct KParams {
  Seg seg0, seg1, seg2, seg3;       // separate members: a dynamically indexed by-value array would be copied to LDS
  int cb1, cb2, cb3;                // first channel block of segments 1..3 (ncb if absent)
  int ncb;
  int B, U, V, su, sv;              // slow / fast axis extents and pixel strides
  int G, T, du0, dv0;               // groups (slow-axis taps) x taps per group (fast axis)
  int stride, Uin, Vin, gkw, dvg0;  // strided mode (stride 2): no tap sharing, G = kh*kw groups decoded as (g / gkw, g % gkw)
  const uint4* wpk;                 // packed weights: [g][cb][t][32-col tile][hi kk0, hi kk1, lo kk0, lo kk1][lane] x 16 bytes
  int Npad;
  const float* bias;
  int Cout;
  float a_scale, out_scale;
  int epi;
  float* dst;
  int dst_cs, dst_co;
  const float* aux0;
  int aux0_cs, aux0_co;
  const float* aux1;
  int aux1_cs, aux1_co;
  float* dst2;
  int dst2_cs, dst2_co;
  int gru_c;
  double* tstats;  // optional per-tile column statistics (linear epilogue), fp64: sum, sum of squares
  const float* addm;   // optional per-pixel bias map (NHWC), added before the epilogue
  int addm_cs, addm_co;
  int tpi;             // > 0: M is tiled PER IMAGE (tpi tiles of 128 rows each, the last one ragged): no tile straddles two images
  const float* in_mr;  // NORM variant: (B, seg0.cstride, 2) mean / rstd of source 0, applied with ReLU while staging
  int n_mt, n_nt;
  unsigned long long* sat;   // fp16x3 range guard: counter of clamped / non-finite activation quads (NULL = check off)
  int sp_tx, sp_ty;          // SPATIAL kernels: 16-pixel-wide / 8-pixel-high patches per image row / column
  int dst_hl, dst2_hl;       // dst / dst2 receive the PRE-SPLIT fp16 hi|lo form (rnnpose_hip.h, "split tensors") instead of fp32
  float* dsth;               // optional second destination of the primary result, always in split form (GRU: h' as fp32 AND split)
  int dsth_cs, dsth_co;
  int ksplit;                // > 1: gridDim.x = tiles * ksplit, workgroup (tile, s) multiplies channel blocks [nit s / ksplit, nit (s + 1) / ksplit)
  float* ks_ws;              // ksplit partial accumulators: [tile][split][acc register][thread] floats
  unsigned* ks_cnt;          // per-tile arrival counters (zero between launches)
  const uint4* wpk_strip;    // the same weights in the strip kernel's order (conv_strip.hip), behind the first copy in w_packed
  int single_product;        // strip kernels, 160-row strips, one column tile per wave: a_hi * b_hi only (cfg.raft.mixed_precision)
  int off32;                 // strip kernels: every destination / epilogue operand spans < 2^32 elements (32-bit offsets in the fast epilogue)
  int stagger;               // persistent strip launches (measurement): 100-MHz ticks of start delay per workgroup slot of a CU
  int n_tiles;               // strip kernels, r06: > 0 = a PERSISTENT launch -- gridDim.x resident workgroups walk n_tiles tiles (conv_strip_kernel.cuh)
};

// One output quad (4 consecutive channels starting at channel ch of the pixel row `row`) in split form: the 8-channel group
// g = ch / 8 occupies 32 bytes = [hi x 8 | lo x 8] fp16; a quad is the 8-byte half (ch / 4) & 1 of each plane.  nv < 4 (the
// ragged tail of a 126-channel layer): only the first nv fp16 of each plane are written -- their neighbours belong to
// another producer (the flow channels of the motion features).
__device__ __forceinline__ void store_quad_hl(float* row, int ch, float y0, float y1, float y2, float y3, int nv, float a_scale,
                                              int& sat_n) {
  h4 hi, lo;
  const float4 v = make_float4(y0, nv > 1 ? y1 : 0.f, nv > 2 ? y2 : 0.f, nv > 3 ? y3 : 0.f);
  split4(v, a_scale, hi, lo);
  sat_n += rp::quad_saturates(v, a_scale) ? 1 : 0;
  float* ph = row + (ch & ~7) + ((ch >> 2) & 1) * 2;
  if (nv == 4) {
    *reinterpret_cast<h4*>(ph) = hi;
    *reinterpret_cast<h4*>(ph + 4) = lo;
  } else {
    _Float16* hh = reinterpret_cast<_Float16*>(ph);
    _Float16* ll = reinterpret_cast<_Float16*>(ph + 4);
    if (nv > 0) { hh[0] = hi.x; ll[0] = lo.x; }
    if (nv > 1) { hh[1] = hi.y; ll[1] = lo.y; }
    if (nv > 2) { hh[2] = hi.z; ll[2] = lo.z; }
  }
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// ---- weight packing: (Cout, Cin, kh, kw) fp32 -> fp16 hi / lo in the consumption order of each kernel family ----
struct PackParams {
  int Cout, Cin, kh, kw, G, T, ncb, Npad, vertical;
  unsigned char cb_seg[MAX_CB];
  short cb_c0[MAX_CB];
  short seg_start[4];     // first input channel (in the concatenated Cin order) of each segment
  short seg_count[4];
  float w_scale;
};

// ---- the dispatch: ONE policy (every switch the kernel choice reads) and ONE plan per launch (conv_igemm.hip: plan_conv) ----
struct ConvPolicy {
  bool spatial = true;       // 3x3 stride-1 convolutions on 8 x 16 image patches (rnnpose_conv_spatial_tiles)
  bool strip = true;         // false: never the strip kernels (conv_strip.hip); true: automatic (rnnpose_conv_strip)
  bool two_wave = true;      // two-wave workgroups (c_out <= 64: the encoder's 64-channel layers at 240 x 320) in the automatic choice
  // Column tiles per wave: 1 unless forced (0: the least-waste shape over both).  The two-tile form (one wave per SIMD, 160 x 64 per wave,
  // 14 fragment reads per 30 MFMAs instead of 12 per 15) is built, tested and SLOWER (r04, profiles/r04_strip_ni2.txt: GRU z|r at B = 8
  // 84.6 vs 76.4 us, even with every memory operation compiled out 70 vs 56 us): a lone wave does not keep its SIMD's matrix pipe busy.
  int ni = 1;
  bool small = true;         // 32-row strips in the automatic choice
  bool s2 = true;            // stride-2 3x3 layers as strips over parity planes (false: the 128-row kernel's tap-per-staging mode)
  bool small32 = true;       // r06: 32- / 96-row strips for launches of <= 256 / 512 waves of 160-row strips (rnnpose_conv_strip(6): off)
  bool persist = false;      // r06: persistent launches of the fp32-source forms (rnnpose_conv_strip(7): ON).  Built, bit-identical, and SLOWER: the
                             // encoder's 64 -> 64 layer at B = 8 takes 190-255 us instead of 155-190 (profiles/r06_persistent_strips.txt) -- OFF by default
  bool ksplit = true;        // K split of launches with few tiles when the caller provides a workspace (rnnpose_conv_ksplit)
  int ks_max_tiles = 24, ks_max_splits = 4;      // (rnnpose_conv_ksplit_limits: measurement)
};

// How ONE launch runs: a pure function of the descriptor and the policy.  The size queries, the launch and strip_launch all read this.
struct ConvPlan {
  int rows;                          // kernel family: 0 = the 128-row kernels, 32 / 96 / 160 = the strip kernels of that height
  int ni, nw;                        // strips: column tiles of 32 per wave, waves
  bool spatial, wide, wide22, deep;  // image patches instead of pixel runs; the 128-row tile shapes (128x128 in 4 column waves / 2x2 waves, deep pipeline)
  int U, V, su, sv, G, T, du0, dv0, stride, Uin, Vin, gkw, dvg0;      // geometry, as in KParams
  int Ho, Wo;                        // output extents
  bool per_image;                    // no tile straddles two images (statistics, fused normalisation, patches)
  int tiles_per_image;               // = records per image of tile_stats
  int sp_tx, sp_ty;                  // patches per image row / column (spatial)
  int n_mt, n_nt;
  unsigned nwg;                      // workgroups of the launch (K splits included; a persistent strip launch shrinks it to the chip)
  int products;                      // fp16 MFMA products per multiply-add: 3, or 1 (single_product honoured)
  bool persist;                      // strips: a form that has a persistent instantiation, and the policy asks for it
  int ksplit;                        // K split: workgroups per tile (1 = none) over the caller's workspace [arrival counters | partial accumulators]
};

// conv_strip.hip: the strip kernels (160-row strips, operands by LDS-DMA).  strip_waves / strip_rows: for plan_conv only
int strip_waves(int c_out, int ni);                            // workgroup shape: 16 * (32-column tiles per wave) + waves; 0 = unsupported width
long long strip_s2_halfs(int c_in, int kh, int kw, int ncb, int Npad, int n_seg);   // size of the stride-2 copy of a layer's packed weights (0: none)
// strip height (160 / 96 / 32 rows) a launch of `batch` images takes, 0 = not a strip launch; request: 0 automatic, else the height to force
int strip_rows(const ConvPolicy& pol, int H, int W, int kh, int kw, int stride, int c_out, int batch, int request);
// launches the strip kernel the plan names for the filled parameter block; sets off32 and, for a persistent launch, n_tiles / stagger.
// hlin: split-tensor sources (LDS-DMA); else fp32 sources through registers (+ fused normalisation when p.in_mr).
int strip_launch(KParams& p, const ConvPlan& pl, int kh, int kw, bool hlin, hipStream_t st);
int strip_launch_r32(const KParams& p, int nw, int ni, bool spatial, bool hlin, bool norm, unsigned nwg, hipStream_t st);      // conv_strip_r32.hip
int strip_launch_r96(const KParams& p, int nw, int ni, bool spatial, bool hlin, bool norm, unsigned nwg, hipStream_t st);      // conv_strip_r96.hip (r06)
int strip_launch_p1(const KParams& p, int nw, int ni, bool spatial, bool hlin, bool norm, unsigned nwg, hipStream_t st);       // conv_strip_p1.hip: 160-row strips, single product
void strip_pack(const float* w, _Float16* pk, const PackParams& q, hipStream_t st);

}  // namespace rpconv
