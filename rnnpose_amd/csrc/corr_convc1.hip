// a3 + a4 (r06): the window lookup and BasicMotionEncoder.convc1 as ONE kernel --
//     corr = CorrBlock.__call__(coords)      thirdparty/raft/corr.py:36-57 (bilinear_sampler: thirdparty/raft/utils/utils.py:57-71)
//     cor  = relu(convc1(corr))              thirdparty/raft/update.py:80,87          (chained by model/CFNet.py:147-152)
// The two-kernel path (csrc/corr_lookup.hip -> csrc/conv1x1_resident.hip) writes the (B,h,w,324) window features to HBM and reads
// them back (25 MB each way per half-batch launch) across a kernel boundary.  Here a workgroup owns 32 consecutive pixels and ALL 256
// output columns, like the resident 1x1 kernel, but its activation tile is COMPUTED, level by level, and never complete in LDS:
//
//   for level l = 0..3:   (a) the four waves fetch the 10 x 10 footprints of 8 pixels each (cooperative loads as in corr_lookup.hip,
//                             all 16 loads of a lane in flight at once) into a 13-KB LDS buffer;                       barrier
//                         (b) 256 threads = 32 pixels x 8 groups of window rows form the level's 81 bilinear taps in fp32 and split
//                             them (fp16 hi | lo, csrc/f16x3.cuh) into a RING of four 32-channel blocks (16 KB);           barrier
//                         (c) the channel blocks the level COMPLETED (0-1 | 2-4 | 5-6 | 7-10: 81 channels do not end on block
//                             boundaries, the partial block stays in its ring slot) go through v_mfma_f32_16x16x32_f16 with the
//                             weights as B fragments straight from convc1's packed array, two blocks ahead;               barrier
//
// 29 KB of LDS per workgroup (33 KB with the epilogue's staging tile aliasing it) instead of 71 KB for "whole tile resident + footprints":
// FOUR workgroups per CU, so a half-batch launch (600 workgroups) is one round and one workgroup's footprint latency runs under the
// others' MFMAs.  (First form of this fusion, r06: the LOOKUP staging phase in front of the unchanged resident kernel -- 71 KB, two
// workgroups per CU, two rounds: 44.5 us against 23.2 + 18.7 for the two kernels; profiles/r06_lookup_convc1_fusion.txt.)
// Numerics: the operations of the two-kernel path per element (fp32 taps in the same order, one split, the same MFMA sequence per block).
#include <type_traits>
#include "corr_lookup.cuh"
#include "resident_tile.cuh"

namespace {

using namespace rplookup;
using namespace rptile;

constexpr int NCB = 11;         // 4 x 81 = 324 channels = 11 blocks of 32 (block 10: channels 320 .. 323, then zeros)
constexpr int NSLOT = 4;        // ring of channel blocks: [hi plane 32 x 32 | lo plane] fp16 = 4 KB each
constexpr int GP = 8;           // pixels per wave in the footprint fetch
constexpr int SLOT_HALFS = 2 * MQ * 32;
constexpr int RING_BYTES = NSLOT * SLOT_HALFS * 2;
constexpr int FOOT_BYTES = MQ * FS * 4;
constexpr int EPI_BYTES = MQ * RSF * 4;
constexpr int LDS_BYTES = RING_BYTES + FOOT_BYTES > EPI_BYTES ? RING_BYTES + FOOT_BYTES : EPI_BYTES;
template <int V>
using Int = std::integral_constant<int, V>;

struct CParams {
  const float* pyr;             // the whole pyramid buffer (csrc/corr_pyramid.hip layout)
  const float* coords;          // (images of this launch, 2, h, w): window centres at level-0 scale
  LookupInfo info;
  int N;                        // h * w
  long long p_off;              // pyramid row of pixel 0 of this launch (= first image x N)
  const uint4* wpk;             // convc1 packed by rnnpose_conv1x1_resident_pack_f16x3 (c_in = 324): record (cb * 16 + column tile) * 128 + part * 64 + lane
  TileOut out;                  // (resident_tile.cuh)
};

// x * s = hi + lo for ONE value: the arithmetic of rp::split4 (round to nearest, clamped at +-65504)
__device__ __forceinline__ void split1(float v, float s, _Float16& hi, _Float16& lo) {
  const float x = v * s;
  const _Float16 cap = static_cast<_Float16>(65504.f);
  _Float16 h = static_cast<_Float16>(x);
  h = h > cap ? cap : (h < -cap ? -cap : h);
  _Float16 l = static_cast<_Float16>(x - static_cast<float>(h));
  l = l > cap ? cap : (l < -cap ? -cap : l);
  hi = h;
  lo = l;
}

__global__ __launch_bounds__(8 * MQ, 3) void corr_convc1_kernel(const CParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
  _Float16* const ring = reinterpret_cast<_Float16*>(lds);            // slot s: [hi 32 x 32 | lo 32 x 32], row * 32 + swizzled chunk * 8 + e
  float* const foot = reinterpret_cast<float*>(lds + RING_BYTES);     // [pixel of the tile][FS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = static_cast<long long>(blockIdx.x) * MQ;
  const int N = p.N;

  // ---- per-thread pixels: the one whose footprint base this lane carries in the fetch (pixel GP * wave + (lane & 7) of the tile) and
  //      the one whose taps it forms (pixel tid & 31); window centres at level-0 scale
  const long long gfirst = m0 + GP * wave;
  const long long gleft = p.out.M - gfirst;
  const int gnpix = gleft >= GP ? GP : (gleft > 0 ? static_cast<int>(gleft) : 1);
  const long long gfrow = p.p_off + (gleft > 0 ? gfirst : p.out.M - 1);
  float gcx, gcy, tcx, tcy;
  int bg, pixg;
  {
    const long long gp = gfirst + (lane & (GP - 1)), tp = m0 + (tid & 31);
    const long long gpc = gp < p.out.M ? gp : p.out.M - 1;
    int b, pix;
    decode_px(gpc, N, b, pix);
    const float2 gc = read_centre(p.coords, b, pix, N);
    gcx = gc.x, gcy = gc.y;
    decode_px(p.p_off + gpc, N, bg, pixg);
    decode_px(tp < p.out.M ? tp : p.out.M - 1, N, b, pix);
    const float2 tc = read_centre(p.coords, b, pix, N);
    tcx = tc.x, tcy = tc.y;
  }
  const int r = tid & 31, g = tid >> 5;                       // tap phase: tile row, group of window rows: g = 0: j = 0, 1; g >= 1: j = g + 1
  const int j0 = g == 0 ? 0 : g + 1, nj = g == 0 ? 2 : 1;
  const int swz = ((r >> 2) & 1) << 1;
  int sat_n = 0;
  const bool tap_in = m0 + r < p.out.M;                       // range guard: a padding row (the taps of the last pixel again) is not counted again

  // ---- MFMA side (resident_tile.cuh): 4 column tiles x 2 pixel tiles x 3 split products = 24 MFMAs per channel block
  const int l15 = lane & 15, lq = lane >> 4;
  const int phys = lq ^ (((l15 >> 2) & 1) << 1);
  f32x4 acc[2][CT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 bq[2][CT][2];                                                 // ring of 2 stages x column tile x (hi, lo)
  load_weights(bq[0], p.wpk, 0, wave, lane);
  load_weights(bq[1], p.wpk, 1, wave, lane);
  __builtin_amdgcn_sched_barrier(0);

  // one pyramid level: fetch -> taps -> the channel blocks [CB0, CB1) it completes
  auto level = [&](auto L_, auto CB0_, auto CB1_) __attribute__((always_inline)) {
    constexpr int lvl = decltype(L_)::value, CB0 = decltype(CB0_)::value, CB1 = decltype(CB1_)::value;
    constexpr float inv = 1.0f / static_cast<float>(1 << lvl);
    int bx, by;
    float ax, ay;
    footprint_base(gcx * inv, gcy * inv, bx, by, ax, ay);
    gather_batches<GP>(AddrSelect{wave_maps(p.pyr, p.info, lvl, N, bg, pixg, gfrow)}, lane, gnpix, bx, by, foot + (GP * wave) * FS);
    if (lvl == 3) {      // block 10 = channels 320 .. 351: zeros behind channel 323 (its slot held block 6, consumed before the last barrier)
      reinterpret_cast<uint4*>(ring + ((NCB - 1) % NSLOT) * SLOT_HALFS)[tid] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    footprint_base(tcx * inv, tcy * inv, bx, by, ax, ay);
    window_taps<2>(foot + r * FS + j0 * FP, ax, ay, nj, [&](int i, int jj, float v) {
      const int c = lvl * (WIN * WIN) + i * WIN + j0 + jj;            // channel (x-major window) -> ring slot of its block, row r, swizzled chunk
      const int k = c & 31;
      const int off = ((c >> 5) % NSLOT) * SLOT_HALFS + r * 32 + (((k >> 3) ^ swz) << 3) + (k & 7);
      _Float16 hi, lo;
      split1(v, p.out.a_scale, hi, lo);
      if (p.out.sat && tap_in) sat_n += !(fabsf(v) <= 65504.f / p.out.a_scale) ? 1 : 0;
      ring[off] = hi;
      ring[off + MQ * 32] = lo;
    });
    __syncthreads();
#pragma unroll
    for (int cb = CB0; cb < CB1; ++cb) {
      const _Float16* sl = ring + (cb % NSLOT) * SLOT_HALFS;
      const int st = cb & 1;
      block_step(acc, sl, sl + MQ * 32, bq[st], l15, phys);
      __builtin_amdgcn_sched_barrier(0);
      if (cb + 2 < NCB) load_weights(bq[st], p.wpk, cb + 2, wave, lane);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();         // the next level overwrites the footprints and the consumed ring slots
  };
  level(Int<0>{}, Int<0>{}, Int<2>{});          // channels   0 ..  80: blocks 0, 1 complete (block 2 up to channel 80)
  level(Int<1>{}, Int<2>{}, Int<5>{});          // channels  81 .. 161: blocks 2, 3, 4
  level(Int<2>{}, Int<5>{}, Int<7>{});          // channels 162 .. 242: blocks 5, 6
  level(Int<3>{}, Int<7>{}, Int<NCB>{});        // channels 243 .. 323: blocks 7 .. 10
  if (p.out.sat && sat_n) atomicAdd(p.out.sat, static_cast<unsigned long long>(sat_n));

  // ---- epilogue through an LDS tile aliasing ring + footprints (the last barrier above has passed)
  tile_epilogue(p.out, acc, reinterpret_cast<float*>(lds), m0, tid);
}

}  // namespace

// Images [b0, b1) of a pyramid built for B_total images; coords (b1 - b0, 2, h, w) and dst (b1 - b0, h, w, dst_c_stride) are the sub-batch tensors.
extern "C" int rnnpose_corr_lookup_convc1_f16x3(const float* pyramid, const float* coords, int B_total, int b0, int b1, int h, int w,
                                                int levels, int radius, const void* w_packed, const float* bias, float a_scale,
                                                float w_scale, int relu, float* dst, int dst_c_stride, int dst_c_offset, int dst_split,
                                                rnnpose_stream_t stream) {
  const char* fn = "rnnpose_corr_lookup_convc1_f16x3";
  RP_REQUIRE(pyramid && coords && w_packed && bias && dst, fn, "null pointer");
  RP_REQUIRE(levels == 4 && radius == R, fn, "4 pyramid levels, radius 4 (324 window features = the c_in the weights were packed for)");
  CParams p{};
  if (int e = lookup_info(fn, B_total, b0, b1, h, w, levels, p.info)) return e;
  if (int e = check_tile_out(fn, dst, dst_c_stride, dst_c_offset, dst_split, a_scale, w_scale, w_packed)) return e;
  const long long n_pixels = static_cast<long long>(b1 - b0) * h * w;
  RP_REQUIRE(n_pixels < (1LL << 31), fn, "bad pixel count");
  p.pyr = pyramid; p.coords = coords; p.N = h * w; p.p_off = static_cast<long long>(b0) * h * w;
  p.wpk = static_cast<const uint4*>(w_packed);
  p.out = tile_out(bias, a_scale, w_scale, relu, dst, dst_c_stride, dst_c_offset, dst_split, n_pixels);
  const dim3 grid(static_cast<unsigned>(rp::cdiv(n_pixels, MQ))), block(8 * MQ);
  hipLaunchKernelGGL(corr_convc1_kernel, grid, block, 0, rp::as_stream(stream), p);
  return rp::check_launch(fn);
}
