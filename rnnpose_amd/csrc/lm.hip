// a9-a11: the Levenberg-Marquardt / Gauss-Newton pose step, fully on device.
//   lm_normal_eq   Hm = sum v w J^T J, bv = sum v w J^T r  (fp64)   geometry/transformation.py:286-297
//   lm_solve       damping, 6x6 Cholesky, NaN->0, clamp, SE(3) exp, G <- exp(xi) G
//                  transformation.py:300-306, geometry/cholesky.py:32-50, geometry/se3.py:228-281,303-306
// The reference materialises J as a (B,1,H,W,2,6) fp64 tensor (29 MB/image at 480x640) and reduces it
// with two einsums; here every pixel's 2x6 Jacobian lives in registers, each thread accumulates the 21
// upper-triangle + 6 right-hand-side sums in fp64 over a strided set of pixels, a wave64 shuffle tree and
// one LDS hop reduce the workgroup, and per-workgroup partials are summed in FIXED order by the solve
// kernel (deterministic: no atomics).  HBM traffic = target + weight + depth read once (16 B/pixel).
//   lm_rgbd_eq     the same sums with an opt-in 3-D residual from the OBSERVED depth of an RGB-D camera (no counterpart in the reference;
//                  include/rnnpose_hip.h): + four gathered taps per pixel
// ONE kernel, lm_eq_kernel<DEPTH, FUSED>, in two instantiation families: DEPTH = false the plain step, DEPTH = true the depth-aware
// one; one launch path, launch_lm_iteration, and one checked loop, lm_run, under all LM entries.
#include <cmath>

#include "geometry.cuh"

namespace {

using rp::Intr;
using rp::Pose;

constexpr int NACC = 27;        // 21 (upper triangle of H, row-major) + 6 (b)
constexpr int NACC_RGBD = 29;   // + the depth term's statistics: [27] active pixels, [28] sum v w omega |r3|^2
constexpr int PSTRIDE = 32;     // doubles per partial record
constexpr int LM_THREADS = 256;
// r04 sweep (B = 4 / B = 8 x 480 x 640, us per fused LM step): 1024 px per workgroup, 4 in flight 40.6 / 70.7; 2048, 4 (r03) 35.9 / 52.4;
// 4096, 8 33.9 / 40.5; 8192, 8 37.1 / 46.9; 16384, 16 58.7 / 59.6 -- fewer partial records shorten the last-arrival tail until the
// main loop of a workgroup becomes the chain
#ifndef RP_LM_BATCH
#define RP_LM_BATCH 8
#endif
#ifndef RP_LM_PPB
#define RP_LM_PPB 4096
#endif
constexpr int LM_BATCH = RP_LM_BATCH;      // pixels per thread whose loads are in flight together
constexpr int LM_PIX_PER_BLOCK = RP_LM_PPB;   // 75 workgroups per 480x640 image
constexpr int LM_MAX_BLOCKS = 256;

__host__ __device__ inline int lm_blocks_per_image(long long P) {
  long long n = (P + LM_PIX_PER_BLOCK - 1) / LM_PIX_PER_BLOCK;
  if (n < 1) n = 1;
  if (n > LM_MAX_BLOCKS) n = LM_MAX_BLOCKS;
  return static_cast<int>(n);
}

__device__ __forceinline__ double shfl_down_f64(double v, int d) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_down(lo, d);
  hi = __shfl_down(hi, d);
  return __hiloint2double(hi, lo);
}

// FUSED tail (r03): the workgroup that arrives LAST for its image (device-scope ticket, one counter per image at the end of
// the workspace) sums the partial records, damps, solves and updates the pose -- lm_finalize + lm_solve_update without their
// two launches and kernel boundaries (~13 us + 2 x ~1.5 us per LM step, 48 steps per refinement).  r02 tried "finalize + solve
// as one 256-thread launch" and lost (the serial fp64 solve waited behind the launch); here it runs in a block that is already
// resident, while the other images' blocks are still computing.  Hand-off = MI355X_MICROARCH.md's counter form: plain stores ->
// barrier -> lane-0 agent-scope release (+ asm vmcnt(0)) -> relaxed agent fetch_add; the last arriver: agent-scope acquire ->
// barrier -> plain loads.  The last arriver resets the counter (zero-initialised with the workspace).
struct LmTail {
  int* tickets;                 // (B) arrival counters, zero between launches
  double* Hm;                   // (B,6,6), (B,6): undamped system, as the unfused path returns it
  double* bv;
  const float* G_in;            // pose the Jacobians were built with (may alias G_out)
  float* G_out;
  float* xi;
  int* info;
  double ep, lm, max_update;
  double* dstats;               // (B,2) depth-term statistics of lm_eq_kernel<true, .>, or null (always null for the plain kernel)
};
__device__ void lm_finalize_block_one(const double* __restrict__ partials, int nblk, int b, double* __restrict__ Hm, double* __restrict__ bv,
                                      double* __restrict__ dstats);
__device__ __forceinline__ void lm_solve_one(const double* Hm, const double* bv, const float* G, int b, double ep, double lm, double max_update,
                             float* G_new, float* xi_out, int* info);

// one pixel's contribution to the 21 + 6 sums (fp64), J and the residual from the TRANSFORMED point (NA >= NACC: the first 27 sums)
template <int NA>
__device__ __forceinline__ void lm_accumulate(double (&acc)[NA], float wgt, float dep, float tx, float ty, int x, int y, int target_mode,
                                          float eps, const Intr& k, const Pose& g) {
  const float Z = dep + eps;
  if (target_mode != 0) {
    tx += static_cast<float>(x);
    ty += static_cast<float>(y);
  }
  const rp::Reproj r = rp::reproject(Z, static_cast<float>(x), static_cast<float>(y), k, g);
  const bool valid = (r.Z0 > rp::kMinDepthValid) && (r.Z1 > rp::kMinDepthValid);   // transformation.py:289
  const double vw = valid ? static_cast<double>(wgt) : 0.0;
  // J_pi in fp32 (projective_ops.py:118-124): zeros where clamped Z <= 0.02
  const bool tiny = r.Zc <= rp::kMinDepthProj + 0.01f;
  const float zi1 = tiny ? 0.f : 1.0f / r.Zc;
  const float zi2 = tiny ? 0.f : 1.0f / (r.Zc * r.Zc);
  const double a = static_cast<double>(k.fx * zi1);
  const double c = static_cast<double>(-k.fx * r.X1 * zi2);
  const double d = static_cast<double>(k.fy * zi1);
  const double e = static_cast<double>(-k.fy * r.Y1 * zi2);
  const double X1 = r.X1, Y1 = r.Y1, Z1 = r.Z1;
  // J = J_pi * J_T with J_T = [I | -[X']x] built from the TRANSFORMED point (transformation.py:27-46,85-90)
  double J0[6], J1[6];
  J0[0] = a;   J0[1] = 0.0; J0[2] = c; J0[3] = c * Y1;            J0[4] = a * Z1 + c * (-X1); J0[5] = a * (-Y1);
  J1[0] = 0.0; J1[1] = d;   J1[2] = e; J1[3] = d * (-Z1) + e * Y1; J1[4] = e * (-X1);          J1[5] = d * X1;
  const double r0 = static_cast<double>(tx) - static_cast<double>(r.u);
  const double r1 = static_cast<double>(ty) - static_cast<double>(r.v);
  int idx = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wi0 = vw * J0[i], wi1 = vw * J1[i];
#pragma unroll
    for (int jj = i; jj < 6; ++jj) {
      acc[idx] += wi0 * J0[jj] + wi1 * J1[jj];
      ++idx;
    }
    acc[21 + i] += wi0 * r0 + wi1 * r1;
  }
}

// the workgroup's 27 sums -> its partial record; FUSED: the last workgroup of the image finalizes, solves and updates the pose
// NA = NACC, or NACC_RGBD for lm_eq_kernel<true, .>: its two statistics ride in slots 27 and 28 of the same 32-slot butterfly and record
template <bool FUSED, int NA = NACC>
__device__ __forceinline__ void lm_reduce_tail(double (&acc)[NA], double* __restrict__ partials, const LmTail& tail, int b, int nblk, int bx) {
  static_assert(NA <= PSTRIDE, "the partial record has 32 slots");
  __shared__ double red[LM_THREADS / 64][NA];
  __shared__ int is_last;
  // wave reduction as a butterfly REDUCE-SCATTER (r04): at offset o = 32, 16, 8, 4, 2 a lane keeps the half of its (32, 16, 8, 4,
  // 2) slots that bit o of its lane number selects, sends the other half to lane ^ o and adds what it receives -- 16 + 8 + 4 + 2 +
  // 1 exchanged doubles per lane, after which lanes 2k and 2k + 1 hold the two halves of slot k = lane >> 1 (bit order below) and one
  // last exchange completes it: 32 double exchanges per lane instead of the 27 x 6 = 162 of a full butterfly per accumulator
  // (the reduction was as long as the fp64 accumulation itself).  Fixed tree: deterministic.  Then across the 4 waves through LDS.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    double v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = i < NA ? acc[i] : 0.0;
#pragma unroll
    for (int o = 32, n = 32; o >= 2; o >>= 1, n >>= 1) {         // n slots live before the step, n / 2 after
      const bool hi = (lane & o) != 0;
#pragma unroll
      for (int i = 0; i < n / 2; ++i) {
        const double send = hi ? v[i] : v[i + n / 2];
        const double keep = hi ? v[i + n / 2] : v[i];
        v[i] = keep + rp::shfl_xor_f64(send, o);
      }
    }
    const double tot = v[0] + rp::shfl_xor_f64(v[0], 1);
    // slot held by this lane pair: bit 5 of the lane chose the upper half of 32, bit 4 of 16, ... bit 1 of 2
    const int slot = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
    if (!(lane & 1) && slot < NA) red[wave][slot] = tot;
  }
  __syncthreads();
  if (threadIdx.x < NA) {
    double v = red[0][threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < LM_THREADS / 64; ++wv) v += red[wv][threadIdx.x];
    partials[(static_cast<long long>(b) * nblk + bx) * PSTRIDE + threadIdx.x] = v;
  }
  if constexpr (FUSED) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (the compiler may drop the wait behind buffer_wbl2: guide, G16 pitfall)
      const int t = __hip_atomic_fetch_add(&tail.tickets[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      is_last = (t == nblk - 1) ? 1 : 0;
      if (is_last) {
        __hip_atomic_store(&tail.tickets[b], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        // ONE agent-scope acquire per workgroup: it invalidates this CU's vector L1 (buffer_inv sc1), which is per CU, not per
        // thread -- followed by the barrier below before any thread of the block loads the other workgroups' partial records
        // (cdna_hip_programming.md, Guideline 16: "consumer: one relaxed poll -> one agent acquire -> __syncthreads() -> plain loads")
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
    }
    __syncthreads();
    if (!is_last) return;
    lm_finalize_block_one(partials, nblk, b, tail.Hm, tail.bv, tail.dstats);   // (ends with the values in global memory, written by this block)
    __syncthreads();
    if (threadIdx.x == 0) lm_solve_one(tail.Hm, tail.bv, tail.G_in, b, tail.ep, tail.lm, tail.max_update, tail.G_out, tail.xi, tail.info);
  }
}

// ---- the depth-aware step (RGB-D): an opt-in 3-D residual from the OBSERVED depth in the same 27 sums -------------------------------
// For a crop pixel with matched position t (crop pixel-index coordinates): where t falls in the full observed frame (the affine map
// that made the image crop, zoom_crop.hip's zoom_crop_pixel continued to non-integer positions), the observed depth zo there
// (hole-aware: bilinear over four present taps that lie within edge_tol of each other, else the nearest tap, else no term), the
// observed point Y = zo K_obs^-1 (ix, iy, 1) and, where v holds and |Y.z - X1.z| <= depth_gate, the residual r3 = Y - X1 with
// J_T = [I | -[X1]x] and the scale omega = depth_weight fx fy / Zc^2 (0 where the `tiny` clamp applies): a lateral 3-D error in the
// pixel^2 units of the 2-D term.  Per-pixel quantities are fp32 in the order written here, the sums fp64.
struct LmDepthTerm {
  const float* obs;             // (S,Ho,Wo) observed depth, 0 / negative / non-finite = no measurement
  const int* src_index;         // (B) frame of every object, or null: object b reads frame b
  const float* theta;           // (B,2,3) the views' crop maps
  const float* K_obs;           // (B,3,3) full-frame intrinsics
  int S, Ho, Wo;
  float weight, gate, edge_tol;
};

struct LmFrame {                // the per-image constants of the depth term, loaded once per workgroup
  const float* obs;             // frame of this object (frame 0 with ok == false)
  bool ok;                      // the frame index is inside [0, S)
  float th[6];
  Intr ko;
  int Ho, Wo;
};

// position of the target of crop pixel (x, y) in the observed frame, pixel-index coordinates (fp32, zoom_crop_pixel's operation order)
__device__ __forceinline__ void lm_obs_position(float tx, float ty, int x, int y, int target_mode, int H, int W, const LmFrame& f, float& ix,
                                                float& iy) {
  if (target_mode != 0) {                                            // (lm_accumulate's own fp32 sum)
    tx += static_cast<float>(x);
    ty += static_cast<float>(y);
  }
  const float bx = (2.f * tx + 1.f) / W - 1.f, by = (2.f * ty + 1.f) / H - 1.f;
  const float gx = f.th[0] * bx + f.th[1] * by + f.th[2];
  const float gy = f.th[3] * bx + f.th[4] * by + f.th[5];
  ix = ((gx + 1.f) * f.Wo - 1.f) * 0.5f;
  iy = ((gy + 1.f) * f.Ho - 1.f) * 0.5f;
}

// north-west tap of (ix, iy); a non-finite or huge position gets a tap far outside every frame
__device__ __forceinline__ void lm_obs_corner(float ix, float iy, int& x0, int& y0) {
  const bool sane = fabsf(ix) < 1.0e8f && fabsf(iy) < 1.0e8f;      // (false for NaN and infinity)
  x0 = sane ? static_cast<int>(floorf(ix)) : -10;
  y0 = sane ? static_cast<int>(floorf(iy)) : -10;
}

__device__ __forceinline__ bool lm_tap_present(bool inside, float z) { return inside && z > 0.f && __builtin_isfinite(z); }

// the observed point at (ix, iy) from the four taps (nw, ne, sw, se; loaded at CLAMPED positions: `inside` decides) -> has a depth?
__device__ __forceinline__ bool lm_obs_point(float ix, float iy, const float (&z)[4], const LmFrame& f, float edge_tol, float& Yx, float& Yy,
                                             float& Yz) {
  int x0, y0;
  lm_obs_corner(ix, iy, x0, y0);
  const bool vx0 = x0 >= 0 && x0 < f.Wo, vx1 = x0 + 1 >= 0 && x0 + 1 < f.Wo;
  const bool vy0 = y0 >= 0 && y0 < f.Ho, vy1 = y0 + 1 >= 0 && y0 + 1 < f.Ho;
  const bool p00 = lm_tap_present(f.ok && vy0 && vx0, z[0]), p10 = lm_tap_present(f.ok && vy0 && vx1, z[1]);
  const bool p01 = lm_tap_present(f.ok && vy1 && vx0, z[2]), p11 = lm_tap_present(f.ok && vy1 && vx1, z[3]);
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
  float zo;
  bool has;
  const float zmax = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])), zmin = fminf(fminf(z[0], z[1]), fminf(z[2], z[3]));
  if (p00 && p10 && p01 && p11 && zmax - zmin <= edge_tol) {
    // weights and order of zoom_crop_pixel (torch's grid_sampler: nw, ne, sw, se)
    const float w00 = (fx1 - ix) * (fy1 - iy), w10 = (ix - fx0) * (fy1 - iy), w01 = (fx1 - ix) * (iy - fy0), w11 = (ix - fx0) * (iy - fy0);
    zo = 0.f;
    zo += z[0] * w00;
    zo += z[1] * w10;
    zo += z[2] * w01;
    zo += z[3] * w11;
    has = true;
  } else {                                                           // a hole or a depth edge under the footprint: the nearest tap, if present
    const bool east = floorf(ix + 0.5f) != fx0, south = floorf(iy + 0.5f) != fy0;
    zo = south ? (east ? z[3] : z[2]) : (east ? z[1] : z[0]);
    has = south ? (east ? p11 : p01) : (east ? p10 : p00);
  }
  Yx = zo * (ix - f.ko.cx) / f.ko.fx;                                // Y = zo K_obs^-1 (ix, iy, 1), the back-projection of geometry.cuh
  Yy = zo * (iy - f.ko.cy) / f.ko.fy;
  Yz = zo;
  return has;
}

// one ACTIVE pixel's depth term in the 21 + 6 sums and the cost statistic: H += s J_T^T J_T, b += s J_T^T r3 with J_T = [I | A],
// A = -[X1]x:  J_T^T J_T = [I A; A^T A^T A],  A^T A = |X1|^2 I - X1 X1^T,  J_T^T r3 = (r3, X1 x r3)
__device__ __forceinline__ void lm_accumulate_depth(double (&acc)[NACC_RGBD], double s, float X1f, float Y1f, float Z1f, float Yx, float Yy,
                                                    float Yz) {
  const double X = X1f, Y = Y1f, Z = Z1f;
  const double rx = static_cast<double>(Yx) - X, ry = static_cast<double>(Yy) - Y, rz = static_cast<double>(Yz) - Z;
  // upper triangle, row-major: row 0 at 0, row 1 at 6, row 2 at 11, row 3 at 15, row 4 at 18, row 5 at 20
  acc[0] += s;            acc[4] += s * Z;         acc[5] += s * (-Y);
  acc[6] += s;            acc[8] += s * (-Z);      acc[10] += s * X;
  acc[11] += s;           acc[12] += s * Y;        acc[13] += s * (-X);
  acc[15] += s * (Y * Y + Z * Z);  acc[16] += s * (-(X * Y));        acc[17] += s * (-(X * Z));
  acc[18] += s * (X * X + Z * Z);  acc[19] += s * (-(Y * Z));
  acc[20] += s * (X * X + Y * Y);
  acc[21] += s * rx;
  acc[22] += s * ry;
  acc[23] += s * rz;
  acc[24] += s * (Y * rz - Z * ry);
  acc[25] += s * (Z * rx - X * rz);
  acc[26] += s * (X * ry - Y * rx);
  acc[28] += s * (rx * rx + ry * ry + rz * rz);
}

struct LmGate {                 // one pixel's gate decision, and what its depth term is built from
  rp::Reproj r;
  bool valid, active;
  float Yx, Yy, Yz;
};

// the gate of one pixel (fp32, no fp64 chain): the observed point from the taps and whether the depth term is active there
__device__ __forceinline__ LmGate lm_depth_gate(float dep, float tx, float ty, int x, int y, int target_mode, float eps, const Intr& k, const Pose& g,
                                                int H, int W, const LmFrame& f, const float (&z)[4], const LmDepthTerm& dt) {
  LmGate q;
  q.r = rp::reproject(dep + eps, static_cast<float>(x), static_cast<float>(y), k, g);
  q.valid = (q.r.Z0 > rp::kMinDepthValid) && (q.r.Z1 > rp::kMinDepthValid);
  float ix, iy;
  lm_obs_position(tx, ty, x, y, target_mode, H, W, f, ix, iy);
  const bool has = lm_obs_point(ix, iy, z, f, dt.edge_tol, q.Yx, q.Yy, q.Yz);
  q.active = has && q.valid && fabsf(q.Yz - q.r.Z1) <= dt.gate;
  return q;
}

// the depth term of one pixel behind the 2-D term: scale omega, then the sums of an ACTIVE pixel
__device__ __forceinline__ void lm_depth_step(double (&acc)[NACC_RGBD], const LmGate& q, float wgt, float depth_weight, const Intr& k) {
  const bool tiny = q.r.Zc <= rp::kMinDepthProj + 0.01f;
  const float zi2 = tiny ? 0.f : 1.0f / (q.r.Zc * q.r.Zc);
  const float omega = depth_weight * (k.fx * k.fy) * zi2;
  const double s = (q.valid ? static_cast<double>(wgt) : 0.0) * static_cast<double>(omega);
  // a pixel without a measurement, outside the gate or with a zero scale adds NOTHING: with depth_weight = 0 or an empty observed
  // depth the 27 sums are the plain step's bit for bit
  if (q.active && s != 0.0) lm_accumulate_depth(acc, s, q.r.X1, q.r.Y1, q.r.Z1, q.Yx, q.Yy, q.Yz);
}

// crop pixel t -> (x, y).  t < H*W < 2^31: 32-bit division (64-bit is a software routine)
__device__ __forceinline__ void lm_pixel_xy(long long t, int W, int& x, int& y) {
  const unsigned tu = static_cast<unsigned>(t);
  y = static_cast<int>(tu / static_cast<unsigned>(W));
  x = static_cast<int>(tu - static_cast<unsigned>(y) * static_cast<unsigned>(W));
}

// ---- the ONE normal-equation kernel: trips, loads, skip, 2-D sums and tail; DEPTH adds the depth term at four sites -----------------------
// DEPTH = false is the plain step, DEPTH = true the depth-aware one (dt is read by it alone): the same trips, the same order of the 2-D
// sums (lm_accumulate itself), the same tail, so that the depth-aware step with its term off IS the plain step.  The kernel itself is
// the template: the same body as a device function under two thin kernels is optimised before it is inlined, outside a kernel's
// launch bounds, and comes out with the trip's loads and waits arranged otherwise (tests/test_isa_guard.py refuses that form).
template <bool DEPTH, bool FUSED>
__global__ __launch_bounds__(LM_THREADS) void lm_eq_kernel(const float* __restrict__ target, int target_mode, const float* __restrict__ weight,
                                                           const float* __restrict__ depth, float eps, const float* __restrict__ K,
                                                           const float* __restrict__ G, int H, int W, const LmDepthTerm dt,
                                                           double* __restrict__ partials, const LmTail tail) {
  constexpr int NA = DEPTH ? NACC_RGBD : NACC;
  const int b = blockIdx.y;
  const int nblk = gridDim.x;
  const long long P = static_cast<long long>(H) * W;
  const Intr k = rp::load_intr(K, b);
  const Pose g = rp::load_pose(G, b);
  LmFrame f{};
  if constexpr (DEPTH) {
    const int s = dt.src_index ? dt.src_index[b] : b;
    f.ok = s >= 0 && s < dt.S;                                       // (the caller has refused it on the host; the second fence)
    f.obs = dt.obs + static_cast<long long>(f.ok ? s : 0) * dt.Ho * dt.Wo;
#pragma unroll
    for (int i = 0; i < 6; ++i) f.th[i] = dt.theta[b * 6 + i];
    f.ko = rp::load_intr(dt.K_obs, b);
    f.Ho = dt.Ho;
    f.Wo = dt.Wo;
  }
  double acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = 0.0;

  // LM_BATCH pixels per trip: their 4-5 loads each are issued (unconditionally, clamped to the last pixel) before the
  // first fp64 chain starts.  One pixel per trip was 8 dependent memory round trips per thread: 26 us per launch for
  // 20 MB (r02).  Pixels are accumulated in the same order as before, so the partial sums are bit-identical.
  const long long stride = static_cast<long long>(nblk) * LM_THREADS;
  for (long long t0 = static_cast<long long>(blockIdx.x) * LM_THREADS + threadIdx.x; t0 < P; t0 += LM_BATCH * stride) {
    float wgt_[LM_BATCH], dep_[LM_BATCH], tx_[LM_BATCH], ty_[LM_BATCH];
#pragma unroll
    for (int j = 0; j < LM_BATCH; ++j) {
      const long long tj = t0 + j * stride;
      const long long t = tj < P ? tj : P - 1;
      wgt_[j] = weight[b * P + t];
      dep_[j] = depth[b * P + t];
      if (target_mode == 0) {
        const float2 tt = *reinterpret_cast<const float2*>(target + (b * P + t) * 2);
        tx_[j] = tt.x;
        ty_[j] = tt.y;
      } else {
        tx_[j] = target[(static_cast<long long>(b) * 2 + 0) * P + t];
        ty_[j] = target[(static_cast<long long>(b) * 2 + 1) * P + t];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // DEPTH, second batch: the four depth taps of the trip's pixels, issued together once the targets have arrived, unconditionally and at
    // positions clamped into the frame (lm_obs_point decides which of them count).  Only the taps stay live across the loads: (ix, iy)
    // are formed again behind them -- keeping 16 more registers took the kernel to 1 wave per SIMD
    float z_[DEPTH ? LM_BATCH : 1][4];
    if constexpr (DEPTH) {
#pragma unroll
      for (int j = 0; j < LM_BATCH; ++j) {
        const long long tj = t0 + j * stride;
        int x, y, x0, y0;
        lm_pixel_xy(tj < P ? tj : P - 1, W, x, y);
        float ix, iy;
        lm_obs_position(tx_[j], ty_[j], x, y, target_mode, H, W, f, ix, iy);
        lm_obs_corner(ix, iy, x0, y0);
        const int xa = min(max(x0, 0), f.Wo - 1), xb = min(max(x0 + 1, 0), f.Wo - 1);
        const int ya = min(max(y0, 0), f.Ho - 1) * f.Wo, yb = min(max(y0 + 1, 0), f.Ho - 1) * f.Wo;
        z_[j][0] = f.obs[ya + xa];
        z_[j][1] = f.obs[ya + xb];
        z_[j][2] = f.obs[yb + xa];
        z_[j][3] = f.obs[yb + xb];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < LM_BATCH; ++j) {
      const long long t = t0 + j * stride;
      if (t >= P) break;
      int x, y;
      lm_pixel_xy(t, W, x, y);
      const float wgt = wgt_[j];
      LmGate q;
      if constexpr (DEPTH) {
        // the gate is evaluated for EVERY pixel, before the skip: the count of active pixels does not depend on the weights
        q = lm_depth_gate(dep_[j], tx_[j], ty_[j], x, y, target_mode, eps, k, g, H, W, f, z_[j], dt);
        acc[27] += q.active ? 1.0 : 0.0;
      }
      // zero-weight pixels (the descriptor weight is 0 on the rendered background) add w * (...) = 0 to every sum, the depth term's
      // included: a wave made of such pixels skips the fp64 chain -- but only pixels whose target and depth are FINITE count as skippable: in the
      // reference 0 * NaN = NaN poisons the system and the NaN -> zero-update guard fires (geometry/cholesky.py:43-44); a
      // lane with a non-finite input keeps its wave in the chain, so that happens here too, whatever the wave is made of.
      const bool skippable = wgt == 0.f && __builtin_isfinite(tx_[j]) && __builtin_isfinite(ty_[j]) && __builtin_isfinite(dep_[j]);
      if (__builtin_amdgcn_ballot_w64(!skippable) == 0ull) continue;
      lm_accumulate(acc, wgt, dep_[j], tx_[j], ty_[j], x, y, target_mode, eps, k, g);
      if constexpr (DEPTH) lm_depth_step(acc, q, wgt, dt.weight, k);
    }
  }
  lm_reduce_tail<FUSED, NA>(acc, partials, tail, b, nblk, static_cast<int>(blockIdx.x));
}

// sums the block partials in fixed order and expands to full H (6x6) and b (6)
// dstats != null (lm_eq_kernel<true, .>'s records only: the plain kernel never writes slots 27, 28): the two depth-term statistics too
__device__ void lm_finalize_block_one(const double* __restrict__ partials, int nblk, int b, double* __restrict__ Hm,
                                      double* __restrict__ bv, double* __restrict__ dstats) {
  // 8 groups of 32 lanes walk the partial records with stride 8 (each load is one coalesced 256-byte record), then
  // the 8 group sums are added in fixed order: deterministic, and 8x shorter than one serial chain per value.
  __shared__ double grp[8][PSTRIDE];
  __shared__ double s[NACC_RGBD];
  const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
  double v = 0.0;
  for (int i = g; i < nblk; i += 8) v += partials[(static_cast<long long>(b) * nblk + i) * PSTRIDE + k];
  grp[g][k] = v;
  __syncthreads();
  if (threadIdx.x < (dstats ? NACC_RGBD : NACC)) {
    double t = 0.0;
    for (int q = 0; q < 8; ++q) t += grp[q][threadIdx.x];
    s[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x < 36) {
    const int i = threadIdx.x / 6, j = threadIdx.x % 6;
    const int r = i < j ? i : j, c = i < j ? j : i;
    const int idx = r * 6 - r * (r - 1) / 2 + (c - r);     // row-major upper triangle
    Hm[b * 36 + threadIdx.x] = s[idx];
  } else if (threadIdx.x < 42) {
    bv[b * 6 + (threadIdx.x - 36)] = s[21 + (threadIdx.x - 36)];
  } else if (dstats && threadIdx.x < 44) {
    dstats[b * 2 + (threadIdx.x - 42)] = s[NACC + (threadIdx.x - 42)];
  }
}

__global__ __launch_bounds__(256) void lm_finalize_kernel(const double* __restrict__ partials, int nblk,
                                                          double* __restrict__ Hm, double* __restrict__ bv, double* __restrict__ dstats) {
  lm_finalize_block_one(partials, nblk, blockIdx.x, Hm, bv, dstats);
}

// ---- SE(3) exponential, fp32, same branch structure as geometry/se3.py:228-281 ----
__device__ void se3_exp_dev(const float* xi, float* Gout /*16*/) {
  const float v0 = xi[0], v1 = xi[1], v2 = xi[2];
  const float w0 = xi[3], w1 = xi[4], w2 = xi[5];
  const float th2 = w0 * w0 + w1 * w1 + w2 * w2;
  const float th = sqrtf(th2);
  const float th4 = th2 * th2;
  const float wx[9] = {0.f, -w2, w1, w2, 0.f, -w0, -w1, w0, 0.f};
  float wx2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) wx2[i * 3 + j] = wx[i * 3 + 0] * wx[0 * 3 + j] + wx[i * 3 + 1] * wx[1 * 3 + j] + wx[i * 3 + 2] * wx[2 * 3 + j];
  float A, Bc, Cc;   // R = I + A wx + Bc wx2 ; V = I + Bc' wx + Cc wx2
  float Bv;
  const float eps = 1e-12f;
  if (th < rp::kMinTheta) {
    A = 1.0f - (1.0f / 6.0f) * th2 + (1.0f / 120.0f) * th4;
    Bc = 0.5f - (1.0f / 12.0f) * th2 + (1.0f / 720.0f) * th4;
    Bv = 0.5f - (1.0f / 24.0f) * th2 + (1.0f / 720.0f) * th4;
    Cc = (1.0f / 6.0f) - (1.0f / 120.0f) * th2 + (1.0f / 5040.0f) * th4;
  } else {
    A = sinf(th) / (th + eps);
    Bc = (1.0f - cosf(th)) / (th2 + eps);
    Bv = Bc;
    Cc = (th - sinf(th)) / (th2 * th + eps);
  }
  float Rm[9], Vm[9];
  for (int i = 0; i < 9; ++i) {
    const float I = (i == 0 || i == 4 || i == 8) ? 1.f : 0.f;
    Rm[i] = I + A * wx[i] + Bc * wx2[i];
    Vm[i] = I + Bv * wx[i] + Cc * wx2[i];
  }
  for (int i = 0; i < 3; ++i) {
    Gout[i * 4 + 0] = Rm[i * 3 + 0];
    Gout[i * 4 + 1] = Rm[i * 3 + 1];
    Gout[i * 4 + 2] = Rm[i * 3 + 2];
    Gout[i * 4 + 3] = Vm[i * 3 + 0] * v0 + Vm[i * 3 + 1] * v1 + Vm[i * 3 + 2] * v2;
  }
  Gout[12] = 0.f; Gout[13] = 0.f; Gout[14] = 0.f; Gout[15] = 1.f;
}

__device__ void mat4_mul(const float* A, const float* Bm, float* C) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      float s = 0.f;
      for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * Bm[k * 4 + j];
      C[i * 4 + j] = s;
    }
}

// damping, 6x6 Cholesky solve, NaN -> 0, clamp of system b -> xi (and xi_out, info) (one thread)
__device__ __forceinline__ void lm_solve_xi(const double* Hm, const double* bv, int b, double ep, double lm, double max_update, float (&xi)[6],
                                            float* xi_out, int* info) {
  // (the fused tail reads H, b that this very thread's block wrote a barrier ago: same CU, same L1 -- plain loads are current)
  // In place on the lower triangle (21 doubles instead of two 6x6 arrays: this function's registers are the floor of every kernel
  // that calls it, r04) -- the same operations in the same order as the two-array form.
  double L[21], xv[6];
#define LT(i_, j_) L[(i_) * ((i_) + 1) / 2 + (j_)]
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) LT(i, j) = Hm[b * 36 + i * 6 + j];
    xv[i] = bv[b * 6 + i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) LT(i, i) = LT(i, i) + ep + lm * LT(i, i);   // H += ep*I + lm*H*I  (transformation.py:300)
  int bad = 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = LT(j, j);
#pragma unroll
    for (int k = 0; k < j; ++k) s -= LT(j, k) * LT(j, k);
    if (!(s > 0.0)) {
      if (!bad) bad = j + 1;
      LT(j, j) = nan;
    } else {
      LT(j, j) = sqrt(s);
    }
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = LT(i, j);
#pragma unroll
      for (int k = 0; k < j; ++k) t -= LT(i, k) * LT(j, k);
      LT(i, j) = t / LT(j, j);
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {              // forward substitution, in place (xv: rhs -> y)
    double t = xv[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= LT(i, k) * xv[k];
    xv[i] = t / LT(i, i);
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {             // back substitution, in place (y -> x)
    double t = xv[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t -= LT(k, i) * xv[k];
    xv[i] = t / LT(i, i);
  }
#undef LT
  for (int i = 0; i < 6; ++i) {
    double v = xv[i];
    if (v != v) v = 0.0;                                   // NaN -> 0      (cholesky.py:43-44)
    v = v < -max_update ? -max_update : (v > max_update ? max_update : v);   // clamp (cholesky.py:45)
    xi[i] = static_cast<float>(v);
    xi_out[b * 6 + i] = xi[i];
  }
  if (info) info[b] = bad;
}

// SE(3) exponential and left increment of image b: G_new <- exp(xi) G (one thread)
__device__ __forceinline__ void lm_pose_update(const float (&xi)[6], const float* G, int b, float* G_new /* may alias G */) {
  float dG[16], Gin[16], Gout[16];
  se3_exp_dev(xi, dG);
  for (int i = 0; i < 16; ++i) Gin[i] = G[b * 16 + i];
  mat4_mul(dG, Gin, Gout);                                 // se3.py:303-306
  for (int i = 0; i < 16; ++i) G_new[b * 16 + i] = Gout[i];
}

// the solve and the pose update of image b (one thread): what every ungrouped LM step ends with
__device__ __forceinline__ void lm_solve_one(const double* Hm, const double* bv, const float* G, int b, double ep, double lm,
                                             double max_update, float* G_new /* may alias G */, float* xi_out, int* info) {
  float xi[6];
  lm_solve_xi(Hm, bv, b, ep, lm, max_update, xi, xi_out, info);
  lm_pose_update(xi, G, b, G_new);
}

// ---- views of one object from several calibrated cameras: ONE increment per group of views ----------------------
// View v has the camera-from-rig transform E_v = (R, t); a rig-frame left increment delta acts in view v as xi_v = Ad(E_v) delta,
// Ad(E) = [[R, [t]x R], [0, R]].  Group system Hg = sum_v Ad_v^T Hm_v Ad_v, bg = sum_v Ad_v^T bv_v (fp64, views in ascending order), the
// solve of every LM step on it, D = exp(delta) once per group, and G_v <- (E_v D E_v^-1) G_v for every view of the group.
struct LmViews {
  const int* group_start;       // (n_groups + 1): the views of group g are rows [group_start[g], group_start[g + 1])
  int n_groups;
  const float* E;               // (B,4,4) camera-from-rig of every view
  double* Hg;                   // (n_groups,6,6), (n_groups,6): the undamped rig-frame system
  double* bg;
};

// entry (i, j) of Ad(E) in fp64 from the fp32 transform e (16 floats, row-major)
__device__ __forceinline__ double lm_adjoint_entry(const float* e, int i, int j) {
  if (i >= 3) return j >= 3 ? static_cast<double>(e[(i - 3) * 4 + (j - 3)]) : 0.0;
  if (j < 3) return static_cast<double>(e[i * 4 + j]);
  // ([t]x R)(i, c) = t_{i+1} R(i+2, c) - t_{i+2} R(i+1, c), indices modulo 3
  const int c = j - 3, i1 = (i + 1) % 3, i2 = (i + 2) % 3;
  const double t1 = e[i1 * 4 + 3], t2 = e[i2 * 4 + 3];
  return t1 * static_cast<double>(e[i2 * 4 + c]) - t2 * static_cast<double>(e[i1 * 4 + c]);
}

// The tail of a grouped iteration behind lm_eq_kernel<., false>: one 256-thread workgroup per group.  Per view: the partial records ->
// Hm_v, bv_v (dstats) by lm_finalize_block_one itself (bit-identical to the ungrouped entries), then Ad_v^T Hm_v Ad_v (36 threads, every
// one the entry (min, max) of its pair: Hg is exactly symmetric) and Ad_v^T bv_v (6 threads) added to per-thread fp64 accumulators in
// ascending view order -- no atomics, deterministic.  One thread damps, solves and clamps (lm_solve_xi: the solve of every LM step) and
// forms D; the views of the group then update their poses in parallel.  Ranges are clamped to [0, B]; an empty group writes info = -1
// and nothing else.  tail: Hm, bv, dstats, G_in, G_out per VIEW, xi and info per GROUP; no tickets are used.
__global__ __launch_bounds__(256) void lm_views_tail_kernel(const double* __restrict__ partials, int nblk, int B, const LmViews vw,
                                                            const LmTail tail) {
  __shared__ double Ad[36], M[36];
  __shared__ float Dg[16];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int v0 = min(max(vw.group_start[g], 0), B), v1 = min(max(vw.group_start[g + 1], 0), B);
  if (v1 <= v0) {
    if (tid == 0) tail.info[g] = -1;
    return;
  }
  const int i = tid < 36 ? tid / 6 : 0, j = tid < 36 ? tid % 6 : tid - 36;
  const int r = i < j ? i : j, c = i < j ? j : i;
  double acc = 0.0;
  for (int v = v0; v < v1; ++v) {
    lm_finalize_block_one(partials, nblk, v, tail.Hm, tail.bv, tail.dstats);   // (ends with the values in global memory, written by this block)
    if (tid < 36) Ad[tid] = lm_adjoint_entry(vw.E + v * 16, i, j);
    __syncthreads();
    if (tid < 36) {                                                            // M = Hm_v Ad_v
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += tail.Hm[v * 36 + i * 6 + k] * Ad[k * 6 + j];
      M[tid] = s;
    }
    __syncthreads();
    if (tid < 36) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += Ad[k * 6 + r] * M[k * 6 + c];
      acc += s;
    } else if (tid < 42) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += Ad[k * 6 + j] * tail.bv[v * 6 + k];
      acc += s;
    }
    __syncthreads();                                                           // (the next view overwrites Ad and M)
  }
  if (tid < 36) vw.Hg[g * 36 + tid] = acc;
  else if (tid < 42) vw.bg[g * 6 + j] = acc;
  __syncthreads();
  if (tid == 0) {
    float xi[6];
    lm_solve_xi(vw.Hg, vw.bg, g, tail.ep, tail.lm, tail.max_update, xi, tail.xi, tail.info);
    se3_exp_dev(xi, Dg);
  }
  __syncthreads();
  for (int v = v0 + tid; v < v1; v += blockDim.x) {                            // G_v <- (E_v D E_v^-1) G_v, fp32
    float e[16], d[16], inv[16], a[16], m[16], Gin[16], Gout[16];
    for (int q = 0; q < 16; ++q) {
      e[q] = vw.E[v * 16 + q];
      d[q] = Dg[q];
      Gin[q] = tail.G_in[v * 16 + q];
    }
    for (int p = 0; p < 3; ++p) {                                              // the rigid inverse, as se3_inverse_kernel forms it
      for (int q = 0; q < 3; ++q) inv[p * 4 + q] = e[q * 4 + p];
      float s = 0.f;
      for (int k = 0; k < 3; ++k) s += e[k * 4 + p] * e[k * 4 + 3];
      inv[p * 4 + 3] = -s;
    }
    inv[12] = 0.f; inv[13] = 0.f; inv[14] = 0.f; inv[15] = 1.f;
    mat4_mul(e, d, a);
    mat4_mul(a, inv, m);
    mat4_mul(m, Gin, Gout);
    for (int q = 0; q < 16; ++q) tail.G_out[v * 16 + q] = Gout[q];
  }
}

__global__ __launch_bounds__(64) void lm_solve_update_kernel(const double* __restrict__ Hm, const double* __restrict__ bv,
                                                             const float* G, int B, double ep, double lm,
                                                             double max_update, float* G_new /* may alias G */,
                                                             float* __restrict__ xi_out, int* __restrict__ info) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) lm_solve_one(Hm, bv, G, b, ep, lm, max_update, G_new, xi_out, info);
}

__global__ void se3_exp_kernel(const float* __restrict__ xi, int B, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float x[6], Gm[16];
  for (int i = 0; i < 6; ++i) x[i] = xi[b * 6 + i];
  se3_exp_dev(x, Gm);
  for (int i = 0; i < 16; ++i) out[b * 16 + i] = Gm[i];
}

__global__ void se3_compose_kernel(const float* __restrict__ A, const float* __restrict__ Bm, int B, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float a[16], c[16], o[16];
  for (int i = 0; i < 16; ++i) {
    a[i] = A[b * 16 + i];
    c[i] = Bm[b * 16 + i];
  }
  mat4_mul(a, c, o);
  for (int i = 0; i < 16; ++i) out[b * 16 + i] = o[i];
}

// [R t; 0 1]^-1 = [R^T  -R^T t; 0 1]   (geometry/se3.py:194-209)
__global__ void se3_inverse_kernel(const float* __restrict__ A, int B, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float a[16], o[16];
  for (int i = 0; i < 16; ++i) a[i] = A[b * 16 + i];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[i * 4 + j] = a[j * 4 + i];
    float s = 0.f;
    for (int k = 0; k < 3; ++k) s += a[k * 4 + i] * a[k * 4 + 3];
    o[i * 4 + 3] = -s;
  }
  o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
  for (int i = 0; i < 16; ++i) out[b * 16 + i] = o[i];
}

// a12, r06: the pose bookkeeping between two outer iterations as ONE launch (model/PoseRefiner.py:241-244) -- Ti <- Tij Ti, then the legacy start pose
// Tij <- Ti Ti^-1 (literal != 0: the reference's product, the identity up to fp32 rounding) or the exact identity.  The same three kernels' arithmetic
// in the same order (se3_compose, se3_inverse, se3_compose above): bit-identical to them; five ~6-us launches fewer per outer iteration.
__global__ void se3_outer_update_kernel(const float* __restrict__ Tij, const float* __restrict__ Ti, int B, int literal, float* __restrict__ Ti_out,
                                        float* __restrict__ Tij_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float a[16], c[16], t[16], inv[16], o[16];
  for (int i = 0; i < 16; ++i) {
    a[i] = Tij[b * 16 + i];
    c[i] = Ti[b * 16 + i];
  }
  mat4_mul(a, c, t);
  for (int i = 0; i < 16; ++i) Ti_out[b * 16 + i] = t[i];
  if (literal) {
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) inv[i * 4 + j] = t[j * 4 + i];
      float s = 0.f;
      for (int k = 0; k < 3; ++k) s += t[k * 4 + i] * t[k * 4 + 3];
      inv[i * 4 + 3] = -s;
    }
    inv[12] = 0.f; inv[13] = 0.f; inv[14] = 0.f; inv[15] = 1.f;
    mat4_mul(t, inv, o);
  } else {
    for (int i = 0; i < 16; ++i) o[i] = (i % 5 == 0) ? 1.f : 0.f;
  }
  for (int i = 0; i < 16; ++i) Tij_out[b * 16 + i] = o[i];
}

// workspace = [B arrival counters, 8 bytes each: zero between launches][partial records]
inline double* lm_partials(void* workspace, int B) { return static_cast<double*>(workspace) + B; }

// what every entry that builds the normal equations reads: the 2-D term's inputs, the crop size, the workspace
struct LmInputs {
  const float* target;
  int target_mode;
  const float* weight;
  const float* depth;
  float eps;
  const float* K;
  int B, H, W;
  void* workspace;
  size_t workspace_bytes;
};

// where an iteration writes and what its solve needs (G_in is set per iteration); G_out == null: no solve, the normal-equation entries
LmTail lm_tail(void* workspace, double* Hm, double* bv, float* G_out, float* xi, int* info, double ep, double lm, double max_update,
               double* dstats) {
  LmTail tail{};
  tail.tickets = static_cast<int*>(workspace);
  tail.Hm = Hm; tail.bv = bv; tail.G_out = G_out; tail.xi = xi; tail.info = info;
  tail.ep = ep; tail.lm = lm; tail.max_update = max_update; tail.dstats = dstats;
  return tail;
}

// per-workgroup partial sums of the pose tail.G_in into the workspace (FUSED: and the tail); dt: the depth term, or null for the plain
// step; -> number of partial records per image
template <bool FUSED>
int launch_lm_eq(const LmInputs& in, const LmDepthTerm* dt, const LmTail& tail, hipStream_t st) {
  const int nblk = lm_blocks_per_image(static_cast<long long>(in.H) * in.W);
  const auto kernel = dt ? lm_eq_kernel<true, FUSED> : lm_eq_kernel<false, FUSED>;
  hipLaunchKernelGGL(kernel, dim3(nblk, in.B), dim3(LM_THREADS), 0, st, in.target, in.target_mode, in.weight, in.depth, in.eps, in.K,
                     tail.G_in, in.H, in.W, dt ? *dt : LmDepthTerm{}, lm_partials(in.workspace, in.B), tail);
  return nblk;
}

// ONE LM iteration.  fused: partial sums + (in the last-arriving workgroup of every image) finalize, damped solve, pose update as ONE
// launch; else partial sums, finalize (with the statistics, given tail.dstats) and -- given tail.G_out -- the solve as three launches
// views: the grouped step -- partial sums, then lm_views_tail_kernel (finalize per view, group system, solve, pose updates): two launches
void launch_lm_iteration(bool fused, const LmInputs& in, const LmDepthTerm* dt, const LmTail& tail, const LmViews* views, hipStream_t st) {
  if (views) {
    const int nblk = launch_lm_eq<false>(in, dt, tail, st);
    hipLaunchKernelGGL(lm_views_tail_kernel, dim3(views->n_groups), dim3(256), 0, st, lm_partials(in.workspace, in.B), nblk, in.B, *views, tail);
    return;
  }
  if (fused) {
    launch_lm_eq<true>(in, dt, tail, st);
    return;
  }
  const int nblk = launch_lm_eq<false>(in, dt, tail, st);
  hipLaunchKernelGGL(lm_finalize_kernel, dim3(in.B), dim3(256), 0, st, lm_partials(in.workspace, in.B), nblk, tail.Hm, tail.bv, tail.dstats);
  // (G_in may alias G_out: each thread reads its whole pose before writing it.  A merged finalize + solve kernel was measured
  //  SLOWER, 26 us vs 7 + 6 us: the solve is a serial fp64 chain that then waits behind the 256-thread reduction's launch)
  if (tail.G_out)
    hipLaunchKernelGGL(lm_solve_update_kernel, dim3(rp::cdiv(in.B, 64)), dim3(64), 0, st, tail.Hm, tail.bv, tail.G_in, in.B, tail.ep, tail.lm,
                       tail.max_update, tail.G_out, tail.xi, tail.info);
}

}  // namespace

extern "C" {

size_t rnnpose_lm_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  // partial records + one arrival counter per image (padded to 8 bytes each); the counters must be ZERO before the first fused
  // step (rnnpose_lm_step_*): allocate the workspace zero-filled.  Every fused launch leaves them at zero.
  return static_cast<size_t>(B) * lm_blocks_per_image(static_cast<long long>(H) * W) * PSTRIDE * sizeof(double) +
         static_cast<size_t>(B) * sizeof(double);
}

static bool g_lm_fused = true;
int rnnpose_lm_fused_tail(int enable) {          // measurement switch: 0 = three launches per LM step (r02), 1 = one (default)
  g_lm_fused = enable != 0;
  return 0;
}

int rnnpose_lm_solve_update_f32(const double* Hm, const double* bv, const float* G, int B, double ep_lambda,
                                double lm_lambda, double max_update, float* G_new, float* xi, int* info,
                                rnnpose_stream_t stream) {
  const char* fn = "rnnpose_lm_solve_update_f32";
  RP_REQUIRE(Hm && bv && G && G_new && xi, fn, "null pointer");
  RP_REQUIRE(B > 0, fn, "bad size");
  hipLaunchKernelGGL(lm_solve_update_kernel, dim3(rp::cdiv(B, 64)), dim3(64), 0, rp::as_stream(stream), Hm, bv, G, B,
                     ep_lambda, lm_lambda, max_update, G_new, xi, info);
  return rp::check_launch(fn);
}

// the depth arguments of the two RGB-D entries
static int lm_rgbd_check(const char* fn, const LmDepthTerm& dt, int B) {
  RP_REQUIRE(dt.obs && dt.theta && dt.K_obs, fn, "null obs_depth / theta / K_obs");
  RP_REQUIRE(dt.S >= 1 && dt.Ho > 0 && dt.Wo > 0 && static_cast<long long>(dt.Ho) * dt.Wo < (1LL << 31), fn,
             "bad observed-frame size (S >= 1, Ho, Wo > 0)");
  RP_REQUIRE(dt.src_index || dt.S == B, fn, "src_index is null: the observed depth must hold one frame per object (S == B)");
  RP_REQUIRE(std::isfinite(dt.weight) && dt.weight >= 0.f, fn, "depth_weight must be finite and >= 0");
  RP_REQUIRE(std::isfinite(dt.gate) && dt.gate >= 0.f, fn, "depth_gate must be finite and >= 0");
  RP_REQUIRE(std::isfinite(dt.edge_tol) && dt.edge_tol >= 0.f, fn, "edge_tol must be finite and >= 0");
  return 0;
}

// the arguments the LM entries share, in the order every entry tests them.  solve: a step entry (G_out and xi are outputs, num_iters
// counts); need_iter: its G_out is written by an iteration only; dt: the depth arguments, tested before the workspace
static int lm_check(const char* fn, const LmInputs& in, const LmDepthTerm* dt, const float* G_in, const LmTail& out, bool solve, int num_iters,
                    bool need_iter) {
  RP_REQUIRE(in.target && in.weight && in.depth && in.K && G_in && in.workspace && out.Hm && out.bv && (!solve || (out.G_out && out.xi)), fn,
             "null pointer");
  RP_REQUIRE(in.target_mode == 0 || in.target_mode == 1, fn, "target_mode must be 0 or 1");
  RP_REQUIRE(in.B > 0 && in.B < 65536 && in.H > 0 && in.W > 0 && static_cast<long long>(in.H) * in.W < (1LL << 31) &&
                 (need_iter || num_iters >= 0), fn, "bad size");
  if (need_iter) RP_REQUIRE(num_iters >= 1, fn, "needs at least one iteration (G_out would stay unwritten)");
  if (dt && lm_rgbd_check(fn, *dt, in.B)) return 1;
  RP_REQUIRE(in.workspace_bytes >= rnnpose_lm_workspace_bytes(in.B, in.H, in.W), fn, "workspace too small");
  return 0;
}

// every LM entry: the checks, then num_iters iterations from G_in in the form that g_lm_fused and the presence of `info` select;
// views: the grouped step's arguments (tested first, the group count once the batch size is known to be good), or null
static int lm_run(const char* fn, const LmInputs& in, const LmDepthTerm* dt, const float* G_in, LmTail tail, bool solve, int num_iters,
                  bool need_iter, rnnpose_stream_t stream, const LmViews* views = nullptr) {
  if (views) RP_REQUIRE(views->group_start && views->E && views->Hg && views->bg && tail.xi && tail.info, fn,
                        "null group_start / E / Hg / bg / xi / info");
  if (lm_check(fn, in, dt, G_in, tail, solve, num_iters, need_iter)) return 1;
  if (views) RP_REQUIRE(views->n_groups >= 1 && views->n_groups <= in.B, fn, "n_groups must lie in [1, B]");
  hipStream_t st = rp::as_stream(stream);
  for (int it = 0; it < num_iters; ++it) {
    tail.G_in = it == 0 ? G_in : tail.G_out;              // later iterations continue in place on the output
    launch_lm_iteration(g_lm_fused && tail.info, in, dt, tail, views, st);
  }
  return rp::check_launch(fn);
}

int rnnpose_lm_normal_eq_f64(const float* target, int target_mode, const float* weight, const float* depth,
                             float depth_eps, const float* K, const float* G, int B, int H, int W, void* workspace,
                             size_t workspace_bytes, double* Hm, double* bv, rnnpose_stream_t stream) {
  const LmInputs in{target, target_mode, weight, depth, depth_eps, K, B, H, W, workspace, workspace_bytes};
  return lm_run("rnnpose_lm_normal_eq_f64", in, nullptr, G, lm_tail(workspace, Hm, bv, nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, nullptr), false,
                1, false, stream);
}

int rnnpose_lm_step_f32(const float* target, int target_mode, const float* weight, const float* depth, float depth_eps,
                        const float* K, float* G, int B, int H, int W, int num_iters, double ep_lambda, double lm_lambda,
                        double max_update, void* workspace, size_t workspace_bytes, double* Hm, double* bv, float* xi,
                        int* info, rnnpose_stream_t stream) {
  const LmInputs in{target, target_mode, weight, depth, depth_eps, K, B, H, W, workspace, workspace_bytes};
  return lm_run("rnnpose_lm_step_f32", in, nullptr, G, lm_tail(workspace, Hm, bv, G, xi, info, ep_lambda, lm_lambda, max_update, nullptr), true,
                num_iters, false, stream);
}

int rnnpose_lm_step_io_f32(const float* target, int target_mode, const float* weight, const float* depth, float depth_eps,
                           const float* K, const float* G_in, float* G_out, int B, int H, int W, int num_iters,
                           double ep_lambda, double lm_lambda, double max_update, void* workspace, size_t workspace_bytes,
                           double* Hm, double* bv, float* xi, int* info, rnnpose_stream_t stream) {
  RP_REQUIRE(num_iters >= 1, "rnnpose_lm_step_io_f32", "needs at least one iteration (G_out would stay unwritten)");
  const LmInputs in{target, target_mode, weight, depth, depth_eps, K, B, H, W, workspace, workspace_bytes};
  return lm_run("rnnpose_lm_step_io_f32", in, nullptr, G_in, lm_tail(workspace, Hm, bv, G_out, xi, info, ep_lambda, lm_lambda, max_update, nullptr),
                true, num_iters, false, stream);
}

int rnnpose_lm_normal_eq_rgbd_f64(const float* target, int target_mode, const float* weight, const float* depth, float depth_eps,
                                  const float* K, const float* G, int B, int H, int W, const float* obs_depth, const int* src_index,
                                  const float* theta, const float* K_obs, int S, int Ho, int Wo, float depth_weight, float depth_gate,
                                  float edge_tol, void* workspace, size_t workspace_bytes, double* Hm, double* bv, double* dstats,
                                  rnnpose_stream_t stream) {
  const LmInputs in{target, target_mode, weight, depth, depth_eps, K, B, H, W, workspace, workspace_bytes};
  const LmDepthTerm dt{obs_depth, src_index, theta, K_obs, S, Ho, Wo, depth_weight, depth_gate, edge_tol};
  return lm_run("rnnpose_lm_normal_eq_rgbd_f64", in, &dt, G, lm_tail(workspace, Hm, bv, nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, dstats), false,
                1, false, stream);
}

int rnnpose_lm_step_rgbd_io_f32(const float* target, int target_mode, const float* weight, const float* depth, float depth_eps,
                                const float* K, const float* G_in, float* G_out, int B, int H, int W, int num_iters, double ep_lambda,
                                double lm_lambda, double max_update, const float* obs_depth, const int* src_index, const float* theta,
                                const float* K_obs, int S, int Ho, int Wo, float depth_weight, float depth_gate, float edge_tol,
                                void* workspace, size_t workspace_bytes, double* Hm, double* bv, float* xi, int* info, double* dstats,
                                rnnpose_stream_t stream) {
  const LmInputs in{target, target_mode, weight, depth, depth_eps, K, B, H, W, workspace, workspace_bytes};
  const LmDepthTerm dt{obs_depth, src_index, theta, K_obs, S, Ho, Wo, depth_weight, depth_gate, edge_tol};
  return lm_run("rnnpose_lm_step_rgbd_io_f32", in, &dt, G_in, lm_tail(workspace, Hm, bv, G_out, xi, info, ep_lambda, lm_lambda, max_update, dstats),
                true, num_iters, true, stream);
}

int rnnpose_lm_step_views_io_f32(const float* target, int target_mode, const float* weight, const float* depth, float depth_eps,
                                 const float* K, const float* G_in, float* G_out, int B, int H, int W, int num_iters, double ep_lambda,
                                 double lm_lambda, double max_update, const float* obs_depth, const int* src_index, const float* theta,
                                 const float* K_obs, int S, int Ho, int Wo, float depth_weight, float depth_gate, float edge_tol,
                                 const int* group_start, int n_groups, const float* E, void* workspace, size_t workspace_bytes, double* Hm,
                                 double* bv, double* Hg, double* bg, float* xi, int* info, double* dstats, rnnpose_stream_t stream) {
  const LmInputs in{target, target_mode, weight, depth, depth_eps, K, B, H, W, workspace, workspace_bytes};
  const LmDepthTerm dt{obs_depth, src_index, theta, K_obs, S, Ho, Wo, depth_weight, depth_gate, edge_tol};
  const LmViews views{group_start, n_groups, E, Hg, bg};
  // (the plain kernel never writes the statistics' slots of its records: without the depth term dstats stays unwritten)
  return lm_run("rnnpose_lm_step_views_io_f32", in, obs_depth ? &dt : nullptr, G_in,
                lm_tail(workspace, Hm, bv, G_out, xi, info, ep_lambda, lm_lambda, max_update, obs_depth ? dstats : nullptr), true, num_iters, true,
                stream, &views);
}

int rnnpose_se3_exp_f32(const float* xi, int B, float* out, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_se3_exp_f32";
  RP_REQUIRE(xi && out && B > 0, fn, "bad argument");
  hipLaunchKernelGGL(se3_exp_kernel, dim3(rp::cdiv(B, 64)), dim3(64), 0, rp::as_stream(stream), xi, B, out);
  return rp::check_launch(fn);
}

int rnnpose_se3_compose_f32(const float* A, const float* Bm, int B, float* out, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_se3_compose_f32";
  RP_REQUIRE(A && Bm && out && B > 0, fn, "bad argument");
  hipLaunchKernelGGL(se3_compose_kernel, dim3(rp::cdiv(B, 64)), dim3(64), 0, rp::as_stream(stream), A, Bm, B, out);
  return rp::check_launch(fn);
}

int rnnpose_se3_outer_update_f32(const float* Tij, const float* Ti, int B, int literal, float* Ti_out, float* Tij_out, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_se3_outer_update_f32";
  RP_REQUIRE(Tij && Ti && Ti_out && Tij_out && B > 0, fn, "null pointer / empty batch");
  hipLaunchKernelGGL(se3_outer_update_kernel, dim3(rp::cdiv(B, 64)), dim3(64), 0, rp::as_stream(stream), Tij, Ti, B, literal, Ti_out, Tij_out);
  return rp::check_launch(fn);
}

int rnnpose_se3_inverse_f32(const float* A, int B, float* out, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_se3_inverse_f32";
  RP_REQUIRE(A && out && B > 0, fn, "bad argument");
  hipLaunchKernelGGL(se3_inverse_kernel, dim3(rp::cdiv(B, 64)), dim3(64), 0, rp::as_stream(stream), A, B, out);
  return rp::check_launch(fn);
}

}  // extern "C"
