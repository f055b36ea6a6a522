/*
 * rnnpose_hip.h -- C ABI of librnnpose_hip.so: the MI355X (gfx950) implementation of RNNPose's
 * recurrent-refinement hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with h_ (host);
 *   - tensors are dense, row-major ("contiguous") in the shape given in the comment;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only ENQUEUE work:
 *     no host synchronisation, no device allocation, no D2H copy happens inside the library;
 *   - return value 0 = success; nonzero = error, with a message in rnnpose_last_error()
 *     (1 = invalid argument, 2 = HIP launch/runtime error).  The library never calls exit()
 *     (the reference's only native precedent does: thirdparty/nn/src/nearest_neighborhood.cu:10-17).
 *   - inference only (tools/eval.py:526 runs under no_grad): no backward entry points.
 *
 * Each entry point names the reference code it replaces (paths relative to the RNNPose repo).
 */
#ifndef RNNPOSE_HIP_H
#define RNNPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rnnpose_stream_t;

/* 4: rnnpose_conv_tiles_per_image and rnnpose_conv_tiles_per_image_ex are gone -- shape-only guesses at a tiling that depends on the
 * whole descriptor; rnnpose_conv_tiles_per_image_desc is the one sizing call.
 * 3 (round 5): rnnpose_conv_desc_t ends with tile_stats_records (the launch checks the statistics buffer it is given);
 * rnnpose_conv_tiles_per_image_desc sizes it from the descriptor itself.
 * 2 (round 4): rnnpose_conv_desc_t grew the split-tensor / K-split members, the packed weight array holds two orders
 * (rnnpose_conv_packed_halfs doubled), tile statistics are fp64, rnnpose_lm_step_* needs a zero-filled workspace: a consumer
 * built against version 1 must not pass the check. */
#define RNNPOSE_ABI_VERSION 4
#define RNNPOSE_MAX_LEVELS 4

int rnnpose_abi_version(void);
const char* rnnpose_last_error(void);
/* gfx arch name of device `dev` copied to h_name (e.g. "gfx950"), CU count to *h_cus */
int rnnpose_device_info(int dev, char* h_name, int name_len, int* h_cus);

/* ---- a1+a2: all-pairs correlation volume + pyramid ------------- thirdparty/raft/corr.py:13-34,59-67
 * level 0: corr[b,i,j] = sum_c fmap1[b,c,i]*fmap2[b,c,j] / sqrt(C); level l = 2x2 mean of level l-1
 * (floor cropping).  `pyramid` is ONE buffer holding all levels back to back; sizes/offsets (in floats) come from
 * rnnpose_corr_pyramid_layout.  Levels 1.. are laid out as (B*h*w, h_l, w_l).  LEVEL 0 (r04) is stored J-PATCH-MAJOR:
 * [b][patch py * ceil(w/16) + px][i][8][16], i.e. corr[b,i,(y,x)] sits at
 *     ((b * n_patch + (y >> 3) * ceil(w/16) + (x >> 4)) * h*w + i) * 128 + (y & 7) * 16 + (x & 15),   n_patch = ceil(h/8) ceil(w/16)
 * (whole 8 x 16 patches: cells outside the image hold zeros).  The volume kernel's 128 (i) x one-patch tile then leaves the
 * chip as one contiguous 64-KB run and the lookup's 10 x 10 window reads a few contiguous patch rows instead of ten rows
 * 4*w bytes apart.  Only the lookup entry points read it; rnnpose_amd.ops.pyramid_level0_dense un-blocks it for inspection.
 * fmap1,fmap2: (B,C,h,w) fp32, C % 4 == 0.                                                       */
int rnnpose_corr_pyramid_layout(int B, int h, int w, int levels, int64_t* h_offsets /*[levels+1]*/,
                                int* h_hl /*[levels]*/, int* h_wl /*[levels]*/);
int rnnpose_corr_pyramid_f32(const float* fmap1, const float* fmap2, int B, int C, int h, int w,
                             int levels, float* pyramid, rnnpose_stream_t stream);
/* Same volume + pyramid with the operands split into fp16 hi/lo halves and multiplied on the fp16 matrix cores with
 * fp32 accumulation (3 MFMAs per k-slab; the dropped lo*lo term is 2^-22 relative: fp32-class accuracy).  One pre-pass
 * launch writes both operands, scaled and split, as pixel-major SPLIT TENSORS (see rnnpose_conv_desc_t) into `workspace`.
 * layout 0: fmaps are (B,C,h,w) as above; layout 1: (B,h,w,C).  a_scale (a power of two, 8 in the host code) scales both
 * operands before the split; |x| * a_scale beyond 65504 saturates (range guard).  C % 32 == 0.
 * rnnpose_corr_pyramid_split: the operands ARE split tensors already ((B,h,w,C), 4*C bytes per pixel, scale a_scale), e.g.
 * written by the encoder's output convolution (rnnpose_conv1x1_resident_f16x3, dst_split): no pre-pass, no workspace. */
size_t rnnpose_corr_pyramid_f16x3_workspace_bytes(int B, int C, int h, int w);
int rnnpose_corr_pyramid_f16x3(const float* fmap1, const float* fmap2, int layout, int B, int C, int h, int w, int levels,
                               float a_scale, void* workspace, size_t workspace_bytes, float* pyramid,
                               rnnpose_stream_t stream);
int rnnpose_corr_pyramid_split(const void* fmap1_split, const void* fmap2_split, int B, int C, int h, int w, int levels,
                               float a_scale, float* pyramid, rnnpose_stream_t stream);
int rnnpose_corr_supertile(int max_side);   /* measurement switch: tile-order supertiles of at most max_side x max_side (default 20) */
int rnnpose_corr_variant(int variant);      /* which fp16x3 volume kernel rnnpose_corr_pyramid_f16x3 / _split launch: 0 = operands through registers
                                             * and ds_write (r03-r05), 1 = operands by LDS-DMA, double-buffered 16-channel slabs (r06); bit-identical results */

/* ---- a3': volume-free lookup ---- thirdparty/raft/corr.py:70-98 (AlternateCorrBlock; its alt_cuda_corr extension is not in the
 * reference tree and the reference never enables it, model/CFNet.py:63-64).  The same (levels*81)-channel window features as
 * rnnpose_corr_lookup_*, computed on the fly from fmap1 and the 2^l-pooled fmap2 (pooling is linear: equal to the pyramid
 * lookup up to fp32 summation order) -- no volume is built.  A measured alternative, not the graded path.
 * fmap1 / fmap2: (B,h,w,C) pixel-major fp32, C % 4 == 0, C <= 512, 16-byte aligned.  rnnpose_fmap_pyramid_f32 writes levels
 * 1..levels-1 of fmap2 (chained 2x2 means, floor cropping) back to back into `pooled` (rnnpose_fmap_pyramid_floats floats).
 * out: pixel-major, channels [out_c_offset, +levels*81) of rows of out_c_stride floats; coords (B,2,h,w) as for the lookup. */
size_t rnnpose_fmap_pyramid_floats(int B, int h, int w, int C, int levels);
int rnnpose_fmap_pyramid_f32(const float* fmap2_nhwc, int B, int h, int w, int C, int levels, float* pooled,
                             rnnpose_stream_t stream);
int rnnpose_corr_alt_lookup_f32(const float* fmap1_nhwc, const float* fmap2_nhwc, const float* pooled, const float* coords, int B,
                                int h, int w, int C, int levels, int radius, float* out, int out_c_stride, int out_c_offset,
                                rnnpose_stream_t stream);

/* ---- a3: pyramid lookup -------- thirdparty/raft/corr.py:36-57, thirdparty/raft/utils/utils.py:57-71
 * coords (B,2,h,w) (ch0 = x, ch1 = y) -> out (B, levels*(2r+1)^2, h, w); channel
 * l*(2r+1)^2 + i*(2r+1) + j samples level l at (x/2^l + i - r, y/2^l + j - r)  [x-major window],
 * bilinear, align_corners=True, zero padding.  radius must be 4 (the only value the reference uses). */
int rnnpose_corr_lookup_f32(const float* pyramid, const float* coords, int B, int h, int w, int levels,
                            int radius, float* out, rnnpose_stream_t stream);
int rnnpose_corr_lookup_variant(int variant);   /* r06 measurement / test switch: 1 (default) = the lookup kernel at half the instructions per wave (one address form per level
                                                 * class, scalar pixel bases, phase 2 on 48 lanes), 0 = the r01-r05 kernel.  Bit-identical results. */

/* ---- a5: GRU_CFUpdator glue -------------------------------------------- model/CFNet.py:124-144
 * context_prep: ctx (B,C,H,W) -> bilinear (align_corners=True) resize to (h,w); first `hdim` channels
 * -> net = tanh(.), remaining C-hdim -> inp = relu(.).
 * flow_to_coords: coords1 (B,2,h,w) = pixel grid + resize(flow_init / (W/w)), flow_init (B,2,H,W);
 * does NOT modify flow_init (the reference divides in place, CFNet.py:141).                        */
int rnnpose_context_prep_f32(const float* ctx, int B, int C, int H, int W, int h, int w, int hdim,
                             float* net, float* inp, rnnpose_stream_t stream);
int rnnpose_flow_to_coords_f32(const float* flow_init, int B, int H, int W, int h, int w, float* coords1,
                               rnnpose_stream_t stream);

/* ---- a6: convex upsampling --------------------------------------------- model/CFNet.py:95-106
 * flow (B,2,h,w), mask (B,9*s*s,h,w) -> flow_up (B,2,s*h,s*w); s must be 8.                       */
int rnnpose_convex_upsample_f32(const float* flow, const float* mask, int B, int h, int w, int scale,
                                float* flow_up, rnnpose_stream_t stream);

/* ---- a7: induced flow of the relative pose --- geometry/transformation.py:184-198,
 *      geometry/projective_ops.py:68-114, model/PoseRefiner.py:313,324-328
 * depth (B,1,H,W) RAW rendered depth (0 = background; the kernel adds depth_eps as PoseRefiner.py:313
 * does), K (B,3,3), G (B,4,4) -> flow (B,2,H,W) = (project(G*backproject) - grid) * [depth+eps > eps],
 * vmask (B,H,W) float = [Z>0.1][Z'>0.1] (may be NULL).  mode 0: masked flow as above (PoseRefiner.py:327);
 * mode 1: the raw re-projected coordinates (u,v) of SE3.transform, unmasked (transformation.py:184-198).
 * induced_coords_lowres fuses a7 with flow_to_coords and evaluates only the 4 taps each 1/8-res pixel
 * needs: coords1 (B,2,h,w).                                                                        */
int rnnpose_induced_flow_f32(const float* depth, const float* K, const float* G, int B, int H, int W,
                             float depth_eps, int mode, float* flow, float* vmask, rnnpose_stream_t stream);
int rnnpose_induced_coords_lowres_f32(const float* depth, const float* K, const float* G, int B, int H,
                                      int W, int h, int w, float depth_eps, float* coords1,
                                      rnnpose_stream_t stream);

/* ---- a8: descriptor reliability weight ---- model/PoseRefiner.py:342-345, projective_ops.py:11-23
 * g1,g2 (B,D,H,W); weight (B,H,W) = exp(-|1 - <g1, bilinear(g2, target)>| / sigma) * [depth > 0];
 * g2 is sampled at pixel ((2x/(W-1)-1+1)*W-1)/2 (the reference's align_corners mismatch), zero pad.
 * target_mode 0: `target` is (B,H,W,2) absolute pixel coordinates (x,y interleaved);
 * target_mode 1: `target` is a planar flow (B,2,H,W) and the pixel grid is added in-kernel.
 * sigma: device pointer to one float (the nn.Parameter PoseRefiner.sigma[0]).                      */
int rnnpose_corr_weight_f32(const float* g1, const float* g2, const float* target, int target_mode,
                            const float* depth, const float* sigma, int B, int D, int H, int W,
                            float* weight, rnnpose_stream_t stream);
int rnnpose_corr_weight_pairs(int enable);    /* r06 measurement / test switch: 1 (default) = the two taps of an image row arrive as ONE 8-byte load (3 load
                                               * instructions per channel and pixel instead of 5; same arithmetic, bit-identical weights for finite descriptors), 0 = four 4-byte tap loads */

/* ---- a9: Gauss-Newton normal equations (fp64) -- geometry/transformation.py:274-297,
 *      geometry/projective_ops.py:116-124, geometry/transformation.py:27-46
 * Hm (B,6,6) = sum v*w*J^T J, bv (B,6) = sum v*w*J^T (target - x'), UNDAMPED, fp64.
 * weight (B,H,W) fp32; target/target_mode as above; depth raw (+depth_eps inside).
 * workspace: at least rnnpose_lm_workspace_bytes(B,H,W) bytes of device memory ([B arrival counters][block partials]). */
size_t rnnpose_lm_workspace_bytes(int B, int H, int W);
int rnnpose_lm_normal_eq_f64(const float* target, int target_mode, const float* weight, const float* depth,
                             float depth_eps, const float* K, const float* G, int B, int H, int W,
                             void* workspace, size_t workspace_bytes, double* Hm, double* bv,
                             rnnpose_stream_t stream);

/* ---- a10+a11: damped 6x6 Cholesky solve + SE(3) exp + left increment -- transformation.py:300-306,
 *      geometry/cholesky.py:32-50, geometry/se3.py:228-281,303-306
 * Hd = Hm + ep_lambda*I + lm_lambda*diag(Hm); xi = float(clamp(nan_to_zero(Hd^-1 bv), +-max_update));
 * G_new = exp(xi) * G.  info[b] = 0, or k>0 if the leading minor of order k is not positive (the
 * reference's torch.cholesky raises there; here xi becomes NaN->0 and the flag is left for the host). */
int rnnpose_lm_solve_update_f32(const double* Hm, const double* bv, const float* G, int B, double ep_lambda,
                                double lm_lambda, double max_update, float* G_new, float* xi, int* info,
                                rnnpose_stream_t stream);

/* fused a9+a10+a11: `num_iters` GN steps (reprojction_optim), G updated in place (B,4,4).
 * Hm/bv/xi/info receive the LAST iteration's values.                                               */
int rnnpose_lm_step_f32(const float* target, int target_mode, const float* weight, const float* depth,
                        float depth_eps, const float* K, float* G, int B, int H, int W, int num_iters,
                        double ep_lambda, double lm_lambda, double max_update, void* workspace,
                        size_t workspace_bytes, double* Hm, double* bv, float* xi, int* info,
                        rnnpose_stream_t stream);
/* same with separate input and output poses (num_iters >= 1; G_out may alias G_in): saves the caller a device copy */
int rnnpose_lm_step_io_f32(const float* target, int target_mode, const float* weight, const float* depth,
                           float depth_eps, const float* K, const float* G_in, float* G_out, int B, int H, int W,
                           int num_iters, double ep_lambda, double lm_lambda, double max_update, void* workspace,
                           size_t workspace_bytes, double* Hm, double* bv, float* xi, int* info,
                           rnnpose_stream_t stream);
/* ---- the depth-aware step (RGB-D): a9 / the fused step with an opt-in 3-D residual from the OBSERVED depth in the same sums.
 * The 2-D terms (v, w, J, X0, X1 = G X0, the clamped Zc, K, target) are those of rnnpose_lm_normal_eq_f64.  In addition, for a
 * crop pixel (x, y) with matched position t = (tx, ty) in crop pixel-index coordinates (after target_mode handling):
 *  1. position in the observed frame, fp32 in this order, theta (B,2,3) the affine map that made the crop (rnnpose_zoom_crop_f32):
 *     bx = (2 tx + 1)/W - 1, by = (2 ty + 1)/H - 1; gx = th0 bx + th1 by + th2, gy = th3 bx + th4 by + th5;
 *     ix = ((gx + 1) Wo - 1)/2, iy = ((gy + 1) Ho - 1)/2;
 *  2. observed depth zo at (ix, iy) from obs_depth[src_index[b]] (S,Ho,Wo); a tap is missing when it is outside the frame, <= 0 or
 *     not finite.  All four bilinear taps present and max - min <= edge_tol: bilinear (weights and order of the crop kernel);
 *     otherwise the nearest tap (floor(ix + 0.5), floor(iy + 0.5)) if present; otherwise the pixel has no depth term.  A non-finite
 *     ix / iy, or one with |.| >= 1e8, has no depth term;
 *  3. observed point Y = zo K_obs^-1 (ix, iy, 1), K_obs (B,3,3) the FULL-FRAME intrinsics of object b (fx, fy, cx, cy are read);
 *  4. the term is active iff v holds and |Y.z - X1.z| <= depth_gate (inclusive);
 *  5. omega = depth_weight fx fy / Zc^2 with the crop's fx, fy, and 0 where Zc <= 0.02 (where the 2-D Jacobian is zeroed);
 *  6. with r3 = Y - X1 and J_T = [I | -[X1]x]:  Hm += v w omega J_T^T J_T,  bv += v w omega J_T^T r3;
 *     dstats (B,2) fp64, may be NULL: [b][0] = number of active pixels, [b][1] = sum v w omega |r3|^2.
 * src_index (B) int32 device pointer, or NULL: S == B and object b reads frame b.  depth_weight = 0, or an observed depth without
 * any present tap, gives Hm, bv (and G, xi, info) bit-identical to the entries without the term.  Workspace and the fused /
 * three-launch forms (rnnpose_lm_fused_tail) as for rnnpose_lm_step_io_f32; the workspace may be shared with it.
 * Returns 1 for a null obs_depth / theta / K_obs, S < 1, a null src_index with S != B, and a negative or non-finite depth_weight,
 * depth_gate or edge_tol.                                                                          */
int rnnpose_lm_normal_eq_rgbd_f64(const float* target, int target_mode, const float* weight, const float* depth,
                                  float depth_eps, const float* K, const float* G, int B, int H, int W,
                                  const float* obs_depth, const int* src_index, const float* theta, const float* K_obs,
                                  int S, int Ho, int Wo, float depth_weight, float depth_gate, float edge_tol,
                                  void* workspace, size_t workspace_bytes, double* Hm, double* bv, double* dstats,
                                  rnnpose_stream_t stream);
int rnnpose_lm_step_rgbd_io_f32(const float* target, int target_mode, const float* weight, const float* depth,
                                float depth_eps, const float* K, const float* G_in, float* G_out, int B, int H, int W,
                                int num_iters, double ep_lambda, double lm_lambda, double max_update,
                                const float* obs_depth, const int* src_index, const float* theta, const float* K_obs,
                                int S, int Ho, int Wo, float depth_weight, float depth_gate, float edge_tol,
                                void* workspace, size_t workspace_bytes, double* Hm, double* bv, float* xi, int* info,
                                double* dstats, rnnpose_stream_t stream);
/* ---- the grouped step (multi-view): ONE increment per object from the summed systems of all its views.
 * The B rows of the batch are VIEWS; the views of group g are rows [group_start[g], group_start[g+1]) (group_start: (n_groups+1) int32
 * device pointer, 0 = group_start[0] < ... < group_start[n_groups] = B).  E (B,4,4) fp32 row-major: the camera-from-rig transform
 * E_v = (R, t) of every view (a single camera: the identity).  With T_v = E_v T_rig, a rig-frame left increment delta acts in view v as
 * xi_v = Ad(E_v) delta, Ad(E) = [[R, [t]x R], [0, R]] (translation first).  Per iteration:
 *  1. Hm (B,6,6), bv (B,6) (and dstats (B,2), with the depth term): every VIEW's undamped system, bit-identical to
 *     rnnpose_lm_normal_eq_f64 (obs_depth == NULL: the plain sums; theta, K_obs, src_index, S, Ho, Wo, depth_weight, depth_gate, edge_tol
 *     are then ignored and dstats stays unwritten) or to rnnpose_lm_normal_eq_rgbd_f64 of the same arguments;
 *  2. Hg (n_groups,6,6) = sum_v Ad_v^T Hm_v Ad_v, bg (n_groups,6) = sum_v Ad_v^T bv_v in fp64, the views in ascending order, no atomics:
 *     deterministic, Hg exactly symmetric;
 *  3. xi (n_groups,6), info (n_groups): the damped solve of rnnpose_lm_solve_update_f32 on Hg, bg (same operations, same order);
 *  4. D = exp(xi) once per group; every view of the group: G_v <- (E_v D E_v^-1) G_v in fp32 (E_v^-1 the rigid inverse).
 * num_iters >= 1; later iterations continue in place on G_out (which may alias G_in); the outputs hold the LAST iteration's values.
 * Two launches per iteration (the partial sums, then one workgroup per group); rnnpose_lm_fused_tail does not apply.  The workspace is
 * that of the other steps (rnnpose_lm_workspace_bytes(B,H,W)) and may be shared with them: no arrival counter is used or left non-zero.
 * The kernel clamps every range to [0, B]; a group that is empty after that gets info = -1 and nothing else of it is written.  With
 * every group of one view and E the identity, G_out, Hm, bv, xi, info are those of rnnpose_lm_step_io_f32 / _rgbd_io_f32 bit for bit.
 * Returns 1 for a null group_start / E / Hg / bg / xi / info, n_groups < 1 or > B, and everything the ungrouped steps refuse. */
int rnnpose_lm_step_views_io_f32(const float* target, int target_mode, const float* weight, const float* depth,
                                 float depth_eps, const float* K, const float* G_in, float* G_out, int B, int H, int W,
                                 int num_iters, double ep_lambda, double lm_lambda, double max_update,
                                 const float* obs_depth, const int* src_index, const float* theta, const float* K_obs,
                                 int S, int Ho, int Wo, float depth_weight, float depth_gate, float edge_tol,
                                 const int* group_start, int n_groups, const float* E,
                                 void* workspace, size_t workspace_bytes, double* Hm, double* bv, double* Hg, double* bg,
                                 float* xi, int* info, double* dstats, rnnpose_stream_t stream);
/* The fused steps run ONE launch per Gauss-Newton iteration: the workgroup that arrives last for an image (device-scope ticket
 * in the workspace, which must therefore be ZERO-FILLED when it is allocated) sums the partial records, solves and updates the
 * pose.  rnnpose_lm_fused_tail(0) restores the three-launch form (normal equations, finalize, solve) for measurements. */
int rnnpose_lm_fused_tail(int enable);

/* ---- a11/a12 helpers: batched SE(3) ------------------------- geometry/se3.py:194-209,228-306
 * se3_exp: xi (B,6) -> (B,4,4);  se3_compose: out = A*Bm (B,4,4);  se3_inverse: out = A^-1.        */
int rnnpose_se3_exp_f32(const float* xi, int B, float* out, rnnpose_stream_t stream);
int rnnpose_se3_compose_f32(const float* A, const float* Bm, int B, float* out, rnnpose_stream_t stream);
int rnnpose_se3_inverse_f32(const float* A, int B, float* out, rnnpose_stream_t stream);
/* r06: the pose bookkeeping between two outer iterations as one launch (model/PoseRefiner.py:241-244): Ti_out = Tij Ti; Tij_out = Ti_out Ti_out^-1 (literal != 0:
 * the reference's legacy product) or the exact identity (literal == 0).  Bit-identical to rnnpose_se3_compose_f32 / _inverse_f32 / _compose_f32 in that order.
 * Tij, Ti, Ti_out, Tij_out: (B,4,4) fp32 row-major; the outputs must not alias the inputs. */
int rnnpose_se3_outer_update_f32(const float* Tij, const float* Ti, int B, int literal, float* Ti_out, float* Tij_out, rnnpose_stream_t stream);

/* ---- a4: SepConvGRU pointwise stages ---------------------------- thirdparty/raft/update.py:45-60
 * zr (B,2C,h,w) = pre-activation outputs of the fused z|r convolution, hcat (B,Ctot,h,w) whose first
 * C channels are h: writes rh = sigmoid(r)*h into rhx[:, :C] (rhx (B,Ctot,h,w), channels >= C untouched)
 * and z = sigmoid(z_pre) into z_out (B,C,h,w).
 * gru_update: h_new = (1-z)*h + z*tanh(q_pre), written to hout (a (B,Ctot_out,h,w) buffer, first C ch). */
int rnnpose_gru_gate_f32(const float* zr, const float* hcat, int B, int C, int Ctot, int hw, float* z_out,
                         float* rhx, rnnpose_stream_t stream);
int rnnpose_gru_update_f32(const float* z, const float* q_pre, const float* hcat, int B, int C, int Ctot_in,
                           int hw, float* hout, int Ctot_out, rnnpose_stream_t stream);

/* ---- a4: dense convolutions of the update block, NHWC, fp16x3-split MFMA (fp32-class accuracy) ----------
 *      thirdparty/raft/update.py:6-14 (FlowHead), :33-60 (SepConvGRU), :79-97 (BasicMotionEncoder), :172-187
 * Zero padding kh/2 x kw/2, odd kernel sizes up to 7 (1x1, 3x3, 1x5, 5x1 are what the update block uses), stride 1 or 2.
 * Input = virtual concat of up to 4 NHWC tensors (B,H,W,c_stride), using channels [c_offset, c_offset+c_count).
 * Weights are packed once by rnnpose_conv_pack_weights_f16x3 from the PyTorch layout (c_out, c_in, kh, kw),
 * with the SAME segment channel counts; w_scale (a power of two) must be the one given to the packer.
 * Output y = conv(x) + bias goes through `epilogue`:
 *   0 linear / 1 ReLU            -> dst[pixel, dst_c_offset + n]
 *   2 GRU z|r (c_out = 2*gru_c)  -> n <  gru_c: dst  = sigmoid(y)                     (z)
 *                                   n >= gru_c: dst2 = sigmoid(y) * aux0[pixel, n-gru_c]   (r*h, aux0 = h)
 *   3 GRU state update           -> dst = (1 - aux1) * aux0 + aux1 * tanh(y)          (aux1 = z, aux0 = h)
 * All destination / aux tensors are NHWC with their own channel stride and offset (so results land directly
 * in a slice of a wider tensor).  dst must not alias a source of the same launch.                      */
typedef struct {
  const float* ptr;
  int c_stride, c_offset, c_count;
} rnnpose_conv_src_t;

typedef struct {
  rnnpose_conv_src_t src[4];
  int n_src;
  int B, H, W;                 /* INPUT spatial size */
  int kh, kw;
  int stride;                  /* 1, or 2 (output = ceil(H/2) x ceil(W/2), padding kh/2, kw/2: the encoder's strided convs) */
  const void* w_packed;        /* from rnnpose_conv_pack_weights_f16x3 (fp16 hi and lo parts, MFMA-fragment order) */
  const float* bias;
  int c_out;
  float a_scale, w_scale;
  int epilogue;
  float* dst;
  int dst_c_stride, dst_c_offset;
  const float* aux0;
  int aux0_c_stride, aux0_c_offset;
  const float* aux1;
  int aux1_c_stride, aux1_c_offset;
  float* dst2;
  int dst2_c_stride, dst2_c_offset;
  int gru_c;
  double* tile_stats;          /* optional (NULL = off), linear epilogue only: (B * tiles_per_image, c_out, 2) FP64 receives, per
                                  128-row output tile, the column sums and sums of squares of the outputs (bias included)
                                  -- the instance-norm statistics pass of the encoder without re-reading the tensor
                                  (rnnpose_instnorm_tiles_nhwc_f32).  With tile_stats (or src0_mean_rstd) the output rows
                                  are tiled PER IMAGE: tiles_per_image = rnnpose_conv_tiles_per_image_desc(this descriptor), the last
                                  tile of an image ragged, so no tile straddles two images. */
  const float* add_map;        /* optional (NULL = off): NHWC tensor added to y before the epilogue, y += add_map[pixel,
                                  add_c_offset + n] -- a per-pixel bias.  Used to hoist the part of a convolution whose input
                                  does not change between calls (the context half `inp` of the GRU input, constant over the
                                  inner iterations: update.py:181 concatenates it anew every step) out of the loop: conv is
                                  linear, conv([h|inp|m]) = conv([h|m]) + conv(inp).  Needs c_out % 4 == 0, 16-byte alignment. */
  int add_c_stride, add_c_offset;
  const float* src0_mean_rstd; /* optional (NULL = off): (B, src[0].c_stride, 2) mean / rstd per image and channel of source 0:
                                  the convolution reads relu((x - mean) * rstd) instead of x -- the instance norm + ReLU
                                  between conv1 and conv2 of a ResidualBlock (extractor.py:48-52) applied in the load, so
                                  the normalised tensor is never written.  One source, 3x3, stride 1 only. */
  /* ---- SPLIT TENSORS (round 3): activations that only feed further convolutions live in HBM already split for the
   * fp16 matrix cores, written once by their producer's epilogue instead of being re-split by every consumer tile (a 3x3
   * layer with 256 outputs re-split each input 12 times).  A split tensor has the shape, strides and SIZE of its fp32
   * NHWC counterpart (4 bytes per element, channel counts / offsets in multiples of 8); every 8-channel group of a pixel
   * occupies 32 bytes = [hi x 8 | lo x 8] fp16 with  x * a_scale = hi + lo  (hi = fp16(x * a_scale) rounded to
   * nearest, lo = fp16(x * a_scale - hi); |x * a_scale| > 65504 is clamped and counted by the range guard).  a_scale must be
   * the same for the producer and every consumer of a tensor (the package uses 8). */
  int src_hl;                  /* != 0: ALL sources are split tensors (stride 1, 1/3/5 taps per group, no src0_mean_rstd) */
  int dst_hl;                  /* != 0: dst receives the split form (no tile_stats) */
  int dst2_hl;                 /* != 0: dst2 (r*h of the GRU z|r epilogue) receives the split form */
  float* dst_split;            /* optional (NULL = off): a second copy of the primary result in split form (GRU state update:
                                  h' is needed as fp32 by the next gate epilogue AND split by the next convolution); not
                                  with epilogue 2 */
  int dst_split_c_stride, dst_split_c_offset;
  int src_bounded;             /* != 0: the caller guarantees |source| < 65504 / a_scale, the range guard skips this launch.  The
                                  encoder sets it: every convolution input there is an instance-normalised map or a ReLU sum of a few
                                  (|(x - mean) * rstd| <= sqrt(H*W); extractor.py:48-58), two orders below the fp16x3 range */
  int tile;                    /* 0 = automatic; 1 = 128x64, 2 = 128x128 as 4 column waves, 3 = 128x128 as 2x2 waves, 4 = 128x64 with
                                  a block-deep register pipeline (3, 4: split sources only); 5 / 6 / 7 = the STRIP kernels with 160- / 32- / 96-row strips (160 / 32 / 96 output
                                  pixels x 64 / 96 / 128 columns per workgroup, weights and split-tensor activations by LDS-DMA:
                                  stride 1, 3x3 / 1x5 / 5x1, c_out > 32, source channel counts in multiples of 32).  How the automatic choice picks a family
                                  and how each family tiles an image: at rnnpose_conv_tiles_per_image_desc below. */
  void* ksplit_ws;             /* optional (NULL = off): workspace of rnnpose_conv_ksplit_workspace_bytes() bytes, 16-byte aligned,
                                  its first 1024 bytes ZERO before the first launch (the kernel leaves them zero).  With it, a
                                  stride-1 launch of few tiles (B = 1 crops: 8-64 workgroups on 256 CUs) splits its K loop over up
                                  to 8 workgroups per tile; the last one to arrive sums the partial accumulators in split order
                                  (deterministic) and runs the epilogue.  Launches that may run CONCURRENTLY (two streams) need
                                  separate workspaces. */
  size_t ksplit_ws_bytes;
  int single_product;          /* != 0: ONE fp16 product per multiply-add (a_hi * b_hi, fp32 accumulation) instead of the three of the
                                  fp16x3 split -- cfg.raft.mixed_precision, the arithmetic the reference runs on a GPU (model/CFNet.py:
                                  47,126,152: fp16 autocast around encoder and update block).  Honoured by the 160-row strip kernels
                                  (the layers the automatic choice gives them: the update block and the encoder's residual layers at
                                  the headline shapes); every other kernel keeps the three-product form.  ~2^-11 relative per product:
                                  NOT the arithmetic of the parity tolerances. */
  int tile_stats_records;      /* with tile_stats: how many (c_out, 2) records the buffer holds.  The launch REFUSES a buffer smaller
                                  than (ABI 3, r06: other than) B * rnnpose_conv_tiles_per_image_desc(this descriptor) -- which kernel family a launch takes
                                  (and with it the tile count: 32-row strips write four times the records of 128-row tiles) is the
                                  library's choice, so the buffer is checked where the choice is made. */
} rnnpose_conv_desc_t;

size_t rnnpose_conv_ksplit_workspace_bytes(void);
int rnnpose_conv_ksplit(int enable);       /* measurement switch (default 1): 0 = never split K */
int rnnpose_conv_ksplit_limits(int max_tiles, int max_splits);   /* measurement: launches of <= max_tiles (default 24, <= 96) tiles
                                                                     split into <= max_splits (default 4, 2..8) ranges */

/* Output tiles per image of exactly the launch this descriptor describes = records per image of its `tile_stats`.  The kernel choice looks
 * at B, H, W, kh, kw, stride, c_out, tile, the sources' channel counts, src_hl and whether src0_mean_rstd is set (pointers are not
 * dereferenced, dst / weights may be NULL); the launch plans itself with the same function, so the answer cannot disagree with
 * rnnpose_conv2d_nhwc_f16x3, which requires tile_stats_records == B * (this answer).  -1 on bad arguments, and for a strip height forced
 * (tile 5 / 6 / 7) on a launch the strip kernels cannot take.  The tiling rules:
 *   - 128-row kernels: 3x3 stride-1 layers run on 8 x 16 image PATCHES (ceil(W/16) * ceil(H/8) tiles per image, nine taps on one staged
 *     halo tile), everything else on runs of 128 output pixels (ceil(H_out*W_out/128) when tiled per image).  rnnpose_conv_spatial_tiles(0)
 *     switches the patch tiling off (measurement: the r02 row-major tiling for 3x3 layers too).
 *   - strip kernels (160 / 96 / 32 rows): 3x3 layers on ceil(W/16) * ceil(H/10) patches of 10 x 16 pixels (96 rows: 6 x 16, 32 rows:
 *     2 x 16), 1x5 / 5x1 layers on ceil(H*W/160) runs of 160 (96, 32) pixels; stride-2 3x3 / 1x1 layers like a 3x3 layer on the OUTPUT grid.
 *   - the automatic choice (tile 0) takes 160-row strips for stride-1 3x3 / 1x5 / 5x1 layers when they give the launch >= 240 workgroups
 *     (or >= 24 per image with more than 8192 pixels) -- r06: 32-row strips instead when those are at most 256 waves, 96-row strips
 *     when at most 512 (the thin layers of a half-batch chain) --, 32-row strips for launches of <= 8192 pixels (single-image crops),
 *     else the 128-row kernels; only for sources of whole 32-channel blocks, with src0_mean_rstd only for 3x3.  Stride 2 (3x3 / 1x1, even
 *     H and W): 160-row strips by the same counts for ONE fp32 source of whole 32-channel blocks without src0_mean_rstd.
 *     rnnpose_conv_strip(0): never strips. */
int rnnpose_conv_tiles_per_image_desc(const rnnpose_conv_desc_t* h_desc);
/* fp16 MFMA products per multiply-add the launch this descriptor describes executes: 3 (fp16x3 split) or 1 (single_product honoured:
 * 160-row strips with one column tile per wave).  For flop accounting (bench.py's pipe_util); -1 where the call above answers -1. */
int rnnpose_conv_products_desc(const rnnpose_conv_desc_t* h_desc);
int rnnpose_conv_spatial_tiles(int enable);
int rnnpose_conv_strip(int mode);          /* measurement switch: 0 = the automatic choice never takes the strip kernels, 1 = default,
                                              2 = automatic without the two-wave workgroups of 64-channel layers, 3 = two 32-column
                                              tiles per wave (one workgroup per CU), 4 = 160-row strips only (>= 24 per image), 5 = automatic
                                              without the stride-2 form (r05: stride-2 3x3 layers as 2x2-tap strips over the four parity
                                              planes of the input; one fp32 source of whole 32-channel blocks, even H and W), 6 = automatic without r06's
                                              32-row strips for launches whose 160-row strips would be at most 256 waves, 7 = automatic WITH persistent launches of the
                                              fp32-source strip forms (r06: resident workgroups walking the tile list; measured slower, off by default) */
/* number of fp16 elements of the packed weight array (hi and lo parts interleaved, in the fragment order of the 128-row kernels
 * followed by the record order of the strip kernels); -1 on bad arguments */
long long rnnpose_conv_packed_halfs(int c_out, int kh, int kw, const int* h_seg_counts, int n_seg);
int rnnpose_conv_pack_weights_f16x3(const float* w_oihw, int c_out, int c_in, int kh, int kw, const int* h_seg_counts,
                                    int n_seg, float w_scale, void* w_packed, rnnpose_stream_t stream);
int rnnpose_conv2d_nhwc_f16x3(const rnnpose_conv_desc_t* h_desc, rnnpose_stream_t stream);

/* fp16x3 range guard.  Activations are split as x*a_scale = hi + lo in fp16: |x*a_scale| > 65504 does not fit, the hi
 * part is clamped and the result is WRONG (the reference computes in fp32 and has no such cliff; a NaN even becomes a
 * finite value).  With the check enabled, every launch that splits fp32 values (convolutions, resident 1x1, lookup +
 * convc1, mask head, encoder stem, flow features, rnnpose_split_hl_f32, the volume build's operand pre-pass) adds to a
 * device counter.  WHAT THE NUMBER MEANS:
 *   - it is ZERO if and only if no element the launch reads inside its windows (channels [c_offset, c_offset + count)
 *     of the launch's pixels), and no element it writes in split form, has |x * a_scale| > 65504 or is not finite.
 *     Where src0_mean_rstd is set, the value that is split -- after the fused normalisation + ReLU -- is the one that
 *     is tested, so what that ReLU turns into 0, a NaN included, is in range.  Channels outside the windows, rows
 *     behind the launch's last pixel, halo / padding positions, the padding rows of a ragged tile and the positions of
 *     a flow-feature row segment past the line's end never count.  A launch with src_bounded set counts nothing, and a
 *     consumer with src_hl checks nothing on its inputs (they arrive split: their producer's epilogue was the check);
 *   - it is EXACT -- the number of offending quads (4 consecutive channels of a pixel; an 8-channel group for
 *     rnnpose_split_hl_f32 and the pixel-major pre-pass, an element for the NCHW pre-pass, a window tap for lookup +
 *     convc1, a channel's 20-pixel row segment for the flow-feature output) -- for the kernels that stage every value
 *     once: resident 1x1, lookup + convc1, mask head, flow features, rnnpose_split_hl_f32, the pre-pass, and the
 *     split-form OUTPUTS of every kernel;
 *   - elsewhere (fp32 sources of the 128-row and strip convolutions, the stem) it is a MULTIPLE of that: a quad is
 *     counted once per staging, i.e. per tap of a 1x5 / 5x1 / stride-2 layer, per 3x3 halo tile or strip patch that
 *     holds it, per share of a K split, per overlapping stem patch (only the first column tile of a row tile counts,
 *     so not per column tile).
 * rnnpose_f16x3_saturation_count synchronises `stream`, returns the count since the last reset and optionally resets
 * it.  The library starts with the check off; the Python package switches it on (the test costs ~3 vector
 * instructions per staged float4).  Process-global switch; not meant to be toggled concurrently with launches. */
int rnnpose_f16x3_saturation_check(int enable);
int rnnpose_f16x3_saturation_count(unsigned long long* h_count, int reset, rnnpose_stream_t stream);
/* Device-side read of the same counter: copies it into *d_count (DEVICE memory) on `stream`, no host synchronisation --
 * callers fold it into their outputs (PoseRefiner returns it as "f16x3_range_events") so that a clamp cannot pass unseen. */
int rnnpose_f16x3_saturation_peek(unsigned long long* d_count, rnnpose_stream_t stream);

/* ---- f1: RAFT encoder stem -- input normalisation + 7x7 stride-2 convolution 3 -> 64 in one kernel -------------
 *      model/CFNet.py:42-43 (image = 2*(image/255) - 1), thirdparty/raft/extractor.py:131,197 (conv1)
 * img (N,3,H,W) fp32 NCHW -> out (N, ceil(H/2), ceil(W/2), 64) fp32 NHWC = conv7x7_s2_p3(normalize ? 2*(img/255)-1 : img) + bias.
 * Weights (64,3,7,7) packed once by rnnpose_stem_pack_weights_f16x3 (2 arrays of rnnpose_stem_packed_halfs() fp16).
 * tile_stats (optional): (N * tiles_per_image, 64, 2) per-tile column sums / sums of squares for
 * rnnpose_instnorm_tiles_nhwc_f32 (8 x 16 output tiles; pixels of a ragged tile outside the image never enter the sums, so the
 * statistics hold for every size -- rnnpose_stem_tiles reports h_exact = 1 always since r03; the field is kept for callers).
 * r06: the kernel is PERSISTENT -- two workgroups per CU walk the tile list with the packed weights resident in LDS and the patch split
 * into fp16 hi / lo once per tile; rnnpose_stem_workgroups(n) caps the number of workgroups (tests: many tiles per workgroup at small
 * sizes; 0 = default).  Results do not depend on it.
 * LIMITS: out, bias and the packed weights 16-byte aligned; N * tiles < 2^31; and, because the kernel addresses image and output with
 * 32-bit byte offsets, the image (N*3*H*W*4 bytes) and the output (N*ceil(H/2)*ceil(W/2)*256 bytes), each extended by the overhang of
 * the last 8 x 16 output tile (its 21 x 37 input patch), must stay below 2^31 bytes: 109 frames of 480 x 640 are accepted, 110 are
 * refused ("batch too large for 32-bit byte offsets") before anything is launched -- callers split larger batches. */
long long rnnpose_stem_packed_halfs(void);
int rnnpose_stem_workgroups(int max_workgroups);
int rnnpose_stem_pack_weights_f16x3(const float* w_oihw, float w_scale, void* w_hi, void* w_lo, rnnpose_stream_t stream);
int rnnpose_stem_tiles(int H, int W, int* h_tiles_per_image, int* h_exact);
int rnnpose_stem_conv7x7_s2_f16x3(const float* img_nchw, int N, int H, int W, int normalize, const void* w_hi,
                                  const void* w_lo, const float* bias, float a_scale, float w_scale, float* out_nhwc,
                                  double* tile_stats, rnnpose_stream_t stream);

/* ---- NHWC companions of the fused update-block engine ----------------------------------------------------
 * corr_lookup_nhwc: a3 with the output laid out (B,h,w,levels*81) (thirdparty/raft/corr.py:36-57).
 * nchw_to_nhwc / nhwc_to_nchw: (B,C,HW) <-> channel window [c_offset, c_offset+C) of a (B,HW,c_stride) tensor.
 * flow_prep: flow = coords1 - grid (model/CFNet.py:150; subtract_grid = 0: coords1 already holds the flow, the
 *   BasicUpdateBlock.forward boundary of update.py:178) written as (B,h,w,4) [fx,fy,0,0] (input of the 7x7 flow
 *   convolution, update.py:84) and into channels [motion_c_offset, +2) of the motion-feature tensor (update.py:97).
 * flow_conv7x7_relu: BasicMotionEncoder.convf1 + ReLU (7x7, 2 -> c_out <= 128, update.py:84,91) as a direct fp32
 *   convolution (K = 98 is too thin for the matrix cores): flow4 from flow_prep, w_t = the (c_out,2,7,7) weight
 *   transposed to (98, c_out), output into channels [out_c_offset, +c_out) of an NHWC tensor.
 * flow_head_out: FlowHead.conv2 (3x3, c_in -> 2, update.py:10,14) on channels [x_c_offset, +c_in) of x, fused with
 *   coords1 += delta (CFNet.py:157): delta (B,h,w,2), coords1_out (B,2,h,w) (may be NULL), flow_lr (B,h,w,2) =
 *   coords1_out - grid.  w_oihw is the PyTorch (2,c_in,3,3) weight.
 * convex_upsample_nhwc: a6 (model/CFNet.py:95-106) with mask (B,h,w,576) and flow_lr (B,h,w,2) -> (B,2,8h,8w). */
int rnnpose_corr_lookup_nhwc_f32(const float* pyramid, const float* coords, int B, int h, int w, int levels, int radius,
                                 float* out, rnnpose_stream_t stream);
/* NHWC lookup of the images [b0, b1) of a pyramid built for batch B: coords (b1-b0,2,h,w) and out (b1-b0,h,w,levels*81)
 * are the sub-batch tensors, `pyramid` the whole buffer (thirdparty/raft/corr.py:36-57 per image). */
int rnnpose_corr_lookup_nhwc_part_f32(const float* pyramid, const float* coords, int B, int b0, int b1, int h, int w,
                                      int levels, int radius, float* out, rnnpose_stream_t stream);
/* r06: the same lookup FORMING its coordinates itself: coords1 = grid + down-sampled pose-induced flow (exactly
 * rnnpose_induced_coords_lowres_f32's values: geometry/transformation.py:184-198, model/PoseRefiner.py:324-328, model/CFNet.py:136-144) from
 * depth (b1-b0,1,H,W), K (b1-b0,3,3), G (b1-b0,4,4) of the part's images; coords_out (b1-b0,2,h,w) receives them for the later consumers of
 * the iteration.  One launch and one dependent kernel boundary fewer per GRU iteration. */
int rnnpose_corr_lookup_induced_nhwc_part_f32(const float* pyramid, const float* depth, const float* K, const float* G, int H, int W,
                                              float eps, int B, int b0, int b1, int h, int w, int levels, int radius, float* coords_out,
                                              float* out, rnnpose_stream_t stream);
int rnnpose_nchw_to_nhwc_f32(const float* src, int B, int C, int HW, float* dst, int dst_c_stride, int dst_c_offset,
                             rnnpose_stream_t stream);
int rnnpose_nhwc_to_nchw_f32(const float* src, int B, int C, int HW, int src_c_stride, int src_c_offset, float* dst,
                             rnnpose_stream_t stream);
int rnnpose_flow_prep_f32(const float* coords1, int subtract_grid, int B, int h, int w, float* flow4, float* motion,
                          int motion_c_stride, int motion_c_offset, rnnpose_stream_t stream);
int rnnpose_flow_conv7x7_relu_f32(const float* flow4, const float* w_t, const float* bias, int B, int h, int w, int c_out,
                                  float* out, int out_c_stride, int out_c_offset, rnnpose_stream_t stream);
/* flow_prep + flow_conv7x7_relu in one launch: coords1 (B,2,h,w) planar (grid subtracted here when subtract_grid != 0) ->
 * relu(convf1(flow)) into `out`, and the flow itself into channels [motion_c_offset, +2) of `motion` (update.py:84,91,97). */
int rnnpose_flow_features_f32(const float* coords1, int subtract_grid, const float* w_t, const float* bias, int B, int h, int w,
                              int c_out, float* out, int out_c_stride, int out_c_offset, float* motion, int motion_c_stride,
                              int motion_c_offset, int out_split, int motion_split, float a_scale, rnnpose_stream_t stream);
/* r06: rnnpose_flow_features_f32 forming coords1 itself from depth (B,1,H,W), K (B,3,3), G (B,4,4) (see
 * rnnpose_corr_lookup_induced_nhwc_part_f32), grid subtracted: flow = coords1 - grid -> relu(convf1(flow)), motion[..., co:co+2]. */
int rnnpose_flow_features_induced_f32(const float* depth, const float* K, const float* G, int H, int W, float eps, const float* w_t,
                                      const float* bias, int B, int h, int w, int c_out, float* out, int out_c_stride, int out_c_offset,
                                      float* motion, int motion_c_stride, int motion_c_offset, int out_split, int motion_split,
                                      float a_scale, rnnpose_stream_t stream);
/* out_split / motion_split != 0: `out` / `motion` are split tensors (rnnpose_conv_desc_t, "SPLIT TENSORS") with scale a_scale.
 * rnnpose_split_hl_f32: channels [src_c_offset, +c_count) of an fp32 NHWC tensor -> the split form in channels
 * [dst_c_offset, +c_count) of `dst` (c_count, dst offsets / strides multiples of 8): hidden state / context input once per
 * outer iteration (model/CFNet.py:131-133 produce them in fp32). */
int rnnpose_split_hl_f32(const float* src, int src_c_stride, int src_c_offset, long long n_pixels, int c_count, float a_scale,
                         float* dst, int dst_c_stride, int dst_c_offset, rnnpose_stream_t stream);
int rnnpose_flow_head_out_f32(const float* x, int x_c_stride, int x_c_offset, int c_in, const float* w_oihw,
                              const float* bias, const float* coords1, int B, int h, int w, float* delta,
                              float* coords1_out, float* flow_lr, rnnpose_stream_t stream);
int rnnpose_convex_upsample_nhwc_f32(const float* flow_lr, const float* mask, int B, int h, int w, float* flow_up,
                                     rnnpose_stream_t stream);
/* ---- SuperPoint2D glue (model/descriptor2D.py; rnnpose_amd/descriptor2d.py) -------------------------------------------
 * Channel windows [c_offset, +C) of NHWC tensors (B,H,W,c_stride): C, offsets and strides multiples of 4, 16-byte aligned
 * tensors; B * H * W (of the larger side) below 2^31.
 * maxpool2x2_nhwc: nn.MaxPool2d(2, 2) (floor): (B,H,W) -> (B,H/2,W/2), NaN propagating.
 * upsample2x_bilinear_nhwc: nn.Upsample(scale_factor=2, mode='bilinear') (align_corners=False): (B,h,w) -> (B,2h,2w).
 *   mean_rstd (B,C,2) of the source window or NULL: every tap is read as (x - mean) * rstd, then ReLU'd when relu != 0 (the
 *   instance norm + ReLU of the decoder stages, applied in the load).
 * pixel_head_nhwc: 1x1 convolution c_in (<= 256) -> c_out (<= 32) with weight (c_out, c_in) fp32 + bias, the source read as
 *   relu?((x - mean) * rstd) when mean_rstd (B,c_in,2) is given (relu alone without it), written NCHW to dst (B,c_out,HW);
 *   mode 0 linear, 1 L2 normalisation over the outputs (F.normalize: y / max(|y|_2, 1e-12)), 2 sigmoid. */
int rnnpose_maxpool2x2_nhwc_f32(const float* src, int B, int H, int W, int src_c_stride, int src_c_offset, int C, float* dst,
                                int dst_c_stride, int dst_c_offset, rnnpose_stream_t stream);
int rnnpose_upsample2x_bilinear_nhwc_f32(const float* src, int B, int h, int w, int src_c_stride, int src_c_offset, int C,
                                         const float* mean_rstd, int relu, float* dst, int dst_c_stride, int dst_c_offset,
                                         rnnpose_stream_t stream);
int rnnpose_pixel_head_nhwc_f32(const float* src, int B, int HW, int src_c_stride, int src_c_offset, int c_in,
                                const float* mean_rstd, int relu, const float* weight, const float* bias, int c_out, int mode,
                                float* dst_nchw, rnnpose_stream_t stream);
/* ---- KPSuperpoint3Dv2 (model/descriptor3D.py on thirdparty/kpconv/kpconv_blocks.py; rnnpose_amd/descriptor3d.py) -----------
 * Rows are points: a feature matrix is (N, C) fp32 with row stride ld >= C (a channel slice of a wider buffer is passed as its
 * first element's address and the buffer's stride).  Neighbour tables are int32 (n_q, width); the value n_s (the support's
 * row count over all stacked clouds) is the shadow neighbour; rows beyond 2^31 elements use 64-bit offsets.
 * point_row_sum: out[i] = sum_c x[i, c] (the positive-sum neighbour count, kpconv_blocks.py:366-369).
 * kpconv_aggregate: KPConv.forward (:300-372; linear influence, sum aggregation, rigid kernel) up to its weight product:
 *   wf (n_q, K * c_in) contiguous, column k * c_in + c = sum_j clamp(1 - |s_j - q - kp_k| / extent, 0) x[j, c] / max(1, #{j real:
 *   row_sum[j] > 0}); neighbours = neighbors[q, :width] (indices in 0..n_s), kernel_points (K, 3), K <= 16, c_in <= 256.
 *   rnnpose_point_linear_f32(wf, .., K * c_in, weights (K, c_in, c_out) as (K c_in, c_out)) finishes the convolution.
 * point_linear: out[i, j] = sum_k a[i, k] w[k, j] (+ bias[j] if bias), w (k, m) contiguous; fp32 FMA in k order (:505, :524,
 *   model/descriptor3D.py:91-93 bottle / proj_gnn).
 * point_norm_stats: InstanceNorm1d over ALL n rows (:456-473, no affine, biased variance): mean_rstd (c, 2) = (mean, 1/sqrt(var + eps)),
 *   fp64 accumulation; workspace of rnnpose_point_norm_workspace_bytes(n, c).
 * point_norm_apply: out = (x - mean) * rstd [+ res, read as (res - mean_r) * rstd_r when res_mean_rstd] [then LeakyReLU(slope) when
 *   leaky]: UnaryBlock / SimpleBlock / the ResnetBottleneckBlock tail (:514-519, :585, :659-687).  out may be x.
 * point_maxpool: max_pool (:88-104): out[q, c] = max_j x[idx[q, j], c] with the shadow row = 0.
 * point_gather_rows: closest_pool (:73-85): out[q, c] = x[idx[q * idx_ld], c], 0 for the shadow.
 * point_l2_normalize: F.normalize(p=2, dim=1, eps=1e-12) of each row (model/descriptor3D.py:134-136); out may be x.
 * grid_voxel_keys: grid_subsampling.cpp:50-56 for one cloud: keys[i] = ix + nx iy + nx ny iz with ix = floor((p.x - ox) / dl) in fp32
 *   (correctly rounded division), likewise iy, iz.
 * radius_count / radius_neighbors: batch_query (cpp_neighbors/neighbors/neighbors.cpp:229-330).  Clouds b = 0..n_clouds-1 are
 *   query rows [q_start[b], q_start[b+1]) and support rows [s_start[b], s_start[b+1]) (device int32, n_clouds + 1 entries);
 *   support j is a neighbour of q when ((dx^2 + dy^2) + dz^2) < radius^2 in fp32.  count: counts[q].  neighbors: offsets[q]
 *   (int64) = exclusive prefix sum of counts, cand_idx / cand_d2 of sum(counts) entries (scratch), out (n_q, width) PRE-FILLED
 *   with the shadow index: the neighbours sorted by (d2, index), the first width of them. */
int rnnpose_point_row_sum_f32(const float* x, int n, int c, long long ldx, float* out, rnnpose_stream_t stream);
int rnnpose_kpconv_aggregate_f32(const float* q_pts, int n_q, const float* s_pts, int n_s, const int* neighbors, int width,
                                 const float* kernel_points, int K, float extent, const float* x, int c_in, long long ldx,
                                 const float* row_sum, float* wf, rnnpose_stream_t stream);
int rnnpose_point_linear_f32(const float* a, int n, int k, long long lda, const float* w, int m, const float* bias, float* out,
                             long long ldo, rnnpose_stream_t stream);
long long rnnpose_point_norm_workspace_bytes(int n, int c);
int rnnpose_point_norm_stats_f32(const float* x, int n, int c, long long ldx, float eps, void* workspace, long long workspace_bytes,
                                 float* mean_rstd, rnnpose_stream_t stream);
int rnnpose_point_norm_apply_f32(const float* x, int n, int c, long long ldx, const float* mean_rstd, const float* res, long long ldr,
                                 const float* res_mean_rstd, int leaky, float slope, float* out, long long ldo,
                                 rnnpose_stream_t stream);
int rnnpose_point_maxpool_f32(const float* x, int n_s, int c, long long ldx, const int* idx, int n_q, int width, float* out,
                              long long ldo, rnnpose_stream_t stream);
int rnnpose_point_gather_rows_f32(const float* x, int n_s, int c, long long ldx, const int* idx, int n_q, int idx_ld, float* out,
                                  long long ldo, rnnpose_stream_t stream);
int rnnpose_point_l2_normalize_f32(const float* x, int n, int c, long long ldx, float* out, long long ldo, rnnpose_stream_t stream);
int rnnpose_grid_voxel_keys_f32(const float* points, int n, float ox, float oy, float oz, float dl, long long nx, long long ny,
                                long long* keys, rnnpose_stream_t stream);
int rnnpose_radius_count_f32(const float* queries, int n_q, const float* supports, const int* q_start, const int* s_start,
                             int n_clouds, float radius, int* counts, rnnpose_stream_t stream);
int rnnpose_radius_neighbors_f32(const float* queries, int n_q, const float* supports, const int* q_start, const int* s_start,
                                 int n_clouds, float radius, const long long* offsets, int* cand_idx, float* cand_d2, int width,
                                 int* out, rnnpose_stream_t stream);
/* 1x1 convolution (+ bias, optional ReLU) with the activation tile resident in LDS: 32 pixels x ALL 256 output columns per
 * workgroup, the tile split into fp16 hi / lo once (the implicit-GEMM kernel re-splits it per 64-column tile).  Used for
 * BasicMotionEncoder.convc1 (thirdparty/raft/update.py:80,87: 324 -> 256).  pack: weight (256, c_in) fp32 -> MFMA fragments
 * (rnnpose_conv1x1_resident_packed_bytes(c_in) bytes, 16-byte aligned) of w_scale * weight; c_in % 4 == 0, c_in <= 352.
 * x: n_pixels rows of x_c_stride floats, channels [x_c_offset, +c_in); dst: rows of dst_c_stride, channels [dst_c_offset, +256).
 * Agrees with rnnpose_conv2d_nhwc_f16x3 to fp32 round-off (the K sum is grouped differently).  dst_split != 0: dst is written
 * as a split tensor (rnnpose_conv_desc_t, "SPLIT TENSORS") with the launch's a_scale. */
size_t rnnpose_conv1x1_resident_packed_bytes(int c_in);
int rnnpose_conv1x1_resident_pack_f16x3(const float* weight, int c_out, int c_in, float w_scale, void* packed,
                                        rnnpose_stream_t stream);
int rnnpose_conv1x1_resident_f16x3(const float* x, int x_c_stride, int x_c_offset, int c_in, const void* w_packed,
                                   const float* bias, float a_scale, float w_scale, int relu, long long n_pixels, float* dst,
                                   int dst_c_stride, int dst_c_offset, int dst_split, rnnpose_stream_t stream);
/* r06: the window lookup and convc1 in ONE launch -- corr = CorrBlock.__call__(coords) (thirdparty/raft/corr.py:36-57, bilinear_sampler:
 * thirdparty/raft/utils/utils.py:57-71) followed by relu(convc1(corr)) (thirdparty/raft/update.py:80,87), as GRU_CFUpdator.forward
 * chains them (model/CFNet.py:147-152).  The 4 x 81 window features of a 32-pixel tile are computed level by level straight into an LDS ring of
 * channel blocks that the 1x1 convolution's MFMAs consume (csrc/corr_convc1.hip); the (B,h,w,324) tensor is never written.  (Measured equal
 * to the two-kernel path, not faster: the engine keeps the two kernels by default.)  pyramid: the buffer of rnnpose_corr_pyramid_* built for B
 * images; [b0, b1): the images of this launch; coords (b1-b0, 2, h, w) fp32 (channel 0 = x): window centres; w_packed / bias / scales:
 * convc1 packed by rnnpose_conv1x1_resident_pack_f16x3 with c_in = 324; dst (b1-b0, h, w, dst_c_stride), channels [dst_c_offset, +256),
 * fp32 or (dst_split) a split tensor.  levels must be 4, radius 4.  Same values as rnnpose_corr_lookup_nhwc_part_f32 followed by
 * rnnpose_conv1x1_resident_f16x3 (identical operations per element; tests compare them to 1e-6). */
int rnnpose_corr_lookup_convc1_f16x3(const float* pyramid, const float* coords, int B, int b0, int b1, int h, int w, int levels,
                                     int radius, const void* w_packed, const float* bias, float a_scale, float w_scale, int relu,
                                     float* dst, int dst_c_stride, int dst_c_offset, int dst_split, rnnpose_stream_t stream);
/* mask.2 + convex up-sampling in ONE kernel: mask = post_scale * mask.2(x) (1x1, 256 -> 576, thirdparty/raft/update.py:183-187)
 * is consumed in registers by the softmax / 3x3 convex combination of model/CFNet.py:95-106; the (B,h,w,576) mask tensor is
 * never written.  pack: weight (576,256) fp32 -> fp16 hi / lo MFMA fragments (rnnpose_mask_upsample_packed_bytes() bytes,
 * 16-byte aligned) of post_scale * w_scale * weight.  x (B,h,w,x_c_stride): channels [x_c_offset, +256) = relu(mask.0(h));
 * bias (576) already multiplied by post_scale; flow_lr (B,h,w,2); flow_up (B,2,8h,8w).  The softmax over the 9 taps is
 * evaluated online (running max / sums): agrees with conv2d + rnnpose_convex_upsample_nhwc_f32 to fp32 round-off. */
size_t rnnpose_mask_upsample_packed_bytes(void);
int rnnpose_mask_upsample_pack_f16x3(const float* weight, float post_scale, float w_scale, void* packed, rnnpose_stream_t stream);
int rnnpose_mask_upsample_f16x3(const float* x, int x_c_stride, int x_c_offset, const void* w_packed, int c_out,
                                const float* bias, float a_scale, float w_scale, const float* flow_lr, int B, int h, int w,
                                float* flow_up, rnnpose_stream_t stream);

/* ---- f1 (adjacent): instance norm of the RAFT encoder on NHWC tensors ---- thirdparty/raft/extractor.py:28-31,48-58
 * x (B,HW,C) -> out = act((x - mean_bc) * rsqrt(var_bc + eps)) (biased variance, no affine, as nn.InstanceNorm2d);
 * relu != 0 applies ReLU; if residual != NULL: out = relu(residual + out) (ResidualBlock tail, extractor.py:58).
 * mean_rstd (B,C,2) receives the statistics.  Deterministic (fixed-order fp64 partial sums in `workspace`). */
size_t rnnpose_instnorm_workspace_bytes(int B, int HW, int C);
int rnnpose_instnorm_nhwc_f32(const float* x, int B, int HW, int C, float eps, int relu, const float* residual,
                              void* workspace, size_t workspace_bytes, float* mean_rstd, float* out,
                              rnnpose_stream_t stream);
/* Same normalisation with the statistics taken from the producing convolution's `tile_stats` (tiles_per_image records per
 * image, as the producer laid them out): only the finalize + apply passes run.  out == NULL: statistics only (mean_rstd
 * for a consumer that normalises in its load, rnnpose_conv_desc_t.src0_mean_rstd).
 * residual_mean_rstd (optional, (B,C,2)): `residual` is itself a RAW convolution output whose instance norm [+ ReLU if
 * residual_relu] is applied on the fly: out = relu(act_r((residual - mean_r) * rstd_r) + act((x - mean) * rstd)) -- the
 * stem output / the down-sampling branch of a ResidualBlock are then never written in normalised form (extractor.py:54-58). */
int rnnpose_instnorm_tiles_nhwc_f32(const float* x, int B, int HW, int C, float eps, int relu, const float* residual,
                                    const float* residual_mean_rstd, int residual_relu, const double* tile_stats,
                                    int tiles_per_image, float* mean_rstd, float* out,
                                    rnnpose_stream_t stream);

/* ---- f3 ("next"): brute-force nearest neighbour for ADD-S ------ thirdparty/nn/src/nearest_neighborhood.cu:48-163
 * idxs[b,q] = argmin_r |ref[b,r,:] - que[b,q,:]|^2, first minimum wins, optional r != q; dim 2 or 3.
 * rnnpose_nn_search_f32: DEVICE pointers, asynchronous.
 * findNearestPointIdxLauncher: the reference's own cffi symbol (thirdparty/nn/src/ext.h:1-10): HOST pointers,
 * synchronous, same argument list -- thirdparty/nn/nn_utils.py binds to this library unchanged.              */
int rnnpose_nn_search_f32(const float* ref_pts, const float* que_pts, int* idxs, int b, int pn1, int pn2, int dim,
                          int exclude_self, rnnpose_stream_t stream);
void findNearestPointIdxLauncher(float* ref_pts, float* que_pts, int* idxs, int b, int pn1, int pn2, int dim,
                                 int exclude_self);

/* ---- f2 ("next"): LINEMOD pose metrics on device -------------------- utils/eval_metric.py:28-37,102-192
 * model (P,3), pose_pred / pose_gt (B,3,4), K (3,3) -> out (B,5) fp64 = [mean ADD distance, mean ADD-S distance
 * (nearest predicted point of every target point; -1 unless symmetric), mean 2-D projection error in px,
 * translation error in cm, rotation error in degrees].  Thresholding (0.1/0.02/0.05 diameter, 5 px, 5 cm 5 deg)
 * is host logic (rnnpose_amd/evaluator.py).  workspace is only needed when symmetric != 0.                    */
size_t rnnpose_pose_metrics_workspace_bytes(int B, int P);
int rnnpose_pose_metrics_f64(const float* model, int P, const float* pose_pred, const float* pose_gt, const float* K, int B,
                             int symmetric, void* workspace, size_t workspace_bytes, double* out, rnnpose_stream_t stream);

/* ---- BOP pose-error functions: MSSD / MSPD and VSD (Hodan et al., "BOP challenge 2020 on 6D object localization") -------------
 * The reference has no code for them and bop_toolkit is absent here: the definitions below are the specification (restated in
 * fp64 numpy by tests/bop_ref.py); PARITY WITH bop_toolkit IS UNPINNED.  All arithmetic is fp64 on values converted from the fp32
 * inputs, without fma contraction.  A pose is (3,4) [R|t]; proj(X) = (fx X/Z + cx, fy Y/Z + cy) with K (3,3) row-major.
 * rnnpose_bop_sym_dist_f64: model (P,3), sym (S,3,4) symmetry transformations, S >= 1 (no symmetry = the identity), pose_est /
 *   pose_gt (B,3,4), K (B,3,3), all device fp32 -> out (B,2) fp64:
 *     out[b][0] = MSSD = min_s max_i | T_est x_i - T_gt (S_s x_i) |_2
 *     out[b][1] = MSPD = min_s max_i | proj(T_est x_i) - proj(T_gt (S_s x_i)) |_2      with K[b]
 *   T_gt S_s is formed first (fp64), then applied.  workspace: (B,S,2) fp64 partial maxima.  Two launches, no atomics.
 * rnnpose_bop_vsd_f64: depth_est / depth_gt (B,H,W) fp32 z-buffer depths of the model under the two poses, depth_obs (S_obs,H,W)
 *   fp32 observed depth, sample b reads depth_obs[src_index[b]] (device int32, B entries), K (B,3,3), diameter (B) device fp32
 *   (> 0: distances are divided by it; <= 0: left as they are), delta and taus[NT] HOST values (1 <= NT <= 16; copied into the
 *   launch arguments, nothing is read from `taus` after the call returns).
 *   A model depth d is EMPTY where !(d > 0) (0, -1, NaN); an observed depth is MISSING where !(d > 0) or it is not finite.
 *   dist = d * sqrt(((u - cx)/fx)^2 + ((v - cy)/fy)^2 + 1) at integer pixel indices u in [0,W), v in [0,H), no half-pixel offset.
 *     vis(m)  = !empty(m) && (missing(obs) || dist_m - dist_obs <= delta)
 *     vis_gt  = vis(gt);   vis_est = vis(est) || (vis_gt && !empty(est));   inter = vis_gt && vis_est;   union = vis_gt || vis_est
 *     e = |dist_gt - dist_est| on inter pixels ( / diameter when normalising);   n_tau = #{inter: e >= tau}
 *     err_tau = (n_tau + #union - #inter) / #union,   1.0 when #union == 0
 *   counts (B, 2+NT) int64 = [#union, #inter, n_tau...], err (B,NT) fp64.  THE CALLER checks the index range on the host
 *   (rnnpose_amd.ops.bop_vsd does); a sample whose index is outside [0,S_obs) reads nothing: zero counts, NaN errors, and the call
 *   still returns 0.  workspace: one int32 record of 2+NT counters per workgroup of 2048 pixels.  Two launches, no atomics:
 *   results are bit-identical from run to run and independent of B.
 * Both: a null pointer, a bad size, NT > 16, S < 1 or a short workspace return 1 and launch nothing; no allocation, no
 *   synchronisation. */
size_t rnnpose_bop_sym_dist_workspace_bytes(int B, int S);
int rnnpose_bop_sym_dist_f64(const float* model, int P, const float* sym, int S, const float* pose_est, const float* pose_gt,
                             const float* K, int B, void* workspace, size_t workspace_bytes, double* out, rnnpose_stream_t stream);
size_t rnnpose_bop_vsd_workspace_bytes(int B, int H, int W, int NT);
int rnnpose_bop_vsd_f64(const float* depth_est, const float* depth_gt, const float* depth_obs, int S_obs, const int* src_index,
                        const float* K, const float* diameter, int B, int H, int W, double delta, const double* taus, int NT,
                        void* workspace, size_t workspace_bytes, long long* counts, double* err, rnnpose_stream_t stream);

/* ---- f4 ("next"): zoom-crop of every outer iteration on device ------- model/PoseRefiner.py:145-218,286-291
 * mask_bbox: bbox (B,4) int32 = [xmin, ymin, xmax, ymax] of depth (B,1,H,W) > 0 ([INT_MAX,INT_MAX,-1,-1] if empty).
 * zoom_crop_params: get_affine_transformation + gen_zoom_crop_grids without the host round trip: K (B,3,3), T (B,4,4)
 *   -> theta (B,2,3) (the F.affine_grid matrices) and K_crop (B,3,3) = inverse(window transform) @ K.
 * zoom_crop: out (B,C,crop_h,crop_w) = F.grid_sample(in (B,C,H,W), F.affine_grid(theta)) (bilinear, zero padding,
 *   align_corners=False); grid_out (B,crop_h,crop_w,2) optionally receives the sampling grid; out may be NULL.  */
/* pointcloud_depth: DiffRender.render_pointcloud (geometry/diff_render_optim.py:369-401) for a batch: image b splats
 *   the vertices verts[vert_offsets[b] .. vert_offsets[b+1]) (device int array of B+1 entries; max_verts >= the largest
 *   count) with pose T (B,4,4) and intrinsics K (B,3,3): out (B,1,H,W) = 0 where nothing lands, else the depth of the
 *   HIGHEST-index vertex on that pixel (the reference leaves the winner of a collision unspecified); pixels are round-half-even and
 *   clamped into the image like the reference's.  workspace: B*H*W ints.  This is the foreground source of the zoom crop. */
size_t rnnpose_pointcloud_depth_workspace_bytes(int B, int H, int W);
int rnnpose_pointcloud_depth_f32(const float* verts, const int* vert_offsets, int max_verts, const float* T, const float* K, int B,
                                 int H, int W, void* workspace, size_t workspace_bytes, float* out, rnnpose_stream_t stream);
int rnnpose_mask_bbox_f32(const float* depth, int B, int H, int W, int* bbox, rnnpose_stream_t stream);
int rnnpose_zoom_crop_params_f32(const int* bbox, const float* K, const float* T, int B, int H, int W, int crop_h, int crop_w,
                                 float margin_ratio, float* theta, float* K_crop, rnnpose_stream_t stream);
int rnnpose_zoom_crop_f32(const float* in, const float* theta, int B, int C, int H, int W, int crop_h, int crop_w, float* out,
                          float* grid_out, rnnpose_stream_t stream);
/* zoom_crop_indexed: the same crop from SHARED sources (several objects of one camera frame): in (S,C,H,W), src_index (B) device
 *   int32 with 0 <= src_index[b] < S; out[b] = grid_sample(in[src_index[b]], affine_grid(theta[b])), the arithmetic of
 *   rnnpose_zoom_crop_f32 operation for operation (src_index = 0..B-1 gives its output bit for bit).  THE CALLER checks the index
 *   range on the host before the launch (the entries are device memory; rnnpose_amd.ops.zoom_crop does); a crop whose index is
 *   outside [0,S) reads nothing: its out is zeros (its grid_out is not written) and the call still returns 0. */
int rnnpose_zoom_crop_indexed_f32(const float* in, const int* src_index, const float* theta, int S, int B, int C, int H, int W,
                                  int crop_h, int crop_w, float* out, float* grid_out, rnnpose_stream_t stream);

/* ---- f4 (second half): triangle-mesh rasteriser of the render hand-off ------------------------------------------------
 *      geometry/diff_render_optim.py:283-367 (DiffRender.forward / render_depth on PyTorch3D's MeshRasterizer,
 *      faces_per_pixel = 1, blur 0) and model/PoseRefiner.py:118-143 (render).  PARITY UNPINNED (PyTorch3D absent).
 * Geometry of a batch: verts (V,3) = the vertices of all loaded models back to back; faces (F,3) int32 = LOCAL vertex
 * indices, models back to back; image b uses vertices from vert_off[b], faces [face_off[b], face_off[b] + face_cnt[b])
 * (device int32 arrays of B entries); T (B,4,4) object->camera, K (B,3,3).  A pixel (x, y) samples the ray through
 * (x + pixel_center, y + pixel_center) (PyTorch3D: 0.5); the nearest face by interpolated camera z wins, equal depths go
 * to the lower face index; faces with a vertex at z <= near are dropped whole (not clipped), and so are faces whose doubled
 * screen area is <= 1e-8 px^2 or not finite (zero-area faces, a NaN / Inf pose).  Coverage is INCLUSIVE: a pixel centre on an
 * edge or a vertex belongs to every face that touches it (no holes along shared edges; the nearest / lowest-index one wins).
 * A face of any screen extent is walked over its bounding box clamped to the image.
 * rnnpose_raster_mesh_f32: pass 1, fills the z-buffer `workspace` (rnnpose_raster_workspace_bytes).
 * rnnpose_raster_resolve_f32: pass 2 from the same workspace and geometry arguments:
 *   out_zbuf   (B,1,H,W)  interpolated depth, `empty_depth` where no face covers the pixel (the reference uses -1);
 *   out_vdepth (B,1,H,W)  camera z of the vertex with the largest barycentric weight, 0 where empty (`render_depth`);
 *   out_attr   (B, 3*with_color + C, H, W): [shaded vertex colour |] attr interpolated with the (perspective-correct if
 *              requested) barycentrics, 0 where empty.  attr = per-vertex rows of C floats, image b's rows start at element
 *              attr_off[b] (device int64 array); colors (V,3) per-vertex albedo aligned with verts (NULL = white);
 *              shade != 0: (0.5 + 0.3 |n.l|) * albedo + 0.2 with the flat face normal and a point light at (1,1,-1) in
 *              object space (PyTorch3D's default Phong terms at shininess 0).  Any output pointer may be NULL. */
size_t rnnpose_raster_workspace_bytes(int B, int H, int W);
int rnnpose_raster_mesh_f32(const float* verts, const int* faces, const int* vert_off, const int* face_off,
                            const int* face_cnt, int max_faces, const float* T, const float* K, int B, int H, int W,
                            float near, float pixel_center, int perspective_correct, void* workspace,
                            size_t workspace_bytes, rnnpose_stream_t stream);
int rnnpose_raster_resolve_f32(const float* verts, const int* faces, const int* vert_off, const int* face_off, const float* T,
                               const float* K, int B, int H, int W, float near, float pixel_center, int perspective_correct,
                               const void* workspace, const float* attr, const long long* attr_off, int C,
                               const float* colors, int with_color, int shade, float empty_depth, float* out_attr,
                               float* out_zbuf, float* out_vdepth, rnnpose_stream_t stream);
/* rnnpose_raster_resolve_tex_f32: pass 2 of a textured, per-pixel shaded render (DiffRender.render_mesh: TexturesUV on
 *   SoftPhongShader, faces_per_pixel = 1).  Workspace, geometry, attr and the three outputs as rnnpose_raster_resolve_f32 with
 *   with_color = 1 (out_attr has 3 + C channels): the two entries run one kernel body and differ in the colour alone, so depth
 *   and attribute channels equal those of rnnpose_raster_resolve_f32 bit for bit.  The albedo of a pixel of image b:
 *     tex_hw[b] = (th, tw) > 0: the texture at uv = sum w_i uv_i (same barycentrics as the attributes), sampled as
 *       grid_sample(flip(map, H), uv * 2 - 1, bilinear, align_corners = True, padding_mode = border) -- uvs (U,2) of all meshes
 *       back to back, image b's start at row uv_off[b]; face_uvs (F,3) int32 = LOCAL uv indices, row for row with faces; tex =
 *       RGBA fp32 texels (16-byte aligned), image b's map starts at texel tex_off[b] (int64) with its th rows stored already
 *       flipped (row 0 = the image's bottom row);
 *     tex_hw[b] = (0,0) or tex NULL: the interpolated vertex colours, white if colors is NULL.
 *   shade 0: the albedo; 1: the flat two-sided terms of rnnpose_raster_resolve_f32; 2: PyTorch3D phong_shading at its
 *   defaults with shininess 0 and a point light at (1,1,-1) in object space: (0.5 + 0.3 relu(n.l)) * albedo + 0.2, n = the
 *   interpolated vnormals (V,3, aligned with verts) normalised with eps 1e-6, l = normalize((1,1,-1) - p, eps 1e-6). */
int rnnpose_raster_resolve_tex_f32(const float* verts, const int* faces, const int* vert_off, const int* face_off, const float* T,
                                   const float* K, int B, int H, int W, float near, float pixel_center, int perspective_correct,
                                   const void* workspace, const float* attr, const long long* attr_off, int C,
                                   const float* colors, const float* uvs, const int* face_uvs, const int* uv_off, const float* tex,
                                   const long long* tex_off, const int* tex_hw, const float* vnormals, int shade,
                                   float empty_depth, float* out_attr, float* out_zbuf, float* out_vdepth,
                                   rnnpose_stream_t stream);
/* rnnpose_raster_occlusion_f32: which pixels of every object's own view are hidden by ANOTHER object of the same batch.
 *   Geometry, T, K, near, pixel_center as rnnpose_raster_mesh_f32; K[b] is the (crop) window of object b's view.
 *   pair_target / pair_occluder (P) device int32, P <= 65535: pair (b, j) rasterises object j under ITS pose T[j] into the
 *     window K[b] of object b, with the coverage and depth arithmetic of rnnpose_raster_mesh_f32 at perspective_correct = 1
 *     (inclusive edges, faces reaching behind `near` and degenerate faces dropped whole).  A pair with an index outside [0,B) or
 *     with b == j writes nothing.  P = 0 is valid: nothing is hidden.
 *   own_keys: the workspace rnnpose_raster_mesh_f32 filled for the same B, H, W, T, K with perspective_correct = 1 (read only);
 *   workspace: a second buffer of rnnpose_raster_workspace_bytes(B, H, W) bytes, distinct from own_keys (overwritten).
 *   With z_own the depth of object b's own nearest face at a pixel and D the smallest depth any of its occluders reaches there,
 *   the pixel is OCCLUDED iff both exist and D + margin < z_own (fp32, one addition, strict): margin is in the meshes' length
 *   unit; an occluder at exactly the own depth hides nothing at margin 0.
 *   visible    (B,1,H,W) fp32   1 where the object covers the pixel and is not occluded there, else 0 (every pixel written);
 *   occluder   (B,1,H,W) int32  batch index of the nearest occluder where occluded (the lower index on equal depths), else -1
 *                               (every pixel written); may be NULL;
 *   depth_inout (B,1,H,W) fp32  occluded pixels are set to 0, every other pixel is left as it is; may be NULL.
 *   Three launches on `stream` (clear, occluder pass [P > 0], apply); no allocation, no synchronisation. */
int rnnpose_raster_occlusion_f32(const float* verts, const int* faces, const int* vert_off, const int* face_off,
                                 const int* face_cnt, int max_faces, const float* T, const float* K, int B, int H, int W,
                                 float near, float pixel_center, const int* pair_target, const int* pair_occluder, int P,
                                 float margin, const void* own_keys, void* workspace, size_t workspace_bytes, float* visible,
                                 int* occluder, float* depth_inout, rnnpose_stream_t stream);

/* ---- Initial poses from 2D-3D descriptor matches: matcher + P3P RANSAC (no counterpart in the reference) ----
 * rnnpose_desc_match_f32: desc3d (total_points, D) fp32, D = 32, the objects' point descriptors back to back (16-byte aligned),
 *   points (total_points, 3); object b owns the rows [pt_off[b], pt_off[b+1]) (device int32, B+1 entries, the layout of the
 *   rasteriser's vert_off; max_points >= the largest count -- an object whose range does not fit gets count = 0);
 *   desc2d (S, D, H, W) fp32 NCHW; src_index (B) device int32; bbox (B,4) device int32 [xmin, ymin, xmax, ymax], inclusive
 *   (rnnpose_mask_bbox_f32), clamped to the image IN the kernel; the pixels of the clamped box with (u - xmin) % step == 0 and
 *   (v - ymin) % step == 0 (xmin, ymin of the CLAMPED box) take part.  An empty box (the mask_bbox sentinel included) or an index
 *   outside [0, S) gives count = 0 -- THE CALLER checks the index range on the host (rnnpose_amd.ops.desc_match does).
 *   s(i, j) = sum_k d3[i][k] d2[j][k]: one fp32 fma chain over k = 0..31 from +0.  Forward: every point's best pixel; backward:
 *   every pixel's best point; equal similarities go to the lowest linear pixel index v W + u / the lowest point index; a NaN
 *   similarity is never a best.  Point i is a correspondence when s_fwd(i) >= min_sim and, with mutual = 1, the best point of its best
 *   pixel is i.  Outputs, compacted per object in ascending point index: X (B,M,3) the point, x (B,M,2) = (u + pixel_center,
 *   v + pixel_center), sim (B,M), point_idx (B,M) the index within the object, count (B) = min(correspondences, M); rows >= count are
 *   NOT written.  workspace: one 64-bit key per point and per box pixel (rnnpose_desc_match_workspace_bytes, 8-byte aligned).
 *   Four launches (clear, forward, backward, select).  The maxima across workgroups meet in 64-bit INTEGER atomicMax on
 *   (orderable similarity bits << 32 | ~index): no floating-point atomics, bit-identical from run to run and independent of B.
 * rnnpose_pnp_ransac_f64: X (B,M,3), x (B,M,2), count (B) as above (count is clamped to [0, M]); K (B,3,3) (fx, fy, cx, cy; no skew);
 *   rnd (B,Hyp,3) device uint32: hypothesis h of object b samples the correspondences rnd[b][h][c] % count[b] -- the kernel has no
 *   generator.  All arithmetic fp64 on values converted from fp32, without fma contraction.  Per hypothesis: repeated indices give no
 *   candidate; else P3P (Grunert's quartic by polynomial arithmetic, Ferrari's roots polished by Newton, the three distances polished by
 *   Newton on the distance equations, pose = rigid alignment of the triangles) -> up to four candidates (finite, the three sample depths
 *   > 0), in the root order csrc/pnp_math.cuh defines; every candidate is scored over all count[b] correspondences: r^2 = |proj(R X + t)
 *   - x|^2, a point with Z <= 1e-6 is an outlier, MSAC cost = sum min(r^2, tau^2), inliers = #{r^2 < tau^2}; the hypothesis keeps its
 *   cheapest candidate (the lower root order on a tie).  cost (B,Hyp) fp64 (+inf without a candidate), inliers (B,Hyp) int32.
 *   Per object: the cheapest hypothesis (the lowest h on a tie) -> best (B) (-1: none); n_polish Gauss-Newton steps on the inliers
 *   re-selected with tau before every step: left increment exp(xi), xi = (translation, rotation), J = J_proj [I | -[X1]x], own 6x6
 *   Cholesky.  T (B,4,4) fp32; inlier_mask (B,M) uint8 (rows < count written), n_inliers (B), final_cost (B) fp64: the inlier set and
 *   the MSAC cost of the FINAL pose; info (B) = 0, or -1 with T[b] NOT written (mask 0, n_inliers 0, final_cost +inf) when
 *   count[b] < min_count, no hypothesis produced a candidate, or a polish system is not positive definite / the pose not finite.
 *   workspace: the candidates of every hypothesis (rnnpose_pnp_ransac_workspace_bytes).  Three launches; fixed-order sums.
 * Both: a null pointer, a bad size, D != 32, step < 1, mutual not 0/1, tau <= 0, min_count < 4, n_polish outside [0,64] or a short
 *   workspace return 1 and launch nothing; no allocation, no synchronisation. */
size_t rnnpose_desc_match_workspace_bytes(int total_points, int B, int H, int W, int step);
int rnnpose_desc_match_f32(const float* desc3d, const float* points, const int* pt_off, int total_points, int max_points,
                           const float* desc2d, int S, int D, int H, int W, const int* src_index, const int* bbox, int B, int step,
                           float min_sim, int mutual, float pixel_center, int M, void* workspace, size_t workspace_bytes, float* X,
                           float* x, float* sim, int* point_idx, int* count, rnnpose_stream_t stream);
size_t rnnpose_pnp_ransac_workspace_bytes(int B, int Hyp);
int rnnpose_pnp_ransac_f64(const float* X, const float* x, const int* count, int M, const float* K, const unsigned* rnd, int B, int Hyp,
                           double tau, int n_polish, int min_count, void* workspace, size_t workspace_bytes, float* T, double* cost,
                           int* inliers, int* best, unsigned char* inlier_mask, int* n_inliers, double* final_cost, int* info,
                           rnnpose_stream_t stream);

/* ---- The K best DISTINCT RANSAC hypotheses, each polished (no counterpart in the reference) ----
 * rnnpose_pnp_ransac_topk_f64: the inputs, `cost` and `inliers` of rnnpose_pnp_ransac_f64 (same solve and score launches), then:
 *   EXTENT of object b: the axis-aligned box [lo, hi] of the X of its first cnt = clamp(count[b], 0, M) correspondences (fp64 on values
 *   converted from fp32); diag = |hi - lo|, sep = sep_frac diag.  DISTANCE of two poses: d(P, Q) = max over the 8 box corners c of
 *   |P c - Q c|, fp64 without fma contraction.
 *   SELECTION (greedy): slot 0 is the cheapest hypothesis (the lowest h on a tie; exactly `best` of rnnpose_pnp_ransac_f64).  Slot
 *   k >= 1 is the cheapest remaining hypothesis (the lowest h on a tie) with a finite cost, inliers[h] >= min_inliers and d > sep
 *   between its candidate pose and the candidate pose of EVERY slot chosen before (the comparison must be true: a NaN distance is
 *   never distinct).  min_inliers does not apply to slot 0.  It stops at Kt slots or when nothing remains: n_found (B) slots;
 *   hyp (B,Kt) the hypothesis of every slot, -1 for k >= n_found.
 *   POLISH of every slot as rnnpose_pnp_ransac_f64 polishes its one: T (B,Kt,4,4) fp32, inlier_mask (B,Kt,M) uint8 (rows < count
 *   written), n_inliers (B,Kt), final_cost (B,Kt) fp64, info (B,Kt) = 0, or -1 with T[b][k] NOT written (mask 0, n_inliers 0,
 *   final_cost +inf); slots k >= n_found have info -1.
 *   dup_of (B,Kt): the lowest k' < k with info 0 whose POLISHED pose (fp64) is not farther than sep from slot k's (not d > sep), else
 *   -1; -1 for a slot with info != 0.  Nothing is removed.
 *   Slot 0 of every output is bit-identical to rnnpose_pnp_ransac_f64 on the same inputs, whatever Kt.  Five launches; no atomics,
 *   fixed-order reductions: bit-identical from run to run, and an object alone gives the bits it gives in a batch.
 *   workspace: the candidates, the polished poses, the extents and one flag per hypothesis (rnnpose_pnp_ransac_topk_workspace_bytes,
 *   0 for a bad size; 8-byte aligned).  The argument errors of rnnpose_pnp_ransac_f64, Kt outside [1, 16], a sep_frac that is negative
 *   or not finite, min_inliers < 0 or a short workspace return 1 and launch nothing; no allocation, no synchronisation. */
size_t rnnpose_pnp_ransac_topk_workspace_bytes(int B, int Hyp, int Kt);
int rnnpose_pnp_ransac_topk_f64(const float* X, const float* x, const int* count, int M, const float* K, const unsigned* rnd, int B, int Hyp,
                                double tau, int n_polish, int min_count, int Kt, double sep_frac, int min_inliers, void* workspace,
                                size_t workspace_bytes, float* T, double* cost, int* inliers, int* hyp, unsigned char* inlier_mask,
                                int* n_inliers, double* final_cost, int* info, int* dup_of, int* n_found, rnnpose_stream_t stream);

/* ---- Pose confidence: render-and-compare score of a pose against its frame (no counterpart in the reference) ----
 * rend_depth (B,h,w) fp32 and rend_desc (B,D,h,w) fp32, D = 32: the object's z-buffer and its per-vertex descriptors rendered under
 *   the pose into a WINDOW of the frame, the principal point shifted by the window's integer corner; window (B,2) device int32
 *   (x0, y0), any sign; desc2d (S,D,H,W) fp32 the frames' descriptor maps; depth_obs (S,H,W) fp32 the observed depth, or NULL;
 *   src_index (B) device int32.  Window pixel (x, y) of pose b IS frame pixel (u, v) = (x0 + x, y0 + y) of frame src_index[b]: nothing
 *   is resampled.  All arithmetic fp64 on values converted from fp32, without fma contraction.
 *   Per window pixel: RENDERED iff z = rend_depth is finite and > 0.  A rendered pixel with (u, v) outside [0,W) x [0,H) is OUTSIDE.
 *   An inside pixel, with d = depth_obs[s,v,u] valid iff finite and > 0 and dd = d - z: dd < -depth_tol OCCLUDED; |dd| <= depth_tol
 *   CONSISTENT; dd > depth_tol VIOLATED; d invalid or depth_obs NULL: HOLE.  Inside pixels that are not occluded are compared: a (the D
 *   channels of rend_desc) against g (those of desc2d); a non-finite channel on either side makes the pixel BAD, else
 *   cos = (sum_k a_k g_k) / (max(|a|, 1e-12) max(|g|, 1e-12)) -- a zero vector gives 0 and counts.
 *   stats (B,10) fp64 = [n_rend, n_out, n_occ, n_cons, n_viol, n_hole, n_desc, sum cos, sum |dd| over consistent, n_bad], with
 *   n_rend = n_out + n_occ + n_cons + n_viol + n_hole and n_desc + n_bad = n_cons + n_viol + n_hole.
 *   score (B) fp64 = max(sum cos / n_desc, 0) * n_cons / (n_cons + n_viol)   (the second factor 1 when its denominator is 0; score 0
 *   when n_desc = 0).  A src_index outside [0, S) gives a zero row and score 0 -- THE CALLER checks the range on the host
 *   (rnnpose_amd.ops.pose_score does).
 *   workspace: one row of 10 doubles per 256-pixel chunk of every window (rnnpose_pose_score_workspace_bytes, 8-byte aligned).
 *   Two launches: partial rows (a lane per window pixel, flat grid over B x chunks, fixed xor butterfly), then their sum per pose in
 *   ascending chunk order.  No atomics: bit-identical from run to run, and a pose alone gives the bits it gives in a batch.
 *   A null pointer other than depth_obs, D != 32, B / S / h / w / H / W < 1, a depth_tol that is negative or not finite or a short
 *   workspace return 1 and launch nothing; no allocation, no synchronisation. */
size_t rnnpose_pose_score_workspace_bytes(int B, int h, int w);
int rnnpose_pose_score_f64(const float* rend_depth, const float* rend_desc, const int* window, const float* desc2d, const float* depth_obs,
                           const int* src_index, int B, int S, int D, int h, int w, int H, int W, double depth_tol, void* workspace,
                           size_t workspace_bytes, double* stats, double* score, rnnpose_stream_t stream);

/* ---- Object onboarding: exact diameter and farthest-point sampling of a point set ----
 * Both: points (total_points,3) fp32, object b owns the rows [pt_off[b], pt_off[b+1]) (device int32, B+1 entries, the layout of the
 *   rasteriser and the matcher); an object whose range does not fit the array counts as empty.  All arithmetic fp64 on values
 *   converted from fp32, without fma contraction: dx = (double)xi - (double)xj, d2 = (dx dx + dy dy) + dz dz.  A point with a
 *   non-finite coordinate takes part in nothing.  No atomics: bit-identical from run to run and independent of B.  total_points = 0
 *   is valid (every object empty).  A null pointer, B < 1, total_points < 0, n < 1 or a short workspace return 1 and launch nothing; no
 *   allocation, no synchronisation.
 * rnnpose_point_diameter_f64: per object the exact largest pairwise squared distance d2 (B) fp64, diameter (B) = sqrt(d2), the pair
 *   that attains it, pair (B,2) int32 indices within the object with i < j (ties: the lowest i, then the lowest j), and bounds (B,2,3)
 *   fp32 the axis-aligned minimum and maximum.  Fewer than two finite points: d2 = diameter = 0, pair = (-1,-1); no finite point:
 *   bounds = (+inf, -inf).  O(P^2): a tiled upper-triangular sweep (256-point tiles, the j tile in LDS), one partial per tile pair in
 *   the workspace (rnnpose_point_diameter_workspace_bytes: B * T (T + 1) / 2 * 16 bytes with T = ceil(total_points / 256), 8-byte
 *   aligned; 0 for a bad size), then one workgroup per object reduces them.  At most 1 048 576 points and 65 535 objects a call.
 * rnnpose_fps_f64: farthest-point sampling, n picks per object; start (B) device int32.  start[b] >= 0: the first pick is that index
 *   (an index outside the object, below -1, or of a point that is not finite makes the object empty).  start[b] == -1: the running
 *   distance starts as every point's squared distance to the origin, so the first pick is the point farthest from the origin.  Every
 *   later pick is the point with the largest running minimum squared distance to the picks so far, the lowest index on a tie; a
 *   picked point's running distance becomes -1, so duplicated points come last, lowest index first, and none twice.
 *   idx (B,n) int32 in pick order; dist2 (B,n) fp64 the running squared distance of each pick when it was picked (+inf for a first
 *   pick given by start); once an object has nothing left to pick the remaining rows hold idx = -1, dist2 = -1.
 *   One workgroup of 1024 threads per object, one barrier per pick; objects of up to 8192 points stay in registers, larger ones keep
 *   their running distances in the workspace (rnnpose_fps_workspace_bytes: one double per point, 8-byte aligned). */
size_t rnnpose_point_diameter_workspace_bytes(int total_points, int B);
int rnnpose_point_diameter_f64(const float* points, const int* pt_off, int total_points, int B, void* workspace, size_t workspace_bytes,
                               double* d2, double* diameter, int* pair, float* bounds, rnnpose_stream_t stream);
size_t rnnpose_fps_workspace_bytes(int total_points, int B);
int rnnpose_fps_f64(const float* points, const int* pt_off, int total_points, int B, int n, const int* start, void* workspace,
                    size_t workspace_bytes, int* idx, double* dist2, rnnpose_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RNNPOSE_HIP_H */
