// f4 (second half): triangle-mesh rasteriser for the render hand-off of every outer refinement iteration -- depth and
// per-vertex attribute maps of the object under the current pose.  Replaces what the reference gets from PyTorch3D through
// geometry/diff_render_optim.py:283-367 (`DiffRender.forward`: MeshRasterizer with faces_per_pixel = 1, blur 0,
// perspective-correct barycentrics + interpolate_face_attributes; `render_depth`: nearest-vertex depth).
// PARITY UNPINNED: PyTorch3D is not in this image and the reference holds no fixture for it; semantics follow PyTorch3D's
// documented ones (pixel centres at +0.5, nearest face by interpolated camera z, ties -> lower face index) and are checked
// against oracle/raster_oracle.py and through properties (tests/test_raster.py), and against an fp64 ray caster and closed-form
// images at the edge cases (tests/test_gpu_raster_edges.py: inclusive edges, ties, clipping, the near plane, attribute paths).
//
// Two passes, no sorting, no per-pixel face lists:
//   1. raster_faces_kernel: one thread per (image, face).  The face is projected, its screen bounding box walked, and for
//      every covered pixel centre a 64-bit key (depth bits << 32 | face index) is atomicMin-ed into the z-buffer: depth
//      is positive, so the float's bit pattern orders like the float, and equal depths resolve to the lower face index.
//      LINEMOD-size meshes project to triangles of a few pixels: the box walk is short and the atomics rarely collide.
//   2. raster_resolve_kernel<TEX>: one thread per pixel reads its key, recomputes the barycentrics of the winning face with the
//      SAME arithmetic as pass 1 and writes depth, nearest-vertex depth and the interpolated vertex attributes
//      ([shaded colour |] C channels, NCHW planes: consecutive lanes are consecutive x -> coalesced plane writes; every
//      lane walks its three attribute rows 16 bytes at a time).  ONE body for both renders; the colour of a hit pixel is all that
//      differs: plain_color (TEX = false), the vertex colours under the flat two-sided terms, or tex_color (TEX = true: render_tex
//      with a UV texture or Phong shading), the colour taken from the mesh's texture map at the interpolated UV (one bilinear
//      grid_sample, four 16-byte RGBA taps) and shaded per pixel with interpolated vertex normals (PyTorch3D's SoftPhongShader
//      with faces_per_pixel = 1).
// Occlusion between the objects of one frame (rnnpose_raster_occlusion_f32; no counterpart in the reference, which refines one class
// per batch): raster_occluder_kernel z-buffers, for every (target, occluder) pair, the occluder's faces into the target's window through
// walk_face, the face walk of pass 1, and raster_occlusion_apply_kernel compares that buffer with the target's own keys per pixel.
#include "common.hpp"

namespace {

struct Cam {
  float r[12];
  float fx, fy, cx, cy;
};

__device__ __forceinline__ Cam load_cam(const float* __restrict__ T, const float* __restrict__ K, int b) {
  Cam c;
#pragma unroll
  for (int i = 0; i < 12; ++i) c.r[i] = T[16 * b + i];
  const float* k = K + 9 * b;
  c.fx = k[0]; c.fy = k[4]; c.cx = k[2]; c.cy = k[5];
  return c;
}

struct Tri {
  float x[3], y[3], z[3];   // screen x, y (pixels) and camera z of the three vertices
  float area;               // signed doubled area in screen space
  bool ok;
};

// shared by both passes: identical arithmetic -> identical coverage decisions
__device__ __forceinline__ Tri project_face(const float* __restrict__ verts, const int* __restrict__ faces, long long f,
                                            int vbase, const Cam& c, float near) {
#pragma clang fp contract(off)
  Tri t;
  t.ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float* v = verts + 3LL * (vbase + faces[3 * f + i]);
    const float X = c.r[0] * v[0] + c.r[1] * v[1] + c.r[2] * v[2] + c.r[3];
    const float Y = c.r[4] * v[0] + c.r[5] * v[1] + c.r[6] * v[2] + c.r[7];
    const float Z = c.r[8] * v[0] + c.r[9] * v[1] + c.r[10] * v[2] + c.r[11];
    t.z[i] = Z;
    t.ok = t.ok && (Z > near);                     // faces that reach behind the near plane are dropped whole
    const float iz = 1.0f / (Z > near ? Z : near);
    t.x[i] = c.fx * X * iz + c.cx;
    t.y[i] = c.fy * Y * iz + c.cy;
  }
  t.area = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.x[2] - t.x[0]) * (t.y[1] - t.y[0]);
  t.ok = t.ok && (fabsf(t.area) > 1e-8f) && (t.area == t.area);
  return t;
}

// barycentric weights of pixel centre (px, py); inside <=> all three >= 0 (either winding).  -> depth of the face there
__device__ __forceinline__ bool bary_at(const Tri& t, float px, float py, int perspective, float& w0, float& w1, float& w2,
                                        float& z) {
#pragma clang fp contract(off)
  const float e0 = (t.x[2] - t.x[1]) * (py - t.y[1]) - (t.y[2] - t.y[1]) * (px - t.x[1]);
  const float e1 = (t.x[0] - t.x[2]) * (py - t.y[2]) - (t.y[0] - t.y[2]) * (px - t.x[2]);
  const float e2 = (t.x[1] - t.x[0]) * (py - t.y[0]) - (t.y[1] - t.y[0]) * (px - t.x[0]);
  const float ia = 1.0f / t.area;
  w0 = e0 * ia; w1 = e1 * ia; w2 = e2 * ia;
  if (!(w0 >= 0.f && w1 >= 0.f && w2 >= 0.f)) return false;
  if (perspective) {                               // PyTorch3D BarycentricPerspectiveCorrection: b_i = (w_i / z_i) / sum
    const float q0 = w0 / t.z[0], q1 = w1 / t.z[1], q2 = w2 / t.z[2];
    const float s = (q0 + q1) + q2;
    w0 = q0 / s; w1 = q1 / s; w2 = q2 / s;
  }
  z = (w0 * t.z[0] + w1 * t.z[1]) + w2 * t.z[2];
  return z > 0.f;
}

constexpr unsigned long long kEmpty = 0xffffffffffffffffull;

__global__ __launch_bounds__(256) void raster_clear_kernel(unsigned long long* __restrict__ zb, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) zb[i] = kEmpty;
}

// THE face walk of both z-buffer passes: the on-screen test, the bounding box, every pixel centre in it through bary_at, and the key
// (depth bits << 32 | low) atomicMin-ed into `img`.  low: the face index (raster_faces_kernel) or the occluder's batch index.
__device__ __forceinline__ void walk_face(const Tri& t, int H, int W, float pix_center, int perspective,
                                          unsigned long long* __restrict__ img, unsigned low) {
  const float xmin = fminf(fminf(t.x[0], t.x[1]), t.x[2]), xmax = fmaxf(fmaxf(t.x[0], t.x[1]), t.x[2]);
  const float ymin = fminf(fminf(t.y[0], t.y[1]), t.y[2]), ymax = fmaxf(fmaxf(t.y[0], t.y[1]), t.y[2]);
  if (!(xmax >= 0.f && ymax >= 0.f && xmin < static_cast<float>(W) && ymin < static_cast<float>(H))) return;
  // clamped to the image IN FLOAT: a face just beyond `near` projects past +-2^31 pixels, where float -> int is undefined
  const int x0 = static_cast<int>(fmaxf(floorf(xmin - pix_center), 0.f));
  const int x1 = static_cast<int>(fminf(ceilf(xmax - pix_center), static_cast<float>(W - 1)));
  const int y0 = static_cast<int>(fmaxf(floorf(ymin - pix_center), 0.f));
  const int y1 = static_cast<int>(fminf(ceilf(ymax - pix_center), static_cast<float>(H - 1)));
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) {
      float w0, w1, w2, z;
      if (bary_at(t, static_cast<float>(x) + pix_center, static_cast<float>(y) + pix_center, perspective, w0, w1, w2, z)) {
        const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(z)) << 32) | low;
        atomicMin(img + static_cast<long long>(y) * W + x, key);
      }
    }
}

__global__ __launch_bounds__(128) void raster_faces_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                           const int* __restrict__ vert_off, const int* __restrict__ face_off,
                                                           const int* __restrict__ face_cnt, const float* __restrict__ T,
                                                           const float* __restrict__ K, int H, int W, float near,
                                                           float pix_center, int perspective,
                                                           unsigned long long* __restrict__ zb) {
  const int b = blockIdx.y;
  const int fl = blockIdx.x * 128 + threadIdx.x;
  if (fl >= face_cnt[b]) return;
  const Cam c = load_cam(T, K, b);
  const long long f = static_cast<long long>(face_off[b]) + fl;
  const Tri t = project_face(verts, faces, f, vert_off[b], c, near);
  if (!t.ok) return;
  walk_face(t, H, W, pix_center, perspective, zb + static_cast<long long>(b) * H * W, static_cast<unsigned>(fl));
}

// The colour of a hit pixel, plain resolve: the vertex colours (white without them) under the flat two-sided terms.  Default fp
// contraction; tex_color's flat form is op by op, so the two may differ in the last bit and stay apart.
__device__ __forceinline__ void plain_color(const float* __restrict__ verts, const float* __restrict__ colors, int vb, int v0, int v1,
                                            int v2, float w0, float w1, float w2, int shade, float* col) {
  float lit = 1.f, spec = 0.f;
  const float* p0 = verts + 3LL * (vb + v0);
  const float* p1 = verts + 3LL * (vb + v1);
  const float* p2 = verts + 3LL * (vb + v2);
  if (shade) {        // Phong terms of PyTorch3D's defaults with shininess 0, flat normal, point light at (1, 1, -1)
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float nn = rsqrtf(fmaxf(nx * nx + ny * ny + nz * nz, 1e-30f));
    nx *= nn; ny *= nn; nz *= nn;
    const float qx = w0 * p0[0] + w1 * p1[0] + w2 * p2[0], qy = w0 * p0[1] + w1 * p1[1] + w2 * p2[1],
                qz = w0 * p0[2] + w1 * p1[2] + w2 * p2[2];
    float lx = 1.f - qx, ly = 1.f - qy, lz = -1.f - qz;
    const float ln = rsqrtf(fmaxf(lx * lx + ly * ly + lz * lz, 1e-30f));
    const float cosv = fabsf((nx * lx + ny * ly + nz * lz) * ln);      // two-sided: the winding of scanned meshes varies
    lit = 0.5f + 0.3f * cosv;
    spec = 0.2f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float a = 1.f;
    if (colors) a = w0 * colors[3LL * (vb + v0) + k] + w1 * colors[3LL * (vb + v1) + k] + w2 * colors[3LL * (vb + v2) + k];
    col[k] = a * lit + spec;
  }
}

// grid_sample(map, g, mode="bilinear", align_corners=True, padding_mode="border") at one point of the pre-flipped RGBA map
// `tex` (th rows of tw texels): the arithmetic of PyTorch's grid sampler step by step -- unnormalise ((g+1)/2)*(size-1), clip
// to [0, size-1], four taps weighted from the floor corner.  A tap at x = tw or y = th has weight 0 and is not read.
__device__ __forceinline__ float4 sample_bilinear_border(const float4* __restrict__ tex, int th, int tw, float gx, float gy) {
#pragma clang fp contract(off)
  float ix = ((gx + 1.f) / 2.f) * static_cast<float>(tw - 1);
  float iy = ((gy + 1.f) / 2.f) * static_cast<float>(th - 1);
  ix = fminf(static_cast<float>(tw - 1), fmaxf(ix, 0.f));     // (fmaxf(NaN, 0) = 0: a NaN coordinate samples the corner)
  iy = fminf(static_cast<float>(th - 1), fmaxf(iy, 0.f));
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = static_cast<int>(fx), y0 = static_cast<int>(fy);
  const float x1f = fx + 1.f, y1f = fy + 1.f;
  const float wnw = (x1f - ix) * (y1f - iy), wne = (ix - fx) * (y1f - iy);
  const float wsw = (x1f - ix) * (iy - fy), wse = (ix - fx) * (iy - fy);
  const bool xin = x0 + 1 < tw, yin = y0 + 1 < th;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* r0 = tex + static_cast<long long>(y0) * tw;
  const float4 nw = r0[x0];
  const float4 ne = xin ? r0[x0 + 1] : z4;
  const float4 sw = yin ? r0[tw + x0] : z4;
  const float4 se = (xin && yin) ? r0[tw + x0 + 1] : z4;
  return make_float4(((nw.x * wnw + ne.x * wne) + sw.x * wsw) + se.x * wse, ((nw.y * wnw + ne.y * wne) + sw.y * wsw) + se.y * wse,
                     ((nw.z * wnw + ne.z * wne) + sw.z * wsw) + se.z * wse, 0.f);
}

// what the textured resolve reads on top of the plain one (rnnpose_raster_resolve_tex_f32); the plain instantiation never touches it
struct TexArgs {
  const float* uvs;
  const int* face_uvs;
  const int* uv_off;
  const float4* tex;
  const long long* tex_off;
  const int* tex_hw;
  const float* vnormals;
};

// The colour of a hit pixel, textured resolve: the albedo is the mesh's texture sampled at the interpolated UV
// (TexturesUV.sample_textures), or its vertex colours (white without them) when the image's mesh has no texture, shaded by `shade`:
// 0 none, 1 flat two-sided terms, 2 PyTorch3D's phong_shading with interpolated vertex normals.
__device__ __forceinline__ void tex_color(const float* __restrict__ verts, const float* __restrict__ colors, const TexArgs& tx, int b,
                                          long long f, int vb, int v0, int v1, int v2, float w0, float w1, float w2, int shade,
                                          float* col) {
#pragma clang fp contract(off)                     // (no contraction here: the colour is PyTorch3D's op-by-op fp32 arithmetic)
  const int th = tx.tex ? tx.tex_hw[2 * b] : 0, tw = tx.tex ? tx.tex_hw[2 * b + 1] : 0;
  float alb[3] = {1.f, 1.f, 1.f};
  if (th > 0 && tw > 0) {                          // TexturesUV: uv = sum w_i uv_i, grid = uv * 2 - 1 on the flipped map
    const float* uvb = tx.uvs + 2LL * tx.uv_off[b];
    const float* t0 = uvb + 2LL * tx.face_uvs[3 * f + 0];
    const float* t1 = uvb + 2LL * tx.face_uvs[3 * f + 1];
    const float* t2 = uvb + 2LL * tx.face_uvs[3 * f + 2];
    const float u = (w0 * t0[0] + w1 * t1[0]) + w2 * t2[0];
    const float v = (w0 * t0[1] + w1 * t1[1]) + w2 * t2[1];
    const float4 s = sample_bilinear_border(tx.tex + tx.tex_off[b], th, tw, u * 2.f - 1.f, v * 2.f - 1.f);
    alb[0] = s.x; alb[1] = s.y; alb[2] = s.z;
  } else if (colors) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      alb[k] = (w0 * colors[3LL * (vb + v0) + k] + w1 * colors[3LL * (vb + v1) + k]) + w2 * colors[3LL * (vb + v2) + k];
  }
  float lit = 1.f, spec = 0.f;
  if (shade) {
    const float* p0 = verts + 3LL * (vb + v0);
    const float* p1 = verts + 3LL * (vb + v1);
    const float* p2 = verts + 3LL * (vb + v2);
    float nx, ny, nz;
    if (shade == 2) {                              // phong_shading: normalize(sum w_i n_i, eps 1e-6) of verts_normals_packed
      const float* n0 = tx.vnormals + 3LL * (vb + v0);
      const float* n1 = tx.vnormals + 3LL * (vb + v1);
      const float* n2 = tx.vnormals + 3LL * (vb + v2);
      nx = (w0 * n0[0] + w1 * n1[0]) + w2 * n2[0];
      ny = (w0 * n0[1] + w1 * n1[1]) + w2 * n2[1];
      nz = (w0 * n0[2] + w1 * n1[2]) + w2 * n2[2];
      const float nn = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-6f);
      nx = nx / nn; ny = ny / nn; nz = nz / nn;
    } else {                                       // plain_color's flat face normal, uncontracted
      const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
      const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
      nx = ay * bz - az * by; ny = az * bx - ax * bz; nz = ax * by - ay * bx;
      const float nn = rsqrtf(fmaxf(nx * nx + ny * ny + nz * nz, 1e-30f));
      nx *= nn; ny *= nn; nz *= nn;
    }
    const float qx = (w0 * p0[0] + w1 * p1[0]) + w2 * p2[0], qy = (w0 * p0[1] + w1 * p1[1]) + w2 * p2[1],
                qz = (w0 * p0[2] + w1 * p1[2]) + w2 * p2[2];
    float lx = 1.f - qx, ly = 1.f - qy, lz = -1.f - qz;   // point light at (1, 1, -1), object space
    float cosv;
    if (shade == 2) {                              // diffuse(): relu(n . normalize(l, eps 1e-6)), one-sided
      const float ln = fmaxf(sqrtf((lx * lx + ly * ly) + lz * lz), 1e-6f);
      lx = lx / ln; ly = ly / ln; lz = lz / ln;
      cosv = fmaxf((nx * lx + ny * ly) + nz * lz, 0.f);
    } else {
      const float ln = rsqrtf(fmaxf(lx * lx + ly * ly + lz * lz, 1e-30f));
      cosv = fabsf((nx * lx + ny * ly + nz * lz) * ln);
    }
    lit = 0.5f + 0.3f * cosv;                      // ambient 0.5 + diffuse 0.3 (PointLights defaults, Materials white)
    spec = 0.2f;                                   // specular 0.2 * pow(., shininess = 0) = 0.2 everywhere
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) col[k] = alb[k] * lit + spec;
}

// Pass 2, both renders.  TEX = false: n_col in {0, 3} colour planes from plain_color, `tx` is not read.  TEX = true: always three,
// from tex_color.  Everything around the colour -- and the attribute channels, which sit in no contract(off) scope -- is one text, so
// depth and attributes of the two renders are equal bit for bit.
template <bool TEX>
__global__ __launch_bounds__(256) void raster_resolve_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                             const int* __restrict__ vert_off, const int* __restrict__ face_off,
                                                             const float* __restrict__ T, const float* __restrict__ K, int H,
                                                             int W, float near, float pix_center, int perspective,
                                                             const unsigned long long* __restrict__ zb,
                                                             const float* __restrict__ attr, const long long* __restrict__ attr_off,
                                                             int C, const float* __restrict__ colors, int n_col, TexArgs tx,
                                                             int shade, float empty_depth, float* __restrict__ out_attr,
                                                             float* __restrict__ out_zbuf, float* __restrict__ out_vdepth) {
  const int b = blockIdx.y;
  const long long P = static_cast<long long>(H) * W;
  const long long pix = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (pix >= P) return;
  const int x = static_cast<int>(pix % W), y = static_cast<int>(pix / W);
  const unsigned long long key = zb[b * P + pix];
  const bool hit = key != kEmpty;
  float w0 = 0.f, w1 = 0.f, w2 = 0.f, z = 0.f;
  int v0 = 0, v1 = 0, v2 = 0;
  long long f = 0;
  Tri t{};
  const int vb = vert_off[b];
  if (hit) {
    const Cam c = load_cam(T, K, b);
    f = static_cast<long long>(face_off[b]) + static_cast<unsigned>(key & 0xffffffffull);
    t = project_face(verts, faces, f, vb, c, near);
    bary_at(t, static_cast<float>(x) + pix_center, static_cast<float>(y) + pix_center, perspective, w0, w1, w2, z);
    v0 = faces[3 * f + 0]; v1 = faces[3 * f + 1]; v2 = faces[3 * f + 2];
  }
  if (out_zbuf) out_zbuf[b * P + pix] = hit ? z : empty_depth;
  if (out_vdepth) {       // render_depth: per-vertex camera z with the barycentrics snapped to the nearest vertex (argmax)
    float vz = 0.f;
    if (hit) vz = (w0 >= w1 && w0 >= w2) ? t.z[0] : (w1 >= w2 ? t.z[1] : t.z[2]);
    out_vdepth[b * P + pix] = vz;
  }
  if (!out_attr) return;
  if constexpr (TEX) n_col = 3;
  float* o = out_attr + static_cast<long long>(b) * (n_col + C) * P + pix;
  if (n_col) {
    float col[3] = {0.f, 0.f, 0.f};
    if (hit) {
      if constexpr (TEX) tex_color(verts, colors, tx, b, f, vb, v0, v1, v2, w0, w1, w2, shade, col);
      else plain_color(verts, colors, vb, v0, v1, v2, w0, w1, w2, shade, col);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k * P] = col[k];
    o += 3 * P;
  }
  if (!attr || C <= 0) return;
  const float* a0 = attr + attr_off[b] + static_cast<long long>(v0) * C;
  const float* a1 = attr + attr_off[b] + static_cast<long long>(v1) * C;
  const float* a2 = attr + attr_off[b] + static_cast<long long>(v2) * C;
  int c = 0;
  if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(attr) & 15) == 0 && (attr_off[b] & 3) == 0) {
    for (; c < C; c += 4) {
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (hit) {
        const float4 q0 = *reinterpret_cast<const float4*>(a0 + c), q1 = *reinterpret_cast<const float4*>(a1 + c),
                     q2 = *reinterpret_cast<const float4*>(a2 + c);
        r = make_float4(w0 * q0.x + w1 * q1.x + w2 * q2.x, w0 * q0.y + w1 * q1.y + w2 * q2.y,
                        w0 * q0.z + w1 * q1.z + w2 * q2.z, w0 * q0.w + w1 * q1.w + w2 * q2.w);
      }
      o[(c + 0) * P] = r.x; o[(c + 1) * P] = r.y; o[(c + 2) * P] = r.z; o[(c + 3) * P] = r.w;
    }
  }
  for (; c < C; ++c) o[c * P] = hit ? w0 * a0[c] + w1 * a1[c] + w2 * a2[c] : 0.f;
}

// ---- occlusion between the objects of one frame (rnnpose_raster_occlusion_f32) ------------------------------------------------
// Occluder pass: one thread per (pair, face of the occluder).  For pair (b, j) the faces of object j are projected with ITS pose
// T[j] into the crop window of the target, K[b], and z-buffered into image b of a second key buffer by walk_face (perspective-correct);
// the low half of the key is j instead of the face index, so the nearest occluder wins and equal depths go to the lower batch index.
__global__ __launch_bounds__(128) void raster_occluder_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                              const int* __restrict__ vert_off, const int* __restrict__ face_off,
                                                              const int* __restrict__ face_cnt, const float* __restrict__ T,
                                                              const float* __restrict__ K, const int* __restrict__ pair_target,
                                                              const int* __restrict__ pair_occluder, int B, int H, int W, float near,
                                                              float pix_center, unsigned long long* __restrict__ zb) {
  const int p = blockIdx.y;
  const int b = pair_target[p], j = pair_occluder[p];
  if (b < 0 || b >= B || j < 0 || j >= B || b == j) return;      // the second fence (the host refuses such pairs first)
  const int fl = blockIdx.x * 128 + threadIdx.x;
  if (fl >= face_cnt[j]) return;
  Cam c = load_cam(T, K, j);                                     // the occluder's pose ...
  const float* k = K + 9 * b;                                    // ... seen through the target's crop window
  c.fx = k[0]; c.fy = k[4]; c.cx = k[2]; c.cy = k[5];
  const long long f = static_cast<long long>(face_off[j]) + fl;
  const Tri t = project_face(verts, faces, f, vert_off[j], c, near);
  if (!t.ok) return;
  walk_face(t, H, W, pix_center, 1, zb + static_cast<long long>(b) * H * W, static_cast<unsigned>(j));
}

// the depth test, op by op in fp32: an occluder at exactly the own depth (margin 0) hides nothing
__device__ __forceinline__ bool occluder_in_front(float D, float margin, float z_own) {
#pragma clang fp contract(off)
  const float d = D + margin;
  return d < z_own;
}

// Apply pass: one thread per pixel of every image reads the own key and the occluder key and writes all of visible / occluder.
__global__ __launch_bounds__(256) void raster_occlusion_apply_kernel(const unsigned long long* __restrict__ own,
                                                                     const unsigned long long* __restrict__ occ, long long n,
                                                                     float margin, float* __restrict__ visible,
                                                                     int* __restrict__ occluder, float* __restrict__ depth_inout) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long ko = own[i], kj = occ[i];
  const bool hit = ko != kEmpty;
  bool hidden = false;
  if (hit && kj != kEmpty)
    hidden = occluder_in_front(__uint_as_float(static_cast<unsigned>(kj >> 32)), margin, __uint_as_float(static_cast<unsigned>(ko >> 32)));
  visible[i] = (hit && !hidden) ? 1.0f : 0.0f;
  if (occluder) occluder[i] = hidden ? static_cast<int>(static_cast<unsigned>(kj & 0xffffffffull)) : -1;
  if (depth_inout && hidden) depth_inout[i] = 0.0f;
}

// what every mesh entry tests first: the geometry, cameras and key buffer with the entry's own pointers (`ptrs`), then the sizes with
// the entry's own (`sizes`)
int raster_check(const char* fn, const float* verts, const int* faces, const int* vert_off, const int* face_off, const float* T,
                 const float* K, const void* workspace, bool ptrs, int B, int H, int W, bool sizes) {
  RP_REQUIRE(verts && faces && vert_off && face_off && T && K && workspace && ptrs, fn, "null pointer");
  RP_REQUIRE(B > 0 && B < 65536 && H > 0 && W > 0 && sizes, fn, "bad size");
  return 0;
}

// the z-buffer entries (own pass, occluder pass): the last test, then every key of `workspace` set to empty
int raster_clear(const char* fn, void* workspace, size_t workspace_bytes, int B, int H, int W, hipStream_t st) {
  RP_REQUIRE(workspace_bytes >= rnnpose_raster_workspace_bytes(B, H, W), fn, "workspace too small");
  const long long n = static_cast<long long>(B) * H * W;
  hipLaunchKernelGGL(raster_clear_kernel, dim3(rp::cdiv(n, 256)), dim3(256), 0, st, static_cast<unsigned long long*>(workspace), n);
  return 0;
}

// both resolve entries: the checks (those of the textured entry in their places), then raster_resolve_kernel<TEX>
template <bool TEX>
int resolve_launch(const char* fn, const float* verts, const int* faces, const int* vert_off, const int* face_off, const float* T,
                   const float* K, int B, int H, int W, float near, float pixel_center, int perspective_correct, const void* workspace,
                   const float* attr, const long long* attr_off, int C, const float* colors, int n_col, const TexArgs& tx, int shade,
                   float empty_depth, float* out_attr, float* out_zbuf, float* out_vdepth, rnnpose_stream_t stream) {
  if (raster_check(fn, verts, faces, vert_off, face_off, T, K, workspace, true, B, H, W, C >= 0)) return 1;
  if constexpr (TEX) RP_REQUIRE(shade >= 0 && shade <= 2, fn, "shade must be 0 (none), 1 (flat) or 2 (phong)");
  RP_REQUIRE(!(attr && C > 0) || attr_off, fn, "attr needs attr_off");
  if constexpr (TEX) {
    RP_REQUIRE(!tx.tex || (tx.uvs && tx.face_uvs && tx.uv_off && tx.tex_off && tx.tex_hw), fn,
               "a texture needs uvs, face_uvs, uv_off, tex_off, tex_hw");
    RP_REQUIRE(!tx.tex || (reinterpret_cast<uintptr_t>(tx.tex) & 15) == 0, fn, "texels must be 16-byte aligned (RGBA fp32)");
    RP_REQUIRE(shade != 2 || tx.vnormals, fn, "phong shading needs vnormals");
  }
  RP_REQUIRE(out_attr || out_zbuf || out_vdepth, fn, "nothing to write");
  const long long P = static_cast<long long>(H) * W;
  const auto kernel = raster_resolve_kernel<TEX>;
  hipLaunchKernelGGL(kernel, dim3(rp::cdiv(P, 256), B), dim3(256), 0, rp::as_stream(stream), verts, faces, vert_off, face_off, T, K, H,
                     W, near, pixel_center, perspective_correct, static_cast<const unsigned long long*>(workspace), attr, attr_off, C,
                     colors, n_col, tx, shade, empty_depth, out_attr, out_zbuf, out_vdepth);
  return rp::check_launch(fn);
}

}  // namespace

extern "C" {

size_t rnnpose_raster_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return static_cast<size_t>(B) * H * W * sizeof(unsigned long long);
}

int rnnpose_raster_mesh_f32(const float* verts, const int* faces, const int* vert_off, const int* face_off,
                            const int* face_cnt, int max_faces, const float* T, const float* K, int B, int H, int W,
                            float near, float pixel_center, int perspective_correct, void* workspace,
                            size_t workspace_bytes, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_raster_mesh_f32";
  if (raster_check(fn, verts, faces, vert_off, face_off, T, K, workspace, face_cnt != nullptr, B, H, W, max_faces > 0 && near > 0.f)) return 1;
  hipStream_t st = rp::as_stream(stream);
  if (raster_clear(fn, workspace, workspace_bytes, B, H, W, st)) return 1;
  hipLaunchKernelGGL(raster_faces_kernel, dim3(rp::cdiv(max_faces, 128), B), dim3(128), 0, st, verts, faces, vert_off, face_off,
                     face_cnt, T, K, H, W, near, pixel_center, perspective_correct, static_cast<unsigned long long*>(workspace));
  return rp::check_launch(fn);
}

int rnnpose_raster_resolve_f32(const float* verts, const int* faces, const int* vert_off, const int* face_off, const float* T,
                               const float* K, int B, int H, int W, float near, float pixel_center, int perspective_correct,
                               const void* workspace, const float* attr, const long long* attr_off, int C,
                               const float* colors, int with_color, int shade, float empty_depth, float* out_attr,
                               float* out_zbuf, float* out_vdepth, rnnpose_stream_t stream) {
  return resolve_launch<false>("rnnpose_raster_resolve_f32", verts, faces, vert_off, face_off, T, K, B, H, W, near, pixel_center,
                               perspective_correct, workspace, attr, attr_off, C, colors, with_color ? 3 : 0, TexArgs{}, shade,
                               empty_depth, out_attr, out_zbuf, out_vdepth, stream);
}

int rnnpose_raster_resolve_tex_f32(const float* verts, const int* faces, const int* vert_off, const int* face_off, const float* T,
                                   const float* K, int B, int H, int W, float near, float pixel_center, int perspective_correct,
                                   const void* workspace, const float* attr, const long long* attr_off, int C,
                                   const float* colors, const float* uvs, const int* face_uvs, const int* uv_off, const float* tex,
                                   const long long* tex_off, const int* tex_hw, const float* vnormals, int shade,
                                   float empty_depth, float* out_attr, float* out_zbuf, float* out_vdepth,
                                   rnnpose_stream_t stream) {
  const TexArgs tx{uvs, face_uvs, uv_off, reinterpret_cast<const float4*>(tex), tex_off, tex_hw, vnormals};
  return resolve_launch<true>("rnnpose_raster_resolve_tex_f32", verts, faces, vert_off, face_off, T, K, B, H, W, near, pixel_center,
                              perspective_correct, workspace, attr, attr_off, C, colors, 3, tx, shade, empty_depth, out_attr, out_zbuf,
                              out_vdepth, stream);
}

int rnnpose_raster_occlusion_f32(const float* verts, const int* faces, const int* vert_off, const int* face_off,
                                 const int* face_cnt, int max_faces, const float* T, const float* K, int B, int H, int W,
                                 float near, float pixel_center, const int* pair_target, const int* pair_occluder, int P,
                                 float margin, const void* own_keys, void* workspace, size_t workspace_bytes, float* visible,
                                 int* occluder, float* depth_inout, rnnpose_stream_t stream) {
  const char* fn = "rnnpose_raster_occlusion_f32";
  if (raster_check(fn, verts, faces, vert_off, face_off, T, K, workspace, face_cnt && own_keys && visible, B, H, W,
                   max_faces > 0 && near > 0.f))
    return 1;
  RP_REQUIRE(P >= 0 && P <= 65535, fn, "pair count must lie in [0, 65535]");
  RP_REQUIRE(P == 0 || (pair_target && pair_occluder), fn, "pairs need pair_target and pair_occluder");
  RP_REQUIRE(margin == margin, fn, "margin is NaN");
  RP_REQUIRE(own_keys != workspace, fn, "the occluder workspace must not be the own key buffer");
  hipStream_t st = rp::as_stream(stream);
  if (raster_clear(fn, workspace, workspace_bytes, B, H, W, st)) return 1;
  unsigned long long* zb = static_cast<unsigned long long*>(workspace);
  if (P > 0)
    hipLaunchKernelGGL(raster_occluder_kernel, dim3(rp::cdiv(max_faces, 128), P), dim3(128), 0, st, verts, faces, vert_off, face_off,
                       face_cnt, T, K, pair_target, pair_occluder, B, H, W, near, pixel_center, zb);
  const long long n = static_cast<long long>(B) * H * W;
  hipLaunchKernelGGL(raster_occlusion_apply_kernel, dim3(rp::cdiv(n, 256)), dim3(256), 0, st,
                     static_cast<const unsigned long long*>(own_keys), zb, n, margin, visible, occluder, depth_inout);
  return rp::check_launch(fn);
}

}  // extern "C"
