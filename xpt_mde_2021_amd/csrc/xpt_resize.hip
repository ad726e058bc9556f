// xpt_resize.hip -- bilinear resize of 16-bit NHWC feature maps to an ARBITRARY size, forward and exact adjoint.
//
// Replaces tf.image.resize(method="bilinear") of TF2 as DepthNetBasic uses it between the two convolutions of every decoder
// level (model/model_util/layer_ops.py:39-50 resize_like, model/build_model/depth_net.py:79): half-pixel centres, no
// antialiasing, source coordinate (dst + 0.5) * in / out - 0.5 clamped to the edges -- the numbers of
// at::upsample_bilinear2d(align_corners=False, antialias=False).
//
// Forward: a thread owns 8 consecutive channels of one output pixel: four 16-byte loads, the interpolation in fp32, one
// rounding, one 16-byte store.
// Adjoint, gather form: a thread owns 8 channels of one INPUT pixel and walks the output pixels that can have read it.  The
// candidate range per axis follows from the two sizes (every output coordinate whose source coordinate lies within one pixel of
// the input coordinate, one more on either side against rounding, everything up to the border for the two clamped edge
// pixels); inside it the taps of every candidate are recomputed with the forward's own function and only those that hit the
// pixel count, so the launch is the exact transpose of the forward whatever the rounding of the coordinates.  No scatter, no
// atomics: fp32 sums in a fixed order (rows outer, columns inner), rounded once.
#include "xpt_common.h"

namespace {

// taps of output coordinate o along an axis of n input pixels: i0 <= i1 (equal on a clamped edge), weight l on i1, 1 - l on i0
__device__ __forceinline__ void resize_taps(int o, int n, float scale, int& i0, int& i1, float& l) {
  float s = scale * ((float)o + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i0 = i0 < n - 1 ? i0 : n - 1;
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  l = s - (float)i0;
}

// weight with which output coordinate o reads input coordinate i (0 when it does not)
__device__ __forceinline__ float resize_weight(int o, int i, int n, float scale) {
  int i0, i1;
  float l;
  resize_taps(o, n, scale, i0, i1, l);
  return (i0 == i ? 1.f - l : 0.f) + (i1 == i ? l : 0.f);
}

// output coordinates [lo, hi] that can read input coordinate i (n inputs, m outputs); a superset, clipped to [0, m - 1]
__device__ __forceinline__ void resize_candidates(int i, int n, int m, float inv_scale, int& lo, int& hi) {
  lo = (int)floorf(((float)i - 0.5f) * inv_scale - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.5f) * inv_scale - 0.5f) + 1;
  if (i == 0 || lo < 0) lo = 0;
  if (i == n - 1 || hi > m - 1) hi = m - 1;
}

__device__ __forceinline__ void unpack8(const uint4& v, float (&f)[8]) {
  f[0] = xpt_h2f_lo(v.x); f[1] = xpt_h2f_hi(v.x);
  f[2] = xpt_h2f_lo(v.y); f[3] = xpt_h2f_hi(v.y);
  f[4] = xpt_h2f_lo(v.z); f[5] = xpt_h2f_hi(v.z);
  f[6] = xpt_h2f_lo(v.w); f[7] = xpt_h2f_hi(v.w);
}

__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  uint4 v;
  v.x = (unsigned)xpt_f2h(f[0]) | ((unsigned)xpt_f2h(f[1]) << 16);
  v.y = (unsigned)xpt_f2h(f[2]) | ((unsigned)xpt_f2h(f[3]) << 16);
  v.z = (unsigned)xpt_f2h(f[4]) | ((unsigned)xpt_f2h(f[5]) << 16);
  v.w = (unsigned)xpt_f2h(f[6]) | ((unsigned)xpt_f2h(f[7]) << 16);
  return v;
}

struct ResizeArgs {
  const unsigned short* src;   // forward: x [B,IH,IW,.]; adjoint: g [B,OH,OW,.]
  unsigned short* dst;         // forward: y [B,OH,OW,.]; adjoint: dx [B,IH,IW,.]
  long long spitch, dpitch;    // pixel pitches in elements
  int IH, IW, OH, OW, C8;      // input / output extents of the FORWARD resize, channel groups of 8
  float sh, sw;                // IH / OH, IW / OW
  float ish, isw;              // OH / IH, OW / IW
  unsigned total;              // threads
};

__global__ __launch_bounds__(256) void resize_bilinear_fwd_kernel(ResizeArgs a) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= a.total) return;
  int c8, ox, oy, b;
  xpt_split4(idx, a.C8, a.OW, a.OH, c8, ox, oy, b);
  int y0, y1, x0, x1;
  float ly, lx;
  resize_taps(oy, a.IH, a.sh, y0, y1, ly);
  resize_taps(ox, a.IW, a.sw, x0, x1, lx);
  const unsigned short* base = a.src + (long long)b * a.IH * a.IW * a.spitch + 8 * c8;
  const uint4 v00 = *(const uint4*)(base + ((long long)y0 * a.IW + x0) * a.spitch);
  const uint4 v01 = *(const uint4*)(base + ((long long)y0 * a.IW + x1) * a.spitch);
  const uint4 v10 = *(const uint4*)(base + ((long long)y1 * a.IW + x0) * a.spitch);
  const uint4 v11 = *(const uint4*)(base + ((long long)y1 * a.IW + x1) * a.spitch);
  float f00[8], f01[8], f10[8], f11[8], r[8];
  unpack8(v00, f00); unpack8(v01, f01); unpack8(v10, f10); unpack8(v11, f11);
  const float wy0 = 1.f - ly, wx0 = 1.f - lx;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = wy0 * (wx0 * f00[e] + lx * f01[e]) + ly * (wx0 * f10[e] + lx * f11[e]);
  *(uint4*)(a.dst + (((long long)b * a.OH + oy) * a.OW + ox) * a.dpitch + 8 * c8) = pack8(r);
}

__global__ __launch_bounds__(256) void resize_bilinear_adjoint_kernel(ResizeArgs a) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= a.total) return;
  int c8, ix, iy, b;
  xpt_split4(idx, a.C8, a.IW, a.IH, c8, ix, iy, b);
  int ylo, yhi, xlo, xhi;
  resize_candidates(iy, a.IH, a.OH, a.ish, ylo, yhi);
  resize_candidates(ix, a.IW, a.OW, a.isw, xlo, xhi);
  const unsigned short* base = a.src + (long long)b * a.OH * a.OW * a.spitch + 8 * c8;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int oy = ylo; oy <= yhi; ++oy) {
    const float wy = resize_weight(oy, iy, a.IH, a.sh);
    if (wy == 0.f) continue;
    for (int ox = xlo; ox <= xhi; ++ox) {
      const float w = wy * resize_weight(ox, ix, a.IW, a.sw);
      if (w == 0.f) continue;
      float f[8];
      unpack8(*(const uint4*)(base + ((long long)oy * a.OW + ox) * a.spitch), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += w * f[e];
    }
  }
  *(uint4*)(a.dst + (((long long)b * a.IH + iy) * a.IW + ix) * a.dpitch + 8 * c8) = pack8(acc);
}

int resize_args(const void* src, long long spitch, void* dst, long long dpitch, int B, int IH, int IW, int OH, int OW, int C,
                bool adjoint, ResizeArgs& a) {
  if (B <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0 || C <= 0) return XPT_ERR_SHAPE;
  if (C % 8 != 0 || spitch < C || spitch % 8 != 0 || dpitch < C || dpitch % 8 != 0 || ((uintptr_t)src) % 16 != 0 ||
      ((uintptr_t)dst) % 16 != 0)
    return XPT_ERR_ARG;
  // 32-bit thread index split with xpt_divmod (divisors below 2^24); source coordinates exact in fp32
  if (IH >= (1 << 20) || IW >= (1 << 20) || OH >= (1 << 20) || OW >= (1 << 20)) return XPT_ERR_SHAPE;
  const long long total = (long long)B * (adjoint ? (long long)IH * IW : (long long)OH * OW) * (C / 8);
  if (total >= 0x7fffffffLL) return XPT_ERR_SHAPE;
  a.src = (const unsigned short*)src; a.dst = (unsigned short*)dst;
  a.spitch = spitch; a.dpitch = dpitch;
  a.IH = IH; a.IW = IW; a.OH = OH; a.OW = OW; a.C8 = C / 8;
  a.sh = (float)IH / (float)OH; a.sw = (float)IW / (float)OW;
  a.ish = (float)OH / (float)IH; a.isw = (float)OW / (float)IW;
  a.total = (unsigned)total;
  return XPT_OK;
}

}  // namespace

extern "C" int xpt_resize_bilinear_fwd(const void* x, long long xpitch, void* y, long long ypitch, int B, int IH, int IW,
                                       int OH, int OW, int C, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(y);
  ResizeArgs a{};
  const int rc = resize_args(x, xpitch, y, ypitch, B, IH, IW, OH, OW, C, false, a);
  if (rc != XPT_OK) return rc;
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(resize_bilinear_fwd_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  return xpt_launch_status();
}

extern "C" int xpt_resize_bilinear_adjoint(const void* g, long long gpitch, void* dx, long long dxpitch, int B, int IH, int IW,
                                           int OH, int OW, int C, void* stream) {
  XPT_CHECK_PTR(g); XPT_CHECK_PTR(dx);
  ResizeArgs a{};
  const int rc = resize_args(g, gpitch, dx, dxpitch, B, IH, IW, OH, OW, C, true, a);
  if (rc != XPT_OK) return rc;
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(resize_bilinear_adjoint_kernel, dim3((a.total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  return xpt_launch_status();
}
