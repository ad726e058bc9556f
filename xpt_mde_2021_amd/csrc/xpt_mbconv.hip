// xpt_mbconv.hip -- the middle of a MobileNetV2 inverted-residual block: depthwise 3x3 -> BatchNorm -> ReLU6.
//
// Reference: model/build_model/pretrained_nets.py:31-34 instantiates tf.keras.applications.MobileNetV2(include_top=False) as one
// of the DepthNetPretrained backbones; its _inverted_res_block is expand 1x1 -> BN -> ReLU6 -> DepthwiseConv2D 3x3 -> BN -> ReLU6
// -> project 1x1 -> BN (+ input).  The two pointwise halves are xpt_pwconv_bn_fwd / xpt_conv1x1_bn_bwd_fused; this file is the
// stage between them.  NASNet's separable convolutions are pre-activation (ReLU -> depthwise -> pointwise -> BN), so the kernels
// of xpt_dwconv.hip know `relu_in` only: nothing there clamps at 6 or puts a BatchNorm on a depthwise output.
//
//   a(v)  = clamp(v, 0, 6) when act_in (the ReLU6 behind the PRECEDING BatchNorm, whose producer stores its pre-activation
//           output: the clamp rides in this kernel's loads, forward and backward), else v
//   u     = sum_{ky,kx<3} w[c,ky,kx] a(x[b, oy S + ky - pad_t, ox S + kx - pad_l, c])        (zero outside the input)
//   y     = clamp(s[c] u + t[c], 0, 6),   s = gamma rsqrt(var + eps),  t = beta - mean s        (moving statistics)
//
// Activations NHWC in the 16-bit format of the build, parameters and accumulation fp32; the 16-byte loads and their halo are
// those of xpt_dwstage.h, stride / act_in / the 3x3 extent are template parameters, index splits go through xpt_divmod.  At
// batch 8 these launches are a few hundred workgroups at one wave per SIMD ("the lesson of the round"): the
// plans first of all keep the workgroup count up -- on the 1/16 and 1/32 maps (<= 4 x 13 pixels, 576 - 960 channels) by
// spreading over channel groups instead of rows.  Workgroups are numbered image-major through xpt_xcd_unit, as every encoder
// launch is.
//
// Backward, ONE launch: re-indexed over the INPUT pixel.  The lane of input pixel p gathers gz = dy [0 < y < 6] at the (up to 9)
// outputs that read p; with them dx(p) = a'(x) s sum_k w_k gz_k, and the same gz_k times a(x(p)) are p's contributions to
// G[c,k] = sum gz a(x)[tap k].  dbeta's sum of gz takes the centre tap, which every output has exactly once (the entry point
// checks that the centre of every window lies inside the input).  No atomics: a workgroup owns a chunk of input rows and a block
// of channel groups, adds its lanes through LDS in a fixed order and writes one row of the partial matrix.
#include "xpt_dwstage.h"

namespace {

template <int ACT>
__device__ __forceinline__ float mb_act(float v) {
  return ACT ? fminf(fmaxf(v, 0.f), 6.f) : v;
}

// the 72 weights [8 channels][9 taps] of channel group cg (288 bytes, 16-byte aligned) and the BatchNorm scale of its channels
__device__ __forceinline__ void mb_load_weights(const float* __restrict__ w, unsigned cg, float (&wf)[72]) {
  const float4* wp = (const float4*)(w + (size_t)cg * 72);
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    const float4 v = wp[i];
    wf[4 * i] = v.x; wf[4 * i + 1] = v.y; wf[4 * i + 2] = v.z; wf[4 * i + 3] = v.w;
  }
}

// ------------------------------------------------------------------------------------------------ forward
// item = ((b OH + oy) OXB + oxb) CG + cg: OXT neighbouring outputs of a row, 8 channels; 256 consecutive items per workgroup
template <int S, int ACT, int OXT>
__global__ __launch_bounds__(256) void mb_fwd_kernel(const void* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                      void* __restrict__ y, DwDims d, unsigned xbytes, unsigned nunits,
                                                      unsigned total, unsigned CG, unsigned OXB, int xcd_on) {
  unsigned unit;
  if (!xpt_xcd_unit(xcd_on != 0, blockIdx.x, nunits, unit)) return;
  const unsigned item = unit * 256u + threadIdx.x;
  if (item >= total) return;
  unsigned cg, oxb, oy;
  unsigned q = xpt_divmod(item, CG, cg);
  q = xpt_divmod(q, OXB, oxb);
  const unsigned b = xpt_divmod(q, (unsigned)d.OH, oy);

  float wf[72];
  mb_load_weights(w, cg, wf);
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned c = cg * 8 + j;
    sc[j] = gamma[c] * (1.0f / sqrtf(var[c] + eps));
    sh[j] = beta[c] - mean[c] * sc[j];
  }

  constexpr int NC = (OXT - 1) * S + 3;                         // input columns the OXT windows span
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)xbytes, 0x00020000);
  const int iy0 = (int)oy * S - d.pad_t, ix0 = (int)(oxb * OXT) * S - d.pad_l;
  const unsigned pix = (unsigned)d.C * 2u, rowpitch = (unsigned)d.W * pix;
  const unsigned base = b * (unsigned)d.H * rowpitch + cg * 16u;
  float acc[OXT][8];
#pragma unroll
  for (int o = 0; o < OXT; ++o)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[o][j] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = iy0 + ky;
    const bool rowok = (unsigned)iy < (unsigned)d.H;
    dw_u32x4 v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int ix = ix0 + c;
      const bool ok = rowok && (unsigned)ix < (unsigned)d.W;
      const unsigned off = ok ? base + (unsigned)iy * rowpitch + (unsigned)ix * pix : DW_OOB;
      v[c] = __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float a[8];
      dw_unpack(v[c], a);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = mb_act<ACT>(a[j]);
#pragma unroll
      for (int o = 0; o < OXT; ++o) {
        const int kx = c - o * S;
        if (kx >= 0 && kx < 3) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[o][j] += wf[j * 9 + ky * 3 + kx] * a[j];
        }
      }
    }
  }
#pragma unroll
  for (int o = 0; o < OXT; ++o) {
    const unsigned ox = oxb * OXT + o;
    if (ox < (unsigned)d.OW) {
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = fminf(fmaxf(sc[j] * acc[o][j] + sh[j], 0.f), 6.f);
      const size_t e = ((size_t)(b * (unsigned)d.OH + oy) * (unsigned)d.OW + ox) * (unsigned)d.C + cg * 8u;
      *(uint4*)((unsigned short*)y + e) = dw_pack(r);
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
constexpr int MB_NE = 11;                 // per channel: 9 weight-gradient entries, dgamma, dbeta
constexpr int MB_MAX_CGB = 64;            // channel groups per workgroup at most
// workgroup = (chunk, channel block cb); thread = (pl, cgl): channel group cb cgb + cgl, input pixels pl, pl + PXT, ... of the chunk
template <int S, int ACT>
__global__ __launch_bounds__(256) void mb_bwd_kernel(const void* __restrict__ x, const void* __restrict__ y,
                                                      const void* __restrict__ dy, unsigned dy_pitch_bytes,
                                                      const float* __restrict__ w, const float* __restrict__ gamma,
                                                      const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                      void* __restrict__ dx, float* __restrict__ partials, DwDims d, DwPlan p,
                                                      unsigned ybytes,
                                                      unsigned dybytes, unsigned nunits, int xcd_on) {
  __shared__ float red[DW_PASS * 8][256];
  unsigned unit;
  if (!xpt_xcd_unit(xcd_on != 0, blockIdx.x, nunits, unit)) return;          // (uniform over the workgroup)
  unsigned cb;
  const unsigned chunk = xpt_divmod(unit, (unsigned)p.ncb, cb);
  unsigned oyc;
  const unsigned b = xpt_divmod(chunk, (unsigned)p.cpi, oyc);
  const int oy0 = (int)oyc * p.rpc, oy1 = min(d.OH, oy0 + p.rpc);
  const int r0 = dw_in_row(oy0, S, d.OH, d.H), r1 = dw_in_row(oy1, S, d.OH, d.H);
  const unsigned npix = (unsigned)(r1 - r0) * (unsigned)d.W;
  const unsigned CGB = (unsigned)p.cgb, PXT = 256u / CGB;
  unsigned cgl;
  const unsigned pl = xpt_divmod(threadIdx.x, CGB, cgl);
  const bool active = pl < PXT;
  const unsigned cg = cb * CGB + cgl;

  float wf[72], sc[8], rstd[8], mu[8];
  mb_load_weights(w, cg, wf);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned c = cg * 8 + j;
    mu[j] = mean[c];
    rstd[j] = 1.0f / sqrtf(var[c] + eps);
    sc[j] = gamma[c] * rstd[j];
  }
  float G[9][8], gb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    gb[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k][j] = 0.f;
  }

  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)y, 0, (int)ybytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, (int)dybytes, 0x00020000);
  const unsigned pix = (unsigned)d.C * 2u;
  if (active) {
    for (unsigned i = pl; i < npix; i += PXT) {
      unsigned ix;
      const int iy = r0 + (int)xpt_divmod(i, (unsigned)d.W, ix);
      const size_t xe = ((size_t)(b * (unsigned)d.H + (unsigned)iy) * (unsigned)d.W + ix) * (unsigned)d.C + cg * 8u;
      float xa[8], live[8];
      dw_unpack(dw_load16(x, xe), xa);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        live[j] = (!ACT || (xa[j] > 0.f && xa[j] < 6.f)) ? 1.f : 0.f;
        xa[j] = mb_act<ACT>(xa[j]);
      }
      // the outputs that read this pixel: tap (ky, kx) of output ((iy + pad_t - ky) / S, (ix + pad_l - kx) / S)
      dw_u32x4 vy[9], vd[9];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int ty = iy + d.pad_t - ky;
        const int oy = S == 2 ? ty >> 1 : ty;
        const bool yok = ty >= 0 && (S == 1 || (ty & 1) == 0) && oy < d.OH;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int tx = (int)ix + d.pad_l - kx;
          const int ox = S == 2 ? tx >> 1 : tx;
          const bool ok = yok && tx >= 0 && (S == 1 || (tx & 1) == 0) && ox < d.OW;
          const unsigned opix = (b * (unsigned)d.OH + (unsigned)oy) * (unsigned)d.OW + (unsigned)ox;
          vy[ky * 3 + kx] = __builtin_amdgcn_raw_buffer_load_b128(ry, ok ? opix * pix + cg * 16u : DW_OOB, 0, 0);
          vd[ky * 3 + kx] = __builtin_amdgcn_raw_buffer_load_b128(rd, ok ? opix * dy_pitch_bytes + cg * 16u : DW_OOB, 0, 0);
        }
      }
      float ds[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) ds[j] = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        float yv[8], gz[8];
        dw_unpack(vy[k], yv);
        dw_unpack(vd[k], gz);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          gz[j] = (yv[j] > 0.f && yv[j] < 6.f) ? gz[j] : 0.f;          // tf.nn.relu6: no gradient at exactly 0 and 6
          ds[j] += wf[j * 9 + k] * gz[j];
          G[k][j] += gz[j] * xa[j];
          if (k == 4) gb[j] += gz[j];                                   // the centre tap: every output exactly once
        }
      }
      if (dx != nullptr) {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = live[j] * sc[j] * ds[j];
        *(uint4*)((unsigned short*)dx + xe) = dw_pack(r);
      }
    }
  }

  // in parameter units: entries 0..8 = s G (dL/dw), 10 = sum gz (dL/dbeta), 9 = rsqrt(var + eps) (sum_k w_k G_k - mean sum gz)
  // (dL/dgamma: d(s u + beta - mean s) / dgamma = (u - mean) rsqrt(var + eps), and sum gz u = sum_k w_k G_k as u = sum_k w_k a(x)_k)
  float out[MB_NE][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      out[k][j] = sc[j] * G[k][j];
      dot += wf[j * 9 + k] * G[k][j];
    }
    out[9][j] = rstd[j] * (dot - mu[j] * gb[j]);
    out[10][j] = gb[j];
  }
  // the workgroup's sum over pl, in pl order; row `chunk` of the partial matrix: [C][9] weights | [C] gamma | [C] beta
  float* prow = partials + (size_t)chunk * MB_NE * (unsigned)d.C;
#pragma unroll
  for (int pass = 0; pass < (MB_NE + DW_PASS - 1) / DW_PASS; ++pass) {
    __syncthreads();                                                     // the previous pass has been read
    if (active) {
#pragma unroll
      for (int el = 0; el < DW_PASS; ++el) {
        const int e = pass * DW_PASS + el;
        if (e < MB_NE) {
#pragma unroll
          for (int j = 0; j < 8; ++j) red[el * 8 + j][threadIdx.x] = out[e][j];
        }
      }
    }
    __syncthreads();
    const int ne = min(DW_PASS, MB_NE - pass * DW_PASS);
    const unsigned nout = (unsigned)ne * 8u * CGB;
    for (unsigned o = threadIdx.x; o < nout; o += 256u) {
      unsigned gl;
      const unsigned v = xpt_divmod(o, CGB, gl);                         // v = el * 8 + j
      float sum = 0.f;
      for (unsigned t = 0; t < PXT; ++t) sum += red[v][t * CGB + gl];
      const unsigned e = (unsigned)pass * DW_PASS + (v >> 3), c = (cb * CGB + gl) * 8u + (v & 7u);
      const unsigned at = e < 9u ? c * 9u + e : (e * (unsigned)d.C + c);   // 9 C + c (gamma), 10 C + c (beta)
      prow[at] = sum;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
template <int S, int ACT, int OXT>
void mb_launch_fwd(const void* x, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                   float eps, void* y, const DwDims& d, hipStream_t stream) {
  const unsigned CG = (unsigned)d.C / 8u, OXB = ((unsigned)d.OW + OXT - 1) / OXT;
  const unsigned total = (unsigned)d.B * (unsigned)d.OH * OXB * CG;
  const unsigned nunits = (total + 255u) / 256u;
  const int on = g_xpt_xcd_affinity;
  const unsigned xbytes = (unsigned)((long long)d.B * d.H * d.W * d.C * 2);
  hipLaunchKernelGGL((mb_fwd_kernel<S, ACT, OXT>), dim3(on ? xpt_xcd_pad(nunits) : nunits), dim3(256), 0, stream, x, w, gamma,
                     beta, mean, var, eps, y, d, xbytes, nunits, total, CG, OXB, on);
}

int g_mb_fwd_outputs = 0;                 // xpt_dwconv_bn_relu6_tune(): outputs per lane of the forward, 0 = automatic

// as many neighbouring outputs per lane (4, 2 or 1) as still leave two workgroups per CU
int mb_fwd_outputs(int B, int OH, int OW, int C) {
  if (g_mb_fwd_outputs) return g_mb_fwd_outputs;
  const long long per_col = (long long)B * OH * (C / 8);
  auto wgs = [&](int oxt) { return (per_col * ((OW + oxt - 1) / oxt) + 255) / 256; };
  if (OW >= 4 && wgs(4) >= 512) return 4;
  if (OW >= 2 && wgs(2) >= 512) return 2;
  return 1;
}

template <int S, int ACT>
void mb_dispatch_fwd(const void* x, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                     float eps, void* y, const DwDims& d, hipStream_t stream) {
  const int oxt = mb_fwd_outputs(d.B, d.OH, d.OW, d.C);
  if (oxt == 4) mb_launch_fwd<S, ACT, 4>(x, w, gamma, beta, mean, var, eps, y, d, stream);
  else if (oxt == 2) mb_launch_fwd<S, ACT, 2>(x, w, gamma, beta, mean, var, eps, y, d, stream);
  else mb_launch_fwd<S, ACT, 1>(x, w, gamma, beta, mean, var, eps, y, d, stream);
}

}  // namespace

extern "C" {

int xpt_dwconv_bn_relu6_fwd(const void* x, const float* w, const float* gamma, const float* beta, const float* mean,
                            const float* var, float eps, void* y, int B, int H, int W, int C, int stride, int pad_t, int pad_l,
                            int OH, int OW, int act_in, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(w); XPT_CHECK_PTR(gamma); XPT_CHECK_PTR(beta); XPT_CHECK_PTR(mean); XPT_CHECK_PTR(var);
  XPT_CHECK_PTR(y);
  const DwDims d{B, H, W, C, OH, OW, pad_t, pad_l};
  const int rc = dw_check(d, 3, stride);
  if (rc != XPT_OK) return rc;
  if (!dw_aligned(x) || !dw_aligned(y) || !dw_aligned(w)) return XPT_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  XPT_BEGIN_LAUNCH();
  if (stride == 1) {
    if (act_in) mb_dispatch_fwd<1, 1>(x, w, gamma, beta, mean, var, eps, y, d, s);
    else mb_dispatch_fwd<1, 0>(x, w, gamma, beta, mean, var, eps, y, d, s);
  } else {
    if (act_in) mb_dispatch_fwd<2, 1>(x, w, gamma, beta, mean, var, eps, y, d, s);
    else mb_dispatch_fwd<2, 0>(x, w, gamma, beta, mean, var, eps, y, d, s);
  }
  return xpt_launch_status();
}

int xpt_dwconv_bn_relu6_tune(int fwd_outputs) {
  if (fwd_outputs != 0 && fwd_outputs != 1 && fwd_outputs != 2 && fwd_outputs != 4) return XPT_ERR_ARG;
  g_mb_fwd_outputs = fwd_outputs;
  return XPT_OK;
}

int xpt_dwconv_bn_relu6_fwd_outputs(int B, int OH, int OW, int C) {
  if (B <= 0 || OH <= 0 || OW <= 0 || C <= 0 || C % 8 != 0) return 0;
  return mb_fwd_outputs(B, OH, OW, C);
}

int xpt_dwconv_bn_relu6_bwd_chunks(int B, int OH, int OW, int C) {
  if (B <= 0 || OH <= 0 || OW <= 0 || C <= 0 || C % 8 != 0) return 0;
  return dw_plan(B, OH, OW, C, MB_MAX_CGB).chunks;
}

int xpt_dwconv_bn_relu6_bwd(const void* x, const void* y, const void* dy, long long dy_pitch, const float* w,
                            const float* gamma, const float* mean, const float* var, float eps, void* dx, float* partials,
                            size_t partial_floats, int B, int H, int W, int C, int stride, int pad_t, int pad_l, int OH, int OW,
                            int act_in, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(y); XPT_CHECK_PTR(dy); XPT_CHECK_PTR(w); XPT_CHECK_PTR(gamma); XPT_CHECK_PTR(mean);
  XPT_CHECK_PTR(var);
  XPT_CHECK_PTR(partials);
  const DwDims d{B, H, W, C, OH, OW, pad_t, pad_l};
  const int rc = dw_check(d, 3, stride);
  if (rc != XPT_OK) return rc;
  if (dy_pitch < C || dy_pitch % 8 != 0) return XPT_ERR_SHAPE;
  const long long opix = (long long)B * OH * OW;
  const long long dybytes = ((opix - 1) * dy_pitch + C) * 2, ybytes = opix * C * 2;
  if (dybytes >= (1LL << 31) || ybytes >= (1LL << 31)) return XPT_ERR_SHAPE;
  if (!dw_aligned(x) || !dw_aligned(y) || !dw_aligned(dy) || !dw_aligned(w) || (dx != nullptr && !dw_aligned(dx)))
    return XPT_ERR_ARG;
  const DwPlan p = dw_plan(B, OH, OW, C, MB_MAX_CGB);
  if (partial_floats < (size_t)p.chunks * MB_NE * (size_t)C) return XPT_ERR_WORKSPACE;
  const unsigned nunits = (unsigned)p.chunks * (unsigned)p.ncb;
  const int on = g_xpt_xcd_affinity;
  const dim3 grid(on ? xpt_xcd_pad(nunits) : nunits);
  const hipStream_t s = (hipStream_t)stream;
  XPT_BEGIN_LAUNCH();
#define MB_BWD(S_, A_)                                                                                                    \
  hipLaunchKernelGGL((mb_bwd_kernel<S_, A_>), grid, dim3(256), 0, s, x, y, dy, (unsigned)(dy_pitch * 2), w, gamma, mean, var, eps, dx, \
                     partials, d, p, (unsigned)ybytes, (unsigned)dybytes, nunits, on)
  if (stride == 1) {
    if (act_in) MB_BWD(1, 1); else MB_BWD(1, 0);
  } else {
    if (act_in) MB_BWD(2, 1); else MB_BWD(2, 0);
  }
#undef MB_BWD
  return xpt_launch_status();
}

}  // extern "C"
