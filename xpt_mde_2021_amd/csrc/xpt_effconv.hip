// xpt_effconv.hip -- the middle of an EfficientNet MBConv block: depthwise k x k -> BatchNorm -> swish -> squeeze-and-excite.
//
// Reference: model/build_model/pretrained_nets.py:11-117 instantiates tf.keras.applications.EfficientNetB0 ... B7
// (include_top=False; config-example.py JOINT_NET "depth", RIGID_EF0 / EF3 / EF5 / EF7); the `block` function of keras
// efficientnet.py is expand 1x1 -> BN -> swish -> DepthwiseConv2D k x k -> BN -> swish -> GlobalAveragePooling2D -> Conv2D 1x1
// (bias, swish) -> Conv2D 1x1 (bias, sigmoid) -> multiply -> project 1x1 -> BN (+ input).  The two pointwise halves are
// xpt_pwconv_bn_fwd / xpt_conv1x1_bn_bwd_fused; this file is everything between them.
//
//   sw(v)  = v sigma(v),   sw'(v) = sigma(v) (1 + v (1 - sigma(v)))
//   a(v)   = sw(v) when act_in (the swish behind the PRECEDING BatchNorm, whose producer stores its pre-activation output), else v
//   u      = sum_{ky,kx<k} w[c,ky,kx] a(x[b, oy S + ky - pad_t, ox S + kx - pad_l, c])          (zero outside the input)
//   v      = s[c] u + t[c],   s = gamma rsqrt(var + eps),  t = beta - mean s                     (moving statistics; STORED)
//   p[b,c] = mean_hw sw(v),   r = W_r p + b_r,   q = sw(r),   e = W_e q + b_e,   gate = sigma(e)
//   z      = sw(v) gate[b,c]                                                                     (input of the projection)
//
// Activations NHWC in the 16-bit format of the build, parameters and accumulation fp32; the 16-byte loads, the halo and the ONE
// row-chunk plan of every kernel that sums over pixels (the pool of the forward, dL/dgate, the parameter gradients of the
// depthwise stage) are those of xpt_dwstage.h.  The k x k weights of the workgroup's channel block sit in LDS ([tap][channel]:
// 25 x 8 weights per lane do not fit the register file next to 25 x 8 accumulators).
//
// The depthwise kernels gather through L2: no LDS tile of the input yet.
#include "xpt_dwstage.h"

namespace {

constexpr int EF_MAX_CGB = 32;                  // channel groups per workgroup at most (LDS: k k x 256 weights)
constexpr int EF_LDS_FLOATS = 12288;            // dynamic LDS of the excite kernels (48 KiB)
constexpr int EF_CB = 64;                       // channels per workgroup of the excite backward

__device__ __forceinline__ float ef_sigmoid(float v) { return 1.0f / (1.0f + __expf(-v)); }
__device__ __forceinline__ float ef_swish(float v) { return v * ef_sigmoid(v); }
__device__ __forceinline__ float ef_dswish(float v) {
  const float g = ef_sigmoid(v);
  return g * (1.0f + v * (1.0f - g));
}

// the workgroup of a unit: chunk (= image b, row chunk oyc) and channel block cb; the lane: (pixel lane pl, channel group cgl)
struct EfWho {
  unsigned chunk, cb, b, CGB, PXT, pl, cgl, cg;
  int oy0, oy1;
  bool active;
};

__device__ __forceinline__ EfWho ef_who(unsigned unit, const DwPlan& p, int OH) {
  EfWho w;
  w.chunk = xpt_divmod(unit, (unsigned)p.ncb, w.cb);
  unsigned oyc;
  w.b = xpt_divmod(w.chunk, (unsigned)p.cpi, oyc);
  w.oy0 = (int)oyc * p.rpc;
  w.oy1 = min(OH, w.oy0 + p.rpc);
  w.CGB = (unsigned)p.cgb;
  w.PXT = 256u / w.CGB;
  w.pl = xpt_divmod(threadIdx.x, w.CGB, w.cgl);
  w.active = w.pl < w.PXT;
  w.cg = w.cb * w.CGB + w.cgl;
  return w;
}

// wl[tap][local channel] <- w[channel][tap] for the 8 CGB channels of channel block cb (coalesced reads)
template <int KK>
__device__ __forceinline__ void ef_stage_weights(const float* __restrict__ w, const EfWho& who, float (*wl)[256]) {
  const unsigned n = who.CGB * 8u * KK;
  const float* src = w + (size_t)who.cb * n;
  for (unsigned i = threadIdx.x; i < n; i += 256u) wl[i % KK][i / KK] = src[i];
}

// sum over the pixel lanes of each (channel group, j) in lane order; row[c] = the sum (c within this channel block)
__device__ __forceinline__ void ef_column_sums(const float (&ps)[8], const EfWho& who, float (*red)[256], float* __restrict__ row) {
  if (who.active) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[j][threadIdx.x] = ps[j];
  }
  __syncthreads();
  for (unsigned o = threadIdx.x; o < 8u * who.CGB; o += 256u) {
    unsigned gl;
    const unsigned j = xpt_divmod(o, who.CGB, gl);
    float sum = 0.f;
    for (unsigned t = 0; t < who.PXT; ++t) sum += red[j][t * who.CGB + gl];
    row[(who.cb * who.CGB + gl) * 8u + j] = sum;
  }
}

// ------------------------------------------------------------------------------------------------ depthwise forward
template <int K, int S, int ACT>
__global__ __launch_bounds__(256) void ef_dw_fwd_kernel(const void* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                         void* __restrict__ vout, float* __restrict__ pool, DwDims d, DwPlan p,
                                                         unsigned xbytes, unsigned nunits, int xcd_on) {
  constexpr int KK = K * K;
  __shared__ float wl[KK][256];
  __shared__ float red[8][256];
  unsigned unit;
  if (!xpt_xcd_unit(xcd_on != 0, blockIdx.x, nunits, unit)) return;          // (uniform over the workgroup)
  const EfWho who = ef_who(unit, p, d.OH);
  ef_stage_weights<KK>(w, who, wl);
  __syncthreads();
  float ps[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) ps[j] = 0.f;
  if (who.active) {
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned c = who.cg * 8 + j;
      sc[j] = gamma[c] * (1.0f / sqrtf(var[c] + eps));
      sh[j] = beta[c] - mean[c] * sc[j];
    }
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)xbytes, 0x00020000);
    const unsigned pix = (unsigned)d.C * 2u, rowpitch = (unsigned)d.W * pix;
    const unsigned base = who.b * (unsigned)d.H * rowpitch + who.cg * 16u;
    const unsigned nout = (unsigned)(who.oy1 - who.oy0) * (unsigned)d.OW;
    for (unsigned i = who.pl; i < nout; i += who.PXT) {
      unsigned ox;
      const unsigned oy = (unsigned)who.oy0 + xpt_divmod(i, (unsigned)d.OW, ox);
      const int iy0 = (int)oy * S - d.pad_t, ix0 = (int)ox * S - d.pad_l;
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int iy = iy0 + ky;
        const bool rowok = (unsigned)iy < (unsigned)d.H;
        dw_u32x4 t[K];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int ix = ix0 + kx;
          const bool ok = rowok && (unsigned)ix < (unsigned)d.W;
          t[kx] = __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? base + (unsigned)iy * rowpitch + (unsigned)ix * pix : DW_OOB, 0, 0);
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          float a[8], wk[8];
          dw_unpack(t[kx], a);
          dw_load8f(&wl[ky * K + kx][who.cgl * 8u], wk);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += wk[j] * (ACT ? ef_swish(a[j]) : a[j]);       // (sw(0) = 0: the halo stays zero)
        }
      }
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        r[j] = sc[j] * acc[j] + sh[j];
        ps[j] += ef_swish(r[j]);                                                             // the fp32 value, before the store rounds it
      }
      const size_t e = ((size_t)(who.b * (unsigned)d.OH + oy) * (unsigned)d.OW + ox) * (unsigned)d.C + who.cg * 8u;
      *(uint4*)((unsigned short*)vout + e) = dw_pack(r);
    }
  }
  ef_column_sums(ps, who, red, pool + (size_t)who.chunk * (unsigned)d.C);
}

// ------------------------------------------------------------------------------------------------ squeeze and excite
// one workgroup per image; dynamic LDS: p [C] | q [S]
__global__ __launch_bounds__(256) void ef_excite_fwd_kernel(const float* __restrict__ pool, int cpi, float inv_hw,
                                                             const float* __restrict__ wr, const float* __restrict__ br,
                                                             const float* __restrict__ we, const float* __restrict__ be,
                                                             float* __restrict__ pout, float* __restrict__ rout,
                                                             float* __restrict__ gate, int C, int S) {
  extern __shared__ float ef_sm[];
  float* ps = ef_sm;
  float* qs = ef_sm + C;
  const unsigned b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    float sum = 0.f;
    for (int k = 0; k < cpi; ++k) sum += pool[((size_t)b * cpi + k) * C + c];          // row order
    const float m = sum * inv_hw;
    ps[c] = m;
    pout[(size_t)b * C + c] = m;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s < S; s += 4) {                                                    // W_r [S][C]: a wave per output
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += wr[(size_t)s * C + c] * ps[c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (lane == 0) {
      const float r = sum + br[s];
      rout[(size_t)b * S + s] = r;
      qs[s] = ef_swish(r);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {                                           // W_e [C][S]
    float sum = be[c];
    for (int s = 0; s < S; ++s) sum += we[(size_t)c * S + s] * qs[s];
    gate[(size_t)b * C + c] = ef_sigmoid(sum);
  }
}

// workgroup = EF_CB channels; every workgroup first repeats the small part all of them need (dq, dr of every image: B S sums of
// length C), then writes its channels' share of the five outputs, each a sum over the batch in image order.  dynamic LDS: q [B S] | dr [B S]
__global__ __launch_bounds__(256) void ef_excite_bwd_kernel(const float* __restrict__ dgate, const float* __restrict__ gate,
                                                             const float* __restrict__ pin, const float* __restrict__ rin,
                                                             const float* __restrict__ wr, const float* __restrict__ we,
                                                             float* __restrict__ dwr, float* __restrict__ dbr,
                                                             float* __restrict__ dwe, float* __restrict__ dbe,
                                                             float* __restrict__ dp, int B, int C, int S) {
  extern __shared__ float ef_sm[];
  float* qs = ef_sm;
  float* drs = ef_sm + B * S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto de = [&](int b, int c) {
    const float g = gate[(size_t)b * C + c];
    return dgate[(size_t)b * C + c] * g * (1.0f - g);
  };
  for (int pair = wave; pair < B * S; pair += 4) {
    const int b = pair / S, s = pair - b * S;
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += we[(size_t)c * S + s] * de(b, c);          // dq = W_e^T de
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (lane == 0) {
      const float r = rin[pair];
      qs[pair] = ef_swish(r);
      drs[pair] = sum * ef_dswish(r);
    }
  }
  __syncthreads();
  const int c0 = blockIdx.x * EF_CB, nc = min(EF_CB, C - c0);
  for (int i = threadIdx.x; i < nc * S; i += 256) {                                      // dW_e [C][S] = sum_b de q
    const int cl = i / S, s = i - cl * S, c = c0 + cl;
    float sum = 0.f;
    for (int b = 0; b < B; ++b) sum += de(b, c) * qs[b * S + s];
    dwe[(size_t)c * S + s] = sum;
  }
  for (int i = threadIdx.x; i < nc; i += 256) {                                          // db_e
    float sum = 0.f;
    for (int b = 0; b < B; ++b) sum += de(b, c0 + i);
    dbe[c0 + i] = sum;
  }
  for (int i = threadIdx.x; i < nc * S; i += 256) {                                      // dW_r [S][C] = sum_b dr p
    const int s = i / nc, c = c0 + (i - s * nc);
    float sum = 0.f;
    for (int b = 0; b < B; ++b) sum += drs[b * S + s] * pin[(size_t)b * C + c];
    dwr[(size_t)s * C + c] = sum;
  }
  for (int i = threadIdx.x; i < nc * B; i += 256) {                                      // dp = W_r^T dr
    const int b = i / nc, c = c0 + (i - b * nc);
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += wr[(size_t)s * C + c] * drs[b * S + s];
    dp[(size_t)b * C + c] = sum;
  }
  if (blockIdx.x == 0) {
    for (int s = threadIdx.x; s < S; s += 256) {                                         // db_r
      float sum = 0.f;
      for (int b = 0; b < B; ++b) sum += drs[b * S + s];
      dbr[s] = sum;
    }
  }
}

// ------------------------------------------------------------------------------------------------ scale
// item = pixel CG + cg; 256 consecutive items per workgroup
__global__ __launch_bounds__(256) void ef_scale_fwd_kernel(const void* __restrict__ v, const float* __restrict__ gate,
                                                            void* __restrict__ z, unsigned total, unsigned CG, unsigned HW,
                                                            unsigned nunits, int xcd_on) {
  unsigned unit;
  if (!xpt_xcd_unit(xcd_on != 0, blockIdx.x, nunits, unit)) return;
  const unsigned item = unit * 256u + threadIdx.x;
  if (item >= total) return;
  unsigned cg, hw;
  const unsigned pixel = xpt_divmod(item, CG, cg);
  const unsigned b = xpt_divmod(pixel, HW, hw);
  float f[8], g[8];
  dw_unpack(dw_load16(v, (size_t)item * 8u), f);
  dw_load8f(gate + ((size_t)b * CG + cg) * 8u, g);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = ef_swish(f[j]) * g[j];
  *(uint4*)((unsigned short*)z + (size_t)item * 8u) = dw_pack(f);
}

// partial rows of dL/dgate[b,c] = sum_hw dz sw(v)
__global__ __launch_bounds__(256) void ef_dgate_kernel(const void* __restrict__ v, const void* __restrict__ dz, unsigned dz_pitch,
                                                        float* __restrict__ part, int OH, int OW, int C, DwPlan p,
                                                        unsigned nunits, int xcd_on) {
  __shared__ float red[8][256];
  unsigned unit;
  if (!xpt_xcd_unit(xcd_on != 0, blockIdx.x, nunits, unit)) return;
  const EfWho who = ef_who(unit, p, OH);
  float ps[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) ps[j] = 0.f;
  if (who.active) {
    const unsigned nout = (unsigned)(who.oy1 - who.oy0) * (unsigned)OW;
    const size_t first = ((size_t)who.b * (unsigned)OH + (unsigned)who.oy0) * (unsigned)OW;
    for (unsigned i = who.pl; i < nout; i += who.PXT) {
      float f[8], g[8];
      dw_unpack(dw_load16(v, (first + i) * (unsigned)C + who.cg * 8u), f);
      dw_unpack(dw_load16(dz, (first + i) * dz_pitch + who.cg * 8u), g);
#pragma unroll
      for (int j = 0; j < 8; ++j) ps[j] += g[j] * ef_swish(f[j]);
    }
  }
  ef_column_sums(ps, who, red, part + (size_t)who.chunk * (unsigned)C);
}

// out[b][c] = sum_k part[b cpi + k][c], rows in order
__global__ __launch_bounds__(256) void ef_finish_rows_kernel(const float* __restrict__ part, float* __restrict__ out, int cpi, int C,
                                                              unsigned total) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  unsigned c;
  const unsigned b = xpt_divmod(i, (unsigned)C, c);
  float sum = 0.f;
  for (int k = 0; k < cpi; ++k) sum += part[((size_t)b * cpi + k) * C + c];
  out[i] = sum;
}

// ------------------------------------------------------------------------------------------------ depthwise backward
// re-indexed over the INPUT pixel: the lane of input pixel q gathers gz = sw'(v) (dz gate + dp / (OH OW)) at
// the (up to k k) outputs that read q
template <int K, int S, int ACT>
__global__ __launch_bounds__(256) void ef_dw_bwd_kernel(const void* __restrict__ x, const void* __restrict__ v,
                                                         const void* __restrict__ dz, unsigned dz_pitch_bytes,
                                                         const float* __restrict__ gate, const float* __restrict__ dp, float inv_hw,
                                                         const float* __restrict__ w, const float* __restrict__ gamma,
                                                         const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                         void* __restrict__ dx, float* __restrict__ partials, DwDims d, DwPlan p,
                                                         unsigned vbytes, unsigned dzbytes, unsigned nunits, int xcd_on) {
  constexpr int KK = K * K, NE = KK + 2;
  __shared__ float wl[KK][256];
  __shared__ float red[DW_PASS * 8][256];
  unsigned unit;
  if (!xpt_xcd_unit(xcd_on != 0, blockIdx.x, nunits, unit)) return;          // (uniform over the workgroup)
  const EfWho who = ef_who(unit, p, d.OH);
  ef_stage_weights<KK>(w, who, wl);
  __syncthreads();
  const int r0 = dw_in_row(who.oy0, S, d.OH, d.H), r1 = dw_in_row(who.oy1, S, d.OH, d.H);
  const unsigned npix = (unsigned)(r1 - r0) * (unsigned)d.W;
  const unsigned cg = who.cg, b = who.b;

  float G[KK][8], gb[8], sc[8], rstd[8], mu[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    gb[j] = 0.f;
    sc[j] = rstd[j] = mu[j] = 0.f;
#pragma unroll
    for (int k = 0; k < KK; ++k) G[k][j] = 0.f;
  }
  if (who.active) {
    float gt[8], dpn[8];
    dw_load8f(gate + (size_t)b * (unsigned)d.C + cg * 8u, gt);
    dw_load8f(dp + (size_t)b * (unsigned)d.C + cg * 8u, dpn);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned c = cg * 8 + j;
      mu[j] = mean[c];
      rstd[j] = 1.0f / sqrtf(var[c] + eps);
      sc[j] = gamma[c] * rstd[j];
      dpn[j] *= inv_hw;
    }
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)v, 0, (int)vbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)dz, 0, (int)dzbytes, 0x00020000);
    const unsigned pix = (unsigned)d.C * 2u;
    for (unsigned i = who.pl; i < npix; i += who.PXT) {
      unsigned ix;
      const int iy = r0 + (int)xpt_divmod(i, (unsigned)d.W, ix);
      const size_t xe = ((size_t)(b * (unsigned)d.H + (unsigned)iy) * (unsigned)d.W + ix) * (unsigned)d.C + cg * 8u;
      float xa[8], slope[8], ds[8];
      dw_unpack(dw_load16(x, xe), xa);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        slope[j] = ACT ? ef_dswish(xa[j]) : 1.f;
        xa[j] = ACT ? ef_swish(xa[j]) : xa[j];
        ds[j] = 0.f;
      }
      // the outputs that read this pixel: tap (ky, kx) of output ((iy + pad_t - ky) / S, (ix + pad_l - kx) / S)
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int ty = iy + d.pad_t - ky;
        const int oy = S == 2 ? ty >> 1 : ty;
        const bool yok = ty >= 0 && (S == 1 || (ty & 1) == 0) && oy < d.OH;
        dw_u32x4 tv[K], td[K];
        bool oks[K];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int tx = (int)ix + d.pad_l - kx;
          const int ox = S == 2 ? tx >> 1 : tx;
          const bool ok = yok && tx >= 0 && (S == 1 || (tx & 1) == 0) && ox < d.OW;
          const unsigned opix = (b * (unsigned)d.OH + (unsigned)oy) * (unsigned)d.OW + (unsigned)ox;
          oks[kx] = ok;
          tv[kx] = __builtin_amdgcn_raw_buffer_load_b128(rv, ok ? opix * pix + cg * 16u : DW_OOB, 0, 0);
          td[kx] = __builtin_amdgcn_raw_buffer_load_b128(rd, ok ? opix * dz_pitch_bytes + cg * 16u : DW_OOB, 0, 0);
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          constexpr int centre = (K / 2) * K + K / 2;
          const int k = ky * K + kx;
          float vv[8], gz[8], wk[8];
          dw_unpack(tv[kx], vv);
          dw_unpack(td[kx], gz);
          dw_load8f(&wl[k][who.cgl * 8u], wk);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            gz[j] = oks[kx] ? ef_dswish(vv[j]) * (gz[j] * gt[j] + dpn[j]) : 0.f;      // (no output there: sw'(0) dp / HW is not zero)
            ds[j] += wk[j] * gz[j];
            G[k][j] += gz[j] * xa[j];
            if (k == centre) gb[j] += gz[j];                                         // the centre tap: every output exactly once
          }
        }
      }
      if (dx != nullptr) {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = slope[j] * sc[j] * ds[j];
        *(uint4*)((unsigned short*)dx + xe) = dw_pack(r);
      }
    }
  }

  // in parameter units: entries 0 .. KK-1 = s G (dL/dw), KK = rsqrt(var + eps) (sum_k w_k G_k - mean sum gz) (dL/dgamma: the
  // derivative of s u + beta - mean s, and sum gz u = sum_k w_k G_k), KK + 1 = sum gz (dL/dbeta)
  float dot[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dot[j] = 0.f;
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    float wk[8];
    dw_load8f(&wl[k][who.cgl * 8u], wk);
#pragma unroll
    for (int j = 0; j < 8; ++j) dot[j] += wk[j] * G[k][j];
  }
  // the workgroup's sum over pl, in pl order; row `chunk` of the partial matrix: [C][KK] weights | [C] gamma | [C] beta
  float* prow = partials + (size_t)who.chunk * NE * (unsigned)d.C;
  const unsigned CGB = who.CGB;
#pragma unroll
  for (int pass = 0; pass < (NE + DW_PASS - 1) / DW_PASS; ++pass) {
    __syncthreads();                                                     // the previous pass has been read
    if (who.active) {
#pragma unroll
      for (int el = 0; el < DW_PASS; ++el) {
        const int e = pass * DW_PASS + el;
        if (e < NE) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            red[el * 8 + j][threadIdx.x] = e < KK ? sc[j] * G[e < KK ? e : 0][j] : (e == KK ? rstd[j] * (dot[j] - mu[j] * gb[j]) : gb[j]);
        }
      }
    }
    __syncthreads();
    const int ne = min(DW_PASS, NE - pass * DW_PASS);
    const unsigned nout = (unsigned)ne * 8u * CGB;
    for (unsigned o = threadIdx.x; o < nout; o += 256u) {
      unsigned gl;
      const unsigned q = xpt_divmod(o, CGB, gl);                         // q = el * 8 + j
      float sum = 0.f;
      for (unsigned t = 0; t < who.PXT; ++t) sum += red[q][t * CGB + gl];
      const unsigned e = (unsigned)pass * DW_PASS + (q >> 3), c = (who.cb * CGB + gl) * 8u + (q & 7u);
      const unsigned at = e < (unsigned)KK ? c * KK + e : (e * (unsigned)d.C + c);   // KK C + c (gamma), (KK + 1) C + c (beta)
      prow[at] = sum;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
int ef_check_map(int B, int OH, int OW, int C) {
  if (B <= 0 || OH <= 0 || OW <= 0 || C <= 0) return XPT_ERR_SHAPE;
  if (C % 8 != 0) return XPT_ERR_ARG;                                    // 16-byte channel groups
  if ((long long)B * OH * OW * C * 2 >= (1LL << 31)) return XPT_ERR_SHAPE;
  return XPT_OK;
}

}  // namespace

extern "C" {

int xpt_dwconv_bn_swish_chunks(int B, int OH, int OW, int C) {
  if (B <= 0 || OH <= 0 || OW <= 0 || C <= 0 || C % 8 != 0) return 0;
  return dw_plan(B, OH, OW, C, EF_MAX_CGB).chunks;
}

int xpt_dwconv_bn_swish_fwd(const void* x, const float* w, const float* gamma, const float* beta, const float* mean,
                            const float* var, float eps, void* v, float* pool_partials, size_t pool_floats, int B, int H, int W,
                            int C, int k, int stride, int pad_t, int pad_l, int OH, int OW, int act_in, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(w); XPT_CHECK_PTR(gamma); XPT_CHECK_PTR(beta); XPT_CHECK_PTR(mean); XPT_CHECK_PTR(var);
  XPT_CHECK_PTR(v); XPT_CHECK_PTR(pool_partials);
  const DwDims d{B, H, W, C, OH, OW, pad_t, pad_l};
  const int rc = dw_check(d, k, stride);
  if (rc != XPT_OK) return rc;
  if (!dw_aligned(x) || !dw_aligned(v) || !dw_aligned(w)) return XPT_ERR_ARG;
  const DwPlan p = dw_plan(B, OH, OW, C, EF_MAX_CGB);
  if (pool_floats < (size_t)p.chunks * (size_t)C) return XPT_ERR_WORKSPACE;
  const unsigned nunits = (unsigned)p.chunks * (unsigned)p.ncb;
  const int on = g_xpt_xcd_affinity;
  const dim3 grid(on ? xpt_xcd_pad(nunits) : nunits);
  const unsigned xbytes = (unsigned)((long long)B * H * W * C * 2);
  const hipStream_t s = (hipStream_t)stream;
  XPT_BEGIN_LAUNCH();
#define EF_FWD(K_, S_, A_)                                                                                                      \
  hipLaunchKernelGGL((ef_dw_fwd_kernel<K_, S_, A_>), grid, dim3(256), 0, s, x, w, gamma, beta, mean, var, eps, v, pool_partials, d, p, \
                     xbytes, nunits, on)
#define EF_FWD_SA(K_)                                       \
  do {                                                      \
    if (stride == 1) {                                      \
      if (act_in) EF_FWD(K_, 1, 1); else EF_FWD(K_, 1, 0);  \
    } else {                                                \
      if (act_in) EF_FWD(K_, 2, 1); else EF_FWD(K_, 2, 0);  \
    }                                                       \
  } while (0)
  if (k == 3) EF_FWD_SA(3); else EF_FWD_SA(5);
#undef EF_FWD_SA
#undef EF_FWD
  return xpt_launch_status();
}

int xpt_se_excite_fwd(const float* pool_partials, int chunks_per_image, int HW, const float* w_reduce, const float* b_reduce,
                      const float* w_expand, const float* b_expand, float* p, float* r, float* gate, int B, int C, int S,
                      void* stream) {
  XPT_CHECK_PTR(pool_partials); XPT_CHECK_PTR(w_reduce); XPT_CHECK_PTR(b_reduce); XPT_CHECK_PTR(w_expand);
  XPT_CHECK_PTR(b_expand); XPT_CHECK_PTR(p); XPT_CHECK_PTR(r); XPT_CHECK_PTR(gate);
  if (B <= 0 || C <= 0 || S <= 0 || chunks_per_image <= 0 || HW <= 0) return XPT_ERR_SHAPE;
  if (C % 8 != 0) return XPT_ERR_ARG;
  if ((long long)C + S > EF_LDS_FLOATS) return XPT_ERR_SHAPE;
  if (!dw_aligned(gate)) return XPT_ERR_ARG;                            // (read with 16-byte loads by the scale and backward kernels)
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(ef_excite_fwd_kernel, dim3(B), dim3(256), (size_t)(C + S) * sizeof(float), (hipStream_t)stream,
                     pool_partials, chunks_per_image, 1.0f / (float)HW, w_reduce, b_reduce, w_expand, b_expand, p, r, gate, C, S);
  return xpt_launch_status();
}

int xpt_se_scale_fwd(const void* v, const float* gate, void* z, int B, int OH, int OW, int C, void* stream) {
  XPT_CHECK_PTR(v); XPT_CHECK_PTR(gate); XPT_CHECK_PTR(z);
  const int rc = ef_check_map(B, OH, OW, C);
  if (rc != XPT_OK) return rc;
  if (!dw_aligned(v) || !dw_aligned(z) || !dw_aligned(gate)) return XPT_ERR_ARG;
  const unsigned CG = (unsigned)C / 8u, total = (unsigned)B * (unsigned)OH * (unsigned)OW * CG;
  const unsigned nunits = (total + 255u) / 256u;
  const int on = g_xpt_xcd_affinity;
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(ef_scale_fwd_kernel, dim3(on ? xpt_xcd_pad(nunits) : nunits), dim3(256), 0, (hipStream_t)stream, v, gate, z,
                     total, CG, (unsigned)(OH * OW), nunits, on);
  return xpt_launch_status();
}

int xpt_se_scale_bwd_reduce(const void* v, const void* dz, long long dz_pitch, float* partials, size_t partial_floats,
                            float* dgate, int B, int OH, int OW, int C, void* stream) {
  XPT_CHECK_PTR(v); XPT_CHECK_PTR(dz); XPT_CHECK_PTR(partials); XPT_CHECK_PTR(dgate);
  const int rc = ef_check_map(B, OH, OW, C);
  if (rc != XPT_OK) return rc;
  if (dz_pitch < C || dz_pitch % 8 != 0) return XPT_ERR_SHAPE;
  if ((((long long)B * OH * OW - 1) * dz_pitch + C) * 2 >= (1LL << 31)) return XPT_ERR_SHAPE;
  if (!dw_aligned(v) || !dw_aligned(dz)) return XPT_ERR_ARG;
  const DwPlan p = dw_plan(B, OH, OW, C, EF_MAX_CGB);
  if (partial_floats < (size_t)p.chunks * (size_t)C) return XPT_ERR_WORKSPACE;
  const unsigned nunits = (unsigned)p.chunks * (unsigned)p.ncb;
  const int on = g_xpt_xcd_affinity;
  const hipStream_t s = (hipStream_t)stream;
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(ef_dgate_kernel, dim3(on ? xpt_xcd_pad(nunits) : nunits), dim3(256), 0, s, v, dz, (unsigned)dz_pitch, partials,
                     OH, OW, C, p, nunits, on);
  const unsigned total = (unsigned)B * (unsigned)C;
  hipLaunchKernelGGL(ef_finish_rows_kernel, dim3((total + 255u) / 256u), dim3(256), 0, s, partials, dgate, p.cpi, C, total);
  return xpt_launch_status();
}

int xpt_se_excite_bwd(const float* dgate, const float* gate, const float* p, const float* r, const float* w_reduce,
                      const float* w_expand, float* dw_reduce, float* db_reduce, float* dw_expand, float* db_expand, float* dp,
                      int B, int C, int S, void* stream) {
  XPT_CHECK_PTR(dgate); XPT_CHECK_PTR(gate); XPT_CHECK_PTR(p); XPT_CHECK_PTR(r); XPT_CHECK_PTR(w_reduce); XPT_CHECK_PTR(w_expand);
  XPT_CHECK_PTR(dw_reduce); XPT_CHECK_PTR(db_reduce); XPT_CHECK_PTR(dw_expand); XPT_CHECK_PTR(db_expand); XPT_CHECK_PTR(dp);
  if (B <= 0 || C <= 0 || S <= 0) return XPT_ERR_SHAPE;
  if (C % 8 != 0) return XPT_ERR_ARG;
  if (2LL * B * S > EF_LDS_FLOATS) return XPT_ERR_SHAPE;
  if (!dw_aligned(dp)) return XPT_ERR_ARG;                              // (read with 16-byte loads by the depthwise backward)
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(ef_excite_bwd_kernel, dim3((C + EF_CB - 1) / EF_CB), dim3(256), (size_t)2 * B * S * sizeof(float),
                     (hipStream_t)stream, dgate, gate, p, r, w_reduce, w_expand, dw_reduce, db_reduce, dw_expand, db_expand, dp, B,
                     C, S);
  return xpt_launch_status();
}

int xpt_dwconv_bn_swish_bwd(const void* x, const void* v, const void* dz, long long dz_pitch, const float* gate, const float* dp,
                            const float* w, const float* gamma, const float* mean, const float* var, float eps, void* dx,
                            float* partials, size_t partial_floats, int B, int H, int W, int C, int k, int stride, int pad_t,
                            int pad_l, int OH, int OW, int act_in, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(v); XPT_CHECK_PTR(dz); XPT_CHECK_PTR(gate); XPT_CHECK_PTR(dp); XPT_CHECK_PTR(w);
  XPT_CHECK_PTR(gamma); XPT_CHECK_PTR(mean); XPT_CHECK_PTR(var); XPT_CHECK_PTR(partials);
  const DwDims d{B, H, W, C, OH, OW, pad_t, pad_l};
  const int rc = dw_check(d, k, stride);
  if (rc != XPT_OK) return rc;
  if (dz_pitch < C || dz_pitch % 8 != 0) return XPT_ERR_SHAPE;
  const long long opix = (long long)B * OH * OW;
  const long long dzbytes = ((opix - 1) * dz_pitch + C) * 2, vbytes = opix * C * 2;
  if (dzbytes >= (1LL << 31)) return XPT_ERR_SHAPE;
  if (!dw_aligned(x) || !dw_aligned(v) || !dw_aligned(dz) || !dw_aligned(w) || !dw_aligned(gate) || !dw_aligned(dp)
      || (dx != nullptr && !dw_aligned(dx)))
    return XPT_ERR_ARG;
  const DwPlan p = dw_plan(B, OH, OW, C, EF_MAX_CGB);
  if (partial_floats < (size_t)p.chunks * (size_t)(k * k + 2) * (size_t)C) return XPT_ERR_WORKSPACE;
  const unsigned nunits = (unsigned)p.chunks * (unsigned)p.ncb;
  const int on = g_xpt_xcd_affinity;
  const dim3 grid(on ? xpt_xcd_pad(nunits) : nunits);
  const float inv_hw = 1.0f / (float)(OH * OW);
  const hipStream_t s = (hipStream_t)stream;
  XPT_BEGIN_LAUNCH();
#define EF_BWD(K_, S_, A_)                                                                                                       \
  hipLaunchKernelGGL((ef_dw_bwd_kernel<K_, S_, A_>), grid, dim3(256), 0, s, x, v, dz, (unsigned)(dz_pitch * 2), gate, dp, inv_hw, w, \
                     gamma, mean, var, eps, dx, partials, d, p, (unsigned)vbytes, (unsigned)dzbytes, nunits, on)
#define EF_BWD_SA(K_)                                       \
  do {                                                      \
    if (stride == 1) {                                      \
      if (act_in) EF_BWD(K_, 1, 1); else EF_BWD(K_, 1, 0);  \
    } else {                                                \
      if (act_in) EF_BWD(K_, 2, 1); else EF_BWD(K_, 2, 0);  \
    }                                                       \
  } while (0)
  if (k == 3) EF_BWD_SA(3); else EF_BWD_SA(5);
#undef EF_BWD_SA
#undef EF_BWD
  return xpt_launch_status();
}

}  // extern "C"
