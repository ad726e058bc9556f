// xpt_flowtail.hip -- PWC-Net's 2-channel layers (model/build_model/flow_net.py): the six Conv2D(2, 3, "same", linear) flow
// heads (_FlowEstimator.out, context[6]) and the eight Conv2DTranspose(2, 4, 2, "same") up-samplers (up_flow 2 -> 2, up_feat
// 32 -> 2), forward and the complete backward, as VALU kernels in the manner of xpt_headconv.hip.
//
// Two output channels: no matrix-core tile fits (30 of 32 MFMA rows would be zero).  Activations are read as 16-bit NHWC with
// a pixel pitch (the up-sampler also takes the fp32 2-channel flow, which the warp consumes unquantised), the fp32 master
// weights are read directly in their channels-last memory order and staged in LDS once per workgroup, results are fp32.
//   flow head    pre[p][n]      = bias[n] + sum_{tap,c} x[p + off(tap)][c] w[n][tap][c]                  w: [2][3][3][C]
//                dx[p][c]       = sum_{tap,n} g[p - off(tap)][n] w[n][tap][c]                             (16 bit, rounded once)
//                dW[n][tap][c]  = sum_p g[p - off(tap)][n] x[p][c],  db[n] = sum_p g[p][n]
//   up-sampler   y[2iy+py][2ix+px][n] = bias[n] + sum_{c, 2 x 2 taps} x[iy+dr][ix+dc][c] W[c][ky][kx][n]  W: [C][4][4][2]
//                  per output phase: ky = 1 (dr 0), 3 (dr -1) for py = 0; ky = 2 (dr 0), 0 (dr +1) for py = 1; the same in x.
//                  One lane group per INPUT pixel writes its 2 x 2 output block: nothing is zero-stuffed, no scratch tensor.
//                dx[iy][ix][c]  = sum_{n,ky,kx} g[2iy-1+ky][2ix-1+kx][n] W[c][ky][kx][n]                  (x's own format)
//                dW[c][ky][kx][n] = sum_pixels x[iy][ix][c] g[2iy-1+ky][2ix-1+kx][n],  db[n] = sum g[..][n]
// The backward of either operator is ONE launch; it writes per-workgroup partial rows (dW in the weight's memory layout, then
// the two bias sums) for the step's finishing launch (xpt_reduce_partials).  No atomics, fixed summation order, every output
// element written exactly once; out-of-range neighbours are unconditional loads from a clamped pixel, zeroed by a select.
#include "xpt_common.h"

namespace {

__device__ inline unsigned pack_h2(float a, float b) { return (unsigned)xpt_f2h(a) | ((unsigned)xpt_f2h(b) << 16); }
__device__ inline void unpack8(const uint4& v, float (&f)[8]) {
  f[0] = xpt_h2f_lo(v.x); f[1] = xpt_h2f_hi(v.x); f[2] = xpt_h2f_lo(v.y); f[3] = xpt_h2f_hi(v.y);
  f[4] = xpt_h2f_lo(v.z); f[5] = xpt_h2f_hi(v.z); f[6] = xpt_h2f_lo(v.w); f[7] = xpt_h2f_hi(v.w);
}

// CPL channels of one pixel: 16-bit (8 or 4 per lane, one 16- / 8-byte load) or fp32 (2 per lane, one 8-byte load);
// `off` in elements of x's type
template <int CPL, bool F32>
__device__ inline void load_channels(const void* __restrict__ x, long long off, bool ok, float (&f)[CPL]) {
  if constexpr (F32) {
    static_assert(CPL == 2, "fp32 input: 2 channels");
    const float2 v = *(const float2*)((const float*)x + off);
    f[0] = ok ? v.x : 0.f; f[1] = ok ? v.y : 0.f;
  } else if constexpr (CPL == 8) {
    const uint4 ld = *(const uint4*)((const unsigned short*)x + off);
    unpack8(ok ? ld : make_uint4(0u, 0u, 0u, 0u), f);
  } else {
    static_assert(CPL == 4, "16-bit input: 8 or 4 channels per lane");
    uint2 v = *(const uint2*)((const unsigned short*)x + off);
    if (!ok) v = make_uint2(0u, 0u);
    f[0] = xpt_h2f_lo(v.x); f[1] = xpt_h2f_hi(v.x); f[2] = xpt_h2f_lo(v.y); f[3] = xpt_h2f_hi(v.y);
  }
}

// ------------------------------------------------------------------------------------------------ flow head
// LPP lanes share one pixel (8 channels each); a wave covers 64 / LPP consecutive pixels
template <int LPP>
__global__ __launch_bounds__(256) void flowhead_fwd_kernel(const unsigned short* __restrict__ x, long long xpitch,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            float2* __restrict__ pre, int B, int H, int W) {
  constexpr int C = 8 * LPP, PPW = 64 / LPP;
  __shared__ float sw[18 * C];
  for (int i = threadIdx.x; i < 18 * C; i += 256) sw[i] = w[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane % LPP, pl = lane / LPP;
  const long long P = (long long)B * H * W;
  const float b0 = bias ? bias[0] : 0.f, b1 = bias ? bias[1] : 0.f;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
  for (long long p0 = wave * PPW; p0 < P; p0 += nwaves * PPW) {
    const long long p = p0 + pl;
    const bool live = p < P;
    const long long pc = live ? p : P - 1;
    unsigned colu, rowu;                          // (P < 2^31, H and W < 2^24: the launcher checks)
    xpt_divmod(xpt_divmod((unsigned)pc, (unsigned)W, colu), (unsigned)H, rowu);
    const int col = (int)colu, row = (int)rowu;
    uint4 v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dr = t / 3 - 1, dc = t % 3 - 1;
      const bool ok = row + dr >= 0 && row + dr < H && col + dc >= 0 && col + dc < W;
      const long long q = ok ? pc + (long long)dr * W + dc : pc;
      const uint4 ld = *(const uint4*)(x + q * xpitch + 8 * sub);
      v[t] = ok ? ld : make_uint4(0u, 0u, 0u, 0u);
    }
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      float f[8];
      unpack8(v[t], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a0 = fmaf(f[e], sw[t * C + 8 * sub + e], a0);
        a1 = fmaf(f[e], sw[(9 + t) * C + 8 * sub + e], a1);
      }
    }
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) {
      a0 += __shfl_xor(a0, o, 64);
      a1 += __shfl_xor(a1, o, 64);
    }
    if (live && sub == 0) pre[p] = make_float2(a0 + b0, a1 + b1);
  }
}

template <int LPP>
__global__ __launch_bounds__(256) void flowhead_bwd_kernel(const unsigned short* __restrict__ x, long long xpitch,
                                                            const float* __restrict__ w, const float2* __restrict__ g,
                                                            unsigned short* __restrict__ dx, float* __restrict__ partials,
                                                            int B, int H, int W) {
  constexpr int C = 8 * LPP, PPW = 64 / LPP, ROW = 18 * C + 2;
  __shared__ float sw[18 * C];
  __shared__ float red[4][ROW];
  for (int i = threadIdx.x; i < 18 * C; i += 256) sw[i] = w[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane % LPP, pl = lane / LPP;
  const long long P = (long long)B * H * W;
  float dw[2][9][8];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) dw[n][t][e] = 0.f;
  float db0 = 0.f, db1 = 0.f;
  const long long wave = (long long)blockIdx.x * 4 + wv, nwaves = (long long)gridDim.x * 4;
  for (long long p0 = wave * PPW; p0 < P; p0 += nwaves * PPW) {
    const long long p = p0 + pl;
    const bool live = p < P;
    const long long pc = live ? p : P - 1;
    unsigned colu, rowu;
    xpt_divmod(xpt_divmod((unsigned)pc, (unsigned)W, colu), (unsigned)H, rowu);
    const int col = (int)colu, row = (int)rowu;
    // both gradients from the MIRRORED neighbours of g (8-byte loads that hit the cache) and ONE 16-byte load of this
    // pixel's features, as in xpt_headconv.hip
    float2 gn[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dr = t / 3 - 1, dc = t % 3 - 1;
      const bool ok2 = live && row - dr >= 0 && row - dr < H && col - dc >= 0 && col - dc < W;
      const long long q2 = ok2 ? pc - (long long)dr * W - dc : pc;
      const float2 gl = g[q2];
      gn[t] = ok2 ? gl : make_float2(0.f, 0.f);
    }
    if (sub == 0) { db0 += gn[4].x; db1 += gn[4].y; }      // tap 4 is the pixel itself (zero for a dead lane)
    float fc[8];
    unpack8(*(const uint4*)(x + pc * xpitch + 8 * sub), fc);
    float d[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        dw[0][t][e] = fmaf(gn[t].x, fc[e], dw[0][t][e]);
        dw[1][t][e] = fmaf(gn[t].y, fc[e], dw[1][t][e]);
        d[e] = fmaf(gn[t].x, sw[t * C + 8 * sub + e], d[e]);
        d[e] = fmaf(gn[t].y, sw[(9 + t) * C + 8 * sub + e], d[e]);
      }
    }
    if (live) {
      uint4 o;
      o.x = pack_h2(d[0], d[1]); o.y = pack_h2(d[2], d[3]); o.z = pack_h2(d[4], d[5]); o.w = pack_h2(d[6], d[7]);
      *(uint4*)(dx + p * C + 8 * sub) = o;
    }
  }
  // wave sum over its PPW pixel slots (lanes with equal `sub`), then the 4 waves through LDS, in wave order
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int o = LPP; o < 64; o <<= 1) dw[n][t][e] += __shfl_xor(dw[n][t][e], o, 64);
#pragma unroll
  for (int o = LPP; o < 64; o <<= 1) {
    db0 += __shfl_xor(db0, o, 64);
    db1 += __shfl_xor(db1, o, 64);
  }
  if (pl == 0) {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wv][(n * 9 + t) * C + 8 * sub + e] = dw[n][t][e];
    if (sub == 0) { red[wv][18 * C] = db0; red[wv][18 * C + 1] = db1; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ROW; i += 256)
    partials[(long long)blockIdx.x * ROW + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// ------------------------------------------------------------------------------------------------ transposed up-sampler
// weight image in LDS: channel c at float offset 32 c + 4 (c / CPL) -- the lanes of one pixel read different channel groups
// with 16-byte LDS loads; the 4-float step between groups keeps them on different banks
template <int CPL>
__device__ inline int wofs(int c) { return 32 * c + 4 * (c / CPL); }

// kernel row ky -> (output phase py, input row offset dr); the same map serves the columns
__device__ constexpr int tap_phase(int k) { return (k == 0 || k == 2) ? 1 : 0; }
__device__ constexpr int tap_offset(int k) { return k == 0 ? 1 : (k == 3 ? -1 : 0); }

template <int LPP, bool F32>
__global__ __launch_bounds__(256) void upconv_fwd_kernel(const void* __restrict__ x, long long xpitch,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ y, int B, int H, int W) {
  constexpr int CPL = F32 ? 2 : 8, C = CPL * LPP, PPW = 64 / LPP;
  __shared__ float4 sw4[(32 * C + 4 * LPP) / 4];
  float* sw = (float*)sw4;
  for (int i = threadIdx.x; i < 32 * C; i += 256) sw[wofs<CPL>(i >> 5) + (i & 31)] = w[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane % LPP, pl = lane / LPP;
  const long long P = (long long)B * H * W;
  const float b0 = bias ? bias[0] : 0.f, b1 = bias ? bias[1] : 0.f;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
  for (long long p0 = wave * PPW; p0 < P; p0 += nwaves * PPW) {
    const long long p = p0 + pl;
    const bool live = p < P;
    const long long pc = live ? p : P - 1;
    unsigned colu, rowu;
    const unsigned img = xpt_divmod(xpt_divmod((unsigned)pc, (unsigned)W, colu), (unsigned)H, rowu);
    const int col = (int)colu, row = (int)rowu;
    float f[9][CPL];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dr = t / 3 - 1, dc = t % 3 - 1;
      const bool ok = row + dr >= 0 && row + dr < H && col + dc >= 0 && col + dc < W;
      const long long q = ok ? pc + (long long)dr * W + dc : pc;
      load_channels<CPL, F32>(x, q * xpitch + CPL * sub, ok, f[t]);
    }
    float acc[2][2][2];                           // [py][px][n]
#pragma unroll
    for (int i = 0; i < 8; ++i) (&acc[0][0][0])[i] = 0.f;
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
      const float4* wc = (const float4*)(sw + wofs<CPL>(CPL * sub + e));
#pragma unroll
      for (int ky = 0; ky < 4; ++ky) {
        const float4 wa = wc[2 * ky], wb = wc[2 * ky + 1];            // (kx0 n0, kx0 n1, kx1 n0, kx1 n1), (kx2 .., kx3 ..)
        const float wk[4][2] = {{wa.x, wa.y}, {wa.z, wa.w}, {wb.x, wb.y}, {wb.z, wb.w}};
        const int py = tap_phase(ky), dr = tap_offset(ky);
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
          const int px = tap_phase(kx), dc = tap_offset(kx);
          const float xv = f[(dr + 1) * 3 + dc + 1][e];
          acc[py][px][0] = fmaf(xv, wk[kx][0], acc[py][px][0]);
          acc[py][px][1] = fmaf(xv, wk[kx][1], acc[py][px][1]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int o = 1; o < LPP; o <<= 1) (&acc[0][0][0])[i] += __shfl_xor((&acc[0][0][0])[i], o, 64);
    if (live && sub == 0) {
#pragma unroll
      for (int py = 0; py < 2; ++py) {                                // two output pixels of one row: one 16-byte store
        const long long op = ((long long)img * 2 * H + 2 * row + py) * 2 * W + 2 * col;
        *(float4*)(y + 2 * op) = make_float4(acc[py][0][0] + b0, acc[py][0][1] + b1, acc[py][1][0] + b0, acc[py][1][1] + b1);
      }
    }
  }
}

// backward: 4 channels per lane in the 16-bit format (32 weight-gradient accumulators per channel stay in registers)
template <int LPP, bool F32>
__global__ __launch_bounds__(256) void upconv_bwd_kernel(const void* __restrict__ x, long long xpitch,
                                                          const float* __restrict__ w, const float2* __restrict__ g,
                                                          void* __restrict__ dx, float* __restrict__ partials, int B, int H,
                                                          int W) {
  constexpr int CPL = F32 ? 2 : 4, C = CPL * LPP, PPW = 64 / LPP, ROW = 32 * C + 2;
  __shared__ float4 sw4[(32 * C + 4 * LPP) / 4];
  __shared__ float red[4][ROW];
  float* sw = (float*)sw4;
  for (int i = threadIdx.x; i < 32 * C; i += 256) sw[wofs<CPL>(i >> 5) + (i & 31)] = w[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane % LPP, pl = lane / LPP;
  const long long P = (long long)B * H * W;
  float dw[CPL][32];
#pragma unroll
  for (int e = 0; e < CPL; ++e)
#pragma unroll
    for (int i = 0; i < 32; ++i) dw[e][i] = 0.f;
  float db0 = 0.f, db1 = 0.f;
  const long long wave = (long long)blockIdx.x * 4 + wv, nwaves = (long long)gridDim.x * 4;
  for (long long p0 = wave * PPW; p0 < P; p0 += nwaves * PPW) {
    const long long p = p0 + pl;
    const bool live = p < P;
    const long long pc = live ? p : P - 1;
    unsigned colu, rowu;
    const unsigned img = xpt_divmod(xpt_divmod((unsigned)pc, (unsigned)W, colu), (unsigned)H, rowu);
    const int col = (int)colu, row = (int)rowu;
    // the 4 x 4 window of g that this input pixel touched: rows 2 row - 1 + ky, columns 2 col - 1 + kx
    const long long own = ((long long)img * 2 * H + 2 * row) * 2 * W + 2 * col;       // (ky, kx) = (1, 1): always in range
    float2 gw[4][4];
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        const int oy = 2 * row - 1 + ky, ox = 2 * col - 1 + kx;
        const bool ok = live && oy >= 0 && oy < 2 * H && ox >= 0 && ox < 2 * W;
        const long long q = ok ? own + (long long)(ky - 1) * 2 * W + (kx - 1) : own;
        const float2 gl = g[q];
        gw[ky][kx] = ok ? gl : make_float2(0.f, 0.f);
      }
    if (sub == 0) {                               // every output pixel belongs to exactly one input pixel's 2 x 2 block
      db0 += (gw[1][1].x + gw[1][2].x) + (gw[2][1].x + gw[2][2].x);
      db1 += (gw[1][1].y + gw[1][2].y) + (gw[2][1].y + gw[2][2].y);
    }
    float fc[CPL];
    load_channels<CPL, F32>(x, pc * xpitch + CPL * sub, true, fc);
    float d[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
      const float4* wc = (const float4*)(sw + wofs<CPL>(CPL * sub + e));
      float s = 0.f;
#pragma unroll
      for (int ky = 0; ky < 4; ++ky) {
        const float4 wa = wc[2 * ky], wb = wc[2 * ky + 1];
        const float wk[4][2] = {{wa.x, wa.y}, {wa.z, wa.w}, {wb.x, wb.y}, {wb.z, wb.w}};
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
          dw[e][ky * 8 + kx * 2] = fmaf(fc[e], gw[ky][kx].x, dw[e][ky * 8 + kx * 2]);
          dw[e][ky * 8 + kx * 2 + 1] = fmaf(fc[e], gw[ky][kx].y, dw[e][ky * 8 + kx * 2 + 1]);
          s = fmaf(gw[ky][kx].x, wk[kx][0], s);
          s = fmaf(gw[ky][kx].y, wk[kx][1], s);
        }
      }
      d[e] = s;
    }
    if (live) {
      if constexpr (F32) {
        *(float2*)((float*)dx + p * C + CPL * sub) = make_float2(d[0], d[1]);
      } else {
        *(uint2*)((unsigned short*)dx + p * C + CPL * sub) = make_uint2(pack_h2(d[0], d[1]), pack_h2(d[2], d[3]));
      }
    }
  }
#pragma unroll
  for (int e = 0; e < CPL; ++e)
#pragma unroll
    for (int i = 0; i < 32; ++i)
#pragma unroll
      for (int o = LPP; o < 64; o <<= 1) dw[e][i] += __shfl_xor(dw[e][i], o, 64);
#pragma unroll
  for (int o = LPP; o < 64; o <<= 1) {
    db0 += __shfl_xor(db0, o, 64);
    db1 += __shfl_xor(db1, o, 64);
  }
  if (pl == 0) {
#pragma unroll
    for (int e = 0; e < CPL; ++e)
#pragma unroll
      for (int i = 0; i < 32; ++i) red[wv][32 * (CPL * sub + e) + i] = dw[e][i];
    if (sub == 0) { red[wv][32 * C] = db0; red[wv][32 * C + 1] = db1; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ROW; i += 256)
    partials[(long long)blockIdx.x * ROW + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// ------------------------------------------------------------------------------------------------ launch plans
constexpr int kMaxBlocks = 512;

int plan_blocks(long long P, int lanes_per_pixel, int passes) {
  const long long ppb = 4 * (64 / lanes_per_pixel);    // pixels per workgroup pass
  long long blocks = (P + ppb * passes - 1) / (ppb * passes);
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

int fwd_blocks(long long P, int lanes_per_pixel) {
  const long long ppb = 4 * (64 / lanes_per_pixel);
  long long blocks = (P + ppb - 1) / ppb;
  if (blocks > 2048) blocks = 2048;
  return (int)blocks;
}

bool head_channels_ok(int C) { return C == 16 || C == 32 || C == 64 || C == 128; }
bool up_channels_ok(int C, int x_fp32) { return x_fp32 ? C == 2 : (C == 8 || C == 16 || C == 32); }
bool extents_ok(int B, int H, int W, long long scale) {
  return B > 0 && H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24) && (long long)B * H * W * scale < 0x7fffffffLL;
}
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p) % a == 0; }
int up_bwd_lanes(int C, int x_fp32) { return x_fp32 ? 1 : C / 4; }

}  // namespace

extern "C" int xpt_flowhead_bwd_blocks(int B, int H, int W, int C) {
  if (!extents_ok(B, H, W, 1) || !head_channels_ok(C)) return 0;
  return plan_blocks((long long)B * H * W, C / 8, 4);
}

extern "C" int xpt_flowhead_fwd(const void* x, long long xpitch, const float* w, const float* bias, float* pre, int B, int H,
                                int W, int C, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(w); XPT_CHECK_PTR(pre);
  if (!extents_ok(B, H, W, 1)) return XPT_ERR_SHAPE;
  if (!head_channels_ok(C) || xpitch < C || xpitch % 8 != 0 || !aligned(x, 16) || !aligned(w, 4) || !aligned(pre, 8) ||
      !aligned(bias, 4))
    return XPT_ERR_ARG;
  const int blocks = fwd_blocks((long long)B * H * W, C / 8);
  hipStream_t s = (hipStream_t)stream;
  const unsigned short* xp = (const unsigned short*)x;
  float2* pp = (float2*)pre;
  XPT_BEGIN_LAUNCH();
  switch (C / 8) {
    case 2: hipLaunchKernelGGL(flowhead_fwd_kernel<2>, dim3(blocks), dim3(256), 0, s, xp, xpitch, w, bias, pp, B, H, W); break;
    case 4: hipLaunchKernelGGL(flowhead_fwd_kernel<4>, dim3(blocks), dim3(256), 0, s, xp, xpitch, w, bias, pp, B, H, W); break;
    case 8: hipLaunchKernelGGL(flowhead_fwd_kernel<8>, dim3(blocks), dim3(256), 0, s, xp, xpitch, w, bias, pp, B, H, W); break;
    default: hipLaunchKernelGGL(flowhead_fwd_kernel<16>, dim3(blocks), dim3(256), 0, s, xp, xpitch, w, bias, pp, B, H, W); break;
  }
  return xpt_launch_status();
}

extern "C" int xpt_flowhead_bwd(const void* x, long long xpitch, const float* w, const float* g, void* dx, float* partials,
                                size_t partial_floats, int B, int H, int W, int C, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(w); XPT_CHECK_PTR(g); XPT_CHECK_PTR(dx); XPT_CHECK_PTR(partials);
  if (!extents_ok(B, H, W, 1)) return XPT_ERR_SHAPE;
  if (!head_channels_ok(C) || xpitch < C || xpitch % 8 != 0 || !aligned(x, 16) || !aligned(dx, 16) || !aligned(g, 8) ||
      !aligned(w, 4) || !aligned(partials, 4))
    return XPT_ERR_ARG;
  const int blocks = plan_blocks((long long)B * H * W, C / 8, 4);
  if (partial_floats < (size_t)blocks * (18 * C + 2)) return XPT_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const unsigned short* xp = (const unsigned short*)x;
  const float2* gp = (const float2*)g;
  unsigned short* dxp = (unsigned short*)dx;
  XPT_BEGIN_LAUNCH();
  switch (C / 8) {
    case 2: hipLaunchKernelGGL(flowhead_bwd_kernel<2>, dim3(blocks), dim3(256), 0, s, xp, xpitch, w, gp, dxp, partials, B, H, W); break;
    case 4: hipLaunchKernelGGL(flowhead_bwd_kernel<4>, dim3(blocks), dim3(256), 0, s, xp, xpitch, w, gp, dxp, partials, B, H, W); break;
    case 8: hipLaunchKernelGGL(flowhead_bwd_kernel<8>, dim3(blocks), dim3(256), 0, s, xp, xpitch, w, gp, dxp, partials, B, H, W); break;
    default: hipLaunchKernelGGL(flowhead_bwd_kernel<16>, dim3(blocks), dim3(256), 0, s, xp, xpitch, w, gp, dxp, partials, B, H, W); break;
  }
  return xpt_launch_status();
}

extern "C" int xpt_upconv4x4s2_bwd_blocks(int B, int H, int W, int C, int x_fp32) {
  if (!extents_ok(B, H, W, 4) || (x_fp32 != 0 && x_fp32 != 1) || !up_channels_ok(C, x_fp32)) return 0;
  return plan_blocks((long long)B * H * W, up_bwd_lanes(C, x_fp32), 2);
}

extern "C" int xpt_upconv4x4s2_fwd(const void* x, long long xpitch, int x_fp32, const float* w, const float* bias, float* y,
                                   int B, int H, int W, int C, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(w); XPT_CHECK_PTR(y);
  if (!extents_ok(B, H, W, 4)) return XPT_ERR_SHAPE;       // (the OUTPUT pixel count stays below 2^31)
  if ((x_fp32 != 0 && x_fp32 != 1) || !up_channels_ok(C, x_fp32) || !aligned(y, 16) || !aligned(w, 4) || !aligned(bias, 4))
    return XPT_ERR_ARG;
  if (x_fp32 ? (xpitch != 2 || !aligned(x, 8)) : (xpitch < C || xpitch % 8 != 0 || !aligned(x, 16))) return XPT_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long long P = (long long)B * H * W;
  XPT_BEGIN_LAUNCH();
  if (x_fp32) {
    hipLaunchKernelGGL((upconv_fwd_kernel<1, true>), dim3(fwd_blocks(P, 1)), dim3(256), 0, s, x, xpitch, w, bias, y, B, H, W);
  } else {
    const int blocks = fwd_blocks(P, C / 8);
    switch (C / 8) {
      case 1: hipLaunchKernelGGL((upconv_fwd_kernel<1, false>), dim3(blocks), dim3(256), 0, s, x, xpitch, w, bias, y, B, H, W); break;
      case 2: hipLaunchKernelGGL((upconv_fwd_kernel<2, false>), dim3(blocks), dim3(256), 0, s, x, xpitch, w, bias, y, B, H, W); break;
      default: hipLaunchKernelGGL((upconv_fwd_kernel<4, false>), dim3(blocks), dim3(256), 0, s, x, xpitch, w, bias, y, B, H, W); break;
    }
  }
  return xpt_launch_status();
}

extern "C" int xpt_upconv4x4s2_bwd(const void* x, long long xpitch, int x_fp32, const float* w, const float* g, void* dx,
                                   float* partials, size_t partial_floats, int B, int H, int W, int C, void* stream) {
  XPT_CHECK_PTR(x); XPT_CHECK_PTR(w); XPT_CHECK_PTR(g); XPT_CHECK_PTR(dx); XPT_CHECK_PTR(partials);
  if (!extents_ok(B, H, W, 4)) return XPT_ERR_SHAPE;
  if ((x_fp32 != 0 && x_fp32 != 1) || !up_channels_ok(C, x_fp32) || !aligned(g, 8) || !aligned(w, 4) || !aligned(partials, 4))
    return XPT_ERR_ARG;
  if (x_fp32 ? (xpitch != 2 || !aligned(x, 8) || !aligned(dx, 8)) : (xpitch < C || xpitch % 8 != 0 || !aligned(x, 16) || !aligned(dx, 16)))
    return XPT_ERR_ARG;
  const long long P = (long long)B * H * W;
  const int blocks = plan_blocks(P, up_bwd_lanes(C, x_fp32), 2);
  if (partial_floats < (size_t)blocks * (32 * C + 2)) return XPT_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const float2* gp = (const float2*)g;
  XPT_BEGIN_LAUNCH();
  if (x_fp32) {
    hipLaunchKernelGGL((upconv_bwd_kernel<1, true>), dim3(blocks), dim3(256), 0, s, x, xpitch, w, gp, dx, partials, B, H, W);
  } else {
    switch (C / 4) {
      case 2: hipLaunchKernelGGL((upconv_bwd_kernel<2, false>), dim3(blocks), dim3(256), 0, s, x, xpitch, w, gp, dx, partials, B, H, W); break;
      case 4: hipLaunchKernelGGL((upconv_bwd_kernel<4, false>), dim3(blocks), dim3(256), 0, s, x, xpitch, w, gp, dx, partials, B, H, W); break;
      default: hipLaunchKernelGGL((upconv_bwd_kernel<8, false>), dim3(blocks), dim3(256), 0, s, x, xpitch, w, gp, dx, partials, B, H, W); break;
    }
  }
  return xpt_launch_status();
}
