// xpt_conv_dilated.hip -- dilated 3 x 3 convolutions (stride 1, TF SAME: `dilation` zeros on every side) on the gfx950 matrix
// cores: forward (+ bias + LeakyReLU), data gradient and split-K weight-gradient partials.
//
// Replaces keras Conv2D(filters, 3, padding="same", dilation_rate=d) as PWC-Net's context network builds it
// (model/build_model/flow_net.py: context[1..4] = 128 -> 128 d=2, 128 -> 128 d=4, 128 -> 96 d=8, 96 -> 64 d=16 on the
// quarter-resolution map) and tape.gradient of those layers.  Operands are those of the undilated kernels (xpt_conv.hip,
// xpt_conv_wgrad.hip): NHWC 16-bit activations with a pixel pitch, the packer's fwd [N][9][Cp] / bwd [Cp][9][Np] weights, fp32
// bias, fp32 partials [splits][N][3][3][Cr] for xpt_reduce_partials.
//
// Forward / data gradient: the direct, no-LDS implicit GEMM of conv_igemm_kernel -- lane (r = lane & 31, h = lane >> 5) holds
// A[row r][8h..8h+7] (packed weights) and B[8h..8h+7][pixel r] (activations), every fragment ONE 16-byte global load whose tap
// address is computed per fragment (t = o + (k - 1) d forward, t = o - (k - 1) d for the gradient on the bwd packing); an
// out-of-range tap is zeros.  A halo tile does not fit (d = 16: 32 pixels on each side), and it is not needed: the taps of one
// pixel are 9 scattered 16-byte rows whatever d is.  Before the K loop the wave votes which of the 9 taps are in range for ANY
// of its pixels and walks only those: with d >= H only the centre tap row survives (3 of 9 taps), at d = 16 on a 32-row map
// half of the rows of every off-centre tap row do not exist.
//
// Weight gradient: dW[n][kh][kw][c] = sum_m g[m][n] x[pixel(m, kh, kw)][c].  The reduction index (pixels) is the slow axis of
// both operands, so, as in conv_wgrad_kernel, tiles are staged row-major in LDS and read back transposed (ds_read_b64_tr_b16).
// A workgroup owns a 64 x 64 (output x input channel) block of dW for all 9 taps; a pixel unit is 32 consecutive columns of ONE
// output row, for which the g tile [32][64] and, per live tap, the shifted x tile [32][64] are staged (9 x 4 KiB + 4 KiB of
// LDS whatever the dilation is: a halo would be (32 + 2 d) x (1 + 2 d) pixels).  Taps whose row, or whose every column, is out
// of range for the unit are neither staged nor multiplied.  Split s takes the units s, s + splits, ... in that order and
// writes its sum as one fp32 partial: fixed summation order, no atomics.
#include "xpt_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef xpt_h16x8 h16x8;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

struct DilArgs {
  const unsigned short* x;   // NHWC activations [B,H,W,C], pixel pitch xpitch elements
  const unsigned short* w;   // packed weights [N][9][C]
  const float* bias;         // [N] or null
  unsigned short* y;         // NHWC output [B,H,W,N], pixel pitch ypitch elements
  long long xpitch, ypitch;
  int B, H, W, C, N;
  int step;                  // +dilation (forward: t = o + (k - 1) d) / -dilation (data gradient: t = o - (k - 1) d)
  float slope;
};

template <int RM, int RN>
__global__ __launch_bounds__(256) void dil_igemm_kernel(DilArgs a) {
  constexpr int G = 4;                           // k-steps whose loads are in flight together
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const long long M = (long long)a.B * a.H * a.W;
  const long long m0 = ((long long)blockIdx.y * 4 + wave) * (32 * RN);
  const int n0 = blockIdx.x * (32 * RM);
  if (m0 >= M) return;                           // uniform per wave; no barrier below

  // ---- per-lane pixel geometry (columns of the B operand); input and output maps coincide (stride 1, SAME)
  int poh[RN], pow_[RN];
  long long pimg[RN];                            // first pixel of the lane's image
  bool pok[RN];
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    long long m = m0 + 32 * j + r;
    pok[j] = m < M;
    if (!pok[j]) m = M - 1;
    unsigned c_, rr_;                            // (pixel index below 2^31: the launcher checks)
    const unsigned q_ = xpt_divmod((unsigned)m, (unsigned)a.W, c_);
    const unsigned b_ = xpt_divmod(q_, (unsigned)a.H, rr_);
    poh[j] = (int)rr_;
    pow_[j] = (int)c_;
    pimg[j] = (long long)b_ * a.H * a.W;
  }
  // ---- taps that are in range for at least one pixel of this wave's tile (wave-uniform 9-bit mask, centre always set)
  unsigned mine = 0;
#pragma unroll
  for (int j = 0; j < RN; ++j) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int th = poh[j] + (t / 3 - 1) * a.step, tw = pow_[j] + (t % 3 - 1) * a.step;
      if (pok[j] && th >= 0 && th < a.H && tw >= 0 && tw < a.W) mine |= 1u << t;
    }
  }
  unsigned mask = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t)
    if (__ballot((mine >> t) & 1u) != 0ull) mask |= 1u << t;
  mask = (unsigned)__builtin_amdgcn_readfirstlane((int)mask);

  // ---- weight rows (rows of the A operand)
  const unsigned short* wrow[RM];
  bool nok[RM];
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    const int n = n0 + 32 * i + r;
    nok[i] = n < a.N;
    wrow[i] = a.w + (long long)(nok[i] ? n : a.N - 1) * 9 * a.C;
  }

  f32x16 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  const int csteps = (a.C + 15) >> 4;
  const int nsteps = __builtin_popcount(mask) * csteps;
  // running (tap, channel step) of the NEXT step to issue
  unsigned rem = mask;
  int tap = rem ? __builtin_ctz(rem) : 0, cs = 0;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  for (int s0 = 0; s0 < nsteps; s0 += G) {
    uint4 fa[G][RM], fb[G][RN];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const bool in = s0 + g < nsteps;                         // steps past the range load from offset 0 and are zeroed
      const int kh = tap / 3, kw = tap - 3 * kh;
      const int c0 = cs * 16 + 8 * h;
      const bool live = in && c0 < a.C;
      const int cc = live ? c0 : 0;
      const long long woff = (long long)tap * a.C + cc;
#pragma unroll
      for (int i = 0; i < RM; ++i) {
        const uint4 v = *(const uint4*)(wrow[i] + woff);
        fa[g][i] = (live && nok[i]) ? v : zero4;
      }
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        const int th = poh[j] + (kh - 1) * a.step, tw = pow_[j] + (kw - 1) * a.step;
        const bool ok = live && pok[j] && th >= 0 && th < a.H && tw >= 0 && tw < a.W;
        const long long xoff = (pimg[j] + (long long)th * a.W + tw) * a.xpitch + cc;
        const uint4 v = *(const uint4*)(a.x + (ok ? xoff : 0));
        fb[g][j] = ok ? v : zero4;
      }
      if (in && ++cs == csteps) {                              // advance to the next step (scalar state)
        cs = 0;
        rem &= rem - 1;
        tap = rem ? __builtin_ctz(rem) : 0;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (s0 + g < nsteps) {                                   // wave-uniform
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j)
            acc[i][j] = XPT_MFMA_32X32X16(__builtin_bit_cast(h16x8, fa[g][i]), __builtin_bit_cast(h16x8, fb[g][j]), acc[i][j]);
      }
    }
  }

  // ---- epilogue.  Register q of tile (i, j): channel n0 + 32 i + (q & 3) + 8 (q >> 2) + 4 h, pixel m0 + 32 j + r
  // (N % 8 == 0, ypitch % 8 == 0 and y 16-byte aligned -- the entry points check --: groups of 4 channels as 8-byte stores)
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    if (!pok[j]) continue;
    const long long opix = m0 + 32 * j + r;
#pragma unroll
    for (int i = 0; i < RM; ++i) {
#pragma unroll
      for (int qg = 0; qg < 4; ++qg) {
        const int n = n0 + 32 * i + 8 * qg + 4 * h;
        if (n >= a.N) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[i][j][4 * qg + e];
          if (a.bias != nullptr) v[e] += a.bias[n + e];
          v[e] = v[e] > 0.f ? v[e] : v[e] * a.slope;
        }
        uint2 pk;
        pk.x = (unsigned)xpt_f2h(v[0]) | ((unsigned)xpt_f2h(v[1]) << 16);
        pk.y = (unsigned)xpt_f2h(v[2]) | ((unsigned)xpt_f2h(v[3]) << 16);
        *(uint2*)(a.y + opix * a.ypitch + n) = pk;
      }
    }
  }
}

template <int RM, int RN>
int launch_dil(const DilArgs& a, hipStream_t s) {
  const long long M = (long long)a.B * a.H * a.W;
  const long long mtiles = (M + 32 * RN - 1) / (32 * RN);
  const long long gy = (mtiles + 3) / 4;
  if (gy > 65535 || M >= 0x7fffffffLL) return XPT_ERR_SHAPE;
  const dim3 grid((a.N + 32 * RM - 1) / (32 * RM), (unsigned)gy);
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL((dil_igemm_kernel<RM, RN>), grid, dim3(256), 0, s, a);
  return xpt_launch_status();
}

int dispatch_dil(const DilArgs& a, hipStream_t s) {
  // 64 x 64 wave tiles (4 MFMAs per 4 fragment loads) when the output has two 32-channel tiles and the launch still has a
  // few waves per SIMD; otherwise 32 x 64
  const long long M = (long long)a.B * a.H * a.W;
  const long long waves22 = ((a.N + 63) / 64) * ((M + 63) / 64);
  if (a.N > 32 && waves22 >= 768) return launch_dil<2, 2>(a, s);
  return launch_dil<1, 2>(a, s);
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int DW_CB = 32, DW_TNB = 64, DW_TCB = 64;            // unit columns, block of output / input channels
constexpr int DW_TILE = DW_CB * 64 * 2;                        // bytes of one staged [32 pixels][64 channels] tile

struct DilWgradArgs {
  const unsigned short* g;   // [B,H,W,N], pixel pitch gpitch
  const unsigned short* x;   // [B,H,W,C], pixel pitch xpitch (C readable channels, the first Cr are weight channels)
  float* part;               // [nsplit][N][9][Cr] fp32
  long long gpitch, xpitch;
  int B, H, W, C, Cr, N, d;
  int nseg, units, nsplit, ntc;
};

__device__ inline h16x8 dil_tr_pair(const char* lds, unsigned off0, unsigned off1) {
  typedef s16x4 __attribute__((address_space(3))) * lds_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(lds + off0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(lds + off1));
  s16x8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(h16x8, v);
}

// unit u -> (image, output row, first column) and the taps with at least one in-range pixel (all workgroup-uniform)
__device__ __forceinline__ unsigned dil_unit(const DilWgradArgs& a, int u, int& b, int& oh, int& ow0) {
  unsigned seg, row;
  const unsigned q = xpt_divmod((unsigned)u, (unsigned)a.nseg, seg);
  b = (int)xpt_divmod(q, (unsigned)a.H, row);
  oh = (int)row;
  ow0 = (int)seg * DW_CB;
  const int ow1 = ow0 + DW_CB < a.W ? ow0 + DW_CB : a.W;       // columns [ow0, ow1) of the unit exist
  unsigned mask = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int ih = oh + (t / 3 - 1) * a.d, sh = (t % 3 - 1) * a.d;
    const int lo = ow0 + sh > 0 ? ow0 + sh : 0, hi = ow1 + sh < a.W ? ow1 + sh : a.W;
    if (ih >= 0 && ih < a.H && lo < hi) mask |= 1u << t;
  }
  return mask;
}

__device__ __forceinline__ void dil_wgrad_fetch(const DilWgradArgs& a, int u, int spix, int gn, bool gn_ok, int xc, bool xc_ok,
                                                uint4 (&stage)[10]) {
  int b, oh, ow0;
  const unsigned mask = dil_unit(a, u, b, oh, ow0);
  const int ow = ow0 + spix;
  const long long img = (long long)b * a.H * a.W;
  {
    const bool ok = gn_ok && ow < a.W;
    const long long off = (img + (long long)oh * a.W + ow) * a.gpitch + gn;
    const uint4 v = *(const uint4*)(a.g + (ok ? off : 0));
    stage[0].x = ok ? v.x : 0u;
    stage[0].y = ok ? v.y : 0u;
    stage[0].z = ok ? v.z : 0u;
    stage[0].w = ok ? v.w : 0u;
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    // (a dead tap -- uniform -- is neither written to LDS nor multiplied; its slot re-reads the tensor's first 16 bytes, so
    //  that every slot is defined and the staging registers stay registers)
    const int ih = oh + (t / 3 - 1) * a.d, iw = ow + (t % 3 - 1) * a.d;
    const bool ok = ((mask >> t) & 1u) && xc_ok && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
    const long long off = (img + (long long)ih * a.W + iw) * a.xpitch + xc;
    const uint4 v = *(const uint4*)(a.x + (ok ? off : 0));
    stage[1 + t].x = ok ? v.x : 0u;
    stage[1 + t].y = ok ? v.y : 0u;
    stage[1 + t].z = ok ? v.z : 0u;
    stage[1 + t].w = ok ? v.w : 0u;
  }
}

__global__ __launch_bounds__(256) void dil_wgrad_kernel(DilWgradArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[10 * DW_TILE];    // g tile, then one x tile per tap: [32][64] 16-bit each
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = (blockIdx.x / a.ntc) * DW_TNB, c0 = (blockIdx.x % a.ntc) * DW_TCB;
  const int wn = wave >> 1, wc = wave & 1;                      // this wave's 32 x 32 sub-tile, all 9 taps
  const bool active = n0 + 32 * wn < a.N && c0 + 32 * wc < a.C; // wave-uniform
  // staging role: one 16-byte chunk (8 channels of one pixel) of every tile
  const int spix = tid >> 3, sc8 = tid & 7;
  const int gn = n0 + 8 * sc8, xc = c0 + 8 * sc8;
  const bool gn_ok = gn < a.N, xc_ok = xc < a.C;
  // lane roles of the transposed reads (conv_wgrad_kernel): 16-lane group g4 = (k half h, channel half), lane li = (pixel q, 4 channels p)
  const int g4 = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3, h = g4 >> 1, half = g4 & 1;
  unsigned a_base[2], b_base[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pc = 8 * h + 4 * i + q;                          // pixel of this lane's row, read i
    a_base[i] = (unsigned)((pc * DW_TNB + wn * 32 + 16 * half + 4 * p) * 2);
    b_base[i] = (unsigned)(DW_TILE + (pc * DW_TCB + wc * 32 + 16 * half + 4 * p) * 2);
  }

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  // software pipeline: the chunks of the split's next unit are fetched into registers while this one is multiplied
  uint4 stage[10];
  int u = blockIdx.y;
  if (u < a.units) dil_wgrad_fetch(a, u, spix, gn, gn_ok, xc, xc_ok, stage);
  for (; u < a.units; u += a.nsplit) {
    int b_, oh_, ow0_;
    const unsigned mask = dil_unit(a, u, b_, oh_, ow0_);
    __syncthreads();                                           // the previous unit's LDS reads are done
    *(uint4*)(smem + tid * 16) = stage[0];
#pragma unroll
    for (int t = 0; t < 9; ++t)
      if ((mask >> t) & 1u) *(uint4*)(smem + (1 + t) * DW_TILE + tid * 16) = stage[1 + t];
    __syncthreads();
    if (u + a.nsplit < a.units) dil_wgrad_fetch(a, u + a.nsplit, spix, gn, gn_ok, xc, xc_ok, stage);
    if (active) {
#pragma unroll
      for (int c16 = 0; c16 < DW_CB; c16 += 16) {
        const h16x8 fa = dil_tr_pair(smem, a_base[0] + c16 * DW_TNB * 2, a_base[1] + c16 * DW_TNB * 2);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          if ((mask >> t) & 1u) {                              // workgroup-uniform
            const unsigned xa = (unsigned)(t * DW_TILE + c16 * DW_TCB * 2);
            const h16x8 fb = dil_tr_pair(smem, b_base[0] + xa, b_base[1] + xa);
            acc[t] = XPT_MFMA_32X32X16(fa, fb, acc[t]);
          }
        }
      }
    }
  }

  // partial of this split (every split writes its whole block, zeros included): register e of tap t -> output channel
  // n0 + 32 wn + (e & 3) + 8 (e >> 2) + 4 h, input channel c0 + 32 wc + (lane & 31)
  if (!active) return;
  const int c = c0 + wc * 32 + (lane & 31);
  const int hh = lane >> 5;
  float* dst = a.part + (long long)blockIdx.y * a.N * 9 * a.Cr;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int n = n0 + wn * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (n < a.N && c < a.Cr) dst[((long long)n * 9 + t) * a.Cr + c] = acc[t][e];
    }
  }
}

// One workgroup per CU is all that runs at once (about 300 vector + accumulator registers per lane: one wave per SIMD), so the
// plan aims at 256 workgroups.  Measured on the context layers (32 images of 32 x 96): 21 splits of 128 -> 128 (the 12 MiB cap
// of the undilated kernel, 84 workgroups) 368 us; the partials a 64-way split adds (38 MB written, read once by the finishing
// launch) cost far less than the idle CUs did.
constexpr long long DW_MAX_PARTIAL_BYTES = 40ll << 20;         // per layer
constexpr int DW_TARGET_BLOCKS = 256;

struct DilWgradPlan {
  int nseg, units, nsplit, ntn, ntc;
};

bool dil_wgrad_plan(int B, int C, int N, int H, int W, DilWgradPlan& p) {
  p.nseg = (W + DW_CB - 1) / DW_CB;
  const long long units = (long long)B * H * p.nseg;
  if (units >= 0x7fffffffLL || H >= (1 << 24) || p.nseg >= (1 << 24)) return false;
  p.units = (int)units;
  p.ntn = (N + DW_TNB - 1) / DW_TNB;
  p.ntc = (C + DW_TCB - 1) / DW_TCB;
  const long long tiles = (long long)p.ntn * p.ntc;
  long long ns = (DW_TARGET_BLOCKS + tiles - 1) / tiles;
  const long long bytes = (long long)N * 9 * C * 4;
  const long long cap = DW_MAX_PARTIAL_BYTES / bytes;
  if (ns > cap) ns = cap;
  if (ns > units) ns = units;
  if (ns > 65535) ns = 65535;
  if (ns < 1) ns = 1;
  p.nsplit = (int)ns;
  return true;
}

// what every entry point refuses before any launch
bool dil_bad_geometry(int KH, int KW, int stride, int dilation) {
  return KH != 3 || KW != 3 || stride != 1 || dilation < 1 || dilation > (1 << 20);
}

}  // namespace

extern "C" int xpt_conv2d_dilated_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C,
                                      long long xpitch, int N, int KH, int KW, int stride, int dilation, long long ypitch,
                                      float slope, void* stream) {
  if (x == nullptr || w == nullptr || y == nullptr) return XPT_ERR_ARG;
  if (dil_bad_geometry(KH, KW, stride, dilation)) return XPT_ERR_ARG;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0) return XPT_ERR_SHAPE;
  if (C % 8 != 0 || N % 8 != 0 || xpitch < C || xpitch % 8 != 0 || ypitch < N || ypitch % 8 != 0 ||
      ((uintptr_t)x) % 16 != 0 || ((uintptr_t)w) % 16 != 0 || ((uintptr_t)y) % 16 != 0)
    return XPT_ERR_ARG;
  DilArgs a{};
  a.x = (const unsigned short*)x; a.w = (const unsigned short*)w; a.bias = bias; a.y = (unsigned short*)y;
  a.xpitch = xpitch; a.ypitch = ypitch;
  a.B = B; a.H = H; a.W = W; a.C = C; a.N = N; a.step = dilation; a.slope = slope;
  return dispatch_dil(a, (hipStream_t)stream);
}

extern "C" int xpt_conv2d_dilated_bwd_data(const void* g, const void* wb, void* dx, int B, int H, int W, int Np,
                                           long long gpitch, int C, int KH, int KW, int stride, int dilation,
                                           long long dxpitch, void* stream) {
  if (g == nullptr || wb == nullptr || dx == nullptr) return XPT_ERR_ARG;
  if (dil_bad_geometry(KH, KW, stride, dilation)) return XPT_ERR_ARG;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Np <= 0) return XPT_ERR_SHAPE;
  if (C % 8 != 0 || Np % 8 != 0 || gpitch < Np || gpitch % 8 != 0 || dxpitch < C || dxpitch % 8 != 0 ||
      ((uintptr_t)g) % 16 != 0 || ((uintptr_t)wb) % 16 != 0 || ((uintptr_t)dx) % 16 != 0)
    return XPT_ERR_ARG;
  DilArgs a{};
  a.x = (const unsigned short*)g; a.w = (const unsigned short*)wb; a.bias = nullptr; a.y = (unsigned short*)dx;
  a.xpitch = gpitch; a.ypitch = dxpitch;
  a.B = B; a.H = H; a.W = W; a.C = Np; a.N = C; a.step = -dilation; a.slope = 1.f;
  return dispatch_dil(a, (hipStream_t)stream);
}

extern "C" int xpt_conv2d_dilated_bwd_weight_splits(int B, int C, int N, int KH, int KW, int stride, int dilation, int H,
                                                    int W) {
  if (dil_bad_geometry(KH, KW, stride, dilation)) return XPT_ERR_ARG;
  if (B <= 0 || C <= 0 || N <= 0 || H <= 0 || W <= 0) return XPT_ERR_SHAPE;
  if (C % 8 != 0 || N % 8 != 0) return XPT_ERR_ARG;
  DilWgradPlan p;
  if (!dil_wgrad_plan(B, C, N, H, W, p)) return XPT_ERR_SHAPE;
  return p.nsplit;
}

extern "C" int xpt_conv2d_dilated_bwd_weight_partials(const void* g, const void* x, float* partials, size_t partial_floats,
                                                      int B, int H, int W, int C, int Cr, long long xpitch, int N,
                                                      long long gpitch, int KH, int KW, int stride, int dilation,
                                                      void* stream) {
  if (g == nullptr || x == nullptr || partials == nullptr) return XPT_ERR_ARG;
  if (dil_bad_geometry(KH, KW, stride, dilation)) return XPT_ERR_ARG;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Cr <= 0 || Cr > C || N <= 0) return XPT_ERR_SHAPE;
  if (C % 8 != 0 || N % 8 != 0 || xpitch < C || xpitch % 8 != 0 || gpitch < N || gpitch % 8 != 0 ||
      ((uintptr_t)g) % 16 != 0 || ((uintptr_t)x) % 16 != 0 || ((uintptr_t)partials) % 4 != 0)
    return XPT_ERR_ARG;
  DilWgradPlan p;
  if (!dil_wgrad_plan(B, C, N, H, W, p)) return XPT_ERR_SHAPE;
  if (partial_floats < (size_t)p.nsplit * N * 9 * Cr) return XPT_ERR_ARG;
  DilWgradArgs a{};
  a.g = (const unsigned short*)g; a.x = (const unsigned short*)x; a.part = partials;
  a.gpitch = gpitch; a.xpitch = xpitch;
  a.B = B; a.H = H; a.W = W; a.C = C; a.Cr = Cr; a.N = N; a.d = dilation;
  a.nseg = p.nseg; a.units = p.units; a.nsplit = p.nsplit; a.ntc = p.ntc;
  const dim3 grid(p.ntn * p.ntc, p.nsplit);
  XPT_BEGIN_LAUNCH();
  hipLaunchKernelGGL(dil_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return xpt_launch_status();
}
